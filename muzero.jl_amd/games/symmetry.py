"""Board symmetries of the two-player board envs: the cell and action permutation tables
the device sampler holds (mz_replay_set_symmetry), built from the same formulae.

Cells are col-major, cell (i, j) = i + W·j with W = observation_shape[0].

Square board (TicTacToe, n = 8, the dihedral group): id s transposes (i, j) -> (j, i) if s >= 4, then
makes s & 3 quarter turns (a, b) -> (b, W - 1 - a).  Action a <-> cell a - 1, so the action table is
the cell table.

Column-drop board (Connect4, n = 2, the left-right mirror): id 1 moves cell (w, h) to (w, H - 1 - h)
and the 0-based action (the column) h to H - 1 - h.

A table row s maps c to the index that cell / action c moves to.
"""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class SymmetryTables:
    cell: np.ndarray            # (n, P) int32
    action: np.ndarray          # (n, A) int32, 0-based
    planes: int                 # board planes C of one observation (observation_shape[2])

    @property
    def n(self):
        return self.cell.shape[0]


def square_cells(W):
    """(8, W·W) cell table of a W x W board."""
    out = np.zeros((8, W * W), np.int32)
    for s in range(8):
        for j in range(W):
            for i in range(W):
                a, b = (j, i) if s >= 4 else (i, j)
                for _ in range(s & 3):
                    a, b = b, W - 1 - a
                out[s, i + W * j] = a + W * b
    return out


def column_cells(W, H):
    """((2, W·H) cell table, (2, H) action table) of a board of H columns of W rows."""
    cell = np.zeros((2, W * H), np.int32)
    for h in range(H):
        for w in range(W):
            cell[0, w + W * h] = w + W * h
            cell[1, w + W * h] = w + W * (H - 1 - h)
    act = np.stack([np.arange(H), H - 1 - np.arange(H)]).astype(np.int32)
    return cell, act


def tables(env_name, observation_shape):
    """The symmetry group of env `env_name` ("tictactoe" / "connect4") on a board of observation_shape
    (W, H, C).  The Atari-like env has none."""
    W, H, C = observation_shape
    if env_name == "tictactoe":
        if W != H:
            raise ValueError("symmetry: a square board is needed")
        cell = square_cells(W)
        return SymmetryTables(cell, cell.copy(), C)
    if env_name == "connect4":
        cell, act = column_cells(W, H)
        return SymmetryTables(cell, act, C)
    raise ValueError(f"symmetry: env {env_name} has no symmetry group")


def for_conf(conf):
    """tables() of a board-game config: one action per cell -> the square board, one per column ->
    the column-drop board."""
    W, H, _ = conf.observation_shape
    A = len(conf.action_space)
    if W == H and A == W * H:
        return tables("tictactoe", conf.observation_shape)
    if A == H:
        return tables("connect4", conf.observation_shape)
    raise ValueError("symmetry: the config is neither a square one-action-per-cell board nor a column-drop board")


def inverse(t, s):
    """The id of s's inverse in the group."""
    for r in range(t.n):
        if np.array_equal(t.cell[r][t.cell[s]], np.arange(t.cell.shape[1])):
            return r
    raise ValueError("symmetry: the table is not a group")
