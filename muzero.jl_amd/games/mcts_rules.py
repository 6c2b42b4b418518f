"""The rules-MCTS opponent, host mirror of mz_mcts_move: vanilla
UCT with uniform random rollouts over the Python envs' own rules (the cell
tuples and step functions of games/expert.py: games/tictactoe.py with quirk
Q14, games/connect4.py, selfplay.game_winner).  No network is involved; the
statistics are integers and the scores IEEE float64, so the mirror is exact.

For a live position s with p to move, S simulations and R rollouts each:
  tree    node 0 = s; an edge (v, a), a legal at v, holds n (simulations
          through it), w (the sum of their outcomes for the player to move at
          v, in rollouts) and a child or none.  N_v = sum of n, L_v = legal count.
  select  score = q + u, q = w / (n R) if n > 0 else 0, u = sqrt(N_v) / ((1 + n) L_v);
          the largest score, ties to the lowest action.
  play    a ends the game with outcome o for the mover: z = o R, no node.  Else
          the edge's child: select there.  Else a new child and R rollouts from
          its position s'; rollout j plays the k-th (ascending) legal action, k =
          rng_below(rng_u32(seed, ROLLOUT, id, rng_step, (i 64 + j) 64 + ply), legal
          count), ply = 0 at s', until the game ends; r_j = the outcome for the
          player to move at s'; z = -sum r_j.
  backup  the last edge: n += 1, w += z; z changes sign at every level going up.
The opponent plays the k-th (ascending) of the root actions with the maximal n.
"""
import math

import numpy as np

from ..rng import MZ_RNG_ROLLOUT, philox_np, rng_below
from . import connect4, tictactoe
from .expert import _cells, _rules

MAX_SIMS, MAX_ROLLOUTS = 1024, 64
DEFAULT_SIMS, DEFAULT_ROLLOUTS = 64, 16
_W, _H = connect4.W, connect4.H
_TTT_LINES = np.asarray(tictactoe.LINES)
_C4_TOP = (_W - 1) + _W * np.arange(_H)
# every four-in-a-row of the Connect4 board as cell indices
_C4_LINES = np.array([[w + k * dw + _W * (h + k * dh) for k in range(4)]
                      for w in range(_W) for h in range(_H) for dw, dh in connect4._DIRS
                      if 0 <= w + 3 * dw < _W and 0 <= h + 3 * dh < _H])


def _rollouts(name, c, p, R, seed, ident, rng_step, i):
    """r_j, j = 0..R-1, of simulation i from the live position (cells c, p to move): the R
    rollouts step together on an (R, cells) array; int64 (R,)."""
    ttt = name == "tictactoe"
    left = c.count(0)                                     # a rollout plays one stone a ply
    cells = np.tile(np.array(c, np.int8), (R, 1))
    idx = ((np.uint64(i) * np.uint64(64) + np.arange(R, dtype=np.uint64))[:, None] * np.uint64(64)
           + np.arange(left, dtype=np.uint64)[None, :])
    draws = philox_np(idx, ident, rng_step, MZ_RNG_ROLLOUT, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    draws = draws.astype(np.uint64)                       # (R, left)
    out = np.zeros(R, np.int64)
    alive = np.ones(R, bool)
    for ply in range(left):
        mover = p if ply % 2 == 0 else 3 - p
        legal = cells == 0 if ttt else cells[:, _C4_TOP] == 0
        k = (draws[:, ply] * legal.sum(1).astype(np.uint64)) >> np.uint64(32)
        a = ((np.cumsum(legal, 1) == (k + np.uint64(1))[:, None]) & legal).argmax(1)
        go = np.flatnonzero(alive)
        if ttt:
            cell = a
        else:                                             # the stone lands on the column's lowest empty cell
            cell = (cells.reshape(R, _H, _W) != 0).sum(2)[np.arange(R), a] + _W * a
        cells[go, cell[go]] = mover
        if ttt:                                           # Q14: the player now to move holds a line and wins
            winner = 3 - mover
            win = (cells[:, _TTT_LINES] == winner).all(2).any(1)
        else:                                             # four in a row through the stone wins for the mover
            winner = mover
            through = (_C4_LINES[None, :, :] == cell[:, None, None]).any(2)
            win = ((cells[:, _C4_LINES] == mover).all(2) & through).any(1)
        done = alive & (win | (cells != 0).all(1))
        out[done & win] = 1 if winner == p else -1
        alive &= ~done
        if not alive.any():
            break
    return out


def mcts_root_stats(name, board, player, sims, rollouts, seed=0, ident=0, rng_step=0):
    """The root's statistics after `sims` simulations of `rollouts` rollouts from the position `board`
    ([p1, p2, empty] planes, taken as not finished) with `player` to move, keyed (seed, id, rng_step):
    (n, w) int32 (A,) each, n = -1 and w = 0 for an illegal action."""
    legal, step, A = _rules(name)
    if player not in (1, 2):
        raise ValueError("mcts opponent: player must be 1 or 2")
    if not 1 <= sims <= MAX_SIMS:
        raise ValueError("mcts opponent: sims must be in 1..1024")
    if not 1 <= rollouts <= MAX_ROLLOUTS:
        raise ValueError("mcts opponent: rollouts must be in 1..64")
    c0 = _cells(name, board)
    R = int(rollouts)
    n_out, w_out = np.full(A, -1, np.int32), np.zeros(A, np.int32)
    if not legal(c0):
        return n_out, w_out
    nodes = [{a: [0, 0, None] for a in legal(c0)}]        # node -> action -> [n, w, child]
    for i in range(int(sims)):
        c, p, v, path = c0, int(player), 0, []
        while True:
            edges = nodes[v]
            sq, L = math.sqrt(sum(e[0] for e in edges.values())), len(edges)
            best, bs = None, 0.0
            for a in sorted(edges):
                n, w, _ = edges[a]
                sc = (w / (n * R) if n > 0 else 0.0) + sq / ((1 + n) * L)
                if best is None or sc > bs:
                    best, bs = a, sc
            e = edges[best]
            path.append(e)
            c, done, winner = step(c, p, best)
            if done:
                z = (0 if winner == 0 else 1 if winner == p else -1) * R
                break
            p = 3 - p
            if e[2] is not None:
                v = e[2]
                continue
            e[2] = len(nodes)
            nodes.append({a: [0, 0, None] for a in legal(c)})
            z = -int(_rollouts(name, c, p, R, int(seed), int(ident), int(rng_step), i).sum())
            break
        for e in reversed(path):
            e[0] += 1
            e[1] += z
            z = -z
    for a, (n, w, _) in nodes[0].items():
        n_out[a], w_out[a] = n, w
    return n_out, w_out


def mcts_pick(n, r):
    """The opponent's 1-based action: the k-th (ascending) of the legal root actions with the most
    simulations, k = rng_below(r, their count) for the 32-bit draw r (the OPPONENT stream)."""
    n = np.asarray(n)
    best = np.flatnonzero((n == n.max()) & (n >= 0))
    return int(best[rng_below(int(r), len(best))]) + 1
