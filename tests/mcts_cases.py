"""Positions and cached mirror results shared by the rules-MCTS opponent's tests
(test_mcts_opponent.py, test_mcts_rules_host.py, test_mcts_opponent_gpu.py).
A position is (board uint8 planes, player), as in expert_cases."""
import functools

import numpy as np

import expert_cases as xc
from expert_cases import HAND, NAMES, random_positions  # noqa: F401  (shared by import)

SETTINGS = ((1, 1), (8, 64), (64, 16), (200, 3))         # (S, R)
SEED = 11                                                # the engines' rng_seed in these tests

# one move from the end, a draw: player 1 fills the last cell and no line appears
TTT_LAST = (xc.ttt_board(["121", "122", "21."]), 1)
# a single legal action with three plies left: only column 6 is open
C4_ONECOL = (xc.c4_board(["112211", "221122", "112211", "221122", "112211", "221122", "112"]), 2)
# two full columns in mid-game: five legal actions
C4_TWOFULL = (xc.c4_board(["121212", "", "212121", "1", "2", "", ""]), 1)

EXTRA = {"tictactoe": (TTT_LAST,), "connect4": (C4_ONECOL, C4_TWOFULL)}


@functools.lru_cache(maxsize=None)
def positions(name):
    """A spread of the random-play positions (every 25th: early, middle and late plies), the
    hand-made positions of expert_cases and the ones above."""
    return tuple(random_positions(name)[::25]) + tuple(HAND[name]) + EXTRA[name]


@functools.lru_cache(maxsize=None)
def _stats(name, key, player, S, R, seed, ident, rng_step):
    from muzero_jl_amd.games.mcts_rules import mcts_root_stats
    n, w = mcts_root_stats(name, np.frombuffer(key, np.uint8), player, S, R, seed, ident, rng_step)
    n.setflags(write=False)
    w.setflags(write=False)
    return n, w


def mirror(name, pos, S, R, ident=0, rng_step=0, seed=SEED):
    """(n, w) of the Python mirror, computed once per distinct call and left unchanged."""
    board, player = pos
    return _stats(name, np.asarray(board, np.uint8).tobytes(), int(player), S, R, seed, ident, rng_step)


def mirror_rows(name, rows, S, R, game_offset=0, rng_step=0, seed=SEED):
    """The mirror of one mz_mcts_eval call: row g is keyed game_offset + g."""
    out = [mirror(name, pos, S, R, game_offset + g, rng_step, seed) for g, pos in enumerate(rows)]
    return np.stack([n for n, _ in out]), np.stack([w for _, w in out])
