"""Shared by test_test_worker.py (CPU) and test_test_worker_gpu.py: the FC
TicTacToe evaluation of the test worker that both play — the
config, the weights, the keys — and the CPU oracle dressed as an engine for
the host mirror.  The CPU test asserts that these keys give an evaluation
whose slots finish on different moves, with a game ended by length and a won
one, so the GPU test that reuses them cannot pass vacuously."""
import dataclasses

import numpy as np

SEED = 5                      # the engines' rng_seed
WSEED = 105                   # init_nets seed
E, SIMS, MAX_MOVES = 5, 8, 6
STEP0, GOFF, TEMP = 200, 7, 1.0
# (opponent, muzero_player) of the GPU test; the three conditions hold for VARIED (asserted on the CPU)
CONFIGS = [("self", 1), ("self", 2), ("random", 1), ("random", 2), ("expert", 1), ("expert", 2)]
VARIED = [("self", 1), ("random", 1), ("random", 2), ("expert", 2)]


def ttt_conf(**kw):
    from muzero_jl_amd.games import tictactoe as ttt
    kw.setdefault("num_iters", SIMS)
    kw.setdefault("max_moves", MAX_MOVES)
    return dataclasses.replace(ttt.conf, replay_buffer_size=64, **kw)


def ttt_nets(conf=None, wseed=WSEED):
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    return init_nets(conf or ttt_conf(), ttt.hyper, seed=wseed)


def oracle_engine(conf=None, wseed=WSEED, seed=SEED):
    """The CPU oracle with the two attributes BatchedSelfPlay reads from an engine."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from muzero_jl_amd.games import tictactoe as ttt
    from oracle import Oracle
    conf = conf or ttt_conf()
    ora = Oracle(to_c_config(conf), to_c_ffhp(ttt.hyper), seed=seed)
    for n, w in enumerate(ttt_nets(conf, wseed)):
        ora.set_weights(n, w)
    ora.conf, ora.rng_seed = conf, seed
    return ora


def same_history(a, b):
    """Two GameHistory records, array for array."""
    x, y = a.as_arrays(), b.as_arrays()
    return all(x[k].shape == y[k].shape and np.array_equal(x[k], y[k]) for k in x)


def same_record(got, want):
    """Two records: the integers, and the float64 sums bit for bit."""
    from muzero_jl_amd.abi import TEST_COUNT_FIELDS, TEST_SUM_FIELDS
    ints = all(int(got[k]) == int(want[k]) for k in TEST_COUNT_FIELDS)
    bits = all(np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() for k in TEST_SUM_FIELDS)
    return ints and bits
