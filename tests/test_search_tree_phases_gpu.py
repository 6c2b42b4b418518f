"""The small kernels' tree phases (csrc/mz_tree_device.h, csrc/mz_small.hip small_body, DESIGN
§4.13) on the GPU: wave 0's loads of the read-outs + backup issued in front of the activations,
and the ballot select with the game's tag read beside the entries and the node statics held in
the selecting wave's registers.  The cases were also cut for the ascending f32 sums of a 16-lane
group (gseqsum<16>: the expansion's double softmax, the root noise, the learner's loss sums)
taken by DPP row broadcasts; that form measured slower and is not in the tree (§4.13), the cases
stay for whoever tries it again.

Every search case forces MZ_SEARCH_KERNEL=small and compares trees, child visits, root values
and actions bit for bit with the C oracle; no case has a tolerance.

* T in {1, 2, 4} with G = 1 (T = 1) and G = 5 (T = 2, 4): the last workgroup holds inactive
  rows beside active ones, where a sum over a DPP row could pick up a foreign lane;
* S in {1, 5, 17};
* A = 9 (TicTacToe: the sum ends inside its third block of four), A = 7 (Connect4 FC: inside
  the second; its 126-feature input keeps it on the tile-16 kernel, whose sums are the same
  function), A = 4 and A = 16 (the block boundaries: TicTacToe's nets with a replaced
  action_space on random inputs and legal masks);
* one legal action per position to S = 17 (one nonzero term per sum; every simulation one level
  deeper, so the backup's loop past its first 16 levels runs behind the early loads), for two
  players and for one (backup_path), all nine legal, exploration on and off, the BatchNorm
  instances;
* the tie regime (an all-zero prediction net): every simulation walks, so every node's statics
  are set on the walk path and read by later ballot passes;
* the fast regime: the select counters, as tests/test_select_ballot_gpu.py asserts them.
The learner cases run one multi-step chunk per plan T against sequential steps (the loss sums
share gseqsum), with the check of tests/test_search_stage_gpu.py.
Reference: src/SelfPlay.jl:88-109, 190-217, 254-283, src/Learning.jl:261-288.
"""
import dataclasses
import functools

import numpy as np
import pytest

from test_bench_sizes_gpu import _oracle_search_threads
from test_gpu_parity import _compare_trees
from test_search_prologue_gpu import _run as _run_biased
from test_search_stage_gpu import test_multi_step_learner_matches_sequential_steps as _learner_chunk_check
from test_select_ballot_gpu import _run as _run_ballot

pytestmark = pytest.mark.gpu

TG = [(1, 1), (2, 5), (4, 5)]


@functools.lru_cache(maxsize=None)
def _setup(S, G, A=9, one_player=False, legal_mode="position"):
    """(conf, hyper, nets, obs, legal, to_play) on TicTacToe's nets.  A != 9: a replaced
    action_space (the policy head and the action encoding follow it) on random inputs.
    legal_mode: "position" (the positions' own, or random masks for A != 9), "single" (the first
    legal action only), "all"."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    from muzero_jl_amd.selfplay import random_positions
    conf = dataclasses.replace(ttt.conf, num_iters=S)
    if A != 9:
        conf = dataclasses.replace(conf, action_space=list(range(1, A + 1)))
    if one_player:
        conf = dataclasses.replace(conf, players=[1])
    nets = init_nets(conf, ttt.hyper, seed=1234)
    if A == 9:
        obs, legal, tp = random_positions(ttt.BatchedTicTacToe, G, seed=100, max_plies=6)
    else:
        rng = np.random.default_rng(A)
        obs = (rng.random((G, 63)) < 0.4).astype(np.float32)
        legal = rng.random((G, A)) < 0.6
        legal[:, A - 1] = True                             # the last lane of the last block is in use
        tp = rng.integers(1, 3, G).astype(np.int32)
    legal = np.array(legal, dtype=bool)
    if legal_mode == "single":
        first = np.argmax(legal, axis=1)
        legal[:] = False
        legal[np.arange(G), first] = True
    elif legal_mode == "all":
        legal[:] = True
    if one_player:
        tp = np.ones(G, np.int32)
    return conf, ttt.hyper, nets, obs, legal, tp


@functools.lru_cache(maxsize=None)
def _reference(S, G, explore, A=9, one_player=False, legal_mode="position"):
    """The oracle's search of one set-up, computed once and shared by the T cases."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    conf, hyper, nets, obs, legal, tp = _setup(S, G, A, one_player, legal_mode)
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=1)
    for n, w in enumerate(nets):
        ora.set_weights(n, w)
    return _oracle_search_threads(ora, obs, legal, tp, chunks=min(16, G), exploration=explore, rng_step=3,
                                  game_offset=0, temperature=1.0)


def _run(monkeypatch, T, S, G, explore, A=9, one_player=False, legal_mode="position"):
    """One GPU search against the oracle; returns (variant, fast, walked, the oracle's stats)."""
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper, nets, obs, legal, tp = _setup(S, G, A, one_player, legal_mode)
    eng = Engine(conf, hyper, device=0, max_games=G, rng_seed=1)
    try:
        for n, w in enumerate(nets):
            eng.set_weights(n, w)
        eng.debug_enable(1)
        cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=3, game_offset=0,
                                      temperature=1.0)
        tree_g = eng.debug_tree(G)
        fast, walked = eng.debug_select_stats(G)
        variant = eng.search_variant()
    finally:
        eng.close()
    cv2, rv2, act2, tree_o, stats = _reference(S, G, explore, A, one_player, legal_mode)
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2), "child visits differ"
    assert np.array_equal(rv, rv2), "root values differ"
    assert np.array_equal(act, act2), "actions differ"
    assert np.all(fast + walked == S)
    return variant, fast, walked, stats


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("S", [1, 5, 17])
def test_default_net(monkeypatch, T, G, S):
    """A = 9 on nets with every Dense bias nonzero (the "biased" regime of the prologue tests)."""
    assert _run_biased(monkeypatch, T, S, G, True) == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("A", [4, 16])
def test_action_count_on_a_block_boundary(monkeypatch, T, G, A):
    """The sum's last block of four is full (A = 4: the unconditional one; A = 16: all four)."""
    variant, _, walked, _ = _run(monkeypatch, T, 5, G, True, A=A)
    assert variant == f"mz_search_small{T}"
    assert np.all(walked >= 1)                             # simulation 0: the root's entry is not computed yet


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("one_player", [False, True])
def test_single_legal_chain(monkeypatch, T, G, one_player):
    """One legal action per position: one nonzero term per sum, and simulation s ends at depth
    s + 1, so simulation 16 backs up 18 levels (two players: the loop behind backup_path_pre's
    first 16 lanes; one player: backup_path).  A single candidate never ties: only simulation 0
    walks, and every later ballot pass reads the statics the earlier ones left in the lanes."""
    variant, fast, walked, stats = _run(monkeypatch, T, 17, G, True, one_player=one_player, legal_mode="single")
    assert variant == f"mz_search_small{T}"
    assert stats[1] >= 16, f"max select depth {stats[1]}: the chain was not reached"
    assert np.all(walked == 1) and np.all(fast == 16)


@pytest.mark.parametrize("T,G", TG)
def test_all_legal(monkeypatch, T, G):
    variant, _, walked, _ = _run(monkeypatch, T, 17, G, True, legal_mode="all")
    assert variant == f"mz_search_small{T}"
    assert np.all(walked >= 1)


@pytest.mark.parametrize("explore", [True, False])
@pytest.mark.parametrize("S", [5, 17])
def test_exploration_on_off(monkeypatch, explore, S):
    """The root noise sum (drawn on the noise wave, G = 7 of 8 rows of its workgroups), or none."""
    variant, _, _, _ = _run(monkeypatch, 2, S, 7, explore)
    assert variant == "mz_search_small2"


@pytest.mark.parametrize("T,G", TG)
def test_one_player(monkeypatch, T, G):
    variant, _, _, _ = _run(monkeypatch, T, 17, G, True, one_player=True)
    assert variant == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_batch_norm(monkeypatch, T, G):
    assert _run_biased(monkeypatch, T, 17, G, True, bn=True) == f"mz_search_small{T}_bn"


@pytest.mark.parametrize("T", [1, 2, 4])
def test_fast_regime(monkeypatch, T):
    """The bench's nets and positions (CPU-derived: 129 of the 6,400 simulations have a tied
    level, 128 of them simulation 0): nearly every leaf is found by the ballot pass."""
    variant, fast, walked, _ = _run_ballot(monkeypatch, T, "ttt", 50, 128, True)
    assert variant == f"mz_search_small{T}"
    assert np.all(fast + walked == 50)
    assert np.all(walked >= 1)
    assert np.all(walked <= 5)
    assert walked.sum() <= 160


@pytest.mark.parametrize("T", [1, 2, 4])
def test_tie_regime(monkeypatch, T):
    """An all-zero prediction net without noise (CPU-derived: 6,166 of the 6,400 simulations
    have a tied level): the new node's statics come from the walk's outcome nearly every time."""
    variant, fast, walked, _ = _run_ballot(monkeypatch, T, "ttt", 50, 128, False, zero_pred=True)
    assert variant == f"mz_search_small{T}"
    assert np.all(fast + walked == 50)
    assert walked.sum() >= 6000


def test_connect4(monkeypatch):
    """A = 7, G = 6 of the tile's 16 rows.  The engine runs Connect4 FC on the tile-16 kernel
    (test_select_ballot_gpu.test_connect4), whose expansion and root noise use the same sums."""
    variant, fast, walked, _ = _run_ballot(monkeypatch, 2, "c4", 50, 6, True)
    if variant.startswith("mz_search_small"):
        assert variant == "mz_search_small2"
        assert np.all(fast + walked == 50)
    else:
        assert variant in ("mz_search_kernel_lds", "mz_search_kernel_hbm", "mz_search_kernel_lds_res",
                           "mz_search_kernel_hbm_res"), variant


# the smallest L at which the plan picks each T at 256 CUs (tests/test_search_stage_gpu.py)
@pytest.mark.parametrize("L,T", [(8, 1), (16, 2), (37, 4)])
def test_multi_step_learner_chunk(L, T):
    """Losses, θ and the read-outs of every step of one chunk against sequential steps, bit for bit."""
    _learner_chunk_check(L, T)
