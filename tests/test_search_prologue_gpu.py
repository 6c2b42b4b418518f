"""The small search kernels' launch prologue (csrc/mz_small.hip small_body) on
the GPU: everything in front of simulation 0 — the setup values loaded ahead of the weight
image, the stage records merged with their biases in registers, the representation on register
sets RO .. RO + n_root with the sim stages preloaded around it, and the reload under the root
prediction's first stages.

Every case forces MZ_SEARCH_KERNEL=small and compares trees, child visits, root values and
actions bit for bit with the C oracle, on nets of the "biased" regime (tests/weight_regimes.py):
every Dense bias nonzero and distinct, so a record merged with the wrong bias shows.

* S in {1, 5}: with one simulation the launch is nearly all prologue, and a register set that
  is stale after the reload decides the only expansion;
* G = 5 at T = 2 and T = 4 (inactive games in the last workgroup), G = 1 at T = 1;
* depth_representation in {0, 1, 3, 4}: n_root = 2, 3, 5, 6; at 6 the representation fills
  sets 2..7 and no sim stage is preloaded above it;
* a shallow net (n_sim = 4) against the deepest representation: RO + n_root > n_sim;
* use_batch_norm: the _bn instances, whose (γ, β) table the prologue builds;
* exploration on and off (the noise drawn in the prologue, or not);
* two searches on one engine with other weights set between them.
Reference: src/SelfPlay.jl:225-283.
"""
import dataclasses
import functools

import numpy as np
import pytest

import weight_regimes as wr
from test_bench_sizes_gpu import _oracle_search_threads
from test_gpu_parity import _compare_trees

pytestmark = pytest.mark.gpu

SHALLOW = (("depth_prediction", 1), ("depth_dynamics", 1), ("depth_state_head", 1))


@functools.lru_cache(maxsize=None)
def _setup(S, G, hp=(), bn=False, seed=1234):
    """(conf, hyper, biased nets, obs, legal, to_play); hp: FeedForwardHP fields to replace."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    from muzero_jl_amd.selfplay import random_positions
    conf = dataclasses.replace(ttt.conf, num_iters=S)
    hyper = dataclasses.replace(ttt.hyper, use_batch_norm=bn, **dict(hp))
    if bn:
        from test_fc_bn import _bn_nets
        nets = _bn_nets(conf, hyper, seed=seed % 1000)
    else:
        nets = init_nets(conf, hyper, seed=seed)
    nets = wr.named(conf, hyper, nets, "biased", seed=seed % 97)
    obs, legal, tp = random_positions(ttt.BatchedTicTacToe, G, seed=100, max_plies=6)
    return conf, hyper, nets, obs, legal, tp


@functools.lru_cache(maxsize=None)
def _reference(S, G, explore, hp=(), bn=False, seed=1234):
    """The oracle's search of one set-up, computed once and shared by the T cases."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    conf, hyper, nets, obs, legal, tp = _setup(S, G, hp, bn, seed)
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=1)
    for n, w in enumerate(nets):
        ora.set_weights(n, w)
    return _oracle_search_threads(ora, obs, legal, tp, chunks=min(16, G), exploration=explore, rng_step=3,
                                  game_offset=0, temperature=1.0)


def _search(eng, S, G, explore, hp=(), bn=False, seed=1234):
    """One search on `eng` with the set-up's weights, against the oracle."""
    conf, hyper, nets, obs, legal, tp = _setup(S, G, hp, bn, seed)
    for n, w in enumerate(nets):
        eng.set_weights(n, w)
    cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=3, game_offset=0, temperature=1.0)
    tree_g = eng.debug_tree(G)
    cv2, rv2, act2, tree_o, _ = _reference(S, G, explore, hp, bn, seed)
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2), "child visits differ"
    assert np.array_equal(rv, rv2), "root values differ"
    assert np.array_equal(act, act2), "actions differ"


def _run(monkeypatch, T, S, G, explore, hp=(), bn=False):
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper = _setup(S, G, hp, bn)[:2]
    eng = Engine(conf, hyper, device=0, max_games=G, rng_seed=1)
    eng.debug_enable(1)
    try:
        _search(eng, S, G, explore, hp, bn)
        return eng.search_variant()
    finally:
        eng.close()


@pytest.mark.parametrize("T,G", [(1, 1), (2, 5), (4, 5)])
@pytest.mark.parametrize("S", [1, 5])
def test_few_simulations(monkeypatch, T, G, S):
    assert _run(monkeypatch, T, S, G, True) == f"mz_search_small{T}"


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("depth", [0, 1, 3, 4])
def test_representation_depth(monkeypatch, T, depth):
    """n_root = depth + 2 = 2, 3, 5, 6 stages on register sets 2 .. 2 + n_root."""
    assert _run(monkeypatch, T, 5, 5, True, (("depth_representation", depth),)) == f"mz_search_small{T}"


@pytest.mark.parametrize("T", [1, 2, 4])
def test_shallow_net_deep_representation(monkeypatch, T):
    """n_sim = 4 < RO + n_root = 8: the representation's upper sets take no sim stage."""
    variant = _run(monkeypatch, T, 5, 5 if T > 1 else 1, True, SHALLOW + (("depth_representation", 4),))
    assert variant == f"mz_search_small{T}"


@pytest.mark.parametrize("T", [1, 2, 4])
def test_batch_norm(monkeypatch, T):
    assert _run(monkeypatch, T, 5, 5 if T > 1 else 1, True, bn=True) == f"mz_search_small{T}_bn"


@pytest.mark.parametrize("explore", [True, False])
@pytest.mark.parametrize("S", [1, 5])
def test_exploration_on_off(monkeypatch, explore, S):
    assert _run(monkeypatch, 2, S, 8, explore) == "mz_search_small2"


@pytest.mark.parametrize("T", [2, 4])
def test_new_weights_between_searches(monkeypatch, T):
    """The second launch's prologue reads the images set after the first."""
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper, nets_a = _setup(5, 5)[:3]
    nets_b = _setup(5, 5, seed=4321)[2]
    assert all(not np.array_equal(a, b) for a, b in zip(nets_a, nets_b))
    assert not np.array_equal(_reference(5, 5, True)[1], _reference(5, 5, True, seed=4321)[1]), "same root values"
    eng = Engine(conf, hyper, device=0, max_games=5, rng_seed=1)
    eng.debug_enable(1)
    try:
        _search(eng, 5, 5, True)
        _search(eng, 5, 5, True, seed=4321)
        _search(eng, 5, 5, True)
        assert eng.search_variant() == f"mz_search_small{T}"
    finally:
        eng.close()
