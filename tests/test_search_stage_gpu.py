"""The small kernels' network stage (csrc/mz_small.hip sm_stage) on the GPU: the
quarter sums formed across the games of a workgroup (sm_qsum), the stage records with absolute
addresses, a per-row stride and the flags in .y (mz_small_params.h), the scalar stage-count
test, and the fused first stage's inputs read in two round trips (sm_fused_in).

The search cases force MZ_SEARCH_KERNEL=small and compare trees, child visits, root values and
actions bit for bit with the C oracle on nets of the "biased" regime (tests/weight_regimes.py),
with the set-ups and helpers of tests/test_search_prologue_gpu.py.  Equality is exact: the
stage performs the oracle's f32 operations in the oracle's order, so no case has a tolerance.

* T in {1, 2, 4} with G = 1 (T = 1) and G = 5 (T = 2, 4): the last workgroup holds inactive
  games, whose accumulators enter the swaps across the games;
* S in {1, 5};
* hidden_state_size 27 and 40: the first layers have kq = 8 and kq = 12, so the stride in the
  record differs between the layers of one launch; with 40 the action-plane rows k >= H of
  the dynamics input fall in another quarter than the state rows.  27 is TicTacToe's (the
  engine takes hidden_state_size = prod(observation_shape) only); 40 is a 5 x 4 x 2
  observation without stacking (40 features, a 20-float action plane) on random inputs;
* width_hidden 32: two layers share a slot, so the rows of one wave-stage have different
  input bases;
* a shallow net (n_sim = 4 < SM_MAX_SIM): the scalar stage-count test ends the stages early;
* use_batch_norm: the _bn instances (the BatchNorm flag in .y);
* exploration off.
The learner cases run one chunk of the multi-step learner per T its plan picks (1, 2, 4)
against the same steps one after another on a second engine (the one-launch step, another T):
losses, θ and the unroll read-outs of every step, bit for bit.
Reference: src/SelfPlay.jl:225-283, src/Learning.jl:293-343.
"""
import dataclasses
import functools

import numpy as np
import pytest

import weight_regimes as wr
from test_bench_sizes_gpu import _oracle_search_threads
from test_gpu_parity import _compare_trees
from test_search_prologue_gpu import SHALLOW, _run

pytestmark = pytest.mark.gpu

TG = [(1, 1), (2, 5), (4, 5)]


@functools.lru_cache(maxsize=None)
def _setup40(S, G):
    """(conf, hyper, biased nets, obs, legal, to_play) with a 40-float hidden state."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    conf = dataclasses.replace(ttt.conf, num_iters=S, observation_shape=(5, 4, 2), stacked_observations=0)
    hyper = dataclasses.replace(ttt.hyper, hidden_state_size=40)
    nets = wr.named(conf, hyper, init_nets(conf, hyper, seed=1234), "biased", seed=1234 % 97)
    rng = np.random.default_rng(40)
    obs = (rng.random((G, 40)) < 0.4).astype(np.float32)
    legal = rng.random((G, len(conf.action_space))) < 0.6
    legal[:, 4] = True
    return conf, hyper, nets, obs, legal, rng.integers(1, 3, G).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference40(S, G, explore):
    """The oracle's search of one 40-float set-up, computed once and shared by the T cases."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    conf, hyper, nets, obs, legal, tp = _setup40(S, G)
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=1)
    for n, w in enumerate(nets):
        ora.set_weights(n, w)
    return _oracle_search_threads(ora, obs, legal, tp, chunks=min(16, G), exploration=explore, rng_step=3,
                                  game_offset=0, temperature=1.0)


def _run40(monkeypatch, T, S, G, explore):
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper, nets, obs, legal, tp = _setup40(S, G)
    eng = Engine(conf, hyper, device=0, max_games=G, rng_seed=1)
    eng.debug_enable(1)
    try:
        for n, w in enumerate(nets):
            eng.set_weights(n, w)
        cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=3, game_offset=0,
                                      temperature=1.0)
        cv2, rv2, act2, tree_o, _ = _reference40(S, G, explore)
        _compare_trees(eng.debug_tree(G), tree_o, G)
        assert np.array_equal(cv, cv2), "child visits differ"
        assert np.array_equal(rv, rv2), "root values differ"
        assert np.array_equal(act, act2), "actions differ"
        return eng.search_variant()
    finally:
        eng.close()


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("S", [1, 5])
def test_default_net(monkeypatch, T, G, S):
    assert _run(monkeypatch, T, S, G, True) == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("S", [1, 5])
def test_hidden_state_40(monkeypatch, T, G, S):
    """kq = 12 (prediction, 40 inputs) and kq = 16 (dynamics, 40 + 20) first layers, where the
    default net (H = 27, test_default_net) has kq = 8 (27 inputs) and kq = 12 (27 + 9)."""
    assert _run40(monkeypatch, T, S, G, True) == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_two_layers_in_a_slot(monkeypatch, T, G):
    assert _run(monkeypatch, T, 5, G, True, (("width_hidden", 32),)) == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_shallow_net(monkeypatch, T, G):
    """n_sim = 4: the stage-count test leaves the unrolled stages after the fourth."""
    assert _run(monkeypatch, T, 5, G, True, SHALLOW) == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_batch_norm(monkeypatch, T, G):
    assert _run(monkeypatch, T, 5, G, True, bn=True) == f"mz_search_small{T}_bn"


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("H", [27, 40])
def test_exploration_off(monkeypatch, T, G, H):
    run = _run if H == 27 else _run40
    assert run(monkeypatch, T, 5, G, False) == f"mz_search_small{T}"


# the plan's choice of T at 256 CUs (tests/test_learner_multi_gpu.py): L·B <= 256 -> T = 1;
# L >= 32 and L·⌈B/4⌉ >= 256 -> T = 4; else T = 2
@pytest.mark.parametrize("L,T", [(8, 1), (16, 2), (37, 4)])
def test_multi_step_learner_matches_sequential_steps(L, T):
    import torch
    from muzero_jl_amd.config import cos_schedule
    from test_learner_multi_gpu import _pair, _theta
    B, t0 = 32, 3
    _, _, _, (e1, e2) = _pair("ttt")
    try:
        nflat = sum(e1.param_count(n) for n in range(3))
        l1 = torch.zeros(8, dtype=torch.float32, device="cuda")
        lm = torch.zeros((L, 8), dtype=torch.float32, device="cuda")
        th = torch.zeros((L, nflat), dtype=torch.float32, device="cuda")
        etas = [cos_schedule(t0 + i) for i in range(L)]
        want = []
        for i in range(L):
            e1.learner_train_dev(B, t0 + i, etas[i], l1.data_ptr())
            e1.sync()
            want.append((l1.cpu().numpy()[:6].copy(), _theta(e1), [x.copy() for x in e1.debug_unroll(B)]))
        e2.learner_train_multi_dev(B, t0, etas, lm.data_ptr(), th.data_ptr())
        e2.sync()
        assert e1.learner_variant().startswith("mz_learn_small"), e1.learner_variant()
        assert "multi" in e2.learner_variant(), e2.learner_variant()
        if torch.cuda.get_device_properties(0).multi_processor_count == 256:
            assert e2.learner_variant().endswith(f"mz_learn_multi{T}"), e2.learner_variant()
        got_l, got_t = lm.cpu().numpy(), th.cpu().numpy()
        for i, (wl, wt, wu) in enumerate(want):
            assert np.array_equal(got_l[i, :6], wl), (i, got_l[i, :6], wl)
            assert np.array_equal(got_t[i], wt), (i, "theta")
            if i >= L - 33:                            # (the read-outs are a ring of >= 33 steps)
                for g, w in zip(e2.debug_unroll_step(i, B), wu):
                    assert np.array_equal(g, w), (i, "read-outs")
    finally:
        e1.close(); e2.close()
