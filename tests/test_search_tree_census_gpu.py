"""The small kernels' simulation loop outside the network stages (csrc/mz_small.hip small_body,
csrc/mz_tree_device.h) on the GPU: the select's LDS addresses formed once per
launch, and wave 0's read-out kind and address held per lane.  The cases were also cut for the
expansion's double softmax on a det_expf with its range guards as selects; that form measured
slower and is not in the tree (§4.14), the cases stay for whoever tries it again.

Every case forces MZ_SEARCH_KERNEL=small, asserts that the small kernel ran, and compares
trees, child visits, root values and actions bit for bit with the C oracle; no case has a
tolerance.  The select counters (fast + walked = S per game, and each regime's own bounds) are
asserted as tests/test_select_ballot_gpu.py does.

* T in {1, 2, 4} with G = 1 (T = 1) and G = 5 (T = 2, 4): the last workgroup holds inactive
  games, whose waves select nothing and whose rows expand nothing;
* S in {1, 5, 17}; A in {4, 9, 16}; exploration on and off; one player and two; the BatchNorm
  instances; the tie regime (every simulation walks); one legal action to S = 17 (paths past
  16 levels);
* the value and reward heads with different read-out activations (tanh / identity, tanh / relu)
  and with the same one (tanh / tanh): wave 0's per-lane kind, even lanes the value's, odd
  lanes the reward's;
* policy logits spread by more than 88 and by more than 104 through the policy head's last
  bias: softmax terms exp(x - max) that are subnormal (x - max in (-103.97, -87.34), down to
  the smallest subnormal just above the guard) and that are zero by det_expf's lower guard
  (below -103.97), all inside the expansion.  The upper guard cannot be met there
  (x - max <= 0).
Reference: src/SelfPlay.jl:88-96, 190-217, 254-283.
"""
import dataclasses
import functools

import numpy as np
import pytest

from test_bench_sizes_gpu import _oracle_search_threads
from test_gpu_parity import _compare_trees
from test_search_prologue_gpu import _run as _run_biased
from test_search_tree_phases_gpu import TG, _run
from test_select_ballot_gpu import _run as _run_ballot

pytestmark = pytest.mark.gpu

# the policy head's last bias per action (A = 9): the logits of init_nets stay within
# 0.25 of it.  "sub": the spread is 96 — past 88, short of 104 — so the smallest terms are
# subnormal; "zero": 120, with entries on both sides of the lower guard and of the first
# subnormal result
SPREAD = {
    "sub": [0.0, -12.0, -96.0, -24.0, -88.0, -48.0, -92.0, -60.0, -95.5],
    "zero": [0.0, -104.5, -30.0, -120.0, -87.5, -103.5, -60.0, -100.0, -90.0],
}


@functools.lru_cache(maxsize=None)
def _setup(S, G, hp=(), spread=None, legal_mode="position"):
    """(conf, hyper, nets, obs, legal, to_play) on TicTacToe; hp: FeedForwardHP fields to replace;
    spread: a key of SPREAD."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets, layer_specs
    from muzero_jl_amd.selfplay import random_positions
    import weight_regimes as wr
    conf = dataclasses.replace(ttt.conf, num_iters=S)
    hyper = dataclasses.replace(ttt.hyper, **dict(hp))
    nets = wr.named(conf, hyper, init_nets(conf, hyper, seed=1234), "biased", seed=11)
    if spread is not None:
        chains = [s[0] for s in layer_specs(conf, hyper, 1)]
        k_pol = max(k for k, ch in enumerate(chains) if ch == 2)      # the policy head's last layer
        (off, n), = [(o, n) for k, o, n in wr.bias_slices(conf, hyper, 1) if k == k_pol]
        assert n == 9
        nets[1][off:off + n] = np.asarray(SPREAD[spread], np.float32)
    obs, legal, tp = random_positions(ttt.BatchedTicTacToe, G, seed=100, max_plies=6)
    legal = np.array(legal, dtype=bool)
    if legal_mode == "all":
        legal[:] = True
    return conf, hyper, nets, obs, legal, tp


@functools.lru_cache(maxsize=None)
def _reference(S, G, explore, hp=(), spread=None, legal_mode="position"):
    """The oracle's search of one set-up, computed once and shared by the T cases."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    conf, hyper, nets, obs, legal, tp = _setup(S, G, hp, spread, legal_mode)
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=1)
    for n, w in enumerate(nets):
        ora.set_weights(n, w)
    return _oracle_search_threads(ora, obs, legal, tp, chunks=min(16, G), exploration=explore, rng_step=3,
                                  game_offset=0, temperature=1.0)


def _run_nets(monkeypatch, T, S, G, explore, hp=(), spread=None, legal_mode="position"):
    """One GPU search of a set-up of this file against the oracle; returns (the oracle's tree, nets)."""
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper, nets, obs, legal, tp = _setup(S, G, hp, spread, legal_mode)
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
    assert variant == f"mz_search_small{T}", variant
    cv2, rv2, act2, tree_o, _ = _reference(S, G, explore, hp, spread, legal_mode)
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2), "child visits differ"
    assert np.array_equal(rv, rv2), "root values differ"
    assert np.array_equal(act, act2), "actions differ"
    assert np.all(fast + walked == S)
    assert np.all(walked >= 1)                             # simulation 0: the root's entry is not computed yet
    return tree_o, nets


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("S", [1, 5, 17])
def test_simulation_counts(monkeypatch, T, G, S):
    """A = 9, exploration on, two players; S = 1: the loop's body once, no recompute."""
    variant, fast, walked, _ = _run(monkeypatch, T, S, G, True)
    assert variant == f"mz_search_small{T}"
    assert np.all(walked >= 1)


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("A", [4, 16])
def test_action_counts(monkeypatch, T, G, A):
    """A = 4 and A = 16 (A = 9: every other case): the expansion's lanes past A hold -inf and count for nothing."""
    variant, _, walked, _ = _run(monkeypatch, T, 5, G, True, A=A)
    assert variant == f"mz_search_small{T}"
    assert np.all(walked >= 1)


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("explore", [True, False])
def test_exploration_on_off(monkeypatch, T, G, explore):
    variant, _, _, _ = _run(monkeypatch, T, 17, G, explore)
    assert variant == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_one_player(monkeypatch, T, G):
    variant, _, _, _ = _run(monkeypatch, T, 17, G, True, one_player=True)
    assert variant == f"mz_search_small{T}"


@pytest.mark.parametrize("T,G", TG)
def test_batch_norm(monkeypatch, T, G):
    assert _run_biased(monkeypatch, T, 17, G, True, bn=True) == f"mz_search_small{T}_bn"


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("one_player", [False, True])
def test_single_legal_chain(monkeypatch, T, G, one_player):
    """One legal action per position: simulation s ends at depth s + 1, so the last paths hold
    more than 16 levels; a single candidate never ties, so only simulation 0 walks."""
    variant, fast, walked, stats = _run(monkeypatch, T, 17, G, True, one_player=one_player, legal_mode="single")
    assert variant == f"mz_search_small{T}"
    assert stats[1] >= 16, f"max select depth {stats[1]}: the chain was not reached"
    assert np.all(walked == 1) and np.all(fast == 16)


@pytest.mark.parametrize("T", [1, 2, 4])
def test_tie_regime(monkeypatch, T):
    """An all-zero prediction net without noise (CPU-derived, tests/test_select_ballot_gpu.py:
    6,166 of the 6,400 simulations have a tied level): the selecting wave hands over to the
    walk, through the addresses formed in front of the loop, nearly every time."""
    variant, fast, walked, _ = _run_ballot(monkeypatch, T, "ttt", 50, 128, False, zero_pred=True)
    assert variant == f"mz_search_small{T}"
    assert np.all(fast + walked == 50)
    assert walked.sum() >= 6000


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("reward_act", ["tanh", "identity", "relu"])
def test_read_out_activations(monkeypatch, T, G, reward_act):
    """The value head's read-out is tanh; the reward head's the same, or identity, or relu: the
    kinds that wave 0's even and odd lanes hold.  With identity or relu a reward's magnitude is
    not bounded by 1, and relu's are never negative: checked on the oracle's tree, so the case
    is known to differ from the tanh one where it matters."""
    tree, _ = _run_nets(monkeypatch, T, 17, G, True, hp=(("reward_activation", reward_act),))
    R, N = tree["R"][:G], tree["N"][:G]
    assert np.any(R[N > 0] != 0)
    if reward_act == "relu":
        assert np.all(R[N > 0] >= 0)
    if reward_act == "tanh":
        assert np.all(np.abs(R[N > 0]) < 1)


@pytest.mark.parametrize("T,G", TG)
@pytest.mark.parametrize("spread", ["sub", "zero"])
def test_policy_logit_spread(monkeypatch, T, G, spread):
    """The expansion's first softmax on logits 96 and 120 apart (all nine actions legal, so the
    second softmax keeps every entry): priors that come from subnormal terms, and from the zeros
    of the lower guard.  That the terms are what the case is for is checked on
    the oracle's own det_expf of the bias differences."""
    from oracle import lib
    _run_nets(monkeypatch, T, 5, G, True, spread=spread, legal_mode="all")
    d = np.asarray(SPREAD[spread], np.float32)
    d = d - d.max()
    L = lib()
    e = np.array([L.ora_det_expf(float(x)) for x in d], np.float32)
    tiny, lo = np.float32(2.0 ** -126), np.float32(-103.97208404541016)
    assert np.any((e > 0) & (e < tiny)), "no subnormal term"
    if spread == "sub":
        assert -103.97 < d.min() < -88 and np.all(e > 0)
    else:
        assert np.any(d < lo) and np.any(e == 0), "no term below the lower guard"
        assert np.any(e == np.float32(2.0 ** -149)), "no term on the smallest subnormal, just above the guard"
