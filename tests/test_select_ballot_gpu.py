"""The small kernels' ballot select (csrc/mz_tree_device.h select_path_ballot,
csrc/mz_small.hip) on the GPU: every case forces MZ_SEARCH_KERNEL=small and
compares trees, child visits, root values and actions bit for bit with the C
oracle; the per-game select counters (mz_debug_select_stats) show which form
found each simulation's leaf.

* fast regime: the bench's nets and positions, where only simulation 0 (N(root)
  = 0, every score 0) and one further simulation in 128 games have a tied level;
* tie regime: an all-zero prediction net without exploration noise, so the
  priors are uniform and nearly every simulation meets a tie below a valid
  prefix (the same-wave hand-over to the serial walk);
* boundaries: S + 1 = 64 fills lane 63 and mask bit 63, S + 1 = 65 no longer
  fits one wave (the walk only), G = 5 leaves inactive games in the last
  workgroup;
* a one-legal-action chain to depth 40 (path levels past the 16 the serial
  walk keeps in registers are written by the ballot pass);
* Connect4 (A = 7).
Reference: src/SelfPlay.jl:254-283.
"""
import dataclasses
import functools

import numpy as np
import pytest

from test_bench_sizes_gpu import _oracle_search_threads
from test_gpu_parity import _compare_trees

pytestmark = pytest.mark.gpu


def _setup(game, S, G, zero_pred=False, players=None, single_legal=False):
    from muzero_jl_amd.games import connect4 as c4
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    from muzero_jl_amd.selfplay import random_positions
    mod = c4 if game == "c4" else ttt
    conf = dataclasses.replace(mod.conf, num_iters=S)
    if players is not None:
        conf = dataclasses.replace(conf, players=players)
    nets = init_nets(conf, mod.hyper, seed=1234)
    if zero_pred:
        nets[1][:] = 0
    env = c4.BatchedConnect4 if game == "c4" else ttt.BatchedTicTacToe
    obs, legal, tp = random_positions(env, G, seed=100, max_plies=16 if game == "c4" else 6)
    if single_legal:
        first = np.argmax(legal, axis=1)
        legal[:] = False
        legal[np.arange(G), first] = True
    if players is not None:
        tp = np.ones(G, np.int32)
    return conf, mod.hyper, nets, obs, legal, tp


@functools.lru_cache(maxsize=None)
def _reference(game, S, G, explore, zero_pred=False, one_player=False, single_legal=False):
    """The oracle's search of one set-up, computed once and shared by the T cases."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    conf, hyper, nets, obs, legal, tp = _setup(game, S, G, zero_pred, [1] if one_player else None, single_legal)
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=1)
    for n, w in enumerate(nets):
        ora.set_weights(n, w)
    return _oracle_search_threads(ora, obs, legal, tp, chunks=min(16, G), exploration=explore, rng_step=3,
                                  game_offset=0, temperature=1.0)


def _run(monkeypatch, T, game, S, G, explore, zero_pred=False, one_player=False, single_legal=False):
    """One GPU search against the oracle; returns (variant, fast, walked, oracle stats)."""
    from muzero_jl_amd.abi import Engine
    monkeypatch.setenv("MZ_SEARCH_KERNEL", "small")
    monkeypatch.setenv("MZ_SMALL_T", str(T))
    conf, hyper, nets, obs, legal, tp = _setup(game, S, G, zero_pred, [1] if one_player else None, single_legal)
    eng = Engine(conf, hyper, device=0, max_games=G, rng_seed=1)
    for n, w in enumerate(nets):
        eng.set_weights(n, w)
    eng.debug_enable(1)
    cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=3, game_offset=0, temperature=1.0)
    tree_g = eng.debug_tree(G)
    fast, walked = eng.debug_select_stats(G)
    variant = eng.search_variant()
    eng.close()
    cv2, rv2, act2, tree_o, stats = _reference(game, S, G, explore, zero_pred, one_player, single_legal)
    print(f"{variant} T={T} {game} S={S} G={G}: fast {fast.sum()} walked {walked.sum()} "
          f"(per game walked min {walked.min()} max {walked.max()})")
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2), "child visits differ"
    assert np.array_equal(rv, rv2), "root values differ"
    assert np.array_equal(act, act2), "actions differ"
    return variant, fast, walked, stats


@pytest.mark.parametrize("T", [1, 2, 4])
def test_fast_regime(monkeypatch, T):
    """CPU-derived: 129 of the 6,400 simulations have a tied level, 128 of them simulation 0."""
    variant, fast, walked, _ = _run(monkeypatch, T, "ttt", 50, 128, True)
    assert variant == f"mz_search_small{T}"
    assert np.all(fast + walked == 50)
    assert np.all(walked >= 1)
    assert np.all(walked <= 5)
    assert walked.sum() <= 160


@pytest.mark.parametrize("T", [2, 4])
def test_tie_regime(monkeypatch, T):
    """CPU-derived: 6,166 of the 6,400 simulations have a tied level, mostly below a valid prefix."""
    variant, fast, walked, _ = _run(monkeypatch, T, "ttt", 50, 128, False, zero_pred=True)
    assert variant == f"mz_search_small{T}"
    assert np.all(fast + walked == 50)
    assert walked.sum() >= 6000


@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("S", [1, 2, 63, 64])
def test_boundaries(monkeypatch, T, S):
    """G = 5: the last workgroup has inactive games.  S = 63: node 63 sits in
    lane 63 / mask bit 63.  S = 64: 65 nodes no longer fit one wave."""
    variant, fast, walked, _ = _run(monkeypatch, T, "ttt", S, 5, True)
    if S <= 63:
        assert variant == f"mz_search_small{T}"       # (LDS-eligible at both T: the small kernel ran)
    if variant.startswith("mz_search_small"):
        assert np.all(fast + walked == S)
        if S == 64:
            assert np.all(fast == 0)
        else:
            assert np.all(walked >= 1)                  # simulation 0: the root's entry is not computed yet


def test_deep_chain(monkeypatch):
    """One legal action per game: every node has one child, simulation s ends at
    depth s + 1.  A single candidate never ties, so only simulation 0 (the
    root's entry not computed yet) walks: the ballot pass writes every level,
    those past the 16 register-held ones included."""
    variant, fast, walked, stats = _run(monkeypatch, 2, "ttt", 40, 8, True, one_player=True, single_legal=True)
    assert variant == "mz_search_small2"
    assert stats[1] >= 39, f"max select depth {stats[1]}: the chain was not reached"
    assert np.all(fast + walked == 40)
    assert np.all(walked == 1)


def test_connect4(monkeypatch):
    """Connect4 FC (A = 7) against the oracle.  Its 126-feature input exceeds
    the small kernels' stage schedule, so the engine runs the
    tile-16 kernel even when the small one is asked for; the counters are then
    0.  Should the schedule ever take it, the counters are checked as above."""
    variant, fast, walked, _ = _run(monkeypatch, 2, "c4", 50, 6, True)
    if variant.startswith("mz_search_small"):
        assert np.all(fast + walked == 50)
        assert np.all(walked >= 1)
    else:
        assert np.all(fast == 0) and np.all(walked == 0)
