"""Reanalyse on the device replay shard (mz_reanalyse.hip, mz_replay_reanalyse;
ReplayBuffer.jl:8, 56-67): the values against mz_net_forward and the oracle,
flags and counter, targets against the host ReplayBuffer carrying the field,
eviction through both store paths, every learner path, current weights, and
the frame-stack refusal.  td_steps = 2 throughout: with TicTacToe's 5 most
positions never bootstrap."""
import dataclasses
import os

import numpy as np
import pytest

from test_reanalyse import rand_history

pytestmark = pytest.mark.gpu

LENS = [1, 10, 7, 5, 9, 6]          # 38 positions: partial tiles, a one-move game, a full-length game


def _setup(kind):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import connect4, tictactoe
    mod, env_kind = (connect4, abi.ENV_CONNECT4) if kind == "c4" else (tictactoe, abi.ENV_TICTACTOE)
    hyper = mod.resnet_hyper if kind.endswith("-rn") else mod.hyper
    if kind.endswith("-bn"):
        hyper = dataclasses.replace(hyper, use_batch_norm=True)
    return mod, env_kind, hyper


def _hand_built(kind="ttt", cap=8, lens=LENS, seed=5, **conf_kw):
    """An engine whose shard holds seeded random games saved from the host, and those games."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod, env_kind, hyper = _setup(kind)
    conf = dataclasses.replace(mod.conf, td_steps=2, replay_buffer_size=cap, batch_size=40, **conf_kw)
    nets = init_nets(conf, hyper, seed=seed + 100)
    eng = abi.Engine(conf, hyper, device=0, max_games=cap, rng_seed=seed)
    for n, w in enumerate(nets):
        eng.set_weights(n, w)
    eng.selfplay_init(env_kind, cap, cap)
    rng = np.random.default_rng(seed)
    osz, A = int(np.prod(conf.observation_shape)), len(conf.action_space)
    games = [rand_history(rng, T, osz, A) for T in lens]
    for h in games:
        eng.replay_save_game(h)
    return conf, hyper, nets, eng, games


def _stacked(conf, h):
    from muzero_jl_amd.selfplay import get_stacked_observations
    plane = conf.observation_shape[0] * conf.observation_shape[1]
    return np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                              conf.stacked_observations, plane)
                     for i in range(1, len(h.root_values) + 1)])


def _forward_values(eng, conf, h):
    return eng.forward(1, eng.forward(0, _stacked(conf, h)))[0][:, 0]


def _flags(eng):
    return [eng.replay_get_reanalysed(i) is not None for i in range(eng.replay_counts()[1])]


@pytest.mark.parametrize("kind", ["ttt", "ttt-bn", "c4", "ttt-rn"])
def test_values_match_net_forward(kind):
    conf, hyper, nets, eng, games = _hand_built(kind)
    assert _flags(eng) == [False] * len(games) and eng.replay_reanalysed_count() == 0
    eng.replay_reanalyse()
    assert eng.replay_reanalysed_count() == len(games)
    if kind == "ttt":
        from muzero_jl_amd.config import to_c_config, to_c_ffhp
        from oracle import Oracle
        ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=5)
        for n, w in enumerate(nets):
            ora.set_weights(n, w)
    for i, h in enumerate(games):
        got = eng.replay_get_reanalysed(i)
        assert got is not None and got.shape == (len(h.root_values),)
        assert np.array_equal(got, _forward_values(eng, conf, h)), (kind, i)
        if kind == "ttt":
            assert np.array_equal(got, ora.forward(1, ora.forward(0, _stacked(conf, h)))[0][:, 0]), i
    eng.close()


@pytest.mark.parametrize("kind,n,check", [
    ("ttt-rn", 416, [0, 408, 409, 410, 415]),       # 4160 ring rows: two staging chunks, game 409 straddles row 4096
    ("ttt", 1700, [0, 1023, 1637, 1638, 1699])])    # 1063 tiles on a 1024-workgroup grid: the grid-stride loop's second pass
def test_more_positions_than_one_round(kind, n, check):
    lens = [1 + (7 * i) % 10 for i in range(n)]
    conf, hyper, nets, eng, games = _hand_built(kind, cap=n, lens=lens)
    eng.replay_reanalyse()
    assert eng.replay_reanalysed_count() == n
    for i in check:
        got = eng.replay_get_reanalysed(i)
        assert got is not None and np.array_equal(got, _forward_values(eng, conf, games[i])), (kind, i)
    eng.close()


def test_subset_flags_and_clear():
    conf, hyper, nets, eng, games = _hand_built()
    eng.replay_reanalyse(first=1, count=3)
    assert _flags(eng) == [False, True, True, True, False, False]
    assert eng.replay_reanalysed_count() == 3
    eng.replay_reanalyse(first=len(games))                  # past the held range: nothing, no error
    eng.replay_reanalyse(first=len(games) + 40, count=2)    # past the capacity
    eng.replay_reanalyse(first=4, count=100)                # clipped to the held games
    assert _flags(eng) == [False, True, True, True, True, True]
    assert eng.replay_reanalysed_count() == 5
    eng.replay_clear_reanalysed()
    assert _flags(eng) == [False] * 6
    eng.close()


@pytest.mark.parametrize("per", [False, True])
def test_targets_match_host_buffer(per):
    from muzero_jl_amd.replay_buffer import ReplayBuffer
    kw = dict(PER=True, PER_alpha=1) if per else {}
    conf, hyper, nets, eng, games = _hand_built(**kw)
    rb = ReplayBuffer(conf, seed=5)
    for h in games:
        rb.save_game(h)                                     # (PER: initial priorities, the field still None)
    plain = {s: rb.get_batch(s) for s in (1, 2, 77)}
    prio0 = [eng.replay_get_priorities(i) for i in range(len(games))]
    eng.replay_reanalyse(first=1, count=3)
    for i, h in enumerate(games):
        v = eng.replay_get_reanalysed(i)
        assert (v is not None) == (1 <= i <= 3)
        h.reanalysed_predicted_root_values = None if v is None else [np.float32(x) for x in v]
    for step in (1, 2, 77):
        idx_h, bh = rb.get_batch(step)
        b, idx_d = eng.replay_sample(40, step, index=True)
        bd = eng.batch_to_host(b)
        assert [tuple(x) for x in idx_d] == [tuple(x) for x in idx_h]
        assert set(bd) == set(bh)
        for k in bh:
            assert np.array_equal(bd[k], bh[k]), (step, k)
        idx_p, bp = plain[step]
        assert idx_p == idx_h
        assert not np.array_equal(bh["target_values"], bp["target_values"])     # not vacuous
        for k in bh:                                        # only the values moved (PER: the weights did not)
            if k != "target_values":
                assert np.array_equal(bh[k], bp[k]), (step, k)
    for i in range(len(games)):                             # reanalysis leaves the priorities alone
        p, g = eng.replay_get_priorities(i)
        assert np.array_equal(p, prio0[i][0]) and g == prio0[i][1]
    eng.close()


def test_saved_game_evicts_the_reanalysed_one():
    from muzero_jl_amd.replay_buffer import ReplayBuffer
    conf, hyper, nets, eng, games = _hand_built(cap=4, lens=[6, 9, 4, 8])
    eng.replay_reanalyse()
    assert _flags(eng) == [True] * 4
    old = [eng.replay_get_reanalysed(i) for i in range(4)]
    fifth = rand_history(np.random.default_rng(77), 7)
    eng.replay_save_game(fifth)                             # takes game 1's slot
    assert _flags(eng) == [True, True, True, False]
    for i in range(3):
        assert np.array_equal(eng.replay_get_reanalysed(i), old[i + 1])
    rb = ReplayBuffer(conf, seed=5)
    for i, h in enumerate(games):
        h.reanalysed_predicted_root_values = [np.float32(x) for x in old[i]]
        rb.save_game(h)
    rb.save_game(fifth)                                     # its field is None: root_values
    hit = False
    for step in (1, 2, 3):
        idx_h, bh = rb.get_batch(step)
        b, idx_d = eng.replay_sample(40, step, index=True)
        bd = eng.batch_to_host(b)
        assert [tuple(x) for x in idx_d] == [tuple(x) for x in idx_h]
        for k in bh:
            assert np.array_equal(bd[k], bh[k]), (step, k)
        hit = hit or any(g == 5 and p <= 4 for g, p in idx_h)   # a bootstrapping position of the fifth game
    assert hit
    eng.close()


def _selfplay_engines(n, G=16, cap=64, moves=14, seed=5):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import tictactoe as mod
    from muzero_jl_amd.networks import init_nets
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=cap, td_steps=2)
    nets = init_nets(conf, mod.hyper, seed=seed + 100)
    out = []
    for _ in range(n):
        e = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=seed)
        for k, w in enumerate(nets):
            e.set_weights(k, w)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        for m in range(moves):
            e.selfplay_move(100 + m, game_offset=7)
        out.append(e)
    return conf, out


def test_selfplay_store_clears_the_flag():
    conf, (eng,) = _selfplay_engines(1, G=16, cap=16, moves=12)
    played0, held0 = int(eng.replay_counts()[0][0]), eng.replay_counts()[1]
    assert held0 > 0
    eng.replay_reanalyse()
    assert _flags(eng) == [True] * held0
    played, held = played0, held0
    for m in range(12, 40):                                 # until a new game took a reanalysed game's slot
        eng.selfplay_move(100 + m, game_offset=7)
        played, held = int(eng.replay_counts()[0][0]), eng.replay_counts()[1]
        if played > played0 and played > 16:
            break
    assert played > played0 and played > 16
    numbers = [played - held + 1 + i for i in range(held)]
    assert _flags(eng) == [g <= played0 for g in numbers]   # stored after the call: `nothing`
    assert any(g > played0 for g in numbers)
    eng.close()


def test_learner_paths_after_reanalyse():
    """e0 is never reanalysed; e1 and e2 are, at the same points.  In ref_semantics the update does not
    read the batch, so the three engines' weights stay equal and only the targets differ."""
    import torch
    from muzero_jl_amd.config import cos_schedule
    B = 32
    conf, (e0, e1, e2) = _selfplay_engines(3)
    grad = torch.empty(e1.grad_count(), dtype=torch.float32, device="cuda")
    ls = [torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(3)]
    lm = torch.zeros((3, 8), dtype=torch.float32, device="cuda")

    def losses(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 8)[:, :6].copy()

    e1.replay_reanalyse(); e2.replay_reanalyse()
    # train_dev == replay_sample + grad_dev (+ apply)
    s = 1
    e0.learner_train_dev(B, s, cos_schedule(s), ls[0].data_ptr())
    e1.learner_train_dev(B, s, cos_schedule(s), ls[1].data_ptr())
    b, _ = e2.replay_sample(B, s)
    e2.learner_grad_dev([b.observation, b.actions, b.target_values, b.target_rewards, b.target_policies,
                         b.gradient_scale], B, grad.data_ptr(), ls[2].data_ptr())
    e2.learner_apply_dev(grad.data_ptr(), 1.0, cos_schedule(s))
    for e in (e0, e1, e2):
        e.sync()
    assert e1.learner_variant().startswith("mz_learn_small")            # the fused one-launch path
    assert np.array_equal(losses(ls[1]), losses(ls[2]))
    assert not np.array_equal(losses(ls[1]), losses(ls[0]))
    # multi (L = 3) == three train_dev calls
    want, plain = [], []
    for i in range(3):
        s = 2 + i
        e0.learner_train_dev(B, s, cos_schedule(s), ls[0].data_ptr())
        e1.learner_train_dev(B, s, cos_schedule(s), ls[1].data_ptr())
        e0.sync(); e1.sync()
        plain.append(losses(ls[0])[0]); want.append(losses(ls[1])[0])
    e2.learner_train_multi_dev(B, 2, [cos_schedule(2 + i) for i in range(3)], lm.data_ptr())
    e2.sync()
    assert "multi" in e2.learner_variant()
    assert np.array_equal(losses(lm), np.array(want))
    assert not np.array_equal(np.array(want), np.array(plain))
    for n in range(3):
        assert np.array_equal(e1.get_weights(n), e2.get_weights(n))
        assert np.array_equal(e1.get_weights(n), e0.get_weights(n))
    # the batch train_dev(s) drew ahead for s + 1 is not reused after a reanalyse (e2: prefetch off)
    e1.replay_clear_reanalysed(); e2.replay_clear_reanalysed()
    s = 5
    e0.learner_train_dev(B, s, cos_schedule(s), ls[0].data_ptr())
    e0.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[0].data_ptr())
    e1.learner_train_dev(B, s, cos_schedule(s), ls[1].data_ptr())
    e1.replay_reanalyse()
    e1.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[1].data_ptr())
    os.environ["MZ_NO_BATCH_PREFETCH"] = "1"
    try:
        e2.learner_train_dev(B, s, cos_schedule(s), ls[2].data_ptr())
        e2.replay_reanalyse()
        e2.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[2].data_ptr())
    finally:
        del os.environ["MZ_NO_BATCH_PREFETCH"]
    for e in (e0, e1, e2):
        e.sync()
    assert np.array_equal(losses(ls[1]), losses(ls[2]))
    assert not np.array_equal(losses(ls[1]), losses(ls[0]))
    for e in (e0, e1, e2):
        e.close()


def test_reanalyse_uses_the_current_weights():
    import torch
    from muzero_jl_amd.config import cos_schedule
    conf, hyper, nets, eng, games = _hand_built()
    eng.replay_reanalyse()
    before = [eng.replay_get_reanalysed(i) for i in range(len(games))]
    eng.learner_train_multi_dev(32, 1, [cos_schedule(1 + i) for i in range(4)])
    eng.replay_reanalyse()
    for i, h in enumerate(games):
        got = eng.replay_get_reanalysed(i)
        assert np.array_equal(got, _forward_values(eng, conf, h)), i
        assert not np.array_equal(got, before[i])
    eng.close()


def test_frame_stack_env_is_refused():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth as at
    conf = dataclasses.replace(at.conf, num_iters=2)
    eng = abi.Engine(conf, at.resnet_hyper, device=0, max_games=4, rng_seed=1)
    eng.selfplay_init(abi.ENV_ATARI, 4, 8)
    counts0 = eng.replay_counts()
    with pytest.raises(abi.MzError, match="reanalyse: frame-stack env not built"):
        eng.replay_reanalyse()
    counts1 = eng.replay_counts()
    assert np.array_equal(counts0[0], counts1[0]) and counts0[1] == counts1[1]
    assert eng.replay_reanalysed_count() == 0
    eng.close()
