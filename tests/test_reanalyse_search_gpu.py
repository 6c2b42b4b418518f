"""Reanalyse by search on the device replay shard (mz_replay_reanalyse_search,
mz_reanalyse_sgather / _sscatter): every stored position against mcts_search
on the host-built inputs, flags and counter, targets against the host
ReplayBuffer carrying both fields, eviction through both store paths, every
learner path, the unsearchable position and the frame-stack refusal.  The
games come from device self-play (hand-built random boards have meaningless
legal masks); G = max_games = 16 rows per round, so games straddle rounds."""
import dataclasses
import os

import numpy as np
import pytest

from test_reanalyse_search import played_game

pytestmark = pytest.mark.gpu

G, STEP, OFF = 16, 900, 3


def _mod(kind):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import connect4, tictactoe
    mod, env_kind = (connect4, abi.ENV_CONNECT4) if kind == "c4" else (tictactoe, abi.ENV_TICTACTOE)
    return mod, env_kind, mod.resnet_hyper if kind.endswith("-rn") else mod.hyper


def _engines(n, kind="ttt", cap=64, min_games=20, seed=5, **conf_kw):
    """n twin engines whose shards hold the same >= min_games self-played games."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod, env_kind, hyper = _mod(kind)
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=cap, td_steps=2, batch_size=40, **conf_kw)
    nets = init_nets(conf, hyper, seed=seed + 100)
    out, moves = [], None
    for _ in range(n):
        e = abi.Engine(conf, hyper, device=0, max_games=G, rng_seed=seed)
        for k, w in enumerate(nets):
            e.set_weights(k, w)
        e.selfplay_init(env_kind, G, cap)
        m = 0
        while (m < moves) if moves is not None else (e.replay_counts()[1] < min_games and m < 400):
            for _ in range(2):
                e.selfplay_move(100 + m, game_offset=7)
                m += 1
        moves = m                                           # the twins play exactly as many moves
        out.append(e)
    assert out[0].replay_counts()[1] >= min_games
    return conf, out


def _stacked(conf, h):
    from muzero_jl_amd.selfplay import get_stacked_observations
    plane = conf.observation_shape[0] * conf.observation_shape[1]
    return np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                              conf.stacked_observations, plane)
                     for i in range(1, len(h.root_values) + 1)])


def _legal(conf, h):
    """The legal masks from the stored board bytes: plane 3 (TicTacToe), its top cell per column (Connect4)."""
    W, H, _ = conf.observation_shape
    b = np.stack(h.observation_history)[:, 2 * W * H:]
    return (b if (W, H) == (3, 3) else b[:, (W - 1) + W * np.arange(H)]).astype(np.uint8)


def _host_search(eng, conf, h, gi, exploration, skip=()):
    """mcts_search of every position of shard game gi as the reanalyse search keys it (max_games rows per call)."""
    Tm = conf.max_moves + 1
    x, legal, tp = _stacked(conf, h), _legal(conf, h), np.array(h.to_play_history, np.int32)
    keep = np.array([t not in skip for t in range(len(tp))])
    cvs, rvs = np.zeros((len(tp), legal.shape[1]), np.float32), np.zeros(len(tp), np.float32)
    # one call per run of consecutive rows (ids game_offset + row), at most max_games of them
    runs = [np.arange(c0, min(c0 + G, len(tp))) for c0 in range(0, len(tp), G)]
    if len(skip):
        runs = [np.array([t]) for t in range(len(tp)) if keep[t]]
    for r in runs:
        cv, rv, _ = eng.mcts_search(x[r], legal[r], tp[r], exploration=exploration, rng_step=STEP,
                                    game_offset=OFF + gi * Tm + int(r[0]), temperature=0.0)
        cvs[r], rvs[r] = cv, rv
    return cvs, rvs


def _flags(eng):
    n = eng.replay_counts()[1]
    return ([eng.replay_get_reanalysed(i) is not None for i in range(n)],
            [eng.replay_get_reanalysed_policies(i) is not None for i in range(n)])


def _train(eng, steps, B=32):
    from muzero_jl_amd.config import cos_schedule
    for s in steps:
        eng.learner_train_dev(B, s, cos_schedule(s))
    eng.sync()


@pytest.mark.parametrize("kind", ["ttt", "c4", "ttt-rn"])
def test_matches_mcts_search(kind):
    conf, (eng,) = _engines(1, kind)
    _train(eng, (1, 2, 3))                                  # the networks move on: the new searches differ
    held = eng.replay_counts()[1]
    games = [eng.replay_get_game(i) for i in range(held)]
    Tm = conf.max_moves + 1
    assert any((gi * Tm) // G != (gi * Tm + len(h.root_values) - 1) // G for gi, h in enumerate(games))
    for e in (False, True):
        eng.replay_reanalyse_search(exploration=e, rng_step=STEP, game_offset=OFF)
        moved_p = moved_v = False
        for gi, h in enumerate(games):
            cv, rv = _host_search(eng, conf, h, gi, e)
            got_p, got_v = eng.replay_get_reanalysed_policies(gi), eng.replay_get_reanalysed(gi)
            assert got_p is not None and got_p.shape == cv.shape
            assert np.array_equal(got_p, cv), (kind, e, gi)
            assert np.array_equal(got_v, rv), (kind, e, gi)
            moved_p = moved_p or not np.array_equal(got_p, np.array(h.child_visits))
            moved_v = moved_v or not np.array_equal(got_v, np.array(h.root_values, np.float32))
        assert moved_p and moved_v
    assert eng.replay_reanalysed_count() == 2 * held
    eng.close()


def _host_buffer(eng, conf, cap):
    """The host mirror of the shard as it stands: the held games in order, both reanalysed fields read back.
    Returns (buffer, game number of the oldest held game - 1)."""
    from muzero_jl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(dataclasses.replace(conf, replay_buffer_size=cap), seed=5)
    counts, held = eng.replay_counts()
    for i in range(held):
        h = eng.replay_get_game(i)
        rb.save_game(h)                                     # (PER: initial priorities, from root_values)
        v, p = eng.replay_get_reanalysed(i), eng.replay_get_reanalysed_policies(i)
        h.reanalysed_predicted_root_values = None if v is None else [np.float32(x) for x in v]
        h.reanalysed_child_visits = None if p is None else [r for r in p]
    return rb, int(counts[0]) - held


def _same_batches(eng, rb, shift, steps):
    for step in steps:
        idx_h, bh = rb.get_batch(step)
        b, idx_d = eng.replay_sample(40, step, index=True)
        bd = eng.batch_to_host(b)
        assert [(g - shift, p) for g, p in idx_d] == [tuple(x) for x in idx_h]
        assert set(bd) == set(bh)
        for k in bh:
            assert np.array_equal(bd[k], bh[k]), (step, k)


@pytest.mark.parametrize("per", [False, True])
def test_targets_match_host_buffer(per):
    kw = dict(PER=True, PER_alpha=1) if per else {}
    conf, (eng,) = _engines(1, **kw)
    held = eng.replay_counts()[1]
    rb0, shift = _host_buffer(eng, conf, 64)
    assert shift == 0
    plain = {s: rb0.get_batch(s) for s in (1, 2, 77)}
    prio0 = [eng.replay_get_priorities(i) for i in range(held)]
    eng.replay_reanalyse_search(first=2, count=14, exploration=True, rng_step=STEP, game_offset=OFF)
    assert _flags(eng) == ([2 <= i < 16 for i in range(held)],) * 2
    rb, _ = _host_buffer(eng, conf, 64)
    _same_batches(eng, rb, 0, (1, 2, 77))
    for step in (1, 2, 77):
        idx_h, bh = rb.get_batch(step)
        idx_p, bp = plain[step]
        assert idx_p == idx_h
        for k in bh:                                        # only the two targets moved (PER: the weights did not)
            assert np.array_equal(bh[k], bp[k]) == (k not in ("target_policies", "target_values")), (step, k)
    for i in range(held):                                   # reanalysis leaves the priorities alone
        p, g = eng.replay_get_priorities(i)
        assert np.array_equal(p, prio0[i][0]) and g == prio0[i][1]
    eng.close()


def test_flags():
    conf, (eng,) = _engines(1)
    held = eng.replay_counts()[1]
    none = [False] * held
    assert _flags(eng) == (none, none) and eng.replay_reanalysed_count() == 0
    eng.replay_reanalyse_search(first=1, count=3, rng_step=STEP, game_offset=OFF)
    sub = [1 <= i <= 3 for i in range(held)]
    assert _flags(eng) == (sub, sub) and eng.replay_reanalysed_count() == 3
    eng.replay_reanalyse_search(first=held)                 # past the held range: nothing, no error
    eng.replay_reanalyse_search(first=64 + 40, count=2)     # past the capacity
    assert _flags(eng) == (sub, sub) and eng.replay_reanalysed_count() == 3
    eng.replay_reanalyse_search(first=held - 2, count=100, rng_step=STEP, game_offset=OFF)   # clipped to the held games
    sub = [1 <= i <= 3 or i >= held - 2 for i in range(held)]
    assert _flags(eng) == (sub, sub) and eng.replay_reanalysed_count() == 5
    pol = [eng.replay_get_reanalysed_policies(i) for i in range(held)]
    val = [eng.replay_get_reanalysed(i) for i in range(held)]
    eng.replay_reanalyse()                                  # value-only: keeps the policies, overwrites the values
    assert _flags(eng) == ([True] * held, sub) and eng.replay_reanalysed_count() == 5 + held
    for i in range(held):
        p = eng.replay_get_reanalysed_policies(i)
        assert (p is None and pol[i] is None) or np.array_equal(p, pol[i])
        want = eng.forward(1, eng.forward(0, _stacked(conf, eng.replay_get_game(i))))[0][:, 0]
        assert np.array_equal(eng.replay_get_reanalysed(i), want)
        assert val[i] is None or not np.array_equal(val[i], want)
    eng.replay_clear_reanalysed()
    assert _flags(eng) == (none, none)
    eng.close()


@pytest.mark.parametrize("path", ["selfplay", "save_game"])
def test_store_clears_both(path):
    conf, (eng,) = _engines(1, cap=16, min_games=16)
    played0 = int(eng.replay_counts()[0][0])
    eng.replay_reanalyse_search(exploration=True, rng_step=STEP, game_offset=OFF)
    assert _flags(eng) == ([True] * 16,) * 2
    if path == "save_game":
        eng.replay_save_game(eng.replay_get_game(3))
    else:
        m = 1000
        while int(eng.replay_counts()[0][0]) == played0 and m < 1040:
            eng.selfplay_move(m, game_offset=7)
            m += 1
    played = int(eng.replay_counts()[0][0])
    assert played0 < played < played0 + 16
    old = [played - 16 + 1 + i <= played0 for i in range(16)]         # stored before the call: still set
    assert _flags(eng) == (old, old) and not all(old) and any(old)
    rb, shift = _host_buffer(eng, conf, 16)
    assert shift == played - 16
    _same_batches(eng, rb, shift, (1, 2, 3))
    new = {i + 1 for i in range(16) if not old[i]}
    assert any(g in new for s in (1, 2, 3) for g, p in rb.get_batch(s)[0])   # the new game was drawn
    eng.close()


def test_learner_paths():
    """e0 is never reanalysed; e1 and e2 are, at the same points.  In ref_semantics the update does not
    read the batch, so the three engines' weights stay equal and only the targets differ."""
    import torch
    from muzero_jl_amd.config import cos_schedule
    B = 32
    conf, (e0, e1, e2) = _engines(3)
    grad = torch.empty(e1.grad_count(), dtype=torch.float32, device="cuda")
    ls = [torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(3)]
    lm = torch.zeros((3, 8), dtype=torch.float32, device="cuda")

    def losses(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 8)[:, :6].copy()

    def rean(e):
        e.replay_reanalyse_search(exploration=True, rng_step=STEP, game_offset=OFF)

    rean(e1); rean(e2)
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
    rean(e1)
    e1.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[1].data_ptr())
    os.environ["MZ_NO_BATCH_PREFETCH"] = "1"
    try:
        e2.learner_train_dev(B, s, cos_schedule(s), ls[2].data_ptr())
        rean(e2)
        e2.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[2].data_ptr())
    finally:
        del os.environ["MZ_NO_BATCH_PREFETCH"]
    for e in (e0, e1, e2):
        e.sync()
    assert np.array_equal(losses(ls[1]), losses(ls[2]))
    assert not np.array_equal(losses(ls[1]), losses(ls[0]))
    for e in (e0, e1, e2):
        e.close()


def test_empty_mask_position_keeps_its_originals():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import tictactoe as mod
    from muzero_jl_amd.networks import init_nets
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=16, td_steps=2)
    eng = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=5)
    for k, w in enumerate(init_nets(conf, mod.hyper, seed=105)):
        eng.set_weights(k, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, G, 16)
    games = [played_game([5, 1, 9, 3, 2, 8, 7]), played_game([1, 5, 2, 9, 4, 3, 6, 7])]
    bad = 4                                                 # player 1 to move, and the board gives it cells 0, 1, 2
    b = np.zeros(27, np.float32)
    b[[0, 1, 2]] = 1
    b[9 + np.array([4, 8])] = 1
    b[18 + np.array([3, 5, 6, 7])] = 1
    assert games[1].to_play_history[bad] == 1
    games[1].observation_history[bad] = b
    for h in games:
        eng.replay_save_game(h)
    eng.replay_reanalyse_search(exploration=True, rng_step=STEP, game_offset=OFF)
    assert eng.replay_reanalysed_count() == 2
    for gi, h in enumerate(games):
        skip = (bad,) if gi == 1 else ()
        cv, rv = _host_search(eng, conf, h, gi, True, skip=skip)
        for t in skip:
            cv[t], rv[t] = h.child_visits[t], np.float32(h.root_values[t])
        assert np.array_equal(eng.replay_get_reanalysed_policies(gi), cv), gi
        assert np.array_equal(eng.replay_get_reanalysed(gi), rv), gi
        assert not np.array_equal(cv[0], h.child_visits[0])
    eng.close()


def test_frame_stack_env_is_refused():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth as at
    conf = dataclasses.replace(at.conf, num_iters=2)
    eng = abi.Engine(conf, at.resnet_hyper, device=0, max_games=4, rng_seed=1)
    eng.selfplay_init(abi.ENV_ATARI, 4, 8)
    counts0 = eng.replay_counts()
    with pytest.raises(abi.MzError, match="reanalyse: frame-stack env not built"):
        eng.replay_reanalyse_search()
    counts1 = eng.replay_counts()
    assert np.array_equal(counts0[0], counts1[0]) and counts0[1] == counts1[1]
    assert eng.replay_reanalysed_count() == 0
    assert _flags(eng) == ([False] * counts0[1],) * 2
    eng.close()
