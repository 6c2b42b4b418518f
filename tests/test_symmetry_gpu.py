"""Board-symmetry augmentation in the device sampler (mz_replay_set_symmetry, mz_batch_symmetry)
against the host mirror (ReplayBuffer.get_batch(step, symmetry=True), apply_symmetry), bit for bit, and through
every learner path that draws its batch on the device."""
import dataclasses

import numpy as np
import pytest

from test_selfplay_gpu import _device_pair, _engines, _env, _per_engines, _play_both

pytestmark = pytest.mark.gpu

MOVES = {"ttt": 14, "c4": 30}
KEYS = ("observation", "actions", "target_values", "target_rewards", "target_policies", "gradient_scale")


def _ptrs(b):
    return [getattr(b, k) for k in KEYS] + ([b.weights] if b.weights else [])


def _mirror(conf, finished, B):
    from muzero_jl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(dataclasses.replace(conf, batch_size=B), seed=5)
    for h in finished:
        rb.save_game(h)
    return rb


def _same_batch(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        assert np.array_equal(got[k], want[k]), (tag, k)


def _weights(e):
    return [e.get_weights(n) for n in range(3)]


def _same_weights(a, b, tag=None):
    for n in range(3):
        assert np.array_equal(a.get_weights(n), b.get_weights(n)), (tag, n)


# ---- 1. the sampler against the mirror
@pytest.mark.parametrize("kind,B,per", [("ttt", 32, False), ("ttt", 40, False), ("c4", 24, False), ("ttt", 40, True)])
def test_symmetric_sample_matches_mirror(kind, B, per):
    from muzero_jl_amd.games import symmetry
    if per:
        conf, sp, eh, ed = _per_engines(16, 30, cap=24)
    else:
        conf, sp, eh, ed = _play_both(kind, 16, MOVES[kind], cap=64)
    rb = _mirror(conf, sp.finished, B)
    t, on = ed.replay_symmetry_get()
    want_t = symmetry.for_conf(conf)
    assert not on and np.array_equal(t.cell, want_t.cell) and np.array_equal(t.action, want_t.action)
    ed.replay_set_symmetry(True)
    assert ed.replay_symmetry_get()[1]
    for step in (1, 2, 3, 77):
        idx_h, bh = rb.get_batch(step, symmetry=True)
        assert set(rb.last_symmetry_ids.tolist()) == set(range(t.n)), step      # every element is exercised
        b, idx_d = ed.replay_sample(B, step, index=True)
        assert [tuple(x) for x in idx_d] == [tuple(x) for x in idx_h]
        _same_batch(ed.batch_to_host(b), bh, step)
        assert not np.array_equal(bh["observation"], rb.get_batch(step)[1]["observation"])
    eh.close(); ed.close()


# ---- 2. mz_batch_symmetry
@pytest.mark.parametrize("kind,B", [("ttt", 32), ("c4", 24), ("ttt", 1), ("ttt", 5)])
def test_batch_symmetry(kind, B):
    from muzero_jl_amd.games import symmetry
    from muzero_jl_amd.replay_buffer import apply_symmetry, symmetry_ids
    conf, sp, eh, ed = _play_both(kind, 16, MOVES[kind], cap=64)
    rb = _mirror(conf, sp.finished, B)
    t = symmetry.for_conf(conf)
    step = 3
    _, plain_h = rb.get_batch(step)
    _, sym_h = rb.get_batch(step, symmetry=True)
    ids = symmetry_ids(5, step, B, t.n)
    plain_d, _ = ed.replay_sample(B, step)                            # the setting is off
    _same_batch(ed.batch_to_host(plain_d), plain_h, "plain")
    _same_batch(ed.batch_to_host(ed.batch_symmetry(plain_d, ids)), sym_h, "plain + transform")
    ed.replay_set_symmetry(True)                                      # it works with the setting on, too
    _same_batch(ed.batch_to_host(ed.batch_symmetry(plain_h, ids)), sym_h, "host batch, setting on")
    ed.replay_set_symmetry(False)
    row = {k: np.repeat(v[:1], t.n + 2, axis=0) for k, v in plain_h.items()}   # one row under every id, then 2 bad ids
    rid = np.array(list(range(t.n)) + [t.n, -1], np.int32)
    got = ed.batch_to_host(ed.batch_symmetry(row, rid))
    _same_batch(got, apply_symmetry(row, rid, t), "one row, each id")
    for j in (0, t.n, t.n + 1):                                       # id 0 and the out-of-range ids: the input
        for k in row:
            assert np.array_equal(got[k][j], row[k][j]), (j, k)
    inv = np.array([symmetry.inverse(t, s) for s in ids], np.int32)
    back = ed.batch_to_host(ed.batch_symmetry(ed.batch_symmetry(plain_d, ids), inv))
    _same_batch(back, plain_h, "s, then its inverse")
    eh.close(); ed.close()


# ---- 3. the learner paths with the setting on
def _separate_step(e, B, step, grad, losses, eta):
    b, _ = e.replay_sample(B, step)
    e.learner_grad_dev(_ptrs(b), B, grad.data_ptr(), losses.data_ptr())
    if b.weights:
        e.replay_update_priorities()
    e.learner_apply_dev(grad.data_ptr(), 1.0, eta)


@pytest.mark.parametrize("kind,resnet,B,per", [("ttt", False, 32, False), ("ttt", False, 40, False),
                                               ("ttt", False, 1100, False), ("ttt", True, 32, False),
                                               ("c4", False, 24, False), ("ttt", False, 32, True)])
def test_fused_learner_matches_separate_calls_symmetric(kind, resnet, B, per):
    """ref_semantics: mz_learner_train_dev and mz_learner_grad_sampled_dev + apply == mz_replay_sample +
    mz_learner_grad_dev + apply with the setting on; the losses read the batch, and differ from the plain ones."""
    import torch
    from muzero_jl_amd.config import cos_schedule
    if per:
        _, _, e1, e2 = _per_engines(16, 20, cap=64, host=False)
    else:
        e1, e2 = _device_pair(kind, 16, MOVES[kind], cap=64, resnet=resnet)
    grad = torch.empty(e1.grad_count(), dtype=torch.float32, device="cuda")
    l0, l1, l2 = (torch.empty(8, dtype=torch.float32, device="cuda") for _ in range(3))
    b, _ = e1.replay_sample(B, 1)                                     # the plain step-1 losses (no update)
    e1.learner_grad_dev(_ptrs(b), B, grad.data_ptr(), l0.data_ptr())
    e1.sync()
    plain1 = l0.cpu().numpy()[:3].copy()
    e1.replay_set_symmetry(True); e2.replay_set_symmetry(True)
    for step in (1, 2, 3, 4):
        eta = cos_schedule(step)
        _separate_step(e1, B, step, grad, l1, eta)
        if step % 2:
            e2.learner_train_dev(B, step, eta, l2.data_ptr())
        else:
            g2 = torch.empty_like(grad)
            e2.learner_grad_sampled_dev(B, step, g2.data_ptr(), l2.data_ptr())
            e2.learner_apply_dev(g2.data_ptr(), 1.0, eta)
        e1.sync(); e2.sync()
        assert np.array_equal(l1.cpu().numpy()[:6], l2.cpu().numpy()[:6]), step
        if step == 1:
            assert not np.array_equal(l1.cpu().numpy()[:3], plain1)
        _same_weights(e1, e2, step)
    e1.close(); e2.close()


@pytest.mark.parametrize("kind,B", [("ttt", 32), ("c4", 24)])
def test_corrected_learner_on_device_batch_matches_host_mirror(kind, B):
    """MZ_LEARN_CORRECTED: the weights read the batch.  mz_learner_train_dev with the setting on == mz_learner_step
    fed the host mirror's symmetric batch on a second engine, losses and weights, three steps."""
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.config import cos_schedule
    conf, sp, eh, ed = _play_both(kind, 16, MOVES[kind], cap=64)
    rb = _mirror(conf, sp.finished, B)
    for e in (eh, ed):
        e.learner_set_mode(abi.LEARN_CORRECTED)
    ed.replay_set_symmetry(True)
    losses = torch.empty(8, dtype=torch.float32, device="cuda")
    plain = None
    for step in (1, 2, 3):
        _, bh = rb.get_batch(step, symmetry=True)
        lh = eh.learner_step(bh, cos_schedule(step))
        ed.learner_train_dev(B, step, cos_schedule(step), losses.data_ptr())
        ed.sync()
        assert np.array_equal(losses.cpu().numpy()[:6], lh), step
        _same_weights(ed, eh, step)
        if step == 1:
            plain = rb.get_batch(1)[1]
    assert not np.array_equal(plain["observation"], rb.get_batch(1, symmetry=True)[1]["observation"])
    eh.close(); ed.close()


def test_multi_step_and_dp_match_single_calls_symmetric():
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.config import cos_schedule
    L, B = 4, 32
    e1, e2 = _device_pair("ttt", 16, 14, cap=64)
    e3, _e = _device_pair("ttt", 16, 14, cap=64)
    _e.close()
    e3.dp_init(0, 1, abi.Engine.dp_unique_id())
    for e in (e1, e2, e3):
        e.replay_set_symmetry(True)
    l1 = torch.empty(8, dtype=torch.float32, device="cuda")
    l3 = torch.empty(8, dtype=torch.float32, device="cuda")
    lm = torch.empty((L, 8), dtype=torch.float32, device="cuda")
    e2.learner_train_multi_dev(B, 1, [cos_schedule(1 + i) for i in range(L)], lm.data_ptr())
    e2.sync()
    for i in range(L):
        e1.learner_train_dev(B, 1 + i, cos_schedule(1 + i), l1.data_ptr())
        e3.learner_train_dp(B, 1 + i, cos_schedule(1 + i), l3.data_ptr())
        e1.sync(); e3.sync()
        assert np.array_equal(l1.cpu().numpy()[:6], lm.cpu().numpy()[i, :6]), i
        assert np.array_equal(l1.cpu().numpy()[:6], l3.cpu().numpy()[:6]), i
    _same_weights(e1, e2)
    _same_weights(e1, e3)
    for e in (e1, e2, e3):
        e.close()


def _train_engine(sym, kind="ttt"):
    mod, _, env_kind = _env(kind)
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=64, checkpoint_interval=4)
    e = _engines(mod, conf, mod.hyper, 16)
    e[1].close()
    e = e[0]
    e.selfplay_init(env_kind, 16, 64)
    if sym:
        e.replay_set_symmetry(True)
    e.train_init(32)
    return e


def _sets(e):
    from muzero_jl_amd import abi
    return [np.concatenate([e.train_weights(w, n) for n in range(3)])
            for w in (abi.TRAIN_LEARNER, abi.TRAIN_ACTOR, abi.TRAIN_QUEUED)]


def test_train_run_matches_split_loop_symmetric():
    """mz_train_run == mz_train_move + mz_train_learn with the setting on; the job's losses are not the off job's."""
    import torch
    moves = 16
    out = []
    for sym, split in ((True, False), (True, True), (False, False)):
        e = _train_engine(sym)
        losses = torch.zeros(8, dtype=torch.float32, device="cuda")
        if split:
            tot = 0
            for m in range(moves):
                st = e.train_learn(e.train_move(50 + m, game_offset=7), losses_ptr=losses.data_ptr())
                tot += st[3]
            st = st[:3] + (tot,)
        else:
            st = e.train_run(moves, move0=50, game_offset=7, losses_ptr=losses.data_ptr())
        e.sync()
        out.append((st, _sets(e), losses.cpu().numpy()[:6].copy()))
        e.close()
    assert out[0][0] == out[1][0] == out[2][0] and out[0][0][3] > 0
    assert np.array_equal(out[0][2], out[1][2])
    for a, b in zip(out[0][1], out[1][1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out[0][2][:3], out[2][2][:3])


# ---- 4. the prefetch
@pytest.mark.parametrize("kind,B", [("ttt", 32), ("c4", 24)])
def test_toggle_invalidates_prefetched_batch(kind, B, monkeypatch):
    import torch
    from muzero_jl_amd.config import cos_schedule
    e1, e2 = _device_pair(kind, 16, MOVES[kind], cap=64)
    e3, _e = _device_pair(kind, 16, MOVES[kind], cap=64)
    _e.close()
    plan = [("t", 1), ("t", 2), ("on", 0), ("t", 3), ("t", 4), ("off", 0), ("t", 5), ("t", 6)]
    rows = {}
    for name, eng, pf, never in (("nopf", e1, False, False), ("pf", e2, True, False), ("never", e3, True, True)):
        if pf:
            monkeypatch.delenv("MZ_NO_BATCH_PREFETCH", raising=False)
        else:
            monkeypatch.setenv("MZ_NO_BATCH_PREFETCH", "1")
        lo = torch.empty(8, dtype=torch.float32, device="cuda")
        rows[name] = []
        for op, step in plan:
            if op == "t":
                eng.learner_train_dev(B, step, cos_schedule(step), lo.data_ptr())
                eng.sync()
                rows[name].append(lo.cpu().numpy()[:6].copy())
            elif not never:
                eng.replay_set_symmetry(op == "on")
    monkeypatch.delenv("MZ_NO_BATCH_PREFETCH", raising=False)
    assert np.array_equal(np.array(rows["nopf"]), np.array(rows["pf"]))
    _same_weights(e1, e2)
    for i in (0, 1, 4, 5):                                            # off: the plain job's losses
        assert np.array_equal(rows["pf"][i], rows["never"][i]), i
    assert not np.array_equal(rows["pf"][2][:3], rows["never"][2][:3])      # step 3 was drawn symmetric
    for e in (e1, e2, e3):
        e.close()


# ---- 5. off is the parent
def test_off_after_on_is_plain():
    import torch
    from muzero_jl_amd.config import cos_schedule
    e1, e2 = _device_pair("ttt", 16, 14, cap=64)
    e1.replay_set_symmetry(True)
    e1.replay_sample(40, 9)
    e1.replay_set_symmetry(False)
    l1 = torch.empty(8, dtype=torch.float32, device="cuda")
    l2 = torch.empty(8, dtype=torch.float32, device="cuda")
    for step in (1, 2):
        b1, i1 = e1.replay_sample(40, step, index=True)
        b2, i2 = e2.replay_sample(40, step, index=True)
        assert np.array_equal(i1, i2)
        _same_batch(e1.batch_to_host(b1), e2.batch_to_host(b2), step)
        e1.learner_train_dev(32, step, cos_schedule(step), l1.data_ptr())
        e2.learner_train_dev(32, step, cos_schedule(step), l2.data_ptr())
        e1.sync(); e2.sync()
        assert np.array_equal(l1.cpu().numpy()[:6], l2.cpu().numpy()[:6])
    _same_weights(e1, e2)
    e1.close(); e2.close()


# ---- 6. snapshots: the setting is the loading host's
def test_snapshot_does_not_carry_the_setting(tmp_path):
    import torch
    from muzero_jl_amd import abi
    cut, moves = 8, 16

    def leg(e, losses, first):
        n, m0 = (cut, 50) if first else (moves - cut, 50 + cut)
        st = e.train_run(n, move0=m0, game_offset=7, losses_ptr=losses.data_ptr())
        e.sync()
        return st, losses.cpu().numpy()[:6].copy(), _sets(e)

    def loader():
        mod, _, _ = _env("ttt")
        conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=64, checkpoint_interval=4)
        return abi.Engine(conf, mod.hyper, device=0, max_games=16, rng_seed=5)

    losses = torch.zeros(8, dtype=torch.float32, device="cuda")
    uncut = _train_engine(True)
    leg(uncut, losses, True)
    want_on = leg(uncut, losses, False)
    snap = str(tmp_path / "cut.safetensors")
    first = _train_engine(True)
    leg(first, losses, True)
    first.snapshot_save(snap, 7)
    # the off job from the same cut: the first leg's games and weights, then plain sampling
    first.replay_set_symmetry(False)
    want_off = leg(first, losses, False)
    first.close(); uncut.close()

    again = loader()
    again.snapshot_load(snap)
    assert not again.replay_symmetry_get()[1]
    again.replay_set_symmetry(True)
    got_on = leg(again, losses, False)
    kept = loader()
    kept.snapshot_load(snap)
    got_off = leg(kept, losses, False)
    for got, want in ((got_on, want_on), (got_off, want_off)):
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
        for a, b in zip(got[2], want[2]):
            assert np.array_equal(a, b)
    assert not np.array_equal(want_on[1][:3], want_off[1][:3])
    # a handle that has the setting keeps it through a load
    again.snapshot_load(snap)
    assert again.replay_symmetry_get()[1]
    again.close(); kept.close()


# ---- 7. refusals
def test_symmetry_refusals(ttt):
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.abi import MzError
    from muzero_jl_amd.games import atari_synth
    from muzero_jl_amd.networks import init_nets
    e = abi.Engine(ttt.conf, ttt.hyper, device=0, max_games=8, rng_seed=1)
    with pytest.raises(MzError, match="mz_selfplay_init first"):
        e.replay_set_symmetry(True)
    with pytest.raises(MzError, match="mz_selfplay_init first"):
        e.replay_symmetry_get()
    e.selfplay_init(abi.ENV_TICTACTOE, 8, 8)
    with pytest.raises(MzError, match="on must be 0"):
        e.replay_set_symmetry(2)
    assert not e.replay_symmetry_get()[1]
    e.replay_set_symmetry(True)
    e.selfplay_init(abi.ENV_TICTACTOE, 8, 16)                         # the same env: kept
    assert e.replay_symmetry_get()[1]
    for m in range(12):
        e.selfplay_move(m)
    b, _ = e.replay_sample(4, 1)
    ids = torch.zeros(4, dtype=torch.int32, device="cuda")
    for name in abi.MzBatch._fields_[1:7]:
        out = e.batch_symmetry(b, np.zeros(4, np.int32))
        setattr(out, name[0], getattr(b, name[0]))                     # one aliased array
        with pytest.raises(MzError, match="overlap"):
            e._check(e.lib.mz_batch_symmetry(e.h, b, ids.data_ptr(), out, None), "mz_batch_symmetry")
    e.replay_sample(4, 2)                                             # still usable
    e.close()
    conf = dataclasses.replace(atari_synth.conf, num_iters=2, max_moves=6, batch_size=4)
    a = abi.Engine(conf, atari_synth.resnet_hyper, device=0, max_games=4, rng_seed=5)
    for n, w in enumerate(init_nets(conf, atari_synth.resnet_hyper, seed=17)):
        a.set_weights(n, w)
    a.selfplay_init(abi.ENV_ATARI, 4, 8)
    with pytest.raises(MzError, match="Atari-like env"):
        a.replay_set_symmetry(True)
    with pytest.raises(MzError, match="Atari-like env"):
        a.replay_symmetry_get()
    a.selfplay_move(0)
    a.close()
