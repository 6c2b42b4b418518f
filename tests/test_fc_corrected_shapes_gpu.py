"""The FC corrected learner (MZ_LEARN_CORRECTED: mz_bp_tile_lv / mz_bp_tile_lv_nobn, mz_bp_tile,
mz_bp_dw, mz_bp_fold, then mz_adam_kernel) on the shape matrix of tests/fc_corrected_shapes.py, off
the TicTacToe preset every other test of it runs.  Per case, one engine:

  * the plan's read-out (mz_debug_bp_plan) lies in the regime the case is there for: arena fallback
    of the forward tensors, of the input gradients, flagged levels in mid-schedule, no cache at all;
  * (a) the data gradient against torch autograd in float64, per net at the project's 1e-5 and per
    parameter tensor (W, b, β, γ of every Dense) on the tensor's own scale at max(1e-5, 4 · e32_t),
    e32_t the float32 reference's own error there (the conditions: test_fc_corrected_shapes.py); a
    layer the unroll does not apply gets exact zeros; losses and read-outs at the project's tolerances.
    Both long unrolls (ttt_k60, ttt_k66) meet the float32 floor and are in (a);
  * (b) the level kernel against the sequential one (MZ_BP_SEQ=1: no cache, a full barrier per
    application) and against its own second launch, bit for bit: a hand-off through the arena that a
    barrier did not order shows as a difference.

On c4_k5 and w20, (c) three corrected steps: mz_learner_step = grad_dev + apply_dev(1.0) bit for bit,
and grad_dev + apply_dev(0.5) against the host mirror (learning.dp_gradient + the oracle's
ora_adam_grad) in θ after every step, in ADAM's m, v, βp through a checkpoint and in mz_net_forward
(the scatter into the weight images).  (d): the first K the plan refuses leaves a working engine.
"""
import ctypes
import os

import numpy as np
import pytest

import fc_corrected_shapes as fs

pytestmark = pytest.mark.gpu

KEYS = ("observation", "actions", "target_values", "target_rewards", "target_policies", "gradient_scale")


def _engine(c, nets, corrected=True):
    from muzero_jl_amd import abi
    eng = abi.Engine(c.conf, c.hyper, device=0, max_games=8, rng_seed=1)
    for n, w in enumerate(nets):
        eng.set_weights(n, w)
    if corrected:
        eng.learner_set_mode(abi.LEARN_CORRECTED)
    return eng


def _dev_batch(batch, wts):
    import torch
    dev = [torch.tensor(batch[k], dtype=torch.float32).cuda() for k in KEYS]      # (copies: the table's are read-only)
    dev.append(torch.tensor(wts, dtype=torch.float32).cuda() if wts is not None else None)
    return dev


def _grad(eng, dev, B):
    """(data term, six losses, read-outs) of one mz_learner_grad_dev."""
    import torch
    grad = torch.zeros(eng.grad_count(), dtype=torch.float32, device="cuda")
    losses = torch.zeros(8, dtype=torch.float32, device="cuda")
    eng.learner_grad_dev([t.data_ptr() if t is not None else None for t in dev], B, grad.data_ptr(),
                         losses.data_ptr())
    eng.sync()
    return grad.cpu().numpy(), losses.cpu().numpy()[:6], [x.copy() for x in eng.debug_unroll(B)]


_RUNS = {}


def _run(cid):
    """_run_once's result, or its exception again: a case that failed on the device is not launched twice."""
    if cid not in _RUNS:
        try:
            _RUNS[cid] = _run_once(cid)
        except Exception as e:
            _RUNS[cid] = e
    if isinstance(_RUNS[cid], Exception):
        raise _RUNS[cid]
    return _RUNS[cid]


def _run_once(cid):
    """The case on one engine: the plan, the level kernel twice, the sequential kernel once."""
    c = fs.cases()[cid]
    eng = _engine(c, fs.nets(cid))
    try:
        plan = eng.debug_bp_plan()
        dev = _dev_batch(*fs.batch(cid))
        had = os.environ.pop("MZ_BP_SEQ", None)
        try:
            lv = _grad(eng, dev, c.B)
            again = _grad(eng, dev, c.B)
            os.environ["MZ_BP_SEQ"] = "1"
            seq = _grad(eng, dev, c.B)
        finally:
            os.environ.pop("MZ_BP_SEQ", None)
            if had is not None:
                os.environ["MZ_BP_SEQ"] = had
    finally:
        eng.close()
    return dict(plan=plan, lv=lv, again=again, seq=seq)


def _split(c, g, nets):
    out, off = [], 0
    for w in nets:
        out.append(g[off:off + w.size])
        off += w.size
    assert off == g.size
    return out


@pytest.mark.parametrize("cid", fs.IDS)
def test_plan_is_in_the_regime(cid):
    plan = _run(cid)["plan"]
    print(f"{cid}: {plan}")
    fs.check_plan(cid, plan)
    assert plan["lds_bytes"] <= 160 * 1024 and plan["nslot"] * plan["slot_floats"] * 4 < plan["lds_bytes"]


def test_preset_reaches_none_of_the_regimes(ttt):
    """Today's blind spot, written down: at the preset every hand-off is in LDS and the only flagged levels
    are the last forward level and the observation gradient's.  A planner change that moves this is noticed."""
    c = fs.Case(ttt.conf, ttt.hyper, 32, False, ("biased", 1, 7), 0)
    assert ttt.conf.num_unroll_steps == 5
    from muzero_jl_amd.networks import init_nets
    eng = _engine(c, init_nets(ttt.conf, ttt.hyper, seed=1))
    try:
        plan = eng.debug_bp_plan()
    finally:
        eng.close()
    assert {k: plan[k] for k in fs.PRESET_PLAN} == fs.PRESET_PLAN, plan
    assert plan["nslot"] > 8


def test_plan_readout_refuses_resnet(ttt):
    from muzero_jl_amd import abi
    eng = abi.Engine(ttt.conf, ttt.resnet_hyper, device=0, max_games=8, rng_seed=1)
    try:
        with pytest.raises(abi.MzError, match="ResNet"):
            eng.debug_bp_plan()
    finally:
        eng.close()


def test_wide_width_is_refused(ttt):
    """The issue's width for `wide`: mz_engine_create refuses it cleanly (the search kernel's LDS budget),
    so the table takes the nearest accepted shape in the regime."""
    import dataclasses
    from muzero_jl_amd import abi
    with pytest.raises(abi.MzError, match="LDS budget exceeded"):
        abi.Engine(ttt.conf, dataclasses.replace(ttt.hyper, width_hidden=fs.WIDE_REFUSED), device=0, max_games=8)


@pytest.mark.parametrize("cid", fs.IDS)
def test_gradient_matches_torch_per_tensor(cid):
    c = fs.cases()[cid]
    nets = fs.nets(cid)
    g, lo, (pv, pp, pr) = _run(cid)["lv"]
    ref, r32 = fs.reference(cid), fs.reference(cid, True)
    got = _split(c, g, nets)
    # per net, as test_corrected_learner_gpu: relative to the net's largest entry
    for n in range(3):
        rn = ref["grads"][n] - 2.0 * np.asarray(nets[n], np.float64)    # grad_dev holds the data term
        scale = np.abs(rn).max()
        if n == 2 and c.K == 0:
            assert scale == 0.0 and np.abs(got[n]).max() == 0.0
            continue
        assert scale > 1e-4, f"net {n}: no data gradient reached it"
        err = np.abs(got[n].astype(np.float64) - rn).max() / scale
        assert err < 1e-5, f"{cid} net {n}: data gradient rel. error {err:.3g}"
    # per parameter tensor, on its own scale
    rows = fs.tensor_errors(c, got, ref["data_grads"], r32["data_grads"])
    worst = max((r for r in rows if r["applied"]), key=lambda r: r["err"] / r["bound"])
    print(f"{cid}: largest err/bound {worst['err'] / worst['bound']:.3g} at (net, layer, tensor) {worst['key']}: "
          f"err {worst['err']:.3g}, e32 {worst['e32']:.3g}, bound {worst['bound']:.3g}; "
          f"largest err {max(r['err'] for r in rows):.3g}")
    for r in rows:
        if r["applied"]:
            assert r["scale"] > 0.0, r["key"]
            assert r["err"] <= r["bound"], f"{cid} {r['key']}: {r['err']:.3g} of the tensor's scale > {r['bound']:.3g}"
        else:
            assert r["scale"] == 0.0 and r["zero"], f"{cid} {r['key']}: an unused layer's data term is not exactly 0"
    np.testing.assert_allclose([lo[0], lo[1], lo[2]], [ref["value"], ref["reward"], ref["policy"]],
                               rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(lo[3:6], ref["l2"], rtol=1e-5)
    np.testing.assert_allclose(pv, ref["values"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pp, ref["policies"], rtol=1e-5, atol=1e-6)
    if c.ir:
        np.testing.assert_allclose(pr, ref["rewards"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cid", fs.IDS)
def test_level_schedule_equals_sequential_and_itself(cid):
    r = _run(cid)
    for name in ("again", "seq"):
        (g0, l0, u0), (g1, l1, u1) = r["lv"], r[name]
        what = "a second launch of the level kernel" if name == "again" else "the sequential kernel"
        assert np.array_equal(g0, g1), f"{cid}: gradients differ from {what} in {np.count_nonzero(g0 != g1)} entries"
        assert np.array_equal(l0, l1), f"{cid}: losses differ from {what}"
        for a, b in zip(u0, u1):
            assert np.array_equal(a, b), f"{cid}: read-outs differ from {what}"
    assert np.all(np.isfinite(r["lv"][0])) and np.any(r["lv"][0] != 0)


@pytest.mark.parametrize("cid", fs.STEP_IDS)
def test_steps_match_apply_and_the_host_mirror(cid, tmp_path):
    import torch
    from muzero_jl_amd import checkpoint as ck
    from muzero_jl_amd.config import cos_schedule, to_c_config, to_c_ffhp
    from muzero_jl_amd.learning import dp_gradient
    from oracle import Oracle, lib
    c = fs.cases()[cid]
    nets = fs.nets(cid)
    e1, e2, e3 = (_engine(c, nets) for _ in range(3))
    L = lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    th = np.concatenate(nets).astype(np.float32)
    m, v, bp = np.zeros_like(th), np.zeros_like(th), np.array([0.9, 0.999])
    rng = np.random.default_rng(c.seed + 100)
    try:
        grad = torch.zeros(e2.grad_count(), dtype=torch.float32, device="cuda")
        losses = torch.zeros(8, dtype=torch.float32, device="cuda")
        for t in range(1, 4):
            batch, wts = fs.make_batch(c, rng)
            eta = cos_schedule(t)
            l1 = e1.learner_step(dict(batch, weights=wts) if wts is not None else batch, eta)
            dev = _dev_batch(batch, wts)
            ptrs = [d.data_ptr() if d is not None else None for d in dev]
            e2.learner_grad_dev(ptrs, c.B, grad.data_ptr(), losses.data_ptr())
            e2.learner_apply_dev(grad.data_ptr(), 1.0, eta)
            e2.sync()
            assert np.array_equal(l1, losses.cpu().numpy()[:6]), t
            for n in range(3):
                assert np.array_equal(e1.get_weights(n), e2.get_weights(n)), (t, n)
            # half the data term, as a rank of two would apply it, against the host's ADAM
            e3.learner_grad_dev(ptrs, c.B, grad.data_ptr(), losses.data_ptr())
            e3.learner_apply_dev(grad.data_ptr(), 0.5, eta)
            e3.sync()
            data = grad.cpu().numpy()
            assert np.any(data != 0)
            g = dp_gradient(data, th, 2, lambda x: None)
            L.ora_adam_grad(vp(th), vp(m), vp(v), vp(g), th.size, vp(bp), eta)
            bp = bp * np.array([0.9, 0.999])
            assert np.array_equal(np.concatenate([e3.get_weights(n) for n in range(3)]), th), f"step {t}: θ differs"
        p = str(tmp_path / "ck.safetensors")
        e3.checkpoint_save(p, 3)
        tensors, _ = ck.read(p)
        assert np.array_equal(tensors["adam.m"], m) and np.array_equal(tensors["adam.v"], v)
        assert np.array_equal(tensors["adam.beta_pow"], bp)
        assert np.any(m != 0) and np.all(v >= 0) and np.any(v > 0)
        # the weight images ADAM scattered into: mz_net_forward against the oracle holding the host's θ
        ora = Oracle(to_c_config(c.conf), to_c_ffhp(c.hyper), seed=1)
        off = 0
        for n, w in enumerate(nets):
            ora.set_weights(n, th[off:off + w.size])
            off += w.size
        for n, x in enumerate(fs.net_rows(c, 5, c.seed + 200)):
            ge, oo = e3.forward(n, x), ora.forward(n, x)
            for a, b in zip(ge if isinstance(ge, tuple) else (ge,), oo if isinstance(oo, tuple) else (oo,)):
                assert np.array_equal(a, b), f"net {n}: mz_net_forward differs from the oracle on the host's θ"
    finally:
        e1.close(); e2.close(); e3.close()


def test_refused_plan_leaves_a_working_engine(ttt):
    """The first K whose level schedule exceeds the LDS: the read-out and mz_learner_grad_dev refuse with the
    LDS message before any launch (the output buffers keep their fill), and the engine goes on working."""
    import dataclasses
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.config import cos_schedule
    from muzero_jl_amd.networks import init_nets
    B = 4

    def case(K):
        conf = dataclasses.replace(ttt.conf, batch_size=B, num_unroll_steps=K, intermediate_rewards=True)
        return fs.Case(conf, ttt.hyper, B, False, ("biased", 3, 7), 3)

    last = case(fs.REFUSED_K - 1)
    eng = _engine(last, init_nets(last.conf, last.hyper, seed=3))
    try:
        assert eng.debug_bp_plan()["nslot"] == 0        # the longest accepted unroll: REFUSED_K is the first refused
    finally:
        eng.close()
    c = case(fs.REFUSED_K)
    nets = init_nets(c.conf, c.hyper, seed=3)
    batch, _ = fs.make_batch(c, np.random.default_rng(3))
    eng, fresh = _engine(c, nets), _engine(c, nets, corrected=False)
    try:
        with pytest.raises(abi.MzError, match="LDS"):
            eng.debug_bp_plan()
        dev = _dev_batch(batch, None)
        grad = torch.full((eng.grad_count(),), 7.0, dtype=torch.float32, device="cuda")
        losses = torch.full((8,), 7.0, dtype=torch.float32, device="cuda")
        with pytest.raises(abi.MzError, match="LDS"):
            eng.learner_grad_dev([d.data_ptr() if d is not None else None for d in dev], B, grad.data_ptr(),
                                 losses.data_ptr())
        eng.sync()
        assert bool((grad == 7.0).all()) and bool((losses == 7.0).all()), "a refused call wrote its outputs"
        for n in range(3):
            assert np.array_equal(eng.get_weights(n), nets[n])
        eng.learner_set_mode(abi.LEARN_REF_SEMANTICS)
        la, lb = eng.learner_step(batch, cos_schedule(1)), fresh.learner_step(batch, cos_schedule(1))
        assert np.all(np.isfinite(la)) and np.array_equal(la, lb)
        for n in range(3):
            assert np.array_equal(eng.get_weights(n), fresh.get_weights(n))
            assert not np.array_equal(eng.get_weights(n), nets[n])
    finally:
        eng.close(); fresh.close()
