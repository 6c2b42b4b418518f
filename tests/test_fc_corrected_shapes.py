"""The conditions on the inputs of the FC corrected learner's shape matrix (tests/fc_corrected_shapes.py),
checked without a GPU: the torch autograd reference in float64 and once more in float32.

The GPU test (test_fc_corrected_shapes_gpu.py) bounds the kernels' error per parameter tensor by
max(1e-5, 4 · e32_t), e32_t being the float32 reference's error against float64 on the tensor's own
scale.  That bound is only a bar if the inputs are well conditioned: here every case must keep e32_t
within E32_MAX = 2.5e-5 on every tensor (no bound above 1e-4), give every tensor of an applied layer a
nonzero gradient (a plain 3x scale of init_nets fails this: it saturates the value and reward heads),
and give the layers the unroll does not apply an exactly zero one.  A case that fails is mended by
another weight regime or seed in the table, never by a wider bound.  Both long unrolls (ttt_k60,
ttt_k66) meet the floor at the table's seed, so both are compared against torch on the GPU as well.
"""
import numpy as np
import pytest

import fc_corrected_shapes as fs


def test_table_is_complete():
    assert list(fs.cases()) == fs.IDS and set(fs.PLAN) == set(fs.IDS)
    assert set(fs.STEP_IDS) <= set(fs.IDS)
    for cid, c in fs.cases().items():
        assert 1 <= c.B <= 33, cid
        b, w = fs.batch(cid)
        assert b["observation"].shape == (c.B, fs.features(c.conf))
        assert (w is not None) == c.per


@pytest.mark.parametrize("cid", fs.IDS)
def test_case_meets_the_conditions(cid):
    c = fs.cases()[cid]
    r64, r32 = fs.reference(cid), fs.reference(cid, True)
    rows = fs.tensor_errors(c, r32["data_grads"], r64["data_grads"], r32["data_grads"])
    worst = max(rows, key=lambda r: r["e32"])
    print(f"{cid}: largest e32 {worst['e32']:.3g} at (net, layer, tensor) {worst['key']}, scale {worst['scale']:.3g}")
    unused = 0
    for r in rows:
        if r["applied"]:
            assert r["scale"] > 0.0, f"{cid} {r['key']}: an applied layer's tensor has no gradient"
            assert r["e32"] <= fs.E32_MAX, f"{cid} {r['key']}: float32 floor {r['e32']:.3g}"
            assert r["bound"] <= 1e-4
        else:
            unused += 1
            assert r["scale"] == 0.0 and r["e32"] == 0.0, f"{cid} {r['key']}: an unused layer has a gradient"
    # the layers the case is there to leave unused are unused
    want_unused = {"ttt_k1": True, "c4_k2_noir": True}.get(cid, False)
    assert (unused > 0) == want_unused, (cid, unused)
    # the two ways of writing the data term agree in float64 (the GPU test's per-net check uses the first)
    for n in range(3):
        d = r64["grads"][n] - 2.0 * np.asarray(fs.nets(cid)[n], np.float64)
        np.testing.assert_allclose(d, r64["data_grads"][n], rtol=0, atol=1e-12 * max(1.0, np.abs(d).max()))
    for k in ("value", "policy") + (("reward",) if c.ir else ()):
        assert r64[k] > 0.0 and abs(r32[k] - r64[k]) <= 1e-5 * r64[k], (cid, k)


def test_plain_scale_would_hide_the_heads(ttt):
    """Why the table does not use test_corrected_learner_gpu's 3x nets: the tanh of their value head and
    reward head saturates, and both layers of either head get no gradient (below 1e-12 of their net's
    largest entry in float64), so those cases carry no value or reward loss backwards."""
    import dataclasses
    from muzero_jl_amd.networks import init_nets
    from test_corrected_learner_gpu import _batch
    from torch_learner_ref import corrected_loss_and_grads
    B, K = 20, 3
    conf = dataclasses.replace(ttt.conf, batch_size=B, num_unroll_steps=K, intermediate_rewards=True)
    nets = [n * np.float32(3.0) for n in init_nets(conf, ttt.hyper, seed=B + K)]
    rng = np.random.default_rng(B)
    batch = _batch(B, K, 9, 63, rng)
    ref = corrected_loss_and_grads(conf, ttt.hyper, nets, batch, None)
    c = fs.Case(conf, ttt.hyper, B, False, ("scale", B + K, 3.0), B)
    rows = {r["key"]: r for r in fs.tensor_errors(c, ref["data_grads"], ref["data_grads"])}
    net_scale = [np.abs(g).max() for g in ref["data_grads"]]
    heads = [k for k, (n, _, ch, *_r) in zip(rows, fs.tensors(conf, ttt.hyper)) if (n, ch) in ((1, 1), (2, 2))]
    assert heads
    for k in heads:
        assert rows[k]["scale"] <= 1e-12 * net_scale[k[0]], (k, rows[k]["scale"])
