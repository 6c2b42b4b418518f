"""CPU half of the downsampler shape matrix (tests/downsample_shapes.py): for
every case the oracle's parameter counts equal Python's, the stride-2 boards are
the table's, the checkpoint table lists the downsampler's arrays first with
shapes (kw, kh, cin, cout), the oracle's representation agrees with the
independent torch fp32 forward at the 1e-5 tolerance of test_resnet_oracle, and
its search equals the independent Python mirror bit for bit.  The GPU half
(test_downsample_shapes_gpu.py) then pins the kernels of csrc/mz_downsample.hip
to this oracle.

Reference: src/Learning.jl:148-191; src/SelfPlay.jl:225-283."""
import numpy as np
import pytest

import downsample_shapes as dsh
from test_resnet_oracle import TOL


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_param_counts(cid):
    from muzero_jl_amd.networks import param_count, resnet_board
    conf, hyper = dsh.cases()[cid]
    o = dsh.oracle(cid)
    assert [param_count(conf, hyper, n) for n in range(3)] == [o.param_count(n) for n in range(3)]
    assert [w.size for w in dsh.lively_nets(cid)] == [o.param_count(n) for n in range(3)]
    W, H = resnet_board(conf, hyper)
    assert (W, H) == dsh.CHAIN[cid][-1] and (W, H) in ((3, 3), (5, 5))
    assert o.H == W * H * 16 and o.plane == W * H and o.A == len(conf.action_space)
    c, s = conf.observation_shape[2], conf.stacked_observations
    assert c * (s + 1) + s == dsh.CHANNELS[cid]


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_boards(cid):
    from muzero_jl_amd.networks import resnet_specs
    conf, hyper = dsh.cases()[cid]
    ops = resnet_specs(conf, hyper, 0)
    s2 = [o for o in ops if o["kind"] != "dense" and o["stride"] == 2]
    assert [o["kind"] for o in s2] == ["conv", "conv", "pool", "pool"]
    assert [(o["W"], o["H"]) for o in s2] == dsh.CHAIN[cid]
    assert [(o["Wi"], o["Hi"]) for o in s2] == [tuple(conf.observation_shape[:2])] + dsh.CHAIN[cid][:-1]
    C = dsh.CHANNELS[cid]
    assert [(o["cin"], o["cout"]) for o in s2] == [(C, C), (C, 2 * C), (2 * C, 2 * C), (2 * C, 2 * C)]


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_param_table(cid):
    """Flux.params order: the first strided conv's W, b; two blocks of (W, b, β, γ) x 2; the second strided conv."""
    from muzero_jl_amd.checkpoint import param_table
    conf, hyper = dsh.cases()[cid]
    kw, kh = hyper.conv_kernel_size
    C = dsh.CHANNELS[cid]
    t = param_table(conf, hyper, 0)
    assert t[0][1:] == ((kw, kh, C, C), 0) and t[1][1:] == ((C,), kw * kh * C * C)
    for i in range(4):                                          # the four block convs at C channels
        assert [e[1] for e in t[2 + 4 * i: 6 + 4 * i]] == [(kw, kh, C, C), (C,), (C,), (C,)]
    first = kw * kh * C * C + C + 4 * (kw * kh * C * C + 3 * C)
    assert t[18][1:] == ((kw, kh, C, 2 * C), first) and t[19][1] == (2 * C,)
    assert t[20][1] == (kw, kh, 2 * C, 2 * C)
    # 12 block convs at 2C channels, then the tail's first conv reads 2C channels into 16 filters
    tail = 20 + 4 * 12
    assert t[tail][1] == (kw, kh, 2 * C, 16)
    from test_corrected_resnet_gpu import _ds_param_count
    assert t[tail][2] == _ds_param_count(conf, hyper)


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_oracle_matches_torch(cid):
    x, want, ref = dsh.forward_reference(cid, 3)
    assert want.shape == ref.shape == (3, dsh.oracle(cid).H)
    err = np.abs(want - ref).max()
    print(f"{cid}: oracle vs torch, largest absolute difference {err:.3g}")
    np.testing.assert_allclose(want, ref, **TOL)


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_oracle_search_matches_mirror(cid):
    from mirror_ref import Mirror
    conf, _ = dsh.cases()[cid]
    G = 4
    o = dsh.oracle(cid, seed=3)
    obs, legal, tp = dsh.search_inputs(conf, G, 17)
    assert legal.any(1).all() and legal[1].sum() == 1
    if len(conf.action_space) > 16:
        assert not legal[2, :16].any()
    cv, rv, act, _, _ = o.mcts_search(obs, legal, tp, exploration=True, rng_step=2, game_offset=5, dump=True)
    cv2, rv2, act2, _ = Mirror(o, conf).search(obs, legal, tp, True, 5, 2)
    assert np.array_equal(cv, cv2) and np.array_equal(rv, rv2) and np.array_equal(act, act2)
    assert np.all(legal[np.arange(G), act - 1])
