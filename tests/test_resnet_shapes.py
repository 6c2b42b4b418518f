"""CPU half of the ResNet shape matrix (tests/resnet_shapes.py): for every case
the oracle's parameter counts equal Python's, its forward of all three nets
agrees with the independent torch fp32 forward at the 1e-5 tolerance of
test_resnet_oracle, and its search equals the independent Python mirror bit for
bit.  The GPU half (test_resnet_shapes_gpu.py) then pins the kernels to this
oracle.  k53 / k35 are the non-square kernels: the residual blocks of the
representation use the whole (kw, kh) tuple (resnet_block(ksize, …),
src/Learning.jl:148-171)."""
import numpy as np
import pytest

import resnet_shapes as rs
from test_resnet_oracle import TOL, _torch_forward


@pytest.mark.parametrize("cid", rs.IDS)
def test_shape_param_counts(cid):
    from muzero_jl_amd.networks import param_count
    conf, hyper = rs.cases()[cid]
    o = rs.oracle(cid)
    assert [param_count(conf, hyper, n) for n in range(3)] == [o.param_count(n) for n in range(3)]
    assert [w.size for w in rs.lively_nets(cid)] == [o.param_count(n) for n in range(3)]
    W, H, _ = conf.observation_shape
    assert o.H == W * H * hyper.num_filters and o.plane == W * H and o.A == len(conf.action_space)


@pytest.mark.parametrize("net", [0, 1, 2])
@pytest.mark.parametrize("cid", rs.IDS)
def test_shape_oracle_matches_torch(cid, net):
    conf, hyper = rs.cases()[cid]
    o = rs.oracle(cid)
    x = rs.net_input(conf, hyper, net, 5, 10 * rs.IDS.index(cid) + net)
    ref = _torch_forward(conf, hyper, net, rs.lively_nets(cid)[net].copy(), x)
    got = o.forward(net, x)
    if net == 0:
        np.testing.assert_allclose(got, ref, **TOL)
    else:
        np.testing.assert_allclose(got[0], ref[0], **TOL)
        np.testing.assert_allclose(got[1], ref[1], **TOL)


@pytest.mark.parametrize("cid", rs.IDS)
def test_shape_oracle_search_matches_mirror(cid):
    from mirror_ref import Mirror
    conf, _ = rs.cases()[cid]
    o = rs.oracle(cid, seed=3)
    obs, legal, tp = rs.search_inputs(conf, rs.SEARCH_G, 17)
    assert legal.any(1).all() and legal[1].sum() == 1
    if len(conf.action_space) > 16:
        assert not legal[2, :16].any()
    cv, rv, act, _, _ = o.mcts_search(obs, legal, tp, exploration=True, rng_step=2, game_offset=5, dump=True)
    cv2, rv2, act2, _ = Mirror(o, conf).search(obs, legal, tp, True, 5, 2)
    assert np.array_equal(cv, cv2) and np.array_equal(rv, rv2) and np.array_equal(act, act2)
    assert np.all(legal[np.arange(rs.SEARCH_G), act - 1])
