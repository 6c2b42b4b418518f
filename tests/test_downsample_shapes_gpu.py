"""GPU half of the downsampler shape matrix (tests/downsample_shapes.py): the
kernels of csrc/mz_downsample.hip at shapes off the 84x84x4 preset.  For every
case, on one engine: the staged flag the engine chose (mz_downsample_staged)
against the table; the representation at n = 5 and n = 1 against the CPU oracle
bit for bit (np.array_equal: the kernels run the oracle's f32 operations in the
oracle's order) and against torch fp32 at 1e-5; a 6-simulation search of 5 games
with and without exploration (trees, child visits, root values, actions; masks
with a single legal action and, for A > 16, legal actions above 16 only); three
ref_semantics learner steps (unroll read-outs, losses, θ of all three nets, the
downsampler's slice included) and a forward on the updated parameters.  Then
mz_dsbp_fwd / mz_dsbp_bwd / mz_dsbp_dw against torch autograd with the
comparison and thresholds of test_corrected_resnet_gpu, corrected steps on a
staged and an unstaged case, and the two shapes the engine refuses at create.

This runs ds_conv_generic (its LDS tap tables, the quarter bounds for K % 16 != 0,
the (kw, kh) flip, layer 0 from HBM), the unstaged layout, the staged layout with
generic convs, the fast forms with their right and bottom taps off the board, and
stacking in front of the downsampler, none of which the preset reaches.

Reference: src/Learning.jl:148-191, :327-404; src/SelfPlay.jl:225-283."""
import dataclasses

import numpy as np
import pytest

import downsample_shapes as dsh
from test_gpu_parity import _compare_trees

pytestmark = pytest.mark.gpu


def _new_engine(cid, max_games=8, seed=7, scale=None):
    from muzero_jl_amd import abi
    conf, hyper = dsh.cases()[cid]
    eng = abi.Engine(conf, hyper, device=0, max_games=max_games, rng_seed=seed)
    for n, w in enumerate(dsh.lively_nets(cid)):
        eng.set_weights(n, w if scale is None else w * np.float32(scale))
    return eng


@pytest.fixture(scope="module", params=dsh.IDS)
def case_eng(request):
    """One engine per case, holding lively_nets whenever a test starts."""
    eng = _new_engine(request.param)
    yield request.param, eng
    eng.close()


def test_ds_shape_staged_flag(case_eng):
    cid, eng = case_eng
    assert eng.downsample_staged() == dsh.STAGED[cid]


def test_ds_shape_staged_flag_preset():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth as at, tictactoe as ttt
    eng = abi.Engine(at.conf, at.resnet_hyper, device=0, max_games=2, rng_seed=1)
    try:
        assert eng.downsample_staged() == dsh.STAGED_PRESET
    finally:
        eng.close()
    eng = abi.Engine(ttt.conf, ttt.resnet_hyper, device=0, max_games=2, rng_seed=1)
    try:
        assert eng.downsample_staged() == -1                  # a ResNet without the downsampler
    finally:
        eng.close()


def test_ds_shape_forward_bitexact(case_eng):
    from test_resnet_oracle import TOL
    cid, eng = case_eng
    for n in (5, 1):
        x, want, ref = dsh.forward_reference(cid, n)
        got = eng.forward(0, x)
        print(f"{cid} n = {n}: {np.count_nonzero(got != want)} of {want.size} differ from the oracle, "
              f"largest |got - torch| {np.abs(got - ref).max():.3g}")
        assert np.array_equal(got, want), (cid, n)
        np.testing.assert_allclose(got, ref, **TOL)


@pytest.mark.parametrize("explore,temp", [(True, 1.0), (False, 0.0)])
def test_ds_shape_search_bitexact(case_eng, explore, temp):
    cid, eng = case_eng
    conf, _ = dsh.cases()[cid]
    G = dsh.SEARCH_G
    o = dsh.oracle(cid)
    obs, legal, tp = dsh.search_inputs(conf, G, 40 + dsh.IDS.index(cid))
    assert legal[1].sum() == 1 and (len(conf.action_space) <= 16 or not legal[2, :16].any())
    eng.debug_enable(1)
    cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=21, game_offset=11, temperature=temp)
    tree_g = eng.debug_tree(G)
    cv2, rv2, act2, tree_o, _ = o.mcts_search(obs, legal, tp, exploration=explore, rng_step=21, game_offset=11,
                                              temperature=temp, dump=True)
    assert np.all(legal[np.arange(G), act - 1]), "an illegal action was chosen"
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2) and np.array_equal(rv, rv2) and np.array_equal(act, act2)


def test_ds_shape_learner_steps(case_eng):
    """Three ref_semantics steps as test_atari_learner_steps, then net 0 forward on the updated parameters: the
    downsampler kernel reads the parameters the learner wrote."""
    from muzero_jl_amd.config import cos_schedule
    cid, eng = case_eng
    conf, _ = dsh.cases()[cid]
    B = conf.batch_size
    o = dsh.oracle(cid)
    try:
        st = o.learner_state()
        rng = np.random.default_rng(dsh.IDS.index(cid))
        for t in range(1, 4):
            batch = dsh.random_batch(conf, rng, 7 * t + dsh.IDS.index(cid))
            eta = cos_schedule(t)
            want = o.unroll(batch["observation"], batch["actions"])
            lg = eng.learner_step(batch, eta)
            lo = o.learner_step(st, batch, eta)
            for g, w in zip(eng.debug_unroll(B), want):
                assert np.array_equal(g, w), f"step {t} unroll differs"
            assert np.array_equal(lg, lo), f"step {t} losses {lg} != oracle {lo}"
            for n in range(3):
                assert np.array_equal(eng.get_weights(n), o.params[n]), f"step {t} net {n} params differ"
        nd = _ds_params(cid)
        assert not np.array_equal(o.params[0][:nd], dsh.lively_nets(cid)[0][:nd]), "the downsampler did not move"
        x, before, _ = dsh.forward_reference(cid, 5)
        want = o.forward(0, x)
        assert not np.array_equal(want, before)
        assert np.array_equal(eng.forward(0, x), want)
    finally:
        for n, w in enumerate(dsh.lively_nets(cid)):
            eng.set_weights(n, w)


def _ds_params(cid):
    from test_corrected_resnet_gpu import _ds_param_count
    return _ds_param_count(*dsh.cases()[cid])


@pytest.mark.parametrize("cid", dsh.IDS)
def test_ds_shape_corrected_gradient_matches_torch(cid):
    """mz_dsbp_fwd / mz_dsbp_bwd / mz_dsbp_dw through every case's taps, strides and channel pairs, B = 3, K = 2:
    the comparison and thresholds of test_corrected_resnet_gradient_matches_torch (1e-5 of the largest entry for
    each net and for the downsampler's slice on its own scale; the floors 1e-4 and 1e-6 for a gradient having
    arrived), importance weights in every other case."""
    from test_corrected_resnet_gpu import _corrected_against_torch
    conf, hyper = dsh.cases()[cid]
    B, K = 3, 2
    conf = dataclasses.replace(conf, batch_size=B, num_unroll_steps=K, intermediate_rewards=True)
    _corrected_against_torch(conf, hyper, B=B, K=K, ir=True, per=dsh.IDS.index(cid) % 2 == 0, ds=True,
                             observation=dsh.observations(conf, B, 300 + dsh.IDS.index(cid)))


@pytest.mark.parametrize("cid", ["odd65", "k53"])
def test_ds_shape_corrected_steps(cid):
    """grad_dev + apply_dev equals mz_learner_step bit for bit over two corrected steps, as
    test_corrected_atari_learner_trains, on a staged (odd65) and an unstaged (k53) case."""
    import torch
    from muzero_jl_amd import abi
    conf, _ = dsh.cases()[cid]
    B = conf.batch_size
    e1, e2 = _new_engine(cid, scale=0.5, seed=2), _new_engine(cid, scale=0.5, seed=2)
    try:
        for e in (e1, e2):
            e.learner_set_mode(abi.LEARN_CORRECTED)
        rng = np.random.default_rng(1)
        grad = torch.zeros(e2.grad_count(), dtype=torch.float32, device="cuda")
        for t in range(1, 3):
            batch = dsh.random_batch(conf, rng, 500 + t)
            l1 = e1.learner_step(batch, 1e-4)
            dev = [torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in
                   ("observation", "actions", "target_values", "target_rewards", "target_policies",
                    "gradient_scale")]
            losses = torch.zeros(8, dtype=torch.float32, device="cuda")
            e2.learner_grad_dev([d.data_ptr() for d in dev] + [None], B, grad.data_ptr(), losses.data_ptr())
            e2.learner_apply_dev(grad.data_ptr(), 1.0, 1e-4)
            e2.sync()
            assert np.array_equal(l1, losses.cpu().numpy()[:6])
            for n in range(3):
                assert np.array_equal(e1.get_weights(n), e2.get_weights(n))
        nd = _ds_params(cid)
        assert not np.array_equal(e1.get_weights(0)[:nd], dsh.lively_nets(cid)[0][:nd] * np.float32(0.5))
    finally:
        e1.close(); e2.close()


def test_ds_shape_refusals():
    """More than 256 taps, and activations past the LDS, are refused at create with a message (both on the host,
    before any launch), and an engine created right after each refusal works."""
    from muzero_jl_amd import abi
    for (conf, hyper), msg in dsh.refused_cases():
        with pytest.raises(abi.MzError, match=msg):
            abi.Engine(conf, hyper, device=0, max_games=8, rng_seed=7).close()
        eng = _new_engine("c1")
        try:
            x, want, _ = dsh.forward_reference("c1", 1)
            assert np.array_equal(eng.forward(0, x), want)
        finally:
            eng.close()
