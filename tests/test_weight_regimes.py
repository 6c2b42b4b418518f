"""CPU tests of the weight regimes of tests/weight_regimes.py (no GPU).

Every FC test of the suite ran on init_nets: every Dense bias exactly 0, the
tanh heads inside |x| < 0.25, the policy nearly uniform.  Here the oracle — the
reference of every GPU parity test — runs with nonzero, all-distinct biases
and with peaked, saturating and underflowing heads against a float64 numpy
forward (torch float64 for the BatchNorm nets) at the project's bar
(rtol = atol = 1e-5), and its search against the independent
Python mirror.  The coverage conditions are computed from the float64
reference alone, so a later change of seeds cannot hollow the tests out.
"""
import dataclasses

import numpy as np
import pytest

import weight_regimes as wr
from conftest import random_positions

N = 64
FEATS = [(0, 63), (1, 27), (2, 36)]


def _oracle(conf, hyper, nets, seed=5):
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    o = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=seed)
    for n, w in enumerate(nets):
        o.set_weights(n, w)
    return o


@pytest.fixture(scope="module")
def ref64(ttt, nets):
    """name -> (regime nets, the three nets' f32 input rows, [(outputs, pre) per net] in float64), computed once."""
    out = {}
    obs = random_positions(N, 3)[0]
    for name in wr.REGIMES:
        r = wr.named(ttt.conf, ttt.hyper, nets, name)
        (h,), _ = wr.forward64(ttt.conf, ttt.hyper, 0, r[0], obs)
        xs = wr.inputs(obs, h, 9)
        out[name] = (r, xs, [wr.forward64(ttt.conf, ttt.hyper, net, r[net], xs[net]) for net in range(3)])
    return out


@pytest.mark.parametrize("name", list(wr.REGIMES))
def test_oracle_forward_matches_float64(ttt, ref64, name):
    r, xs, want = ref64[name]
    ora = _oracle(ttt.conf, ttt.hyper, r)
    for net in range(3):
        got = ora.forward(net, xs[net])
        got = got if isinstance(got, tuple) else (got,)
        for k, (g, w) in enumerate(zip(got, want[net][0])):
            assert g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5, err_msg=f"{name}: net {net} output {k}")


@pytest.mark.parametrize("name", ["biased", "peaked"])
def test_oracle_bn_forward_matches_torch_float64(ttt, name):
    from test_fc_bn import _bn_nets, _torch_forward
    hyper = dataclasses.replace(ttt.hyper, use_batch_norm=True)
    r = wr.named(ttt.conf, hyper, _bn_nets(ttt.conf, hyper), name)
    ora = _oracle(ttt.conf, hyper, r)
    obs = random_positions(N, 3)[0]
    f64 = lambda net, x: _torch_forward(ttt.conf, hyper, net, r[net].astype(np.float64), x.astype(np.float64))  # noqa: E731
    xs = wr.inputs(obs, f64(0, obs)[0], 9)
    for net in range(3):
        got = ora.forward(net, xs[net])
        got = got if isinstance(got, tuple) else (got,)
        for k, (g, w) in enumerate(zip(got, f64(net, xs[net]))):
            assert w.dtype == np.float64
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5, err_msg=f"{name}: net {net} output {k}")


def test_oracle_connect4_forward_matches_float64():
    """The other FC shape: 294 stacked features, a 126-wide hidden state, A = 7."""
    from muzero_jl_amd.games import connect4 as c4
    from muzero_jl_amd.networks import init_nets
    r = wr.named(c4.conf, c4.hyper, init_nets(c4.conf, c4.hyper, seed=11), "biased")
    ora = _oracle(c4.conf, c4.hyper, r)
    obs = random_positions(37, 3, A=7, feat=294)[0]
    xs = wr.inputs(obs, wr.forward64(c4.conf, c4.hyper, 0, r[0], obs)[0][0], 7)
    for net in range(3):
        got = ora.forward(net, xs[net])
        got = got if isinstance(got, tuple) else (got,)
        for g, w in zip(got, wr.forward64(c4.conf, c4.hyper, net, r[net], xs[net])[0]):
            assert g.shape == w.shape
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5, err_msg=f"net {net}")


def test_regimes_cover_the_elementary_functions(ref64):
    """det_tanhf's regimes above the polynomial's |x| < 0.55 — the (1-e)/(1+e) form below 9.5 and ±1
    above — and, counted apart, the polynomial's, each get >= 8 of the 64 pre-activations of the
    value head and of the reward head in some regime; peaked spreads the logits by >= 10; underflow
    yields >= 8 policy entries in [2^-150, 2^-126) (subnormal or just representable in f32) and >= 8
    below 2^-150 (zero in f32).  All from the float64 reference."""
    for net, head in ((1, 0), (2, 1)):                              # the value head, the reward head
        bins = np.zeros(3, int)
        for name in wr.REGIMES:
            a = np.abs(ref64[name][2][net][1][head])
            assert a.shape == (N, 1)
            b = np.array([(a < 0.55).sum(), ((a >= 0.55) & (a < 9.5)).sum(), (a >= 9.5).sum()])
            bins = np.maximum(bins, b)
        assert np.all(bins >= 8), (net, bins)
    lg = ref64["peaked"][2][1][1][1]
    assert (lg.max(1) - lg.min(1)).max() >= 10
    p = ref64["underflow"][2][1][0][1]
    assert p.shape == (N, 9)
    assert ((p < 2.0 ** -126) & (p >= 2.0 ** -150)).sum() >= 8
    assert (p < 2.0 ** -150).sum() >= 8
    sat = ref64["saturated"][2][1][0][0]
    assert (np.abs(sat).astype(np.float32) == 1.0).sum() >= 8       # tanh rounds to ±1 exactly in f32


@pytest.mark.parametrize("name", list(wr.REGIMES))
@pytest.mark.parametrize("S,players,explore", [(10, 2, True), (25, 2, True), (15, 1, True), (12, 2, False)])
def test_oracle_search_matches_independent_mirror(ttt, nets, name, S, players, explore):
    import test_cpu_oracle
    r = wr.named(ttt.conf, ttt.hyper, nets, name)
    test_cpu_oracle.test_oracle_search_matches_independent_mirror(ttt, r, S, players, explore)


def test_ref_semantics_learner_never_creates_a_bias(ttt, nets):
    """The ref_semantics gradient is 2θ (Q11): a zero bias has zero gradient and zero ADAM moments and
    stays 0 for ever, while every nonzero bias moves — why no learner test on init_nets, nor any
    search after one, ever read a nonzero Dense bias."""
    from muzero_jl_amd.config import cos_schedule
    from test_gpu_parity import _random_batch
    conf, hyper = ttt.conf, ttt.hyper
    for start, moved in ((nets, False), (wr.named(conf, hyper, nets, "biased"), True)):
        ora = _oracle(conf, hyper, start)
        st = ora.learner_state()
        rng = np.random.default_rng(1)
        for t in range(1, 6):
            ora.learner_step(st, _random_batch(conf.batch_size, conf.num_unroll_steps, 9, rng), cos_schedule(t))
        b0, b1 = wr.biases(conf, hyper, start), wr.biases(conf, hyper, ora.params)
        assert np.all(b1 != b0) if moved else (np.all(b0 == 0) and np.all(b1 == 0))
        for n in range(3):                                          # the steps did run: every weight moved
            still = sum(k for _, _, k in wr.bias_slices(conf, hyper, n)) if not moved else 0
            assert np.sum(ora.params[n] == start[n]) == still


@pytest.mark.parametrize("bn", [False, True])
def test_checkpoint_names_every_bias(ttt, nets, tmp_path, bn):
    """With zero biases two bias tensors of equal length could be swapped unseen: each "<net>.<i>"
    bias tensor of a written checkpoint is its layer's slice of the flat vector."""
    from muzero_jl_amd import checkpoint as ck
    from muzero_jl_amd.networks import init_nets, layer_specs
    hyper = dataclasses.replace(ttt.hyper, use_batch_norm=bn)
    r = wr.named(ttt.conf, hyper, init_nets(ttt.conf, hyper, seed=11) if bn else nets, "biased")
    p = str(tmp_path / "biased.safetensors")
    ck.write(p, ttt.conf, hyper, r)
    t, _ = ck.read(p)
    for net in range(3):
        specs = layer_specs(ttt.conf, hyper, net, True)
        for k, off, n in wr.bias_slices(ttt.conf, hyper, net):
            idx = sum(4 if s[4] else 2 for s in specs[:k]) + 1      # W, b (, β, γ) per layer before it, then W
            got = t[f"{ck.NETS[net]}.{idx}"]
            assert got.shape == (n,) and np.array_equal(got, r[net][off:off + n]), (net, k)
            assert np.any(got != 0)
    for a, b in zip(ck.nets_from(t, ttt.conf, hyper), r):
        assert np.array_equal(a, b)
