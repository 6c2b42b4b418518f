"""Weight regimes for the FC nets, and a float64 numpy forward (tests only).

init_nets gives Glorot weights with every Dense bias exactly 0, and holds the
value / reward heads' tanh and the policy logits in a corner (|x| < 0.25).
`regime` returns copies of a set of nets with
  * every Dense bias ~ N(0, bias_sd), all values distinct (so that a bias read
    from the wrong slot, layer or net cannot go unnoticed),
  * the W of the three last layers that feed an elementary function — the
    value head (net 1, chain 1), the policy head (net 1, chain 2) and the
    reward head (net 2, chain 2) — multiplied by head_scale.
BatchNorm β, γ stay as the caller passed them.

REGIMES names the four head scales: `biased` (1) keeps the heads where
init_nets has them, `peaked` (16) puts the tanh pre-activations into det_tanhf's
(1-e)/(1+e) regime and spreads the logits by > 10, `saturated` (32) drives most
pre-activations past 9.5 (tanh = ±1 exactly), `underflow` (160) makes softmax
entries subnormal or zero in f32.

`forward64` is the high-precision reference of net_forward for the FC nets
without BatchNorm: matmul, bias, relu, np.tanh and a max-subtracted softmax in
float64 from `unflatten`; `inputs` builds the rows the tests feed the nets.
"""
import numpy as np

from muzero_jl_amd.config import ACT_RELU, ACT_TANH
from muzero_jl_amd.networks import layer_specs, unflatten

REGIMES = {"biased": 1, "peaked": 16, "saturated": 32, "underflow": 160}
HEADS = ((1, 1), (1, 2), (2, 2))            # (net, chain) of the last layers that head_scale multiplies


def bias_slices(conf, hyper, net):
    """[(layer index, offset, length)] of the Dense biases in the net's flat vector."""
    out, off = [], 0
    for k, (_, i, o, _, bn) in enumerate(layer_specs(conf, hyper, net, True)):
        off += i * o
        out.append((k, off, o))
        off += o + (2 * o if bn else 0)
    return out


def regime(conf, hyper, nets, head_scale, bias_sd=0.25, seed=7):
    rng = np.random.default_rng(seed)
    out = [np.array(n, dtype=np.float32, copy=True) for n in nets]
    for net in range(3):
        specs = layer_specs(conf, hyper, net, True)
        last = {ch: k for k, (ch, *_) in enumerate(specs)}           # the last layer of each chain
        off = 0
        for k, (ch, i, o, _, bn) in enumerate(specs):
            if (net, ch) in HEADS and last[ch] == k:
                out[net][off:off + i * o] *= np.float32(head_scale)
            off += i * o
            out[net][off:off + o] = rng.normal(0, bias_sd, o).astype(np.float32)
            off += o + (2 * o if bn else 0)
        assert off == out[net].size
    b = np.concatenate([out[net][o:o + n] for net in range(3) for _, o, n in bias_slices(conf, hyper, net)])
    assert np.unique(b).size == b.size, "bias values are not all distinct"
    return out


def named(conf, hyper, nets, name, **kw):
    return regime(conf, hyper, nets, REGIMES[name], **kw)


def biases(conf, hyper, nets):
    """Every Dense bias of the three nets, back to back."""
    return np.concatenate([nets[net][o:o + n] for net in range(3) for _, o, n in bias_slices(conf, hyper, net)])


def forward64(conf, hyper, net, flat, x):
    """(outputs, pre): outputs as Oracle.forward gives them (net 0: (h,); net 1: (value, policy);
    net 2: (h', reward)), all float64; pre = the last layer's pre-activations of the same heads
    (the hidden states' are the outputs themselves, the policy's are the logits)."""
    layers = unflatten(conf, hyper, net, np.asarray(flat, np.float64))

    def chain(ch, v):
        pre = v
        for c, W, b, act in layers:
            if c != ch:
                continue
            pre = v @ W.T + b
            v = np.maximum(pre, 0.0) if act == ACT_RELU else np.tanh(pre) if act == ACT_TANH else pre
        return v, pre

    t, pre = chain(0, np.asarray(x, np.float64))
    if net == 0:
        return (t,), (pre,)
    (o0, p0), (o1, p1) = chain(1, t), chain(2, t)
    if net == 1:
        e = np.exp(p1 - p1.max(axis=1, keepdims=True))
        o1 = e / e.sum(axis=1, keepdims=True)
    return (o0, o1), (p0, p1)


def inputs(obs, hidden, A):
    """The f32 rows fed to the three nets: the observations, the reference's hidden states of them,
    and those hidden states with a one-hot action plane (row i plays action i mod A)."""
    n = obs.shape[0]
    h = np.asarray(hidden, np.float32)
    plane = np.zeros((n, (hidden.shape[1] // 3)), np.float32)
    plane[np.arange(n), np.arange(n) % A] = 1
    return [np.asarray(obs, np.float32), h, np.concatenate([h, plane], 1)]
