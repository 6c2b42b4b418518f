"""The downsampler shape matrix shared by tests/test_downsample_shapes.py (CPU:
oracle against torch and the Python mirror) and tests/test_downsample_shapes_gpu.py
(the kernels of csrc/mz_downsample.hip against the oracle bit for bit, and
mz_dsbp_* against torch autograd).

The preset (games/atari_synth: 84x84x4, a 3x3 kernel) stages its observation in
LDS and runs every conv through one of the four compile-time forms.  Each case
here is atari_synth's (conf, resnet_hyper) with the board, stacking, action space
and kernel replaced, 16 filters and one block behind the downsampler, on
synthetic inputs (no environment), and reaches what the preset does not.  The
hidden board is ⌈W/16⌉ x ⌈H/16⌉, 3x3 or 5x5 in every case: plane sizes the
ResNet matrix (tests/resnet_shapes.py) covers, so a failure points at the
downsampler.

id      board, stack   kernel A   C  staged  what it reaches
odd65   (65,67,4), 0   (3,3)  18  4  yes     the four fast forms at odd, non-square boards 33x34 -> 17x17 -> 9x9
                                             -> 5x5; right / bottom stride-2 taps off the board; A > 16
c4u     (37,45,4), 0   (3,3)  5   4  no      the preset's channel pairs through ds_conv_generic (the `stage &&` of
                                             k3); layer 0 from HBM; K = 36: quarter 3 is empty
c3s     (37,45,1), 1   (3,3)  9   3  no      stacking in front of the downsampler (C = c(s+1) + s); in_feat = 4995:
                                             item bases are not 16-byte aligned; K = 27 / 54
c2st    (48,47,2), 0   (3,3)  7   2  yes     the staged observation and the parameter image with generic convs (2 -> 2,
                                             2 -> 4; the 4 -> 4 blocks behind them match ds_conv_valu<4,4,1>)
k31     (40,40,4), 0   (3,1)  20  4  yes     staged, the preset's channels, kh = 1: the k3 test must say no; A > 16
k53     (36,41,2), 0   (5,3)  6   2  no      a non-square kernel, pw != ph, dx in -2..2; mz_dsbp_dw with kk = 15
k35     (41,36,2), 0   (3,5)  6   2  no      the same transposed
c8      (35,33,8), 0   (3,3)  4   8  no      8 -> 8 stride 2, 8 -> 16, 16 -> 16 (K = 144); 3,072 mz_dsbp_dw jobs for
                                             the widest layers
c5k55   (34,34,5), 0   (5,5)  3   5  no      K = 250 of the 256 tap-table entries; w_floats = 2500
c1      (33,48,1), 0   (3,3)  16  1  yes     one channel: K = 9 (kq = 4, three empty quarters) and K = 18

Staged (DsPlan.stage_in, ds_build): the observation's floats are a multiple of 4, twice the activation buffer
plus every conv's parameters fit in them, and the staged layout fits the LDS.  The tests read the flag from the
engine (mz_downsample_staged) and compare it with STAGED.

Reference: src/Learning.jl:148-191 (the representation and its downsampler), src/SelfPlay.jl:128-149 (stacking)."""
import dataclasses
import functools

import numpy as np

import resnet_shapes as rs

SEARCH_S, SEARCH_G = 6, 5
LEARN_B, LEARN_K = 5, 2


def _case(board, stack, kernel, A, B=LEARN_B):
    from muzero_jl_amd.games import atari_synth as at
    from muzero_jl_amd.networks import resnet_board
    conf = dataclasses.replace(at.conf, observation_shape=tuple(board), stacked_observations=stack,
                               action_space=list(range(1, A + 1)), num_iters=SEARCH_S, batch_size=B,
                               num_unroll_steps=LEARN_K, intermediate_rewards=True)
    hyper = dataclasses.replace(at.resnet_hyper, conv_kernel_size=tuple(kernel), num_filters=16, num_blocks=1)
    W, H = resnet_board(conf, hyper)
    hyper = dataclasses.replace(hyper, hidden_state_size=W * H * 16, representation_output_size=(W, H, 16))
    return conf, hyper


@functools.lru_cache(maxsize=None)
def cases():
    return {
        "odd65": _case((65, 67, 4), 0, (3, 3), 18),
        "c4u": _case((37, 45, 4), 0, (3, 3), 5),
        "c3s": _case((37, 45, 1), 1, (3, 3), 9),
        "c2st": _case((48, 47, 2), 0, (3, 3), 7),
        "k31": _case((40, 40, 4), 0, (3, 1), 20),
        "k53": _case((36, 41, 2), 0, (5, 3), 6),
        "k35": _case((41, 36, 2), 0, (3, 5), 6),
        "c8": _case((35, 33, 8), 0, (3, 3), 4),
        "c5k55": _case((34, 34, 5), 0, (5, 5), 3),
        "c1": _case((33, 48, 1), 0, (3, 3), 16),
    }


IDS = ["odd65", "c4u", "c3s", "c2st", "k31", "k53", "k35", "c8", "c5k55", "c1"]

# The downsampler's input channels C = c(s + 1) + s
CHANNELS = {"odd65": 4, "c4u": 4, "c3s": 3, "c2st": 2, "k31": 4, "k53": 2, "k35": 2, "c8": 8, "c5k55": 5, "c1": 1}

# The boards behind the two stride-2 convs and the two MeanPools (each ⌈n/2⌉ of the one before)
CHAIN = {
    "odd65": [(33, 34), (17, 17), (9, 9), (5, 5)],
    "c4u": [(19, 23), (10, 12), (5, 6), (3, 3)],
    "c3s": [(19, 23), (10, 12), (5, 6), (3, 3)],
    "c2st": [(24, 24), (12, 12), (6, 6), (3, 3)],
    "k31": [(20, 20), (10, 10), (5, 5), (3, 3)],
    "k53": [(18, 21), (9, 11), (5, 6), (3, 3)],
    "k35": [(21, 18), (11, 9), (6, 5), (3, 3)],
    "c8": [(18, 17), (9, 9), (5, 5), (3, 3)],
    "c5k55": [(17, 17), (9, 9), (5, 5), (3, 3)],
    "c1": [(17, 24), (9, 12), (5, 6), (3, 3)],
}

# mz_downsample_staged of each case, and of the preset
STAGED = {"odd65": 1, "c4u": 0, "c3s": 0, "c2st": 1, "k31": 1, "k53": 0, "k35": 0, "c8": 0, "c5k55": 0, "c1": 1}
STAGED_PRESET = 1


def refused_cases():
    """The two shapes mz_engine_create_resnet refuses, with the message each gets: 25 taps x 12 channels = 300
    entries for the 256-entry tap tables; and two 75x75x4 activation buffers (the observation does not fit beside
    them, so nothing is staged) plus 1,688 parameter / table floats = 186,752 B of LDS."""
    return [(_case((34, 34, 6), 0, (5, 5), 3), "256 taps"),
            (_case((150, 150, 4), 0, (3, 3), 18), "exceed the LDS")]


features = rs.features


@functools.lru_cache(maxsize=None)
def lively_nets(cid):
    """init_nets with the conv biases, β and γ away from (0, 0, 1); read-only."""
    from muzero_jl_amd.networks import init_nets
    from test_resnet_oracle import _perturb_bn
    conf, hyper = cases()[cid]
    seed = 80 + IDS.index(cid)
    nets = _perturb_bn(conf, hyper, init_nets(conf, hyper, seed=seed), seed=seed + 1)
    for w in nets:
        w.setflags(write=False)
    return nets


def oracle(cid, seed=7):
    """A fresh oracle of the case holding copies of lively_nets."""
    from muzero_jl_amd.config import to_c_config, to_c_resnet_hp
    from oracle import Oracle
    conf, hyper = cases()[cid]
    o = Oracle(to_c_config(conf), to_c_resnet_hp(hyper), seed=seed)
    for n, w in enumerate(lively_nets(cid)):
        o.set_weights(n, w.copy())
    return o


def observations(conf, n, seed):
    """n observations (n, features), column-major (W, H, C) planes.  Plain noise comes out of the two MeanPools
    nearly the same for every item, so item i is U[0, 1) noise times (i + 1) / n, and the odd-numbered items have
    the last column and the last row of every channel at 4.0 (what the off-board taps of the right and bottom
    edges sit next to).  With stacking, the action planes between the frames hold a / |A| of a drawn action."""
    W, H, c = conf.observation_shape
    s, A = conf.stacked_observations, len(conf.action_space)
    C = c * (s + 1) + s
    assert W * H * C == features(conf)
    rng = np.random.default_rng(seed)
    x = rng.random((n, C, H, W), dtype=np.float32)
    x *= ((np.arange(n, dtype=np.float32) + 1) / np.float32(n))[:, None, None, None]
    x[1::2, :, :, W - 1] = 4.0
    x[1::2, :, H - 1, :] = 4.0
    for past in range(s):                       # [obs_t, (action plane, obs_{t-1}), ...]
        a = rng.integers(1, A + 1, n).astype(np.float32) / np.float32(A)
        x[:, c + past * (c + 1)] = a[:, None, None]
    return np.ascontiguousarray(x.reshape(n, -1))


def assert_items_differ(out):
    """Two items' outputs differ by more than 1e-3 somewhere: the inputs did not collapse in the pools."""
    assert out.shape[0] < 2 or np.abs(out[0] - out[1]).max() > 1e-3


@functools.lru_cache(maxsize=None)
def forward_reference(cid, n):
    """(x, the oracle's net 0 output, torch's) for n observations of the case; computed once, read-only."""
    from test_resnet_oracle import _torch_forward
    conf, hyper = cases()[cid]
    x = observations(conf, n, 100 * IDS.index(cid) + n)
    want = oracle(cid).forward(0, x)
    ref = _torch_forward(conf, hyper, 0, lively_nets(cid)[0].copy(), x)
    assert_items_differ(want)
    for a in (x, want, ref):
        a.setflags(write=False)
    return x, want, ref


def search_inputs(conf, G, seed):
    """(obs, legal, to_play): resnet_shapes.search_inputs' masks (game 1 has one legal action; with A > 16 game 2's
    are all above 16), this module's observations, one player."""
    _, legal, _ = rs.search_inputs(conf, G, seed)
    return observations(conf, G, seed), legal, np.ones(G, np.int32)


def random_batch(conf, rng, seed):
    batch = rs.random_batch(conf, rng)
    batch["observation"] = observations(conf, conf.batch_size, seed)
    return batch
