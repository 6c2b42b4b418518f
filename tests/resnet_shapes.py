"""The ResNet shape matrix shared by tests/test_resnet_shapes.py (CPU: oracle
against torch and the Python mirror) and tests/test_resnet_shapes_gpu.py (the
kernels of csrc/mz_resnet.hip against the oracle, bit for bit).

The presets run the ResNet kernels at three shapes, all with 64 filters.  Each
case here is TicTacToe's (conf, resnet_hyper) with the board, action space and
ResNetHP replaced, on random inputs (no environment: forward, mcts_search and
learner_step need none), and reaches a generic branch the presets do not:

id      board     A   nf  blocks kernel  what it reaches
nf24    (5,4,2)   7   24  1      (3,3)   partial 16-row output blocks (24 = 16 + 8); K % 64 != 0 everywhere, so
                                         no k-blocked layout; dynamics K = 25; plane 20 = 2 column blocks at one
                                         sample; 3 / 5 head filters, depth_value 0, width_hidden 40 (not k 16)
nf16    (4,4,1)   16  16  0      (1,1)   no residual block; a 1x1 representation; plane exactly 16; A = 16 fills
                                         the 16-lane group; depth_value 2
nf128   (3,3,3)   9   128 1      (5,5)   8 row blocks; K = 128 k-blocked; a 5x5 kernel wider than the board
nb3     TicTacToe 9   64  3      (3,3)   dyn_split = 14 != RD_NL: chain1 + pred_n1 at 64 filters
fh64    TicTacToe 9   64  2      (3,3)   64 value-head filters: rp_pred_ok false, rd_chain_ok true
row17   (17,1,2)  20  64  2      (3,3)   plane 17 = a full column block + 1; a one-row board; A > 16 (32-lane
                                         kernels); width_hidden 100
nf80    (5,5,2)   25  80  2      (5,5)   K = 80 plain (nq = 5 padded to 8); plane 25; A = 25; a smaller tile
k63     TicTacToe 9   64  2      (3,3)   learner only, B = 2, K = 63: K + 1 < 64 fails, chain_r + pred_r
k53     (3,3,3)   9   64  1      (5,3)   a non-square kernel: the residual blocks are (kw, kh) as the first conv
k35     (4,3,3)   12  32  1      (3,5)   the same transposed, on a non-square board
wh5780  TicTacToe 9   64  2      (3,3)   width_hidden 5780, depth_value 0: the one-sample plans take 156,160 B of
                                         LDS (the representation's: 64 + 2·576 + 3·5780 activation floats, the zero
                                         float's 4, 19,456 offset-table ints, 1,024 slack), inside the window where
                                         rp_pred_lds (+5,120) fits the 160 KB and rd_chain_lds (+10,240) does not:
                                         chain1 + pred_r.  A tile of 2 games would fit the LDS with its k tables
                                         past offset 32767, which the packed layer entry cannot hold: rn_ng = 1

Reference: src/Learning.jl:148-255 (the nets), src/SelfPlay.jl:225-283 (the search)."""
import dataclasses
import functools

import numpy as np

SEARCH_S, SEARCH_G = 6, 5
LEARN_B, LEARN_K = 5, 2


def _case(board=None, stack=None, A=None, B=LEARN_B, K=LEARN_K, **hp):
    from muzero_jl_amd.games import tictactoe as ttt
    W, H, C = board or ttt.conf.observation_shape
    stack = ttt.conf.stacked_observations if stack is None else stack
    A = A or len(ttt.conf.action_space)
    hyper = dataclasses.replace(ttt.resnet_hyper, **hp)
    nf = hyper.num_filters
    hyper = dataclasses.replace(hyper, hidden_state_size=W * H * nf, representation_output_size=(W, H, nf))
    conf = dataclasses.replace(ttt.conf, observation_shape=(W, H, C), stacked_observations=stack,
                               action_space=list(range(1, A + 1)), num_iters=SEARCH_S, batch_size=B,
                               num_unroll_steps=K)
    return conf, hyper


@functools.lru_cache(maxsize=None)
def cases():
    return {
        "nf24": _case((5, 4, 2), 0, 7, num_filters=24, num_blocks=1, conv_kernel_size=(3, 3),
                      num_first_head_filters=3, num_second_head_filters=5, depth_value=0, width_hidden=40),
        "nf16": _case((4, 4, 1), 1, 16, num_filters=16, num_blocks=0, conv_kernel_size=(1, 1),
                      num_first_head_filters=1, num_second_head_filters=2, depth_value=2, width_hidden=16),
        "nf128": _case((3, 3, 3), 1, 9, num_filters=128, num_blocks=1, conv_kernel_size=(5, 5),
                       num_first_head_filters=2, num_second_head_filters=2, depth_value=1, width_hidden=64),
        "nb3": _case(num_blocks=3),
        "fh64": _case(num_first_head_filters=64, num_second_head_filters=2),
        "row17": _case((17, 1, 2), 0, 20, num_filters=64, num_blocks=2, conv_kernel_size=(3, 3), width_hidden=100),
        "nf80": _case((5, 5, 2), 0, 25, num_filters=80, num_blocks=2, conv_kernel_size=(5, 5), width_hidden=64),
        "k63": _case(B=2, K=63),
        "k53": _case((3, 3, 3), 1, 9, num_filters=64, num_blocks=1, conv_kernel_size=(5, 3)),
        "k35": _case((4, 3, 3), 1, 12, num_filters=32, num_blocks=1, conv_kernel_size=(3, 5)),
        "wh5780": _case(depth_value=0, width_hidden=5780),
    }


IDS = ["nf24", "nf16", "nf128", "nb3", "fh64", "row17", "nf80", "k63", "k53", "k35", "wh5780"]
FULL_IDS = [i for i in IDS if i != "k63"]            # k63 runs the learner only

# The ResNet search is one launch sequence (root, then per simulation the tree step and the
# networks) under one name: mz_mcts_search's ResNet branch sets it without a condition.
SEARCH_VARIANT = "mz_rsearch"

# The unroll's launch form, from runroll_launch (csrc/mz_engine.hip).  None of these batches
# fills the chip, so wide_p is false (B·max(K, 1) / rn_ng < 256 CUs) and the form follows
# from rd_chain_ok (one column block, dyn_split = 2 + 4·blocks = RD_NL = 10, every chain
# layer a 64-channel 1x1 conv) and rp_pred_ok (the same for the 1 + 2·blocks = RP_NL = 5
# trunk layers, and a first head conv that is not 64 wide); both, with K + 1 < 64, fuse.
#   nf24, nf16, nf128, nf80, k35: not 64 filters                -> neither
#   nb3: dyn_split = 14, trunk 7; k53: dyn_split = 6, trunk 3   -> neither
#   row17: plane 17 is two column blocks                         -> neither
#   fh64: the value head's conv is 64 wide                       -> rd_chain_ok only
#   k63: both hold, K + 1 = 64                                   -> the split launches
#   wh5780: both but for the LDS: rd_chain_lds = 166,400 B > 160 KB >= rp_pred_lds = 161,280 B
#                                                                -> rp_pred_ok only
LEARNER_VARIANT = {i: "mz_runroll_chain1+mz_runroll_pred_n1" for i in IDS}
LEARNER_VARIANT["fh64"] = "mz_runroll_chain_r+mz_runroll_pred_n1"
LEARNER_VARIANT["k63"] = "mz_runroll_chain_r+mz_runroll_pred_r"
LEARNER_VARIANT["wh5780"] = "mz_runroll_chain1+mz_runroll_pred_r"

# The tile width the engine must choose (rn_ng: the widest of 16 .. 1 whose plans fit the LDS
# and keep their k tables within the 16-bit offset of the packed layer entry), where the case
# is about it
TILE_GAMES = {"wh5780": 1}


def refused_case():
    """wh5780's neighbour the engine refuses: with width_hidden 11476 the one-game plans still fit
    the LDS (64 + 2·576 + 3·11476 activation floats, 2,368 of k tables, 1,024 slack: 156,144 B),
    but the representation's k tables start at float 35,644, past what the packed layer entry's
    16 signed bits hold."""
    return _case(depth_value=0, width_hidden=11476)


def features(conf):
    from muzero_jl_amd.config import stacked_features
    return stacked_features(conf)


@functools.lru_cache(maxsize=None)
def lively_nets(cid):
    """init_nets with the conv biases, β and γ away from (0, 0, 1); read-only."""
    from muzero_jl_amd.networks import init_nets
    from test_resnet_oracle import _perturb_bn
    conf, hyper = cases()[cid]
    seed = 50 + IDS.index(cid)
    nets = _perturb_bn(conf, hyper, init_nets(conf, hyper, seed=seed), seed=seed + 1)
    for w in nets:
        w.setflags(write=False)
    return nets


def oracle(cid, conf=None, seed=7):
    """A fresh oracle of the case holding copies of lively_nets."""
    from muzero_jl_amd.config import to_c_config, to_c_resnet_hp
    from oracle import Oracle
    c, hyper = cases()[cid]
    o = Oracle(to_c_config(conf or c), to_c_resnet_hp(hyper), seed=seed)
    for n, w in enumerate(lively_nets(cid)):
        o.set_weights(n, w.copy())
    return o


def net_input(conf, hyper, net, n, seed):
    """n rows of net's input: 0/1 observations, N(0, 1) hidden states, and for
    the dynamics the action plane a / |A| behind the state."""
    W, H, _ = conf.observation_shape
    A, hid = len(conf.action_space), W * H * hyper.num_filters
    rng = np.random.default_rng(seed)
    if net == 0:
        return (rng.random((n, features(conf))) < 0.4).astype(np.float32)
    h = rng.normal(0, 1, (n, hid)).astype(np.float32)
    if net == 1:
        return h
    a = rng.integers(1, A + 1, n)
    plane = np.repeat((a / A).astype(np.float32)[:, None], W * H, 1)
    return np.concatenate([h, plane], 1)


def search_inputs(conf, G, seed):
    """(obs, legal, to_play): about 60 % of the actions legal and none of the
    games without one; game 1 has a single legal action; with A > 16 game 2's
    legal actions are all above 16 (the upper half of the 32-lane group)."""
    A = len(conf.action_space)
    rng = np.random.default_rng(seed)
    obs = (rng.random((G, features(conf))) < 0.4).astype(np.float32)
    legal = rng.random((G, A)) < 0.6
    legal[np.arange(G), rng.integers(0, A, G)] = True
    legal[1] = False
    legal[1, A // 2] = True
    if A > 16:
        legal[2] = False
        legal[2, 16:] = rng.random(A - 16) < 0.6
        legal[2, A - 1] = True
    return obs, legal, rng.integers(1, 3, G).astype(np.int32)


def random_batch(conf, rng):
    B, K, A = conf.batch_size, conf.num_unroll_steps, len(conf.action_space)
    tpol = rng.random((B, K + 1, A)).astype(np.float32)
    return dict(observation=(rng.random((B, features(conf))) < 0.4).astype(np.float32),
                actions=rng.integers(1, A + 1, (B, K + 1)).astype(np.float32),
                target_values=rng.uniform(-1, 1, (B, K + 1)).astype(np.float32),
                target_rewards=rng.uniform(-1, 1, (B, K + 1)).astype(np.float32),
                target_policies=tpol / tpol.sum(-1, keepdims=True),
                gradient_scale=rng.integers(1, max(K, 1) + 1, B).astype(np.float32))
