"""The FC corrected learner's shape matrix, shared by tests/test_fc_corrected_shapes.py (CPU: the
conditions on the inputs) and tests/test_fc_corrected_shapes_gpu.py (mz_bp_tile_lv*, mz_bp_tile,
mz_bp_dw, mz_bp_fold and mz_adam_kernel against torch autograd, the sequential kernel and the host
mirror).

Every other GPU test of MZ_LEARN_CORRECTED on the FC nets runs TicTacToe's preset (63 inputs, width
64, H = 27, A = 9, K <= 5), where build_bp's plan (csrc/mz_backprop_host.hip) gives every tensor that
is read again an LDS copy, accumulates every input gradient with a producer in LDS, flags only the
last forward level and the observation gradient's level, and every GEMM is one k-chunk.  Each case
here is a preset's (conf, hyper) with fields replaced, on random batches, and reaches a plan regime or
a kernel path the preset does not.  PLAN holds what mz_debug_bp_plan must read for the case (the
regime, not the numbers); the numbers it read on an MI355X when the table was written are under PLAN.

id          nets / conf                          K  ir PER B   there for
c4_k5       Connect4 preset FC                   5  y  y   20  forward and backward arena fallback, a flagged level in
                                                               mid-schedule; in = 294 / 168 / 126: 5 / 3 / 2 k-chunks, the
                                                               last partial; out = 126: 8 row blocks, the last of 14 rows; A = 7
c4_k2       Connect4 preset FC                   2  y  n   17  the backward fallback only (two ∂L/∂x in the arena, no forward
                                                               tensor); the second tile has one live sample
c4_k2_noir  Connect4 preset FC                   2  n  n   17  the issue's c4_k2 as written: without the reward heads every
                                                               ∂L/∂x of the unroll fits the 8 slots (the read-out shows no
                                                               fallback at any K without them), so the fallback case above
                                                               has the rewards on and this one keeps what else the row
                                                               asked for: the reward head unused (exact-zero data gradient),
                                                               the k-chunks, one live sample in the second tile
c4_bn_k3    Connect4 preset, use_batch_norm      3  y  y   20  mz_bp_tile_lv (MAYBN) with the backward fallback; z tensors; dβ, dγ
ttt_k1      TicTacToe preset                     1  y  y   1   the state head unused (exact-zero data gradient); one live sample
ttt_k60     TicTacToe preset                     60 y  n   16  4 slots: dozens of flagged forward levels, hundreds of arena
                                                               accumulations
ttt_k66     TicTacToe preset                     66 y  n   15  no cache: bp_lv_levels' C == nullptr branch
w20         TicTacToe, width 20, A = 4, r relu   2  y  y   33  one row block and a 4-row tail, nk = 5, A = 4, three tiles
w80         TicTacToe, width 80                  2  y  n   17  5 row blocks; two k-chunks, the second 4 k-steps of 16
h40         (5,4,2) board, H = 40, A = 16,       3  y  y   16  H and the action plane off the preset, A = 16 (a full block), a
            reward identity                                    full tile
wide        TicTacToe, width 192                 16 y  y   20  12 row blocks: 60 units in a level on 16 waves, 3 k-chunks, with
                                                               both fallbacks.  The issue's width 272 at K = 5 (17 row
                                                               blocks) is refused by mz_engine_create: the search kernel's
                                                               activation layout passes the LDS from width 256 on ("LDS
                                                               budget exceeded", test_wide_width_is_refused).  At 192, a
                                                               width the engine accepts, K = 5 leaves 11 slots and no
                                                               fallback; K = 16 is the shortest unroll with both (7 slots)

Weights: init_nets under weight_regimes "biased" (every Dense bias nonzero and distinct, the heads where
init_nets has them: a plain 3x scale saturates the value and reward heads' tanh and zeroes their
gradients), BatchNorm β, γ off (0, 1) where there are any; `wide` takes init_nets as it is with biases
drawn the same way ("biased" insists on all-distinct f32 values, which its 4,000 biases are not; a 1.5x
scale over 16 steps overflows the float32 floor).  The seeds are chosen on the CPU
(test_fc_corrected_shapes.py) so that the float32 torch reference stays within E32_MAX of the float64
one on every parameter tensor's own scale: the per-tensor bound of the GPU test is
max(1e-5, 4 · e32_t), never above 1e-4.
"""
import dataclasses
import functools

import numpy as np

E32_MAX = 2.5e-5          # the float32 reference's largest allowed error on a tensor's own scale
FLOOR = 1e-5              # the project's bar
ORDER_FACTOR = 4.0        # the kernel sums in another order than torch's float32 GEMM (MFMA k-steps of 4,
                          # tiles, then applications); det_tanhf / det_expf are within 2 ulp


WIDE, WIDE_REFUSED = 192, 272   # `wide`'s width; the issue's, which mz_engine_create refuses (the table above)


@dataclasses.dataclass(frozen=True)
class Case:
    conf: object
    hyper: object
    B: int
    per: bool
    weights: tuple        # ("biased", init seed, bias seed) or ("scale", init seed, factor of init_nets)
    seed: int             # of the batch

    @property
    def K(self):
        return self.conf.num_unroll_steps

    @property
    def ir(self):
        return bool(self.conf.intermediate_rewards)


def _case(game, K, ir, per, B, weights, seed, conf_kw=None, **hp):
    from muzero_jl_amd.games import connect4, tictactoe
    mod = {"ttt": tictactoe, "c4": connect4}[game]
    conf = dataclasses.replace(mod.conf, batch_size=B, num_unroll_steps=K, intermediate_rewards=ir,
                               **(conf_kw or {}))      # (PER: the batch's weights; the learner reads no flag)
    return Case(conf, dataclasses.replace(mod.hyper, **hp), B, per, weights, seed)


@functools.lru_cache(maxsize=None)
def cases():
    return {
        "c4_k5": _case("c4", 5, True, True, 20, ("biased", 11, 7), 1),
        "c4_k2": _case("c4", 2, True, False, 17, ("biased", 12, 7), 2),
        "c4_k2_noir": _case("c4", 2, False, False, 17, ("biased", 12, 7), 2),
        "c4_bn_k3": _case("c4", 3, True, True, 20, ("biased", 13, 7), 3, use_batch_norm=True),
        "ttt_k1": _case("ttt", 1, True, True, 1, ("biased", 14, 7), 4),
        "ttt_k60": _case("ttt", 60, True, False, 16, ("biased", 0, 7), 5),
        "ttt_k66": _case("ttt", 66, True, False, 15, ("biased", 0, 7), 6),
        "w20": _case("ttt", 2, True, True, 33, ("biased", 15, 7), 7, dict(action_space=[1, 2, 3, 4]),
                     width_hidden=20, reward_activation="relu"),
        "w80": _case("ttt", 2, True, False, 17, ("biased", 16, 7), 8, width_hidden=80),
        "h40": _case("ttt", 3, True, True, 16, ("biased", 17, 7), 9,
                     dict(observation_shape=(5, 4, 2), stacked_observations=0, action_space=list(range(1, 17))),
                     hidden_state_size=40, reward_activation="identity"),
        "wide": _case("ttt", 16, True, True, 20, ("scale", 18, 1.0), 10, width_hidden=WIDE),
    }


IDS = ["c4_k5", "c4_k2", "c4_k2_noir", "c4_bn_k3", "ttt_k1", "ttt_k60", "ttt_k66", "w20", "w80", "h40", "wide"]
STEP_IDS = ["c4_k5", "w20"]                  # the three-step ADAM check

# What mz_debug_bp_plan must read (abi.BP_PLAN_FIELDS): "+" > 0, "0" == 0; "mid" under fwd_flagged /
# bwd_flagged: more flagged levels than the one (the last forward level, the observation gradient's)
# every plan has.  chunks: max(in, out) > 64 of some Dense, where k-chunks are the point.
PLAN = {
    "c4_k5": dict(arena_reads="+", unslotted_outputs="+", arena_accumulations="+", fwd_flagged="mid",
                  bwd_flagged="mid", nslot="+", chunks=True),
    "c4_k2": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="+", fwd_flagged="1",
                  bwd_flagged="mid", nslot="+", chunks=True),
    "c4_k2_noir": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="0", fwd_flagged="1",
                       bwd_flagged="1", nslot="+", chunks=True),
    "c4_bn_k3": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="+", fwd_flagged="1",
                     bwd_flagged="mid", nslot="+", chunks=True),
    "ttt_k1": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="0", fwd_flagged="1",
                   bwd_flagged="1", nslot="+"),
    "ttt_k60": dict(arena_reads="+", unslotted_outputs="+", arena_accumulations="+", fwd_flagged="mid",
                    bwd_flagged="mid", nslot="+"),
    "ttt_k66": dict(arena_reads="+", unslotted_outputs="+", arena_accumulations="+", fwd_flagged="mid",
                    bwd_flagged="mid", nslot="0"),
    "w20": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="0", fwd_flagged="1", bwd_flagged="1",
                nslot="+"),
    "w80": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="0", fwd_flagged="1", bwd_flagged="1",
                nslot="+", chunks=True),
    "h40": dict(arena_reads="0", unslotted_outputs="0", arena_accumulations="0", fwd_flagged="1", bwd_flagged="1",
                nslot="+"),
    "wide": dict(arena_reads="+", unslotted_outputs="+", arena_accumulations="+", fwd_flagged="mid",
                 bwd_flagged="mid", nslot="+", chunks=True),
}

# As read on an MI355X (slots; arena reads / unslotted outputs / arena accumulations; flagged forward /
# backward levels of the levels there are):
#   c4_k5       7   1 / 1 / 3           2 / 3 of 48 / 49        c4_k2     8   0 / 0 / 2   1 / 3 of 21 / 22
#   c4_k2_noir  8   0 / 0 / 0           1 / 1 of 20 / 22        c4_bn_k3  8   0 / 0 / 2   1 / 3 of 30 / 31
#   ttt_k1      39  0 / 0 / 0           1 / 1 of 12 / 14        w20       38  0 / 0 / 0   1 / 1 of 21 / 22
#   ttt_k60     4   68 / 66 / 302       64 / 125 of 543 / 544   w80       30  0 / 0 / 0   1 / 1 of 21 / 22
#   ttt_k66     0   1262 / 1063 / 1262  597 / 598 of 597 / 598  h40       37  0 / 0 / 0   1 / 1 of 30 / 31
#   wide        7   1 / 1 / 3           2 / 3 of 147 / 148
# TicTacToe's nets at K = 64, 65 keep one slot, at 66, 67 none; 68 is refused.  Width 192 at K = 5 reads 11
# slots and 0 / 0 / 0; widths 256 .. 512 are refused by mz_engine_create.

# The TicTacToe preset at K = 5, the shape of every other corrected-learner test: none of the above
PRESET_PLAN = dict(arena_reads=0, unslotted_outputs=0, arena_accumulations=0, fwd_flagged=1, bwd_flagged=1)

# The first K at which the engine refuses TicTacToe's preset nets (with the reward heads): the
# schedule and the descriptors alone pass the LDS.  K - 1 runs (without the cache, as ttt_k66)
REFUSED_K = 68


def check_plan(cid, plan):
    """Assert that the read-out `plan` (Engine.debug_bp_plan()) lies in the regime PLAN[cid] names."""
    from muzero_jl_amd.networks import layer_specs
    want = PLAN[cid]
    for k, w in want.items():
        if k == "chunks":
            c = cases()[cid]
            assert max(max(i, o) for n in range(3) for _, i, o, _ in layer_specs(c.conf, c.hyper, n)) > 64
        elif w == "+":
            assert plan[k] > 0, (cid, k, plan)
        elif w == "0":
            assert plan[k] == 0, (cid, k, plan)
        elif w == "1":
            assert plan[k] == 1, (cid, k, plan)
        else:
            assert w == "mid" and plan[k] > 1, (cid, k, plan)


def features(conf):
    from muzero_jl_amd.config import stacked_features
    return stacked_features(conf)


@functools.lru_cache(maxsize=None)
def nets(cid):
    """The case's three flat vectors, read-only."""
    import weight_regimes as wr
    from muzero_jl_amd.networks import init_nets, layer_specs
    c = cases()[cid]
    kind, s0, s1 = c.weights
    out = init_nets(c.conf, c.hyper, seed=s0)
    if getattr(c.hyper, "use_batch_norm", False):             # β, γ away from (0, 1)
        rng = np.random.default_rng(s0 + 100)
        for n in range(3):
            off = 0
            for _, i, o, _, bn in layer_specs(c.conf, c.hyper, n, True):
                off += i * o + o
                if bn:
                    out[n][off:off + o] = rng.normal(0, 0.2, o).astype(np.float32)
                    out[n][off + o:off + 2 * o] = (1 + rng.normal(0, 0.2, o)).astype(np.float32)
                    off += 2 * o
    if kind == "biased":
        out = wr.named(c.conf, c.hyper, out, "biased", seed=s1)
    else:                                                     # a plain scale, the biases as "biased" draws them
        out = [w * np.float32(s1) for w in out]
        rng = np.random.default_rng(s0 + 200)
        for n in range(3):
            for _, off, cnt in wr.bias_slices(c.conf, c.hyper, n):
                out[n][off:off + cnt] = rng.normal(0, 0.25, cnt).astype(np.float32)
    for w in out:
        w.setflags(write=False)
    return out


def make_batch(c, rng):
    """(batch, PER weights or None) of the case from rng, by test_corrected_learner_gpu's _batch."""
    from test_corrected_learner_gpu import _batch
    b = _batch(c.B, c.K, len(c.conf.action_space), features(c.conf), rng)
    w = (rng.random(c.B).astype(np.float32) * 0.9 + 0.1) if c.per else None
    return b, w


@functools.lru_cache(maxsize=None)
def batch(cid):
    c = cases()[cid]
    b, w = make_batch(c, np.random.default_rng(c.seed))
    for a in list(b.values()) + ([w] if w is not None else []):
        a.setflags(write=False)
    return b, w


@functools.lru_cache(maxsize=None)
def reference(cid, f32=False):
    """torch autograd on the case's inputs, float64 or float32; computed once, shared, read-only."""
    import torch
    from torch_learner_ref import corrected_loss_and_grads
    c = cases()[cid]
    b, w = batch(cid)
    return corrected_loss_and_grads(c.conf, c.hyper, nets(cid), b, w, dtype=torch.float32 if f32 else torch.float64)


def tensors(conf, hyper):
    """[(net, layer, chain, name, offset, length)]: W, b (β, γ) of every Dense in its net's flat vector."""
    from muzero_jl_amd.networks import layer_specs
    out = []
    for n in range(3):
        off = 0
        for k, (ch, i, o, _, bn) in enumerate(layer_specs(conf, hyper, n, True)):
            for name, cnt in (("W", i * o), ("b", o)) + ((("beta", o), ("gamma", o)) if bn else ()):
                out.append((n, k, ch, name, off, cnt))
                off += cnt
    return out


def applied(c, net, chain):
    """Whether the unroll applies the chain on a path to the loss (build_bp; Learning.jl:347-370):
    the dynamics trunk from K = 1 on when something reads it, the state head for k < K only, the
    reward head with intermediate_rewards only."""
    if net != 2:
        return True
    if chain == 1:
        return c.K >= 2
    if chain == 2:
        return c.K >= 1 and c.ir
    return c.K >= 2 or (c.K >= 1 and c.ir)


def tensor_errors(c, got, ref64, ref32=None):
    """Per parameter tensor: dict(key, applied, scale, err, e32, bound) with err = max |got - ref64| on
    the tensor's own scale (its largest float64 entry; the absolute error where that is 0), e32 the same
    of the float32 reference, bound = max(FLOOR, ORDER_FACTOR · e32).  got / ref64 / ref32: three flat
    data-term vectors each."""
    rows = []
    for n, k, ch, name, off, cnt in tensors(c.conf, c.hyper):
        r = np.asarray(ref64[n][off:off + cnt], np.float64)
        g = np.asarray(got[n][off:off + cnt], np.float64)
        scale = float(np.abs(r).max())
        d = float(np.abs(g - r).max())
        row = dict(key=(n, k, name), applied=applied(c, n, ch), scale=scale, err=d / scale if scale else d,
                   zero=bool(np.all(g == 0.0)))
        if ref32 is not None:
            e = float(np.abs(np.asarray(ref32[n][off:off + cnt], np.float64) - r).max())
            row["e32"] = e / scale if scale else e
            row["bound"] = max(FLOOR, ORDER_FACTOR * row["e32"])
        rows.append(row)
    return rows


def net_rows(c, n, seed):
    """n rows of each net's input: 0/1 observations, N(0, 1) hidden states, and those with the action
    plane a / |A| behind them."""
    rng = np.random.default_rng(seed)
    W, Hh, _ = c.conf.observation_shape
    A, hid = len(c.conf.action_space), c.hyper.hidden_state_size
    obs = (rng.random((n, features(c.conf))) < 0.4).astype(np.float32)
    h = rng.normal(0, 1, (n, hid)).astype(np.float32)
    plane = np.repeat((rng.integers(1, A + 1, n) / A).astype(np.float32)[:, None], W * Hh, 1)
    return [obs, h, np.concatenate([h, plane], 1)]
