"""The FC engine under the weight regimes of tests/weight_regimes.py: nonzero,
all-distinct Dense biases everywhere, and peaked / saturating / underflowing
heads where an elementary function reads them.  On init_nets (every bias 0,
and the ref_semantics learner never makes one nonzero) the bias gathers, merges
and scatters of mz_small.hip, the image writers of the engine host and the
upper regimes of det_tanhf / det_expf never carried a value on the device.

Every case: the GPU bit-equal to the oracle (or to the host driver / the
sequential path that the oracle pins, where the existing test of that path
takes that route), and within the project's bar (rtol = atol = 1e-5) of the
float64 reference where one exists.  The existing tests' bodies run again
with init_nets replaced by the regime's nets (`use_regime`) wherever they
build their own nets.
"""
import dataclasses

import numpy as np
import pytest

import weight_regimes as wr
from conftest import random_positions
from test_gpu_parity import KERNELS, _compare_trees, _engine, _force, _oracle, _random_batch

pytestmark = pytest.mark.gpu

KIDS = ["tile16", "small1", "small2", "small4"]


@pytest.fixture
def use_regime(monkeypatch):
    """use_regime(name): init_nets(...) gives the regime's nets from here on (FC nets only)."""
    def use(name):
        import muzero_jl_amd.networks as nw
        real = nw.init_nets

        def init_nets(conf, hyper, seed=0):
            return wr.named(conf, hyper, real(conf, hyper, seed=seed), name)
        monkeypatch.setattr(nw, "init_nets", init_nets)
    return use


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def _forward_case(conf, hyper, r, ref, obs, A, name):
    """The three nets on rows built from the reference's own hidden states: GPU == oracle, both within
    the bar of ref(net, x) -> float64 outputs."""
    eng, ora = _engine(conf, hyper, r, 16), _oracle(conf, hyper, r)
    xs = wr.inputs(obs, ref(0, obs)[0], A)
    for net in range(3):
        g, o = _tuple(eng.forward(net, xs[net])), _tuple(ora.forward(net, xs[net]))
        for k, (gi, oi, wi) in enumerate(zip(g, o, ref(net, xs[net]))):
            assert gi.shape == wi.shape
            assert np.array_equal(gi, oi), f"{name} net {net} output {k}: GPU != oracle (max {np.abs(gi - oi).max()})"
            np.testing.assert_allclose(gi, wi, rtol=1e-5, atol=1e-5, err_msg=f"{name} net {net} output {k}")
        if name == "underflow" and net == 1:
            tiny = np.float32(2.0 ** -126)
            assert np.array_equal(g[1] == 0, o[1] == 0), "exact-zero sets differ"
            assert np.array_equal((g[1] > 0) & (g[1] < tiny), (o[1] > 0) & (o[1] < tiny)), "subnormal sets differ"
            if len(obs) >= 37:                                    # (the regime is there: the oracle has both)
                assert (o[1] == 0).any() and ((o[1] > 0) & (o[1] < tiny)).any()
    eng.close()


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("name", list(wr.REGIMES))
def test_net_forward(ttt, nets, name, n):
    r = wr.named(ttt.conf, ttt.hyper, nets, name)
    _forward_case(ttt.conf, ttt.hyper, r, lambda net, x: wr.forward64(ttt.conf, ttt.hyper, net, r[net], x)[0],
                  random_positions(n, 3)[0], 9, name)


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("name", ["biased", "peaked"])
def test_net_forward_batch_norm(ttt, name, n):
    from test_fc_bn import _bn_nets, _torch_forward
    hyper = dataclasses.replace(ttt.hyper, use_batch_norm=True)
    r = wr.named(ttt.conf, hyper, _bn_nets(ttt.conf, hyper), name)
    _forward_case(ttt.conf, hyper, r,
                  lambda net, x: _torch_forward(ttt.conf, hyper, net, r[net].astype(np.float64), x.astype(np.float64)),
                  random_positions(n, 3)[0], 9, name)


def _c4_nets():
    from muzero_jl_amd.games import connect4 as c4
    from muzero_jl_amd.networks import init_nets
    return c4, wr.named(c4.conf, c4.hyper, init_nets(c4.conf, c4.hyper, seed=11), "biased")


def test_net_forward_connect4():
    """294 stacked features, a 126-wide hidden state, A = 7."""
    c4, r = _c4_nets()
    _forward_case(c4.conf, c4.hyper, r, lambda net, x: wr.forward64(c4.conf, c4.hyper, net, r[net], x)[0],
                  random_positions(37, 3, A=7, feat=294)[0], 7, "biased")


# ------------------------------------------------------------------------------------------- search
def _search_case(conf, hyper, r, G, seed, explore, temp, A=9, feat=63, small=False):
    eng, ora = _engine(conf, hyper, r, G, seed), _oracle(conf, hyper, r, seed)
    obs, legal, tp = random_positions(G, seed, A=A, feat=feat)
    eng.debug_enable(1)
    cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=explore, rng_step=seed * 3, game_offset=100,
                                  temperature=temp)
    tree_g = eng.debug_tree(G)
    if small:                                        # (the kernel the case is for, not a silent fallback)
        assert eng.search_variant().startswith("mz_search_small"), eng.search_variant()
    cv2, rv2, act2, tree_o, _ = ora.mcts_search(obs, legal, tp, exploration=explore, rng_step=seed * 3,
                                                game_offset=100, temperature=temp, dump=True)
    _compare_trees(tree_g, tree_o, G)
    assert np.array_equal(cv, cv2)
    assert np.array_equal(rv, rv2)
    assert np.array_equal(act, act2)
    assert np.all(legal[np.arange(G), act - 1])
    np.testing.assert_allclose(cv.sum(1), 1.0, rtol=1e-6)
    eng.close()
    return tree_o


def _saturation_reached_the_tree(tree, G):
    """From the oracle's tree: every reward is ±1 exactly, and at least one game holds a run of nodes
    whose one backed-up value is the same ±1 exactly (a node visited once keeps the value of its
    simulation in W): MinMaxStats and the UCB scores meet runs of exactly equal values.

    A game in which EVERY backed-up value is equal — max == min at a normalisation — was looked for
    and does not exist under these nets.  In 80 oracle searches (seeds 1..40 of both cases, the
    mirror recording every value handed to backpropagate) no game qualified: the dynamics net's
    hidden states do not all saturate the value head.  And with two players max == min cannot be met
    at a normalisation at all: after the first simulation the statistics hold r + γv (leaf) and γr
    (root), equal only for v = r(γ - 1)/γ, and |v| = |r| = 1 here; the mirror counted 0
    normalisations with max == min against 1320 / 5100 with max > min per search."""
    N, W, R = tree["N"][:G], tree["W"][:G], tree["R"][:G]
    assert np.all(np.isin(R[N > 0], (-1.0, 1.0))), "a reward of a visited node is not saturated"
    runs = [int(np.sum(np.abs(W[g][N[g] == 1]) == 1.0)) for g in range(G)]
    assert max(runs) >= 5, runs


@pytest.mark.parametrize("kernel", KERNELS, ids=KIDS)
@pytest.mark.parametrize("S,G,explore,temp,seed", [(12, 20, True, 1.0, 1), (25, 17, False, 0.0, 2)])
@pytest.mark.parametrize("name", ["biased", "saturated"])
def test_search(ttt, nets, name, S, G, explore, temp, seed, kernel, monkeypatch):
    _force(monkeypatch, kernel)
    conf = dataclasses.replace(ttt.conf, num_iters=S)
    tree = _search_case(conf, ttt.hyper, wr.named(conf, ttt.hyper, nets, name), G, seed, explore, temp,
                        small=kernel[0] == "small")
    if name == "saturated":
        _saturation_reached_the_tree(tree, G)


def test_search_nonresident_kernel(ttt, nets, monkeypatch):
    monkeypatch.setenv("MZ_NO_RESIDENT", "1")
    _force(monkeypatch, ("tile16", None))
    conf = dataclasses.replace(ttt.conf, num_iters=25)
    _search_case(conf, ttt.hyper, wr.named(conf, ttt.hyper, nets, "biased"), 20, 21, True, 1.0)


def test_search_connect4(monkeypatch):
    monkeypatch.delenv("MZ_SEARCH_KERNEL", raising=False)
    monkeypatch.delenv("MZ_SMALL_T", raising=False)
    c4, r = _c4_nets()
    conf = dataclasses.replace(c4.conf, num_iters=12)
    _search_case(conf, c4.hyper, r, 6, 3, True, 1.0, A=7, feat=294)


# ------------------------------------------------------------------------------ ref_semantics learner
@pytest.mark.parametrize("kernel", [KERNELS[2], KERNELS[0]], ids=["small2", "tile16"])
@pytest.mark.parametrize("B", [32, 45])
@pytest.mark.parametrize("name", ["biased", "peaked"])
def test_learner_steps_then_search(ttt, nets, name, B, kernel, monkeypatch):
    """mz_learner_step x 6 against the oracle after every step (the bias ADAM state is nonzero from
    step 1), then a search on the engine against the oracle holding the stepped parameters: the
    search images received the updated biases."""
    from muzero_jl_amd.config import cos_schedule
    _force(monkeypatch, kernel)
    S, G = 12, 20
    conf = dataclasses.replace(ttt.conf, batch_size=B, num_iters=S)
    r = wr.named(conf, ttt.hyper, nets, name)
    eng, ora = _engine(conf, ttt.hyper, r, G), _oracle(conf, ttt.hyper, r)
    st = ora.learner_state()
    rng = np.random.default_rng(B)
    for t in range(1, 7):
        batch = _random_batch(B, conf.num_unroll_steps, 9, rng)
        eta = cos_schedule(t)
        want = ora.unroll(batch["observation"], batch["actions"])
        lg = eng.learner_step(batch, eta)
        lo = ora.learner_step(st, batch, eta)
        for g, o in zip(eng.debug_unroll(B), want):
            assert np.array_equal(g, o), f"step {t} unroll differs"
        assert np.all(np.isfinite(lo)) and np.array_equal(lg, lo), f"step {t} losses {lg} != oracle {lo}"
        for n in range(3):
            assert np.array_equal(eng.get_weights(n), ora.params[n]), f"step {t} net {n} params differ"
    assert np.all(wr.biases(conf, ttt.hyper, ora.params) != wr.biases(conf, ttt.hyper, r))
    obs, legal, tp = random_positions(G, 8)
    eng.debug_enable(1)
    out_g = eng.mcts_search(obs, legal, tp, exploration=True, rng_step=5, game_offset=50)
    tree_g = eng.debug_tree(G)
    if kernel[0] == "small":
        assert eng.search_variant().startswith("mz_search_small"), eng.search_variant()
    *out_o, tree_o, _ = ora.mcts_search(obs, legal, tp, exploration=True, rng_step=5, game_offset=50, dump=True)
    _compare_trees(tree_g, tree_o, G)
    for a, b in zip(out_g, out_o):
        assert np.array_equal(a, b)
    eng.close()


# ----------------------------------------------------------------------------- device-sampled learner
@pytest.mark.parametrize("kind,B,L", [("ttt", 40, 5), ("ttt", 32, 37), ("ttt-bn", 40, 5), ("ttt-bn", 32, 37)])
def test_multi_matches_sequential_steps(use_regime, kind, B, L):
    import test_learner_multi_gpu as m
    use_regime("biased")
    m.test_multi_matches_sequential_steps(kind, B, L)


def test_multi_matches_oracle_steps(use_regime):
    import test_learner_multi_gpu as m
    use_regime("biased")
    m.test_multi_matches_oracle_steps()


# ---------------------------------------------------------------------------------- corrected learner
@pytest.mark.parametrize("B,K,ir,per", [(20, 3, True, True), (32, 5, False, False)])
@pytest.mark.parametrize("name", ["biased", "peaked"])
def test_corrected_gradient_matches_torch(ttt, name, B, K, ir, per):
    """mz_backprop.hip against torch float64 autograd, by test_corrected_learner_gpu's measure and bar:
    each net's data gradient relative to its largest entry below 1e-5, losses and read-outs."""
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets, layer_specs
    from test_corrected_learner_gpu import _batch
    from torch_learner_ref import corrected_loss_and_grads
    conf = dataclasses.replace(ttt.conf, batch_size=B, num_unroll_steps=K, intermediate_rewards=ir)
    r = wr.named(conf, ttt.hyper, init_nets(conf, ttt.hyper, seed=B + K), name)
    eng = _engine(conf, ttt.hyper, r, 8, 1)
    eng.learner_set_mode(abi.LEARN_CORRECTED)
    rng = np.random.default_rng(B)
    batch = _batch(B, K, 9, 63, rng)
    wts = (rng.random(B).astype(np.float32) * 0.9 + 0.1) if per else None
    dev = [torch.from_numpy(np.ascontiguousarray(batch[k])).cuda() for k in
           ("observation", "actions", "target_values", "target_rewards", "target_policies", "gradient_scale")]
    dev.append(torch.from_numpy(wts).cuda() if per else None)
    grad = torch.zeros(eng.grad_count(), dtype=torch.float32, device="cuda")
    losses = torch.zeros(8, dtype=torch.float32, device="cuda")
    eng.learner_grad_dev([t.data_ptr() if t is not None else None for t in dev], B, grad.data_ptr(),
                         losses.data_ptr())
    eng.sync()
    ref = corrected_loss_and_grads(conf, ttt.hyper, r, batch, wts)
    g = grad.cpu().numpy()
    off = 0
    for n in range(3):
        gn = g[off: off + r[n].size].astype(np.float64)       # grad_dev holds the data term (2θ: apply)
        rn = ref["grads"][n] - 2.0 * r[n].astype(np.float64)
        off += r[n].size
        scale = np.abs(rn).max()
        assert scale > 1e-4, f"net {n}: no data gradient reached it"
        err = np.abs(gn - rn).max() / scale
        print(f"{name} B={B} K={K} net {n}: data gradient rel. error {err:.3g} (scale {scale:.3g})")
        assert err < 1e-5, f"net {n}: data gradient rel. error {err:.3g}"
        chains = [s[0] for s in layer_specs(conf, ttt.hyper, n)]
        for k, o, cnt in wr.bias_slices(conf, ttt.hyper, n):  # every bias layer has a gradient to get right
            if ir or (n, chains[k]) != (2, 2):                # (no reward loss: the reward head gets none)
                assert np.abs(rn[o:o + cnt]).max() > 0, (n, k)
    lo = losses.cpu().numpy()
    np.testing.assert_allclose([lo[0], lo[1], lo[2]], [ref["value"], ref["reward"], ref["policy"]],
                               rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(lo[3:6], ref["l2"], rtol=1e-5)
    pv, pp, pr = eng.debug_unroll(B)
    np.testing.assert_allclose(pv, ref["values"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pp, ref["policies"], rtol=1e-5, atol=1e-6)
    if ir:
        np.testing.assert_allclose(pr, ref["rewards"], rtol=1e-5, atol=1e-6)
    eng.close()


# ------------------------------------------------------------------------------------------ reanalyse
def test_reanalyse_values_saturated(use_regime):
    """mz_replay_reanalyse (the MFMA value refresh) on a shard that device self-play filled, saturated
    nets: every held game's values against mz_net_forward and against the oracle's forward."""
    import test_reanalyse_gpu as m
    from muzero_jl_amd.games import tictactoe as mod
    use_regime("saturated")
    from muzero_jl_amd.networks import init_nets               # (the regime's, as _selfplay_engines takes it)
    conf, (eng,) = m._selfplay_engines(1, G=16, cap=16, moves=12)
    ora = _oracle(conf, mod.hyper, init_nets(conf, mod.hyper, seed=105))
    held = eng.replay_counts()[1]
    assert held > 0
    eng.replay_reanalyse()
    assert eng.replay_reanalysed_count() == held
    hit = 0
    for i in range(held):
        h = eng.replay_get_game(i)
        x = m._stacked(conf, h)
        got = eng.replay_get_reanalysed(i)
        want = ora.forward(1, ora.forward(0, x))[0][:, 0]
        assert got is not None and np.array_equal(got, want), i
        assert np.array_equal(got, m._forward_values(eng, conf, h)), i
        hit += int(np.sum(np.abs(want) > 0.99))
    assert hit > 0                          # (oracle side) values far outside det_tanhf's polynomial were refreshed
    eng.close()


def test_reanalyse_search_biased(use_regime):
    import test_reanalyse_search_gpu as m
    use_regime("biased")
    m.test_matches_mcts_search("ttt")


# ------------------------------------------------------------------- self-play, train loop, arena
def test_device_selfplay_matches_host(use_regime):
    import test_selfplay_gpu as m
    use_regime("biased")
    m.test_device_selfplay_matches_host("ttt", 24, 13)


def test_train_loop_matches_oracle(use_regime, ttt):
    """The actors' and the queued images are written by the chain: now with biases in them."""
    import test_train_loop_gpu as m
    use_regime("biased")
    m.test_train_loop_matches_oracle(ttt, False, 9, 3)


def test_arena_opponent_set_holds_biases():
    """The second weight set's bias images have only ever held zeros: the learner's nets are init_nets
    (zero biases), the opponent's are biased — the device against the host driver with two engines."""
    import test_arena_gpu as m
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    name, G, mzp, moves = "tictactoe", 10, 1, 14
    conf, hyper = m._conf(name)
    opp = wr.named(conf, hyper, m._nets(name, 211), "biased")
    _, env_cls = m._mod(name)
    ea, eb, ed = m._engine(name, G, 105), m._engine(name, G, 105), m._engine(name, G, 105)
    for k, w in enumerate(opp):
        eb.set_weights(k, w)
    m._fill(ed, opp)
    for k in range(3):
        assert np.array_equal(ed.opponent_get_weights(k), opp[k]), k
    sp = BatchedSelfPlay(ea, env_cls, G, opponent="network", opponent_engine=eb, muzero_player=mzp, game_offset=7,
                         step0=100)
    ed.selfplay_init(m.ENV[name], G, 64)
    ed.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, mzp)
    trace = []
    for mv in range(moves):
        sp.play_move(0.0)
        ed.selfplay_move(100 + mv, game_offset=7, temperature=0.0)
        trace.append(ed.selfplay_slots())
        assert np.array_equal(trace[-1][1], sp.env.board.astype(np.uint8)), mv
    t = [0, 0, 0, 0]
    for h in sp.finished:
        w = game_winner(name, h.reward_history[-1], h.to_play_history[-1])
        t[0] += 1
        t[3 if w == 0 else 1 if w == mzp else 2] += 1
    assert t[0] > 0 and ed.eval_results() == tuple(t)
    ln, board, player = ed.selfplay_slots()
    assert np.array_equal(ln, [len(h.action_history) for h in sp.histories])
    assert np.array_equal(board, sp.env.board.astype(np.uint8)) and np.array_equal(player, sp.env.player)
    # the biases matter: the same opponent with its biases zeroed (init_nets(211)) plays another match
    m._fill(ed, m._nets(name, 211))
    other, _ = m._play(ed, name, G, abi.OPP_NETWORK, mzp, moves)
    assert not np.array_equal(m._boards(other), m._boards(trace))
    ea.close(); eb.close(); ed.close()


# ------------------------------------------------------------------------------------------- snapshot
def test_snapshot_exact_resume(use_regime, tmp_path, monkeypatch):
    import test_snapshot_gpu as m
    use_regime("biased")
    m.test_exact_resume_of_train_run("ttt_fc", tmp_path, monkeypatch)
