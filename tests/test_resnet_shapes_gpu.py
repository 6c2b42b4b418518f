"""GPU half of the ResNet shape matrix (tests/resnet_shapes.py): the kernels of
csrc/mz_resnet.hip at shapes off the three presets, against the CPU oracle bit
for bit (np.array_equal: the kernels run the oracle's f32 operations in the
oracle's order, so no case has a tolerance) — the forward of all three nets at
n = 1 and n = 19 (a partly filled last tile for every tile width), a 6-simulation
search of 5 games (trees, child visits, root values, actions; masks with a
single legal action and, for A > 16, legal actions above 16 only), and three
ref_semantics learner steps (unroll read-outs, losses, θ of all three nets),
with the search and unroll launch forms asserted by name (resnet_shapes.
LEARNER_VARIANT).  This runs mz_runroll_chain_r+mz_runroll_pred_n1 (fh64) and
mz_runroll_chain_r+mz_runroll_pred_r (k63) and mz_runroll_chain1+mz_runroll_pred_r
(wh5780), which no other test launches, and compares
mz_runroll_chain1+mz_runroll_pred_n1 exactly.  Then the multi-step
learner against single steps (fh64, on a shard of stored random games) and the
corrected gradient against torch autograd (nf24, k53) with the comparison of
test_corrected_resnet_gpu; and the one shape of the matrix's neighbourhood the
engine refuses by design (a k table past the layer entry's 16-bit LDS offset).

Reference: src/Learning.jl:148-255, :327-404; src/SelfPlay.jl:225-283."""
import dataclasses

import numpy as np
import pytest

import resnet_shapes as rs
from test_gpu_parity import _compare_trees

pytestmark = pytest.mark.gpu


def _engine(cid, conf=None, max_games=8, seed=7):
    from muzero_jl_amd import abi
    c, hyper = rs.cases()[cid]
    eng = abi.Engine(conf or c, hyper, device=0, max_games=max_games, rng_seed=seed)
    for n, w in enumerate(rs.lively_nets(cid)):
        eng.set_weights(n, w)
    ng = eng.resnet_tile_games()
    assert ng in (1, 2, 4, 8, 16) and ng == rs.TILE_GAMES.get(cid, ng), ng
    print(f"{cid}: rn_ng = {ng}")
    return eng


@pytest.mark.parametrize("cid", rs.FULL_IDS)
def test_shape_forward_bitexact(cid):
    conf, hyper = rs.cases()[cid]
    o, eng = rs.oracle(cid), _engine(cid, max_games=32)
    try:
        for n in (1, 19):
            for net in range(3):
                x = rs.net_input(conf, hyper, net, n, 100 * net + n)
                want, got = o.forward(net, x), eng.forward(net, x)
                if net == 0:
                    assert np.array_equal(got, want), (net, n)
                else:
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (net, n)
    finally:
        eng.close()


@pytest.mark.parametrize("cid", rs.FULL_IDS)
def test_shape_search_bitexact(cid):
    conf, _ = rs.cases()[cid]
    G = rs.SEARCH_G
    o, eng = rs.oracle(cid), _engine(cid, max_games=G)
    try:
        obs, legal, tp = rs.search_inputs(conf, G, 40 + rs.IDS.index(cid))
        eng.debug_enable(1)
        cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=True, rng_step=21, game_offset=11, temperature=1.0)
        assert eng.search_variant() == rs.SEARCH_VARIANT
        tree_g = eng.debug_tree(G)
        cv2, rv2, act2, tree_o, _ = o.mcts_search(obs, legal, tp, exploration=True, rng_step=21, game_offset=11,
                                                  temperature=1.0, dump=True)
        assert np.all(legal[np.arange(G), act - 1]), "an illegal action was chosen"
        _compare_trees(tree_g, tree_o, G)
        assert np.array_equal(cv, cv2) and np.array_equal(rv, rv2) and np.array_equal(act, act2)
    finally:
        eng.close()


@pytest.mark.parametrize("cid", rs.IDS)
def test_shape_learner_steps(cid):
    from muzero_jl_amd.config import cos_schedule
    conf, _ = rs.cases()[cid]
    B = conf.batch_size
    o, eng = rs.oracle(cid), _engine(cid)
    try:
        st = o.learner_state()
        rng = np.random.default_rng(rs.IDS.index(cid))
        for t in range(1, 4):
            batch = rs.random_batch(conf, rng)
            eta = cos_schedule(t)
            want = o.unroll(batch["observation"], batch["actions"])
            lg = eng.learner_step(batch, eta)
            lo = o.learner_step(st, batch, eta)
            assert eng.learner_variant() == rs.LEARNER_VARIANT[cid], eng.learner_variant()
            for g, w in zip(eng.debug_unroll(B), want):
                assert np.array_equal(g, w), f"step {t} unroll differs"
            assert np.array_equal(lg, lo), f"step {t} losses {lg} != oracle {lo}"
            for n in range(3):
                assert np.array_equal(eng.get_weights(n), o.params[n]), f"step {t} net {n} params differ"
    finally:
        eng.close()


def test_shape_refused_k_table_offset():
    """A plan that fits the LDS only with a k table past LDS offset 32767 is refused at create, with
    a message, instead of running with a truncated offset."""
    from muzero_jl_amd import abi
    conf, hyper = rs.refused_case()
    with pytest.raises(abi.MzError, match="32767"):
        abi.Engine(conf, hyper, device=0, max_games=8, rng_seed=7).close()


def _random_game(conf, rng):
    """A stored game of random moves: 0/1 observation planes, visit distributions, values."""
    from muzero_jl_amd.selfplay import GameHistory
    A, osz = len(conf.action_space), int(np.prod(conf.observation_shape))
    T = int(rng.integers(3, conf.max_moves + 1))
    cv = rng.random((T, A)).astype(np.float32)
    cv /= cv.sum(1, keepdims=True)
    return GameHistory(observation_history=[(rng.random(osz) < 0.4).astype(np.float32) for _ in range(T)],
                       action_history=[int(a) for a in rng.integers(1, A + 1, T)],
                       reward_history=[float(r) for r in rng.uniform(-1, 1, T).astype(np.float32)],
                       to_play_history=[1 + (m % 2) for m in range(T)], child_visits=list(cv),
                       root_values=[float(v) for v in rng.uniform(-1, 1, T).astype(np.float32)])


def test_shape_multi_matches_sequential_steps():
    """mz_learner_train_multi_dev, L = 3, against three single steps on a second engine with the same
    shard, as test_learner_multi_gpu.test_multi_matches_sequential_steps, for fh64 (chain_r + pred_n1
    with the steps on gridDim.z).  The shard holds random games stored with mz_replay_save_game.
    The shard needs mz_selfplay_init, which takes the three environments' boards only, so nf24
    (a 5x4x2 board) has no such path and no multi-step case."""
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.config import cos_schedule
    cid, L, cap = "fh64", 3, 16
    conf = dataclasses.replace(rs.cases()[cid][0], replay_buffer_size=cap)
    B = conf.batch_size
    e1, e2 = _engine(cid, conf, max_games=cap), _engine(cid, conf, max_games=cap)
    try:
        rng = np.random.default_rng(5)
        games = [_random_game(conf, rng) for _ in range(cap)]
        for e in (e1, e2):
            e.selfplay_init(abi.ENV_TICTACTOE, cap, cap)
            for g in games:
                e.replay_save_game(g)
        nflat = sum(e1.param_count(n) for n in range(3))
        l1 = torch.zeros(8, dtype=torch.float32, device="cuda")
        lm = torch.zeros((L, 8), dtype=torch.float32, device="cuda")
        th = torch.zeros((L, nflat), dtype=torch.float32, device="cuda")
        etas = [cos_schedule(1 + i) for i in range(L)]
        want = []
        for i in range(L):
            e1.learner_train_dev(B, 1 + i, etas[i], l1.data_ptr())
            e1.sync()
            assert e1.learner_variant() == rs.LEARNER_VARIANT[cid], e1.learner_variant()
            want.append((l1.cpu().numpy()[:6].copy(), np.concatenate([e1.get_weights(n) for n in range(3)]),
                         [x.copy() for x in e1.debug_unroll(B)]))
        e2.learner_train_multi_dev(B, 1, etas, lm.data_ptr(), th.data_ptr())
        e2.sync()
        assert e2.learner_variant() == f"mz_learn_chain+{rs.LEARNER_VARIANT[cid]}+mz_learner_loss_multi", \
            e2.learner_variant()
        got_l, got_t = lm.cpu().numpy(), th.cpu().numpy()
        for i, (wl, wt, wu) in enumerate(want):
            assert np.array_equal(got_l[i, :6], wl), (i, got_l[i, :6], wl)
            assert np.array_equal(got_t[i], wt), (i, "theta")
            for g, w in zip(e2.debug_unroll_step(i, B), wu):
                assert np.array_equal(g, w), (i, "read-outs")
        assert not np.array_equal(want[0][1], want[-1][1])
    finally:
        e1.close(); e2.close()


@pytest.mark.parametrize("cid", ["nf24", "k53"])
def test_shape_corrected_gradient_matches_torch(cid):
    """mz_rbp_sample / mz_rbp_dw at a partial row block with two column blocks (nf24) and through
    the non-square kernel's taps (k53), B = 4, K = 2: the comparison and tolerances of
    test_corrected_resnet_gradient_matches_torch."""
    from test_corrected_resnet_gpu import _corrected_against_torch
    conf, hyper = rs.cases()[cid]
    conf = dataclasses.replace(conf, batch_size=4, num_unroll_steps=2, intermediate_rewards=True)
    _corrected_against_torch(conf, hyper, B=4, K=2, ir=True, per=True)
