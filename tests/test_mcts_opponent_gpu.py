"""The rules-MCTS opponent on the device (mz_mcts_move): mz_mcts_eval
against the Python mirror (games/mcts_rules.py) bit for bit, evaluation play
with MZ_OPP_MCTS move for move against the host driver, the same through the
test worker with its record, exact resume from a snapshot, the refusals, and
that the setting changes nothing outside its mode."""
import dataclasses

import numpy as np
import pytest

import mcts_cases as mc
import worker_ref as wr

pytestmark = pytest.mark.gpu

ENV = {"tictactoe": 0, "connect4": 1}
SR = (16, 8)                                             # evaluation play's budget in these tests


def _mod(name):
    from muzero_jl_amd.games import connect4, tictactoe
    return (tictactoe, tictactoe.BatchedTicTacToe) if name == "tictactoe" else (connect4, connect4.BatchedConnect4)


def _engines(name, G, n=1, seed=mc.SEED, wseed=105, **kw):
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod, _ = _mod(name)
    kw.setdefault("num_iters", 6)
    conf = dataclasses.replace(mod.conf, replay_buffer_size=64, **kw)
    nets = init_nets(conf, mod.hyper, seed=wseed)
    out = []
    for _ in range(n):
        e = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=seed)
        for k, w in enumerate(nets):
            e.set_weights(k, w)
        out.append(e)
    return out


def _eval(eng, name, rows, S, R, rng_step=0, game_offset=0):
    boards = np.stack([b for b, _ in rows])
    players = np.array([p for _, p in rows], np.int32)
    return eng.mcts_eval(ENV[name], boards, players, S, R, rng_step=rng_step, game_offset=game_offset)


def _same(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, "nw"[k],
                                                                                    np.argwhere(g != w)[:4])


@pytest.mark.parametrize("name", mc.NAMES)
def test_mcts_eval_matches_mirror(name):
    """G = 1 and 5 at every setting (4 rows a workgroup, so 5 leaves three idle waves); G = 67 at
    (8, 4): a partial last workgroup."""
    (eng,) = _engines(name, 4)
    pos = mc.positions(name)
    for rows in (pos[2:3], pos[-5:]):
        for S, R in mc.SETTINGS:
            _same(_eval(eng, name, rows, S, R, rng_step=9, game_offset=4),
                  mc.mirror_rows(name, rows, S, R, game_offset=4, rng_step=9), (len(rows), S, R))
    rows = mc.random_positions(name)[:67]
    _same(_eval(eng, name, rows, 8, 4, rng_step=2), mc.mirror_rows(name, rows, 8, 4, rng_step=2), (67, 8, 4))
    eng.close()


def test_mcts_eval_largest_tree():
    """(1024, 64) on the empty TicTacToe board: the largest tree, one row per workgroup, every lane a rollout."""
    (eng,) = _engines("tictactoe", 4)
    rows = (mc.xc.TTT_EMPTY,)
    got = _eval(eng, "tictactoe", rows, 1024, 64, rng_step=1, game_offset=3)
    _same(got, mc.mirror_rows("tictactoe", rows, 1024, 64, game_offset=3, rng_step=1), "largest")
    assert got[0].sum() == 1024
    eng.close()


@pytest.mark.parametrize("S,rows_per_block", [(450, 3), (600, 2)])
def test_mcts_eval_fewer_rows_per_workgroup(S, rows_per_block):
    """TicTacToe trees of which three and two fit a workgroup's LDS: G = 4 leaves a partial last workgroup."""
    assert min(4, 160 * 1024 // ((S + 1) * 9 * 12)) == rows_per_block
    (eng,) = _engines("tictactoe", 4)
    rows = mc.positions("tictactoe")[:3] + (mc.xc.TTT_EMPTY,)
    _same(_eval(eng, "tictactoe", rows, S, 2, rng_step=4, game_offset=1),
          mc.mirror_rows("tictactoe", rows, S, 2, game_offset=1, rng_step=4), ("rows per block", S))
    eng.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_mcts_eval_keys_reach_the_rollouts(name):
    """Two (game_offset, rng_step) pairs: each equals its own mirror, and they differ from each other."""
    (eng,) = _engines(name, 4)
    rows = mc.positions(name)[:3]
    a = _eval(eng, name, rows, 64, 16, rng_step=5, game_offset=0)
    b = _eval(eng, name, rows, 64, 16, rng_step=6, game_offset=100)
    _same(a, mc.mirror_rows(name, rows, 64, 16, game_offset=0, rng_step=5), "keys a")
    _same(b, mc.mirror_rows(name, rows, 64, 16, game_offset=100, rng_step=6), "keys b")
    assert not np.array_equal(a[1], b[1])
    eng.close()


CASES = [("tictactoe", 5, 1, 14), ("tictactoe", 5, 2, 14), ("connect4", 3, 1, 30), ("connect4", 3, 2, 30)]


@pytest.mark.parametrize("name,G,mzp,moves", CASES)
def test_mcts_evaluation_play_matches_host(name, G, mzp, moves):
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    _, env_cls = _mod(name)
    eh, ed = _engines(name, G, n=2)
    sp = BatchedSelfPlay(eh, env_cls, G, game_offset=7, step0=100, opponent="mcts", muzero_player=mzp,
                         mcts_sims=SR[0], mcts_rollouts=SR[1])
    ed.selfplay_init(ENV[name], G, 64)
    ed.mcts_opponent(*SR)
    ed.selfplay_mode(abi.SP_EVAL, abi.OPP_MCTS, mzp)
    for m in range(moves):
        sp.play_move(0.0)
        ed.selfplay_move(100 + m, game_offset=7, temperature=0.0)
        ln, board, player = ed.selfplay_slots()
        assert np.array_equal(ln, [len(h.action_history) for h in sp.histories]), m
        assert np.array_equal(board, sp.env.board.astype(np.uint8)) and np.array_equal(player, sp.env.player), m
    t = [0, 0, 0, 0]
    for h in sp.finished:
        w = game_winner(name, h.reward_history[-1], h.to_play_history[-1])
        t[0] += 1
        t[3 if w == 0 else 1 if w == mzp else 2] += 1
    assert t[0] > 0 and ed.eval_results() == tuple(t)
    assert ed.replay_counts()[0][0] == 0                      # evaluation play saves nothing
    eh.close(); ed.close()


@pytest.mark.parametrize("name,E,mzp", [(n, g, p) for n, g, p, _ in CASES])
def test_mcts_through_the_test_worker(name, E, mzp):
    """mz_test_play with MZ_OPP_MCTS: every slot's game and the record against evaluate / evaluation_record."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import evaluate
    _, env_cls = _mod(name)
    kw = dict(num_iters=4) if name == "connect4" else dict(num_iters=wr.SIMS, max_moves=wr.MAX_MOVES)
    eh, ed = _engines(name, E, n=2, **kw)
    ed.selfplay_init(ENV[name], E, E)
    ed.mcts_opponent(*SR)
    ed.test_config(E, abi.OPP_MCTS, mzp)
    hs, want = evaluate(eh, env_cls, E, opponent="mcts", muzero_player=mzp, rng_step0=300, game_offset=11,
                        temperature=1.0, training_step=17, mcts_sims=SR[0], mcts_rollouts=SR[1])
    ed.test_play(17, 300, game_offset=11, temperature=1.0)
    total, recs = ed.test_results(max_records=1)
    assert total == 1 and len(recs) == 1
    print(name, mzp, "device", recs[0], "mirror", want)
    for g in range(E):
        assert wr.same_history(ed.test_get_game(g), hs[g]), (name, mzp, g)
    assert wr.same_record(recs[0], want), (recs[0], want)
    assert want["games"] == E and want["value_moves"] < want["moves"]
    eh.close(); ed.close()


def test_mcts_eval_run_resumes_from_snapshot(tmp_path):
    from muzero_jl_amd import abi
    G, cap = 6, 12

    def start(wseed=17, cap=cap):
        (e,) = _engines("tictactoe", G, wseed=wseed)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        e.mcts_opponent(*SR)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_MCTS, 2)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(10 + m, 3, temperature=0.0)

    uncut = start()
    drive(uncut, 0, 24)
    first = start()
    drive(first, 0, 12)
    at_cut = first.eval_results()
    snap = str(tmp_path / "mcts.safetensors")
    first.snapshot_save(snap, 0)
    first.close()
    second = start(wseed=99, cap=cap + 5)                     # other weights, another shard size, other moves
    drive(second, 40, 45)
    second.snapshot_load(snap)                                # keeps the handle's (S, R)
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_MCTS, 2)
    assert second.eval_results() == at_cut and at_cut[0] > 0
    drive(second, 12, 24)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    for a, b in zip(uncut.selfplay_slots(), second.selfplay_slots()):
        assert np.array_equal(a, b)
    uncut.close(); second.close()


def test_mcts_refusals():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth
    from muzero_jl_amd.networks import init_nets
    (e,) = _engines("tictactoe", 4)
    b, p = mc.xc.TTT_EMPTY
    n, w = e.mcts_eval(abi.ENV_TICTACTOE, b, [p], 9, 1)       # needs no selfplay_init
    assert n.sum() == 9 and n.min() >= 0 and (abs(w) <= n).all()
    for s, r in ((-1, 0), (1025, 0), (0, -1), (0, 65)):
        with pytest.raises(abi.MzError, match="mcts opponent: (sims|rollouts) must be in"):
            e.mcts_opponent(s, r)
    e.mcts_opponent(0, 0)
    e.mcts_opponent(1024, 64)
    for s, r in ((0, 1), (1025, 1), (1, 0), (1, 65)):
        with pytest.raises(abi.MzError, match="mcts opponent: (sims|rollouts) must be in"):
            e.mcts_eval(abi.ENV_TICTACTOE, b, [p], s, r)
    for bad in mc.xc.bad_boards("tictactoe"):
        with pytest.raises(abi.MzError, match="exactly one plane"):
            e.mcts_eval(abi.ENV_TICTACTOE, bad, [1], 4, 2)
    for bad_p in (0, 3):
        with pytest.raises(abi.MzError, match="player"):
            e.mcts_eval(abi.ENV_TICTACTOE, b, [bad_p], 4, 2)
    with pytest.raises(abi.MzError, match="Connect4 needs"):  # the shape check of mz_selfplay_init
        e.mcts_eval(abi.ENV_CONNECT4, mc.xc.C4_WIN[0], [1], 4, 2)
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    for opp in (5, -1):
        with pytest.raises(abi.MzError, match="opponent must be"):
            e.selfplay_mode(abi.SP_EVAL, opp, 1)
        with pytest.raises(abi.MzError, match="opponent must be"):
            e.test_config(2, opp, 1)
    e.selfplay_mode(abi.SP_EVAL, abi.OPP_MCTS, 1)
    e.test_config(2, abi.OPP_MCTS, 2)
    e.close()
    conf = dataclasses.replace(atari_synth.conf, num_iters=2, max_moves=6, batch_size=4)
    a = abi.Engine(conf, atari_synth.resnet_hyper, device=0, max_games=4, rng_seed=5)
    for k, w in enumerate(init_nets(conf, atari_synth.resnet_hyper, seed=17)):
        a.set_weights(k, w)
    a.selfplay_init(abi.ENV_ATARI, 4, 8)
    with pytest.raises(abi.MzError, match="mcts opponent: needs a two-player board env"):
        a.selfplay_mode(abi.SP_EVAL, abi.OPP_MCTS, 1)
    with pytest.raises(abi.MzError, match="mcts opponent: needs a two-player board env"):
        a.test_config(2, abi.OPP_MCTS, 1)
    with pytest.raises(abi.MzError, match="mcts opponent: needs a two-player board env"):
        a.mcts_eval(abi.ENV_ATARI, np.zeros((1, 27), np.uint8), [1], 4, 2)
    a.close()


@pytest.mark.parametrize("mode", ["train", "random"])
def test_mcts_setting_changes_nothing_outside_its_mode(mode):
    """A TRAIN-mode run and an MZ_OPP_RANDOM evaluation: the same games with mz_mcts_opponent set and unset."""
    from muzero_jl_amd import abi
    G = 5
    plain, tuned = _engines("tictactoe", G, n=2)
    tuned.mcts_opponent(32, 4)
    for e in (plain, tuned):
        e.selfplay_init(abi.ENV_TICTACTOE, G, 64)
        if mode == "random":
            e.selfplay_mode(abi.SP_EVAL, abi.OPP_RANDOM, 2)
    for m in range(14):
        for e in (plain, tuned):
            e.selfplay_move(50 + m, game_offset=2, temperature=1.0 if mode == "train" else 0.0)
        for x, y in zip(plain.selfplay_slots(), tuned.selfplay_slots()):
            assert np.array_equal(x, y), m
    if mode == "random":
        assert plain.eval_results() == tuned.eval_results() and plain.eval_results()[0] > 0
    else:
        (counts, held), (counts2, held2) = plain.replay_counts(), tuned.replay_counts()
        assert held == held2 and held > 0 and np.array_equal(counts, counts2)
        for i in range(held):
            assert wr.same_history(plain.replay_get_game(i), tuned.replay_get_game(i)), i
    plain.close(); tuned.close()
