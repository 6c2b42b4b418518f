"""Judging MuZero's moves in the test worker (mz_test_audit, mz_expert_judge,
DESIGN §20.1): the judge mode of the search kernel on given positions against
the mirror's rule, and the audit row of an evaluation against
selfplay.evaluation_audit over the games read back, with the solved table on
and off, next to records and games that judging leaves bit-identical; the
audit ring beside the record ring, the refusals, and a train_run job that is
the same job with judging on and off."""
import numpy as np
import pytest

import expert_cases as xc
import worker_ref as wr

pytestmark = pytest.mark.gpu

ENV = {"tictactoe": 0, "connect4": 1}
OFF_ROW = [-1, 0, 0, 0]                                        # an evaluation run with judging off


def _tw():
    import test_test_worker_gpu as tw
    return tw


def _moves(name, seed=1):
    """expert_cases' random positions, each with a random legal action (1-based)."""
    rng = np.random.default_rng(seed)
    pos = xc.random_positions(name)
    cells = 9 if name == "tictactoe" else 42
    acts = []
    for b, _ in pos:
        if name == "tictactoe":
            legal = np.flatnonzero(b[2 * cells:])
        else:                                                  # a column whose top cell (w = 5) is empty
            legal = np.flatnonzero(b[2 * cells:].reshape(7, 6)[:, 5])
        acts.append(int(rng.choice(legal)) + 1)
    return pos, np.array(acts, np.int32)


@pytest.mark.parametrize("name,depths", [("tictactoe", (9, 3)), ("connect4", (2, 4))])
def test_expert_judge_matches_the_rule(name, depths):
    import test_expert_gpu as xg
    from muzero_jl_amd import abi
    from muzero_jl_amd.games.expert import expert_scores, judge_move
    (e,) = xg._engines(name, 4)
    pos, acts = _moves(name)
    for d in depths:
        terms = np.array([judge_move(expert_scores(name, b, p, d), a) for (b, p), a in zip(pos[:67], acts[:67])])
        for G in (1, 5, 67):
            boards = np.stack([b for b, _ in pos[:G]])
            players = np.array([p for _, p in pos[:G]], np.int32)
            got = e.expert_judge(ENV[name], boards, players, acts[:G], d)
            assert got == tuple(int(x) for x in terms[:G].sum(0)), (name, d, G, got)
        if d == depths[0]:
            assert 0 < terms[:, 1].sum() < 67 and terms[:, 2].sum() > 0 and terms[:, 3].sum() > 0   # not vacuous
        # the expert's own picks are never faulted
        boards = np.stack([b for b, _ in pos[:67]])
        players = np.array([p for _, p in pos[:67]], np.int32)
        best = e.expert_eval(ENV[name], boards, players, d).argmax(1) + 1
        assert e.expert_judge(ENV[name], boards, players, best, d) == (67, 67, 0, 0)
    b, p = pos[3]
    taken = int(np.flatnonzero(b[:18])[0] % 9) + 1 if name == "tictactoe" else 0
    for bad in (taken, 0, 10 if name == "tictactoe" else 8):
        with pytest.raises(abi.MzError, match="action not legal on its board"):
            e.expert_judge(ENV[name], b, [p], [bad], depths[0])
    with pytest.raises(abi.MzError, match="depth"):
        e.expert_judge(ENV[name], b, [p], [int(acts[3])], 0)
    with pytest.raises(abi.MzError, match="player"):
        e.expert_judge(ENV[name], b, [3], [int(acts[3])], 2)
    e.close()


def _evaluate(e, E, env_name, opponent, mzp, depth, key):
    """One evaluation; (record, games, audit row, the mirror's audit of those games)."""
    from muzero_jl_amd.selfplay import evaluation_audit
    tstep, s0, goff, temp = key
    e.test_play(tstep, s0, game_offset=goff, temperature=temp)
    (rec,) = e.test_results(1)[1]
    games = [e.test_get_game(g) for g in range(E)]
    total, rows = e.test_audit_results(1)
    assert total == e.test_results(0)[0] and rows.shape == (1, 4) and rows.dtype == np.int64
    return rec, games, rows[0].tolist(), list(evaluation_audit(games, env_name, opponent, mzp, depth))


def _check_judging(e, E, env_name, opponent, mzp, depth, key, table):
    """Judging off, on, and (TicTacToe at depth 9) on with the solved table: the same record and games
    each time, the audit row = the mirror's rule over those games."""
    e.test_audit(False)
    rec0, games0, row0, want = _evaluate(e, E, env_name, opponent, mzp, depth, key)
    assert row0 == OFF_ROW
    rows = []
    for tab in ((False, True) if table else (False,)):
        e.test_audit(True)
        if table:
            e.expert_table(tab)
            assert e.expert_table_get(scores=False)[2] == tab
        rec, games, row, want2 = _evaluate(e, E, env_name, opponent, mzp, depth, key)
        print(env_name, opponent, mzp, "table", tab, "audit", row, "mirror", want2)
        assert wr.same_record(rec, rec0), (rec, rec0)
        assert all(wr.same_history(a, b) for a, b in zip(games, games0))
        assert row == want2 == want, (tab, row, want)
        rows.append(row)
    if table:
        e.expert_table(False)
    every = opponent == "self"
    n = sum(sum(1 for tp in g.to_play_history if every or tp == mzp) for g in games0)
    assert rows[0][0] == n > 0 and 0 <= rows[0][1] <= n and 0 <= rows[0][2] <= n - rows[0][1]
    return rows[0]


@pytest.fixture(scope="module")
def ttt_engine():
    tw = _tw()
    e = tw._engine("ttt", 8, num_iters=wr.SIMS, max_moves=wr.MAX_MOVES)
    e.selfplay_init(tw._game("ttt")[2], 8, 16)
    yield e
    e.close()


@pytest.mark.parametrize("opponent,mzp", wr.CONFIGS)
def test_tictactoe_audit_matches_the_mirror(ttt_engine, opponent, mzp):
    e = ttt_engine
    e.test_config(wr.E, _tw().OPP[opponent], mzp)
    _check_judging(e, wr.E, "tictactoe", opponent, mzp, None, (3, wr.STEP0, wr.GOFF, wr.TEMP), table=True)


def test_audit_with_a_temperature_threshold():
    tw = _tw()
    e = tw._engine("ttt", 8, num_iters=wr.SIMS, max_moves=wr.MAX_MOVES, temperature_threshold=3)
    e.selfplay_init(tw._game("ttt")[2], 2, 4)
    e.test_config(7, tw.OPP["random"], 2)
    _check_judging(e, 7, "tictactoe", "random", 2, None, (1, wr.STEP0, wr.GOFF, wr.TEMP), table=True)
    e.expert_depth(4)                                          # another depth: the search kernel judges, table or not
    e.expert_table(True)
    assert not e.expert_table_get(scores=False)[2]
    _check_judging(e, 7, "tictactoe", "random", 2, 4, (1, wr.STEP0, wr.GOFF, wr.TEMP), table=False)
    e.close()


def test_connect4_audit_with_the_expert():
    tw = _tw()
    E = 6
    e = tw._engine("c4", E, num_iters=4)
    e.selfplay_init(tw._game("c4")[2], E, E)
    e.expert_depth(2)
    e.test_config(E, tw.OPP["expert"], 2)
    _check_judging(e, E, "connect4", "expert", 2, 2, (17, 300, 11, 1.0), table=False)
    e.close()


def test_resnet_audit_against_a_second_weight_set():
    from muzero_jl_amd.networks import init_nets
    tw = _tw()
    E = 5
    e = tw._engine("ttt", E, resnet=True, num_iters=4, max_moves=wr.MAX_MOVES)
    e.selfplay_init(tw._game("ttt")[2], E, E)
    for k, w in enumerate(init_nets(e.conf, e.hyper, seed=211)):
        e.opponent_set_weights(k, w)
    e.test_config(E, tw.OPP["network"], 1)
    _check_judging(e, E, "tictactoe", "network", 1, None, (5, wr.STEP0, wr.GOFF, 1.0), table=True)
    e.close()


def test_audit_ring_beside_the_records(ttt_engine):
    from muzero_jl_amd import abi
    e = ttt_engine
    e.test_clear()
    assert e.test_audit_results()[0] == 0 and e.test_audit_results()[1].shape == (0, 4)
    e.test_config(wr.E, abi.OPP_RANDOM, 2)
    keys = [(10, wr.STEP0, wr.GOFF, wr.TEMP), (11, wr.STEP0 + 50, wr.GOFF + 3, wr.TEMP), (12, wr.STEP0 + 90, 1, wr.TEMP)]
    want = []
    for i, key in enumerate(keys):                             # judged, not judged, judged
        e.test_audit(i != 1)
        _, _, row, mirror = _evaluate(e, wr.E, "tictactoe", "random", 2, None, key)
        assert row == (mirror if i != 1 else OFF_ROW)
        want.append(row)
    total, rows = e.test_audit_results()
    assert total == 3 and rows.tolist() == want
    assert [r["training_step"] for r in e.test_results()[1]] == [10, 11, 12]
    assert e.test_audit_results(2)[1].tolist() == want[1:]
    e.test_clear()
    assert e.test_audit_results()[0] == 0 and e.test_results() == (0, [])
    e.test_audit(False)
    e.test_play(0, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    assert e.test_audit_results()[1].tolist() == [OFF_ROW]    # the cleared ring forgot the old rows
    e.test_clear()


def test_more_evaluations_than_the_ring_holds():
    """E = 1, T = 3: 1026 evaluations, every fifth one with judging off."""
    from muzero_jl_amd import abi
    tw = _tw()
    e = tw._engine("ttt", 4, num_iters=4, max_moves=2)
    e.selfplay_init(abi.ENV_TICTACTOE, 1, 2)
    e.test_config(1, abi.OPP_SELF, 1)
    e.expert_table(True)
    n = abi.TEST_RECORDS + 2
    for i in range(n):
        e.test_audit(i % 5 != 0)
        e.test_play(i, wr.STEP0 + i, game_offset=wr.GOFF, temperature=wr.TEMP)
    total, rows = e.test_audit_results()
    _, recs = e.test_results()
    assert total == n and rows.shape == (abi.TEST_RECORDS, 4)
    assert [r["training_step"] for r in recs] == list(range(2, n))
    for r, row in zip(recs, rows.tolist()):
        if r["training_step"] % 5 == 0:
            assert row == OFF_ROW
        else:                                                  # three moves, all MuZero's, all judged
            assert row[0] == r["moves"] == 3 and 0 <= row[1] <= 3
    assert len({tuple(r) for r in rows.tolist()}) > 2         # the evaluations differ
    e.test_audit(True)
    _, _, row, mirror = _evaluate(e, 1, "tictactoe", "self", 1, None, (7, wr.STEP0 + 7, wr.GOFF, wr.TEMP))
    assert row == mirror == rows[7 - 2].tolist()
    e.close()


def test_audit_refused_on_the_atari_like_env():
    from muzero_jl_amd import abi
    tw = _tw()
    a = tw._engine("atari", 4, num_iters=2, max_moves=6)
    a.test_audit(True)                                         # no env yet: stored ...
    a.selfplay_init(abi.ENV_ATARI, 4, 4)
    a.test_config(4, abi.OPP_SELF, 1)
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        a.test_play(0, 100, game_offset=7)                     # ... and checked again by the evaluation
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        a.test_audit(True)
    a.test_audit(False)
    a.test_play(0, 100, game_offset=7)
    assert a.test_audit_results()[1].tolist() == [OFF_ROW]
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        a.expert_judge(abi.ENV_ATARI, np.zeros((1, 27), np.uint8), [1], [1], 3)
    a.close()


def test_train_run_with_judging_on_and_off(tmp_path):
    """The 24-move job of the test-worker test with the worker on, on two engines: judging on and off.
    Every public read-out and every record is equal; the audit rows are those of explicit test_play
    calls on a third engine that is given the learner's weights of that moment."""
    import test_snapshot_gpu as snap
    from muzero_jl_amd import abi
    tw = _tw()
    T, E = 10, 5
    on, off = tw._train_engine(False), tw._train_engine(False)
    third = tw._engine("ttt", 16, wseed=99, num_iters=8)
    third.selfplay_init(abi.ENV_TICTACTOE, 4, 4)
    for e in (on, off, third):
        e.test_config(E, abi.OPP_RANDOM, 2)
    for e in (on, off):
        e.train_set_test(tw.INTERVAL, tw.TEST_GOFF, tw.TEST_TEMP)
    on.test_audit(True)
    on.expert_table(True)
    third.test_audit(True)                                     # the third judges with the search kernel
    t0, crossed = 0, []
    for m in range(tw.MOVES):
        s_on = on.train_run(1, move0=tw.MOVE0 + m, game_offset=tw.GOFF_TR)
        s_off = off.train_run(1, move0=tw.MOVE0 + m, game_offset=tw.GOFF_TR)
        assert s_on == s_off, m
        t1 = s_off[0]
        if t1 // tw.INTERVAL > t0 // tw.INTERVAL:
            crossed.append(t1)
            for k in range(3):
                third.set_weights(k, off.train_weights(abi.TRAIN_LEARNER, k))
            third.test_play(t1, (t1 * T) & 0xffffffff, game_offset=tw.TEST_GOFF, temperature=tw.TEST_TEMP)
        t0 = t1
    assert len(crossed) >= 3
    snap._same(snap._readout(on, tmp_path, "on"), snap._readout(off, tmp_path, "off"))
    (total, recs), (total_off, recs_off) = on.test_results(), off.test_results()
    assert total == total_off == len(crossed) and [r["training_step"] for r in recs] == crossed
    assert all(wr.same_record(a, b) for a, b in zip(recs, recs_off))
    for g in range(E):
        assert wr.same_history(on.test_get_game(g), off.test_get_game(g)), g
    rows, rows3 = on.test_audit_results()[1].tolist(), third.test_audit_results()[1].tolist()
    assert rows == rows3 and len(rows) == len(crossed) and all(r[0] > 0 for r in rows)
    assert off.test_audit_results()[1].tolist() == [OFF_ROW] * len(crossed)
    on.close(); off.close(); third.close()
