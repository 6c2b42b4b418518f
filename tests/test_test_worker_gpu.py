"""The test worker on the device (mz_test_*, mz_train_set_test), bit
for bit: every slot's game and the evaluation's record against the host mirror
(BatchedSelfPlay.play_games + selfplay.evaluation_record), against today's
evaluation mode on a second engine, consecutive evaluations and the record
ring, a train_run job that is the same job with and without the worker, the
loop's records against explicit test_play calls, the refusals and the lifetime
of slots, settings and records.  E = 5, 6 and 4 leave idle waves in the last
workgroup of the one-wave-per-slot kernels."""
import dataclasses

import numpy as np
import pytest

import worker_ref as wr

pytestmark = pytest.mark.gpu

OPP = {"self": 0, "random": 1, "expert": 2, "network": 3}


def _game(name):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth, connect4, tictactoe
    return {"ttt": (tictactoe, tictactoe.BatchedTicTacToe, abi.ENV_TICTACTOE),
            "c4": (connect4, connect4.BatchedConnect4, abi.ENV_CONNECT4),
            "atari": (atari_synth, atari_synth.BatchedAtariSynth, abi.ENV_ATARI)}[name]


def _engine(name, max_games, wseed=wr.WSEED, resnet=False, **conf_kw):
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod = _game(name)[0]
    hyper = mod.resnet_hyper if (resnet or name == "atari") else mod.hyper
    conf = dataclasses.replace(mod.conf, replay_buffer_size=64, **conf_kw)
    e = abi.Engine(conf, hyper, device=0, max_games=max_games, rng_seed=wr.SEED)
    for k, w in enumerate(init_nets(conf, hyper, seed=wseed)):
        e.set_weights(k, w)
    return e


def _check_evaluation(ed, eh, name, E, opponent, mzp, step0, goff, temp, tstep, **mirror_kw):
    """One evaluation on the device engine `ed` (configured by the caller) against the mirror on `eh`;
    returns (the mirror's histories, its record)."""
    from muzero_jl_amd.selfplay import evaluate
    env_cls = _game(name)[1]
    hs, want = evaluate(eh, env_cls, E, opponent=opponent, muzero_player=mzp, rng_step0=step0, game_offset=goff,
                        temperature=temp, training_step=tstep, **mirror_kw)
    ed.test_play(tstep, step0, game_offset=goff, temperature=temp)
    total, recs = ed.test_results(max_records=1)
    assert total >= 1 and len(recs) == 1
    print(name, opponent, mzp, "device", recs[0], "mirror", want)
    for g in range(E):
        assert wr.same_history(ed.test_get_game(g), hs[g]), (name, opponent, mzp, g)
    assert wr.same_record(recs[0], want), (recs[0], want)
    assert want["games"] == E
    return hs, want


@pytest.fixture(scope="module")
def ttt_pair():
    """(device engine with E test slots' worth of shard, mirror engine), FC TicTacToe of worker_ref."""
    conf_kw = dict(num_iters=wr.SIMS, max_moves=wr.MAX_MOVES)
    ed, eh = _engine("ttt", 8, **conf_kw), _engine("ttt", 8, **conf_kw)
    ed.selfplay_init(_game("ttt")[2], 8, 16)
    yield ed, eh
    ed.close(); eh.close()


@pytest.mark.parametrize("opponent,mzp", wr.CONFIGS)
def test_tictactoe_games_and_record_match_the_mirror(ttt_pair, opponent, mzp):
    ed, eh = ttt_pair
    ed.test_config(wr.E, OPP[opponent], mzp)
    hs, want = _check_evaluation(ed, eh, "ttt", wr.E, opponent, mzp, wr.STEP0, wr.GOFF, wr.TEMP, 3)
    lens = [len(h.action_history) for h in hs]
    if (opponent, mzp) in wr.VARIED:                           # (asserted on the CPU oracle as well)
        assert len(set(lens)) >= 2 and want["draws"] > 0 and want["muzero_wins"] + want["opponent_wins"] > 0
    # the self-play slots were never touched
    ln, board, player = ed.selfplay_slots()
    assert not ln.any() and (player == 1).all() and (board[:, 18:] == 1).all() and not board[:, :18].any()
    assert ed.replay_counts()[0][0] == 0 and ed.eval_results() == (0, 0, 0, 0)


def test_temperature_threshold_applies_per_slot():
    """temperature_threshold = 3: from its fourth move on every test slot plays at temperature 0 (the test
    slots' own per-slot temperatures), as mz_selfplay_move does; more test slots than self-play slots."""
    kw = dict(num_iters=wr.SIMS, max_moves=wr.MAX_MOVES, temperature_threshold=3)
    ed, eh = _engine("ttt", 8, **kw), _engine("ttt", 8, **kw)
    ed.selfplay_init(_game("ttt")[2], 2, 4)
    ed.test_config(7, OPP["random"], 2)
    hs, _ = _check_evaluation(ed, eh, "ttt", 7, "random", 2, wr.STEP0, wr.GOFF, wr.TEMP, 1)
    cold = _engine("ttt", 8, num_iters=wr.SIMS, max_moves=wr.MAX_MOVES)      # no threshold: another evaluation
    cold.selfplay_init(_game("ttt")[2], 2, 4)
    cold.test_config(7, OPP["random"], 2)
    cold.test_play(1, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    assert not all(wr.same_history(cold.test_get_game(g), hs[g]) for g in range(7))
    ed.close(); eh.close(); cold.close()


def test_connect4_with_the_expert():
    E = 6
    ed, eh = _engine("c4", E, num_iters=4), _engine("c4", E, num_iters=4)
    ed.selfplay_init(_game("c4")[2], E, E)
    ed.expert_depth(2)
    ed.test_config(E, OPP["expert"], 2)
    hs, want = _check_evaluation(ed, eh, "c4", E, "expert", 2, 300, 11, 1.0, 17, expert_depth=2)
    assert want["moves"] == sum(len(h.action_history) for h in hs) and want["value_moves"] < want["moves"]
    ed.close(); eh.close()


def test_resnet_against_a_second_weight_set():
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    E = 5
    kw = dict(resnet=True, num_iters=4, max_moves=wr.MAX_MOVES)
    ed, eh, eo = _engine("ttt", E, **kw), _engine("ttt", E, **kw), _engine("ttt", E, wseed=211, **kw)
    ed.selfplay_init(_game("ttt")[2], E, E)
    with pytest.raises(abi.MzError, match="opponent"):         # NETWORK before the opponent set is complete
        ed.test_config(E, OPP["network"], 1)
    for k, w in enumerate(init_nets(eo.conf, eo.hyper, seed=211)):
        ed.opponent_set_weights(k, w)
    ed.test_config(E, OPP["network"], 1)
    _check_evaluation(ed, eh, "ttt", E, "network", 1, wr.STEP0, wr.GOFF, 1.0, 5, opponent_engine=eo)
    ed.close(); eh.close(); eo.close()


def test_atari_like_env():
    from muzero_jl_amd import abi
    E = 4
    kw = dict(num_iters=2, max_moves=6)
    ed, eh = _engine("atari", E, **kw), _engine("atari", E, **kw)
    ed.selfplay_init(abi.ENV_ATARI, E, E)
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        ed.test_config(E, OPP["expert"], 1)
    with pytest.raises(abi.MzError, match="opponent network: needs a two-player board env"):
        ed.test_config(E, OPP["network"], 1)
    ed.test_config(E, OPP["self"], 1)
    hs, want = _check_evaluation(ed, eh, "atari", E, "self", 1, 100, 7, 1.0, 2)
    assert want["value_moves"] == want["moves"] and want["reward_opponent"] == 0.0    # one player: every record
    with pytest.raises(abi.MzError, match="initial games"):    # the self-play slots still wait for their first move
        ed.selfplay_slots()
    ed.close(); eh.close()


def test_against_todays_evaluation_mode(ttt_pair):
    """The same T moves in MZ_SP_EVAL on an engine of E slots: its tally (only first games can finish
    inside T = 7 moves: a TicTacToe game has at least 5) and its slots after every move."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import evaluate
    ed, eh = ttt_pair
    E, T = wr.E, wr.MAX_MOVES + 1
    ed.test_config(E, OPP["random"], 1)
    ed.test_play(0, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    games = [ed.test_get_game(g) for g in range(E)]
    lens = [len(h.action_history) for h in games]
    assert 2 * min(lens) > T
    _, want = evaluate(eh, _game("ttt")[1], E, opponent="random", muzero_player=1, rng_step0=wr.STEP0,
                       game_offset=wr.GOFF, temperature=wr.TEMP)
    eh.selfplay_init(abi.ENV_TICTACTOE, E, E)
    eh.selfplay_mode(abi.SP_EVAL, abi.OPP_RANDOM, 1)
    for m in range(T):
        eh.selfplay_move(wr.STEP0 + m, game_offset=wr.GOFF, temperature=wr.TEMP)
        ln, board, _ = eh.selfplay_slots()
        for g in range(E):
            if m + 1 < lens[g]:                                # the board after m + 1 moves = the next record's observation
                assert ln[g] == m + 1 and np.array_equal(board[g], games[g].observation_history[m + 1]), (m, g)
            elif m + 1 == lens[g]:
                assert ln[g] == 0, (m, g)                      # ended on this move: the old mode restarts the slot
    tally = eh.eval_results()
    assert tally == (want["games"], want["muzero_wins"], want["opponent_wins"], want["draws"]) and tally[0] == E
    _, recs = ed.test_results(1)
    assert wr.same_record(recs[0], dict(want, training_step=0))


def test_consecutive_evaluations_and_the_ring(ttt_pair):
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import evaluate
    ed, eh = ttt_pair
    env_cls = _game("ttt")[1]
    ed.test_clear()
    assert ed.test_results() == (0, [])
    ed.test_config(wr.E, OPP["random"], 2)
    keys = [(10, wr.STEP0, wr.GOFF), (11, wr.STEP0 + 50, wr.GOFF + 3)]
    want = []
    for tstep, s0, goff in keys:
        ed.test_play(tstep, s0, game_offset=goff, temperature=wr.TEMP)
        want.append(evaluate(eh, env_cls, wr.E, opponent="random", muzero_player=2, rng_step0=s0, game_offset=goff,
                             temperature=wr.TEMP, training_step=tstep))
    total, recs = ed.test_results()
    assert total == 2 and len(recs) == 2
    for r, (_, w) in zip(recs, want):                          # oldest first; the second holds its own games only
        assert wr.same_record(r, w), (r, w)
    assert recs[1]["games"] == wr.E and not wr.same_record(recs[0], dict(recs[1], training_step=10, rng_step0=wr.STEP0))
    for g in range(wr.E):                                      # the slots hold the second evaluation's games
        assert wr.same_history(ed.test_get_game(g), want[1][0][g]), g
    assert ed.test_results(1)[1] == recs[1:]
    # the ring keeps the latest MZ_TEST_RECORDS records
    ed.test_clear()
    n = abi.TEST_RECORDS + 2
    for i in range(n):
        ed.test_play(i, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    total, recs = ed.test_results()
    assert total == n and [r["training_step"] for r in recs] == list(range(2, n))
    assert [r["training_step"] for r in ed.test_results(3)[1]] == [n - 3, n - 2, n - 1]
    assert all(wr.same_record(r, dict(want[0][1], training_step=r["training_step"])) for r in recs[::97])
    ed.test_clear()
    assert ed.test_results() == (0, [])


# ---- inside mz_train_run
G_TR, CAP, B, MOVES, MOVE0, GOFF_TR = 8, 32, 8, 24, 30, 2
TEST_GOFF, TEST_TEMP, INTERVAL = 500, 0.0, 4


def _train_engine(rean):
    from muzero_jl_amd import abi
    e = _engine("ttt", 16, wseed=17, num_iters=8, batch_size=B, checkpoint_interval=3, training_steps=10000)
    e.selfplay_init(abi.ENV_TICTACTOE, G_TR, CAP)
    e.train_init(B)
    if rean:
        e.train_set_reanalyse(abi.REAN_BY_SEARCH, 1)
    return e


@pytest.mark.parametrize("rean", [False, True])
def test_train_run_with_and_without_the_worker(rean, tmp_path):
    """The same job on two engines, 24 moves one at a time: with the worker every 4 learner steps and
    without it.  Everything the public read-outs show is equal; and the worker's records are those of
    explicit test_play calls on a third engine that is given the learner's weights of that moment."""
    import test_snapshot_gpu as snap
    from muzero_jl_amd import abi
    T = 10                                                     # TicTacToe's max_moves + 1
    on, off = _train_engine(rean), _train_engine(rean)
    third = _engine("ttt", 16, wseed=99, num_iters=8)
    third.selfplay_init(abi.ENV_TICTACTOE, 4, 4)
    E = 5
    for e in (on, third):
        e.test_config(E, abi.OPP_RANDOM, 2)
    on.train_set_test(INTERVAL, TEST_GOFF, TEST_TEMP)
    t0, crossed = 0, []
    for m in range(MOVES):
        s_on = on.train_run(1, move0=MOVE0 + m, game_offset=GOFF_TR)
        s_off = off.train_run(1, move0=MOVE0 + m, game_offset=GOFF_TR)
        assert s_on == s_off, m
        t1 = s_off[0]
        if t1 // INTERVAL > t0 // INTERVAL:
            crossed.append(t1)
            for k in range(3):
                third.set_weights(k, off.train_weights(abi.TRAIN_LEARNER, k))
            third.test_play(t1, (t1 * T) & 0xffffffff, game_offset=TEST_GOFF, temperature=TEST_TEMP)
        t0 = t1
    assert len(crossed) >= 3 and s_off[2] >= 2                 # evaluations ran, and the actors were refreshed
    snap._same(snap._readout(on, tmp_path, "on"), snap._readout(off, tmp_path, "off"))
    total, recs = on.test_results()
    total3, recs3 = third.test_results()
    assert total == total3 == len(crossed) and [r["training_step"] for r in recs] == crossed
    for a, b in zip(recs, recs3):
        assert wr.same_record(a, b), (a, b)
    assert all(r["games"] == E for r in recs) and len({r["value_sum"] for r in recs}) > 1   # the nets moved
    assert off.test_results() == (0, [])
    on.close(); off.close(); third.close()


def test_refusals_and_lifetime(tmp_path):
    from muzero_jl_amd import abi
    kw = dict(num_iters=wr.SIMS, max_moves=wr.MAX_MOVES)
    e = _engine("ttt", 8, **kw)
    with pytest.raises(abi.MzError, match="mz_selfplay_init first"):
        e.test_config(4, abi.OPP_SELF, 1)
    with pytest.raises(abi.MzError, match="mz_selfplay_init first"):
        e.test_play(0, 0)
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    with pytest.raises(abi.MzError, match="no test slots"):     # games == 0: off
        e.test_play(0, 0)
    with pytest.raises(abi.MzError, match="no test slots"):
        e.train_set_test(4)
    with pytest.raises(abi.MzError, match="interval must be >= 0"):
        e.train_set_test(-1)
    e.train_set_test(0)
    for games, opp, mzp, msg in ((9, 0, 1, "games must be in 0..max_games"), (-1, 0, 1, "games must be in"),
                                 (4, 7, 1, "opponent must be"), (4, 1, 3, "muzero_player must be 1 or 2"),
                                 (4, 1, 0, "muzero_player must be 1 or 2"), (4, abi.OPP_NETWORK, 1, "opponent")):
        with pytest.raises(abi.MzError, match=msg):
            e.test_config(games, opp, mzp)
    e.test_config(wr.E, abi.OPP_RANDOM, 1)
    with pytest.raises(abi.MzError, match="no evaluation"):
        e.test_get_game(0)
    e.test_play(1, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    with pytest.raises(abi.MzError, match="slot out of range"):
        e.test_get_game(wr.E)
    total, recs = e.test_results()
    games = [e.test_get_game(g) for g in range(wr.E)]
    assert total == 1 and recs[0]["games"] == wr.E
    e.test_config(0, abi.OPP_RANDOM, 1)                        # off again: the call is refused, the record stays
    with pytest.raises(abi.MzError, match="no test slots"):
        e.test_play(2, wr.STEP0)
    e.test_config(wr.E, abi.OPP_RANDOM, 1)

    # mz_selfplay_init drops the slots; the settings and the records stay
    e.selfplay_move(5, 1)
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    assert e.test_results() == (total, recs)
    with pytest.raises(abi.MzError, match="no evaluation"):
        e.test_get_game(0)
    e.test_play(2, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)     # no new test_config needed
    total2, recs2 = e.test_results()
    assert total2 == 2 and wr.same_record(recs2[0], recs[0]) and wr.same_record(recs2[1], dict(recs[0], training_step=2))
    assert all(wr.same_history(e.test_get_game(g), games[g]) for g in range(wr.E))

    # a snapshot carries neither; the loading engine evaluates with its own settings on fresh slots
    e.selfplay_move(6, 1)
    path = str(tmp_path / "snap.safetensors")
    e.snapshot_save(path, 7)
    other = _engine("ttt", 8, wseed=99, **kw)
    other.selfplay_init(abi.ENV_TICTACTOE, 6, 12)
    other.test_config(wr.E, abi.OPP_RANDOM, 1)
    other.test_play(0, 1, temperature=wr.TEMP)
    assert other.snapshot_load(path) == 7
    assert other.test_results()[0] == 1                        # its record stayed
    with pytest.raises(abi.MzError, match="no evaluation"):
        other.test_get_game(0)
    other.test_play(2, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    assert wr.same_record(other.test_results(1)[1][0], recs2[1])
    assert all(wr.same_history(other.test_get_game(g), games[g]) for g in range(wr.E))
    for a, b in zip(e.selfplay_slots(), other.selfplay_slots()):
        assert np.array_equal(a, b)
    e.close(); other.close()


def test_worker_off_adds_no_launch():
    """mz_debug_enable(2) counts the ResNet search's network launches: a train_run with the worker
    configured but off launches what an engine that never heard of it launches; on, each evaluation
    adds exactly T searches of num_iters network launches."""
    from muzero_jl_amd import abi
    S, T, E, moves = 4, wr.MAX_MOVES + 1, 5, 8
    counts = {}
    for mode in ("plain", "off", "on"):
        e = _engine("ttt", 6, wseed=17, resnet=True, num_iters=S, max_moves=wr.MAX_MOVES, batch_size=4,
                    checkpoint_interval=3, training_steps=10000)
        e.selfplay_init(abi.ENV_TICTACTOE, 6, 16)
        e.train_init(4)
        if mode != "plain":
            e.test_config(E, abi.OPP_SELF, 1)
            e.train_set_test(2 if mode == "on" else 0, TEST_GOFF, 0.0)
        e.debug_enable(2)
        st = e.train_run(moves, move0=MOVE0, game_offset=GOFF_TR)
        counts[mode] = (e.debug_kernel_time()[1], st, e.test_results()[0])
        e.close()
    assert counts["plain"][1] == counts["off"][1] == counts["on"][1] and counts["plain"][1][0] >= 2
    assert counts["plain"][0] == counts["off"][0] == moves * S and counts["off"][2] == 0
    assert counts["on"][2] >= 1 and counts["on"][0] == counts["off"][0] + counts["on"][2] * T * S
