"""The test worker on the CPU: the host mirror of its record
(selfplay.evaluation_record) on hand-written histories, `evaluate` with stub
engines, the Python binding against the header, and — with the CPU oracle as
the engine — the evaluation the GPU test replays, which must be a varied one."""
import ctypes
import os
import re

import numpy as np
import pytest

import worker_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hist(tp, rew, rv):
    from muzero_jl_amd.selfplay import GameHistory
    n = len(tp)
    return GameHistory(observation_history=[np.zeros(27, np.float32)] * n, action_history=list(range(1, n + 1)),
                       reward_history=[float(x) for x in rew], to_play_history=list(tp),
                       child_visits=[np.zeros(9, np.float32)] * n, root_values=[float(np.float32(x)) for x in rv])


def _bits(x):
    return np.float64(x).tobytes()


def test_record_sums_in_the_stated_order():
    """f32 root values 1e8, 1, -1e8: in f64 the serial sum (1e8 + 1) - 1e8 is 1; a game's sum starts
    at +0 and runs in record order, and the games join in (length, slot) order, not slot order."""
    from muzero_jl_amd.selfplay import evaluation_record
    big = float(np.float32(1e8))
    one = _hist([1, 1, 1], [0, 0, 0], [big, 1.0, -big])
    rec = evaluation_record([one], "tictactoe", "self", 1, 2)
    assert _bits(rec["value_sum"]) == _bits((np.float64(0.0) + big + 1.0) - big) == _bits(1.0)
    # across games: slot 0 = a (3 moves, -2^53), slot 1 = b (1 move, 1), slot 2 = c (2 moves, 2^53); the
    # (move, slot) order b, c, a and the slot order a, b, c give different f64 sums
    p53 = float(2.0 ** 53)
    a, b, c = _hist([1] * 3, [0] * 3, [0, 0, -p53]), _hist([1], [0], [1.0]), _hist([1] * 2, [0] * 2, [0, p53])
    rec = evaluation_record([a, b, c], "tictactoe", "self", 1, 2)
    want = ((np.float64(0.0) + 1.0) + p53) + -p53               # b, c, a: 1 + 2^53 rounds to 2^53 -> 0
    assert _bits(rec["value_sum"]) == _bits(want) == _bits(0.0)
    slot_order = ((np.float64(0.0) + -p53) + 1.0) + p53         # a, b, c: -2^53 + 1 is exact -> 1
    assert _bits(slot_order) == _bits(1.0) != _bits(rec["value_sum"])
    assert rec["moves"] == 6 and rec["value_moves"] == 6 and rec["games"] == 3 and rec["draws"] == 3
    # a game's own sum starts at +0: a lone -0.0 reward leaves +0.0
    z = evaluation_record([_hist([1], [-0.0], [-0.0])], "tictactoe", "self", 1, 2)
    assert _bits(z["reward_muzero"]) == _bits(0.0) and _bits(z["value_sum"]) == _bits(0.0)


def test_record_muzero_moves_rule():
    from muzero_jl_amd.selfplay import evaluation_record
    h = _hist([1, 2, 1, 2], [0.5, 0.25, 0.125, 2.0], [1.0, 10.0, 100.0, 1000.0])
    me = evaluation_record([h], "connect4", "random", 1, 2, training_step=9, rng_step0=2 ** 32 + 5)
    assert (me["reward_muzero"], me["reward_opponent"], me["value_sum"], me["value_moves"]) == (0.625, 2.25, 101.0, 2)
    assert me["training_step"] == 9 and me["rng_step0"] == 5 and me["moves"] == 4
    other = evaluation_record([h], "connect4", "expert", 2, 2)
    assert (other["reward_muzero"], other["reward_opponent"], other["value_sum"], other["value_moves"]) == \
        (2.25, 0.625, 1010.0, 2)
    for opp, players in (("self", 2), ("random", 1)):           # self-play, and the one-player env: every record
        r = evaluation_record([h], "connect4", opp, 1, players)
        assert (r["reward_muzero"], r["reward_opponent"], r["value_sum"], r["value_moves"]) == (2.875, 0.0, 1111.0, 4)


def test_record_winners():
    """TicTacToe with Q14: a nonzero last reward means the player to move AFTER it holds a line;
    Connect4: the mover's own four."""
    from muzero_jl_amd.selfplay import evaluation_record
    won_by_2 = _hist([1, 2, 1], [0, 0, 1.0], [0, 0, 0])         # last mover 1 -> winner 3 - 1 = 2
    won_by_1 = _hist([1, 2], [0, -1.0], [0, 0])                 # last mover 2 -> winner 1
    draw = _hist([1, 2, 1, 2], [0, 0, 0, 0], [0, 0, 0, 0])
    r = evaluation_record([won_by_2, won_by_1, draw], "tictactoe", "random", 1, 2)
    assert (r["games"], r["muzero_wins"], r["opponent_wins"], r["draws"]) == (3, 1, 1, 1)
    r = evaluation_record([won_by_2, won_by_1, draw], "tictactoe", "random", 2, 2)
    assert (r["muzero_wins"], r["opponent_wins"], r["draws"]) == (1, 1, 1)
    r = evaluation_record([won_by_2, won_by_2], "tictactoe", "random", 2, 2)
    assert (r["muzero_wins"], r["opponent_wins"]) == (2, 0)
    c4 = _hist([1, 2, 1], [0, 0, 1.0], [0, 0, 0])               # the mover (1) wins
    r = evaluation_record([c4, draw], "connect4", "random", 1, 2)
    assert (r["muzero_wins"], r["opponent_wins"], r["draws"]) == (1, 0, 1)
    r = evaluation_record([c4], "connect4", "random", 2, 2)
    assert (r["muzero_wins"], r["opponent_wins"]) == (0, 1)


class _Stub:
    """An engine that always plays the first legal action (TicTacToe cells 1, 2, 3, ...)."""

    def __init__(self, conf):
        self.conf, self.rng_seed, self.calls = conf, 5, []

    def mcts_search(self, obs, legal, tp, exploration=True, rng_step=0, game_offset=0, temperature=1.0):
        self.calls.append((rng_step, game_offset, temperature, exploration, legal.copy()))
        G, A = legal.shape
        cv = np.tile(np.arange(A, dtype=np.float32), (G, 1))
        rv = np.arange(G, dtype=np.float32) + np.float32(len(self.calls))
        act = np.array([np.flatnonzero(legal[g])[0] + 1 for g in range(G)], np.int32)
        return cv, rv, act


def test_evaluate_plays_one_game_per_slot():
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import evaluate, evaluation_record
    E = 3
    stub = _Stub(wr.ttt_conf(max_moves=9))
    hs, rec = evaluate(stub, ttt.BatchedTicTacToe, E, opponent="self", rng_step0=40, game_offset=9, temperature=0.0,
                       training_step=12)
    # cells 1..: X 1 3 5 7, O 2 4 6 — X's line 3-5-7 stands after move 7 and, with Q14 (the win test
    # looks at the player to move), ends the game one move later: 8 moves, the last mover 2, winner 1
    assert [h.action_history for h in hs] == [list(range(1, 9))] * E
    assert [c[0] for c in stub.calls] == list(range(40, 48)) and {c[1] for c in stub.calls} == {9}
    assert all(c[2] == 0.0 and c[3] for c in stub.calls)
    assert rec == evaluation_record(hs, "tictactoe", "self", 1, 2, 12, 40)
    assert (rec["games"], rec["moves"], rec["value_moves"], rec["training_step"], rec["rng_step0"]) == (3, 24, 24, 12, 40)
    assert rec["muzero_wins"] + rec["opponent_wins"] == 3


def test_evaluate_drops_a_finished_slots_later_games():
    """Slots that end on different moves: the host mirror restarts a finished slot (lockstep play), but
    the evaluation holds each slot's first game only."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay, evaluate
    conf = wr.ttt_conf(max_moves=9)
    stub = _Stub(conf)
    sp = BatchedSelfPlay(stub, ttt.BatchedTicTacToe, 2, step0=0)
    sp.env.board[1, [0, 2]] = 1                                  # slot 1 starts with X on cells 1 and 3 ...
    sp.env.board[1, [18, 20]] = 0                                # ... so its game is shorter than slot 0's
    hs = sp.play_games(0.0)
    lens = [len(h.action_history) for h in hs]
    assert lens[0] == 8 and lens[1] < 8
    assert len(stub.calls) == 8                                  # play goes on until the last slot is done
    assert len(sp.finished) == 2 and sp.finished[0] is hs[1] and sp.finished[1] is hs[0]
    assert len(sp.histories[1].action_history) == 8 - lens[1]   # slot 1's second game: in progress, not reported
    hs2, rec = evaluate(_Stub(conf), ttt.BatchedTicTacToe, 4, opponent="random", muzero_player=2, rng_step0=7)
    assert rec["games"] == 4 and rec["moves"] == sum(len(h.action_history) for h in hs2)


def test_binding_matches_the_header():
    from muzero_jl_amd import abi
    hdr = open(os.path.join(ROOT, "include", "mz.h")).read()
    assert int(re.search(r"\bMZ_TEST_RECORDS\s*=\s*(\d+)", hdr).group(1)) == abi.TEST_RECORDS == 1024
    vp, ci = ctypes.c_void_p, ctypes.c_int
    i32, i64, u32, f32 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float
    want = {"mz_test_config": (ci, [vp, i32, ci, ci]),
            "mz_test_play": (ci, [vp, i64, u32, u32, f32, vp]),
            "mz_test_results": (ci, [vp, vp, vp, vp, i32]),
            "mz_test_clear": (ci, [vp]),
            "mz_test_get_game": (ci, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
            "mz_train_set_test": (ci, [vp, i64, u32, f32])}
    ctype_of = {"int32_t": i32, "int64_t": i64, "uint32_t": u32, "float": f32, "int": ci}
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in want.items():
        assert abi.SIGNATURES[name] == sig, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", body, flags=re.M)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        assert len(params) == len(sig[1]), name
        for p, t in zip(params, sig[1]):                         # scalars by type, every pointer as void*
            assert (t is vp) == ("*" in p), (name, p)
            if "*" not in p:
                assert ctype_of[p.rsplit(" ", 1)[0]] is t, (name, p)
    for meth in ("test_config", "test_play", "test_results", "test_clear", "test_get_game", "train_set_test"):
        assert callable(getattr(abi.Engine, meth))
    assert len(abi.TEST_COUNT_FIELDS) == 8 and len(abi.TEST_SUM_FIELDS) == 3
    jl = open(os.path.join(ROOT, "julia", "LibMZ.jl")).read()
    for name in want:
        assert f"(:{name}, libmz)" in jl, name


@pytest.mark.parametrize("opponent,mzp", wr.CONFIGS)
def test_oracle_evaluation_is_varied(opponent, mzp):
    """The evaluation the GPU test replays (worker_ref's keys), on the CPU oracle: slots finish on at least
    two different moves, one game is ended by length (max_moves + 1 = 7 moves, no winner), one is won."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import evaluate, game_winner
    hs, rec = evaluate(wr.oracle_engine(), ttt.BatchedTicTacToe, wr.E, opponent=opponent, muzero_player=mzp,
                       rng_step0=wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP, training_step=3)
    lens = [len(h.action_history) for h in hs]
    winners = [game_winner("tictactoe", h.reward_history[-1], h.to_play_history[-1]) for h in hs]
    assert len(hs) == wr.E and all(1 <= n <= wr.MAX_MOVES + 1 for n in lens)
    assert rec["games"] == wr.E and rec["moves"] == sum(lens)
    assert rec["muzero_wins"] + rec["opponent_wins"] == sum(w != 0 for w in winners)
    if (opponent, mzp) in wr.VARIED:
        assert len(set(lens)) >= 2, lens
        assert any(n == wr.MAX_MOVES + 1 and w == 0 for n, w in zip(lens, winners)), (lens, winners)
        assert any(w != 0 for w in winners), winners
    if opponent == "self":
        assert rec["value_moves"] == rec["moves"] and rec["reward_opponent"] == 0.0
    else:
        assert rec["value_moves"] == sum(sum(t == mzp for t in h.to_play_history) for h in hs)
