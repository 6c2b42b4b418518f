"""The run log's host side on the CPU: learning.run_log_record, the
exact mirror of mz_log_steps / mz_log_games / mz_log_commit, on hand-made
histories and loss rows — every field, the outcome classes of TicTacToe (Q14:
a nonzero last reward is a win of 3 - mover) and Connect4 (of the mover), the
missed count, the pinned order of the float64 adds — and the JSONL writer."""
import json

import numpy as np

from muzero_jl_amd import abi
from muzero_jl_amd.learning import run_log_derived, run_log_jsonl, run_log_record
from muzero_jl_amd.selfplay import GameHistory


def _game(rewards, movers, values, visits):
    n = len(rewards)
    return GameHistory(observation_history=[np.zeros(27, np.float32)] * n, action_history=[1] * n,
                       reward_history=list(rewards), to_play_history=list(movers),
                       child_visits=[np.asarray(v, np.float32) for v in visits], root_values=list(values))


def _f64(x):
    return np.float64(np.float32(x))


# three games: player 1 moved last and was paid (TicTacToe: player 2's line; Connect4: player 1's four),
# player 2 moved last and was paid, and a draw
GAMES = [
    _game([0.0, 0.0, 1.0], [1, 2, 1], [0.25, -0.5, 0.75], [[0.5, 0.5], [0.9, 0.1], [0.2, 0.8]]),
    _game([0.0, -1.0], [1, 2], [0.1, 0.2], [[1.0, 0.0], [0.3, 0.7]]),
    _game([0.0, 0.0, 0.0, 0.0], [1, 2, 1, 2], [0.5, 0.5, 0.5, 0.5], [[0.6, 0.4]] * 4),
]
LOSSES = np.array([[1.5, 0.0, 2.25, 10.0, 20.0, 30.0],
                   [0.5, 0.0, 0.75, 11.0, 21.0, 31.0],
                   [0.25, 0.0, 1.0, 12.0, 22.0, 32.0]], np.float32)
COUNTERS = (40, 300, 210, 32, 7)


def test_every_field_of_a_record():
    r = run_log_record(LOSSES, GAMES, COUNTERS, t1=15, eta=0.05, refreshes=4, missed=2, env_name="tictactoe")
    assert list(r) == list(abi.LOG_COUNT_FIELDS) + list(abi.LOG_SUM_FIELDS)
    assert [r[k] for k in abi.LOG_COUNT_FIELDS] == [15, 3, 40, 300, 210, 32, 7, 3, 9, 1, 1, 1, 4, 2, 0, 0]
    assert all(isinstance(r[k], int) for k in abi.LOG_COUNT_FIELDS)
    assert all(isinstance(r[k], np.float64) for k in abi.LOG_SUM_FIELDS)
    for j, k in enumerate(abi.LOG_SUM_FIELDS[:6]):             # exact: small dyadic values
        assert r[k] == LOSSES[:, j].astype(np.float64).sum() and r["last_" + k] == np.float64(LOSSES[2, j])
    assert r["eta"] == 0.05
    assert r["reward_sum"] == 0.0 and r["root_value_sum"] == _f64(0.25) - 0.5 + 0.75 + _f64(0.1) + _f64(0.2) + 2.0
    want = (_f64(0.5) + _f64(0.9) + _f64(0.8)) + (_f64(1.0) + _f64(0.7)) + (_f64(0.6) + _f64(0.6) + _f64(0.6) + _f64(0.6))
    assert r["sharpness_sum"].tobytes() == np.float64(want).tobytes()


def test_outcome_classes_per_env():
    ttt = run_log_record(LOSSES, GAMES, COUNTERS, 15, 0.05, 4, env_name="tictactoe")
    c4 = run_log_record(LOSSES, GAMES, COUNTERS, 15, 0.05, 4, env_name="connect4")
    # game 0: mover 1 paid -> TicTacToe player 2, Connect4 player 1; game 1: mover 2 paid -> the reverse
    assert (ttt["wins_p1"], ttt["wins_p2"], ttt["draws"]) == (1, 1, 1)
    assert (c4["wins_p1"], c4["wins_p2"], c4["draws"]) == (1, 1, 1)
    one = run_log_record(LOSSES[:0], GAMES[:1], COUNTERS, 15, 0.05, 4, env_name="tictactoe")
    assert (one["wins_p1"], one["wins_p2"], one["draws"]) == (0, 1, 0)
    one = run_log_record(LOSSES[:0], GAMES[:1], COUNTERS, 15, 0.05, 4, env_name="connect4")
    assert (one["wins_p1"], one["wins_p2"], one["draws"]) == (1, 0, 0)
    one = run_log_record(LOSSES[:0], GAMES[1:2], COUNTERS, 15, 0.05, 4, env_name="atari")   # one player: the mover
    assert (one["wins_p1"], one["wins_p2"], one["draws"]) == (0, 1, 0)
    assert ttt["missed"] == 0 and run_log_record(LOSSES, GAMES, COUNTERS, 15, 0.05, 4, missed=5)["missed"] == 5


def test_an_empty_record():
    r = run_log_record(np.zeros((0, 6), np.float32), [], (0, 0, 0, 0, 0), t1=0, eta=0.1, refreshes=0)
    assert [r[k] for k in abi.LOG_COUNT_FIELDS] == [0] * 16
    assert all(r[k] == 0.0 and not np.signbit(r[k]) for k in abi.LOG_SUM_FIELDS if k != "eta") and r["eta"] == 0.1


def test_the_order_of_the_adds_is_the_stated_one():
    """f32 values of widely different magnitude: (2^60 + 1) - 2^60 in ascending order is 0 in float64, the
    same terms with the small one last give 1.  The mirror's bits are those of the stated order."""
    big, one = np.float32(2.0 ** 60), np.float32(1.0)
    rows = np.zeros((3, 6), np.float32)
    rows[:, 0] = [big, one, -big]
    swapped = rows[[0, 2, 1]]
    a = run_log_record(rows, [], COUNTERS, 3, 0.0, 0)["value"]
    b = run_log_record(swapped, [], COUNTERS, 3, 0.0, 0)["value"]
    assert a == 0.0 and b == 1.0                               # ((2^60 + 1) - 2^60 = 0; (2^60 - 2^60) + 1 = 1
    # a game's own chain in record order, then the games in the order given
    g1 = _game([big, one, -big], [1, 2, 1], [big, one, -big], [[big, 0.0], [one, 0.0], [0.0, -big]])
    g2 = _game([-big, big, one], [1, 2, 1], [0.0, 0.0, one], [[0.5, 0.0]] * 3)
    r = run_log_record(rows[:0], [g1, g2], COUNTERS, 3, 0.0, 0)
    assert r["reward_sum"] == 1.0                              # g1's chain gives 0, g2's gives 1
    assert r["root_value_sum"] == 1.0
    assert r["sharpness_sum"] == np.float64(big)               # maxima 2^60, 1, max(0, -2^60) = 0; then + 1.5: all absorbed
    g3 = _game([big], [1], [0.0], [[1.0, 0.0]])
    g4 = _game([one], [1], [0.0], [[1.0, 0.0]])
    g5 = _game([-big], [1], [0.0], [[1.0, 0.0]])
    assert run_log_record(rows[:0], [g3, g4, g5], COUNTERS, 3, 0.0, 0)["reward_sum"] == 0.0
    assert run_log_record(rows[:0], [g3, g5, g4], COUNTERS, 3, 0.0, 0)["reward_sum"] == 1.0


def test_jsonl_round_trip(tmp_path):
    recs = [run_log_record(LOSSES, GAMES, COUNTERS, 15, 0.05, 4, missed=2),
            run_log_record(LOSSES[:0], [], COUNTERS, 15, 0.05, 4)]
    path = tmp_path / "run.jsonl"
    run_log_jsonl(str(path), recs[:1])
    run_log_jsonl(str(path), recs[1:])                         # appends
    lines = path.read_text().splitlines()
    assert len(lines) == 2
    back = [json.loads(x) for x in lines]
    assert back == [run_log_derived(r) for r in recs]
    d = back[0]
    assert d["training_step"] == 15 and d["steps"] == 3 and d["games"] == 3 and d["missed"] == 2
    assert d["mean_value_loss"] == 0.75 and d["last_value_loss"] == 0.25 and d["mean_policy_loss"] == 4.0 / 3
    assert d["win_p1_fraction"] == d["win_p2_fraction"] == d["draw_fraction"] == 1.0 / 3
    assert d["mean_game_length"] == 3.0 and d["mean_root_value"] == float(recs[0]["root_value_sum"]) / 9
    assert d["mean_sharpness"] == float(recs[0]["sharpness_sum"]) / 9
    assert back[1]["mean_value_loss"] is None and back[1]["draw_fraction"] is None and back[1]["games"] == 0
