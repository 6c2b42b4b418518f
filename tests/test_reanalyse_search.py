"""Reanalyse by search on the host mirror (replay_buffer.py): make_target takes
its policies from reanalysed_child_visits unless the field is None, and
ReplayBuffer.reanalyse_search hands every stored position of a game to a
search function and keeps what it returns.  CPU only; the device shard is
checked against this mirror in tests/test_reanalyse_search_gpu.py."""
import dataclasses

import numpy as np
import pytest

from muzero_jl_amd.replay_buffer import ReplayBuffer, make_target, stored_legal_mask
from muzero_jl_amd.selfplay import GameHistory, get_stacked_observations


def played_game(moves, A=9):
    """A TicTacToe history from a list of 1-based cells: the boards are real, the search records seeded noise."""
    rng = np.random.default_rng(len(moves) * 131 + moves[0])
    h = GameHistory()
    board = np.zeros(27, np.float32)
    board[18:] = 1
    player = 1
    for a in moves:
        h.observation_history.append(board.copy())
        h.to_play_history.append(player)
        h.action_history.append(a)
        h.reward_history.append(0.0)
        cv = rng.random(A).astype(np.float32)
        h.child_visits.append(cv / cv.sum())
        h.root_values.append(float(np.float32(rng.uniform(-1, 1))))
        board[18 + a - 1] = 0
        board[9 * (player - 1) + a - 1] = 1
        player = player % 2 + 1
    return h


GAMES = [[5, 1, 9, 3, 2, 8, 7], [1, 2, 3], [4], [9, 8, 7, 6, 5, 4, 3, 2, 1], [2, 5, 8, 1]]


def test_field_is_last_and_defaults_to_none():
    names = [f.name for f in dataclasses.fields(GameHistory)]
    assert names[-1] == "reanalysed_child_visits" and GameHistory().reanalysed_child_visits is None


def test_make_target_reads_the_reanalysed_policies_when_set(ttt):
    conf = dataclasses.replace(ttt.conf, td_steps=2)
    h = played_game(GAMES[0])
    T = len(h.root_values)
    plain = [make_target(conf, h, i, seed=3, sample=1, step=2) for i in range(1, T + 1)]
    rng = np.random.default_rng(4)
    new = rng.random((T, 9)).astype(np.float32)
    new /= new.sum(axis=1, keepdims=True)
    h.reanalysed_child_visits = [r for r in new]
    K = conf.num_unroll_steps
    for i in range(1, T + 1):
        tv, tr, tp, ta = make_target(conf, h, i, seed=3, sample=1, step=2)
        for k in range(K + 1):
            if i + k < T:
                assert np.array_equal(tp[k], new[i + k - 1]), (i, k)
                assert not np.array_equal(tp[k], plain[i - 1][2][k])
            else:                                           # past the game: uniform, as before
                assert np.array_equal(tp[k], plain[i - 1][2][k])
        for got, was in zip((tv, tr, ta), (plain[i - 1][0], plain[i - 1][1], plain[i - 1][3])):
            assert np.array_equal(got, was)                 # values, rewards and actions do not move
    h.reanalysed_child_visits = None
    for i in range(1, T + 1):
        for got, was in zip(make_target(conf, h, i, seed=3, sample=1, step=2), plain[i - 1]):
            assert np.array_equal(got, was)


def test_stored_legal_mask(ttt):
    from muzero_jl_amd.games import connect4
    h = played_game(GAMES[0])
    for t, board in enumerate(h.observation_history):
        want = np.ones(9, np.uint8)
        want[[a - 1 for a in h.action_history[:t]]] = 0
        assert np.array_equal(stored_legal_mask(ttt.conf, board, h.to_play_history[t]), want)
    line = np.zeros(27, np.float32)
    line[[0, 1, 2]] = 1                                     # player 1 holds the first column
    line[[9 + 4, 9 + 5]] = 1
    line[18 + np.array([3, 6, 7, 8])] = 1
    assert not stored_legal_mask(ttt.conf, line, 1).any()   # Q14: the player who holds the line has no move
    assert np.array_equal(stored_legal_mask(ttt.conf, line, 2), line[18:].astype(np.uint8))
    assert not stored_legal_mask(ttt.conf, line, 3).any()
    W, H = 6, 7
    b = np.zeros(3 * W * H, np.float32)
    b[2 * W * H:] = 1
    for w in range(W):                                      # column 3 (h = 2) is full
        b[2 * W * H + w + W * 2] = 0
        b[(w % 2) * W * H + w + W * 2] = 1
    assert list(stored_legal_mask(connect4.conf, b, 1)) == [1, 1, 0, 1, 1, 1, 1]


def _buffer(ttt, cap=4):
    conf = dataclasses.replace(ttt.conf, td_steps=2, replay_buffer_size=cap, batch_size=40)
    rb = ReplayBuffer(conf, seed=9)
    for m in GAMES:                                         # ids 1..5, the FIFO holds 2..5
        rb.save_game(played_game(m))
    return conf, rb


def test_reanalyse_search_calls_search_fn_per_game_and_keeps_its_results(ttt):
    conf, rb = _buffer(ttt)
    assert list(rb.buffer.keys()) == [2, 3, 4, 5]
    _, plain = rb.get_batch(step=4)
    calls = []

    def search_fn(obs, legal, to_play, p0):
        calls.append((obs.copy(), legal.copy(), to_play.copy(), p0))
        T = obs.shape[0]
        cv = legal.astype(np.float32) * (1.0 + np.arange(T, dtype=np.float32))[:, None] + np.float32(p0)
        return cv, -0.5 - np.arange(T, dtype=np.float32) - p0

    ids = [1, 3, 5]                                         # 1 was evicted: skipped, its rows keep their place
    done = rb.reanalyse_search(search_fn, game_ids=ids)
    assert done == [3, 5] and rb.num_reanalysed_games == 2 and len(calls) == 2
    Tm = conf.max_moves + 1
    for (obs, legal, tp, p0), gid in zip(calls, done):
        h = rb.buffer[gid]
        T = len(h.root_values)
        assert p0 == ids.index(gid) * Tm
        want = np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                                  conf.stacked_observations, 9) for i in range(1, T + 1)])
        assert np.array_equal(obs, want)
        assert np.array_equal(tp, np.array(h.to_play_history))
        for t in range(T):
            assert np.array_equal(legal[t], stored_legal_mask(conf, h.observation_history[t], h.to_play_history[t]))
            assert legal[t].any()
        assert np.array_equal(np.array(h.reanalysed_child_visits),
                              legal.astype(np.float32) * (1.0 + np.arange(T, dtype=np.float32))[:, None] + p0)
        assert np.array_equal(np.array(h.reanalysed_predicted_root_values, np.float32),
                              (-0.5 - np.arange(T) - p0).astype(np.float32))
    for gid in (2, 4):
        assert rb.buffer[gid].reanalysed_child_visits is None
        assert rb.buffer[gid].reanalysed_predicted_root_values is None
    _, after = rb.get_batch(step=4)
    for k in plain:
        if k in ("target_policies", "target_values"):
            assert not np.array_equal(after[k], plain[k]), k
        else:
            assert np.array_equal(after[k], plain[k]), k
    assert rb.reanalyse_search(search_fn) == [2, 3, 4, 5] and rb.num_reanalysed_games == 6
    assert [c[3] for c in calls[2:]] == [0, Tm, 2 * Tm, 3 * Tm]


def test_reanalyse_search_keeps_the_originals_of_an_unsearchable_position(ttt):
    conf, rb = _buffer(ttt)
    h = rb.buffer[2]                                        # [1, 2, 3]: make position 2 one where the mover holds a line
    b = np.zeros(27, np.float32)
    b[9 + np.array([0, 1, 2])] = 1
    b[18 + np.array([5, 6, 7, 8])] = 1
    b[[3, 4]] = 1
    h.observation_history[1] = b
    seen = []

    def search_fn(obs, legal, to_play, p0):
        seen.append((obs.copy(), legal.copy(), to_play.copy()))
        return np.full((obs.shape[0], 9), 7.0, np.float32), np.full(obs.shape[0], 7.0, np.float32)

    assert rb.reanalyse_search(search_fn, game_ids=[2]) == [2]
    obs, legal, tp = seen[0]
    assert not obs[1].any() and legal[1].all() and tp[1] == 1          # rides along as the dummy
    cv, rv = np.array(h.reanalysed_child_visits), np.array(h.reanalysed_predicted_root_values, np.float32)
    assert np.array_equal(cv[1], h.child_visits[1]) and rv[1] == np.float32(h.root_values[1])
    assert (cv[[0, 2]] == 7.0).all() and (rv[[0, 2]] == 7.0).all()


def test_frame_stack_buffer_is_refused(ttt):
    rb = ReplayBuffer(ttt.conf, seed=1, frame_stack=4)
    with pytest.raises(ValueError, match="frame-stack env not built"):
        rb.reanalyse_search(lambda *a: None)
