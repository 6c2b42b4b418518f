"""The Reanalyse worker's round on the host mirror (replay_buffer.py): pack_round,
the restatement of kernel mz_reanalyse_pack, against a brute-force reading of
its rule, and ReplayBuffer.reanalyse_next on top of it.  CPU only; the device
rounds are checked against this mirror in tests/test_reanalyse_next_gpu.py."""
import dataclasses

import numpy as np
import pytest

from muzero_jl_amd.replay_buffer import REAN_BY_SEARCH, REAN_BY_VALUE, ReplayBuffer, pack_round

from test_reanalyse_search import played_game

T = 10


def brute(lens, cursor, played, cap, R):
    """The rule, one game at a time: (first, the games taken, new cursor)."""
    if played == 0:
        return cursor, [], cursor
    held = [g for g in range(1, played + 1) if g > played - cap]
    g = cursor if cursor in held else held[0]
    first, taken, used = g, [], 0
    while g in held and used + lens[g] <= R:
        taken.append(g)
        used += lens[g]
        g += 1
    return first, taken, g


def _case(rng):
    cap, R = int(rng.integers(3, 13)), int(rng.integers(10, 41))
    played = int(rng.choice([0, rng.integers(1, cap), cap, rng.integers(cap + 1, 4 * cap)]))
    oldest = max(played - cap, 0) + 1
    where = rng.integers(0, 3)
    cursor = int([rng.integers(-2, oldest), rng.integers(oldest, max(played, oldest) + 1),
                  rng.integers(played + 1, played + 5)][where])
    lens = {g: int(rng.integers(1, T + 1)) for g in range(oldest, played + 1)}
    return lens, cursor, played, cap, R


def test_pack_round_against_the_rule():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(3000):
        lens, cursor, played, cap, R = _case(rng)
        first, games, rows, cur = pack_round(lens, cursor, played, cap, R)
        bf, taken, bcur = brute(lens, cursor, played, cap, R)
        assert (first, list(range(first, first + games)), cur) == (bf, taken, bcur)
        if played == 0:
            assert (games, rows, cur) == (0, [], cursor)
            seen.add("empty")
            continue
        oldest = max(played - cap, 0) + 1
        assert oldest <= first <= played and first + games - 1 <= played
        # whole games only, in (game, pos) order
        assert rows == [(g, p) for g in taken for p in range(lens[g])]
        assert rows == sorted(rows)
        assert len(rows) == sum(lens[g] for g in taken) <= R
        assert games >= 1
        ended = cur == played + 1
        if not ended:
            assert R - len(rows) < T                        # fewer than T dead rows
            assert len(rows) + lens[cur] > R
        seen.add(("ended" if ended else "full", "lt" if played < cap else "eq" if played == cap else "gt",
                  "before" if cursor < oldest else "after" if cursor > played else "inside"))
    assert "empty" in seen
    for end in ("ended", "full"):
        for where in ("before", "inside", "after"):
            assert any(s[0] == end and s[2] == where for s in seen if s != "empty"), (end, where)
    assert {s[1] for s in seen if s != "empty"} == {"lt", "eq", "gt"}


def test_chained_rounds_visit_every_held_game_once_per_lap():
    rng = np.random.default_rng(5)
    for _ in range(200):
        lens, cursor, played, cap, R = _case(rng)
        if played == 0:
            continue
        held = sorted(lens)
        # from wherever the cursor is, to the end of its lap: the rest of the held games, once each
        cur, visited = cursor, []
        while cur != played + 1 or not visited:
            first, games, rows, cur = pack_round(lens, cur, played, cap, R)
            visited += list(range(first, first + games))
        assert visited == held[held.index(visited[0]):]
        # and from a lap's start every held game comes up exactly once
        for lap in range(2):
            visited, rounds = [], 0
            while True:
                first, games, rows, cur = pack_round(lens, cur, played, cap, R)
                visited += list(range(first, first + games))
                rounds += 1
                if cur == played + 1:
                    break
                assert rounds <= len(held)
            assert visited == held, (lap, visited, held)


def _buffer(ttt, cap, moves):
    rb = ReplayBuffer(dataclasses.replace(ttt.conf, replay_buffer_size=cap, td_steps=2), seed=3)
    for m in moves:
        rb.save_game(played_game(m))
    return rb


MOVES = [[5, 1, 9, 3, 2, 8, 7], [1, 2, 3], [4], [9, 8, 7, 6, 5, 4, 3, 2, 1], [2, 5, 8, 1], [3, 1, 2, 4, 6], [7, 8]]


@pytest.mark.parametrize("mode", [REAN_BY_VALUE, REAN_BY_SEARCH])
def test_reanalyse_next_fills_exactly_the_taken_games(ttt, mode):
    cap, R = 5, 12
    rb = _buffer(ttt, cap, MOVES)                           # games 3..7 held, lengths 1, 9, 4, 5, 2
    lens = {g: len(h.root_values) for g, h in rb.buffer.items()}
    assert sorted(lens) == [3, 4, 5, 6, 7] and rb.reanalyse_cursor == 1
    calls = []

    def value_fn(x):
        calls.append(("v", x.shape[0]))
        return np.full(x.shape[0], 0.25, np.float32) + np.arange(x.shape[0], dtype=np.float32)

    def search_fn(x, legal, tp, p0):
        calls.append(("s", x.shape[0], p0))
        return np.full(legal.shape, 0.5, np.float32), np.full(len(tp), 100.0 + p0, np.float32)

    fn = value_fn if mode == REAN_BY_VALUE else search_fn
    cursor, lap = 1, []
    for _ in range(6):
        want = pack_round(lens, cursor, rb.num_played_games, cap, R)
        before = {g: (h.reanalysed_predicted_root_values, h.reanalysed_child_visits) for g, h in rb.buffer.items()}
        n0, calls[:] = rb.num_reanalysed_games, []
        got = rb.reanalyse_next(fn, mode, R)
        assert got == want and rb.reanalyse_cursor == want[3]
        first, games, rows, cursor = got
        taken = list(range(first, first + games))
        assert rb.num_reanalysed_games == n0 + games
        if mode == REAN_BY_VALUE:
            assert calls == [("v", lens[g]) for g in taken]
        else:                                               # p0: the game's first row in the packed round
            assert calls == [("s", lens[g], rows.index((g, 0))) for g in taken]
        for g, h in rb.buffer.items():
            if g in taken:
                assert len(h.reanalysed_predicted_root_values) == lens[g]
                assert (h.reanalysed_child_visits is not None) == (mode == REAN_BY_SEARCH or before[g][1] is not None)
                if mode == REAN_BY_SEARCH:
                    assert float(h.reanalysed_predicted_root_values[0]) == 100.0 + rows.index((g, 0))
            else:                                           # the very same objects as before
                assert h.reanalysed_predicted_root_values is before[g][0]
                assert h.reanalysed_child_visits is before[g][1]
        lap += taken
    assert lap[:5] == [3, 4, 5, 6, 7] and lap[5:10] == [3, 4, 5, 6, 7]      # [3, 4] [5, 6, 7] [3, 4] ...
    # a game saved into an evicted game's slot starts as `nothing`, and the cursor skips what left
    assert all(h.reanalysed_predicted_root_values is not None for h in rb.buffer.values())
    rb.save_game(played_game([6, 2]))
    assert sorted(rb.buffer) == [4, 5, 6, 7, 8]
    new = rb.buffer[8]
    assert new.reanalysed_predicted_root_values is None and new.reanalysed_child_visits is None
    rb.reanalyse_cursor = 3                                 # game 3 has left
    first, games, rows, cursor = rb.reanalyse_next(fn, mode, R)
    assert first == 4 and games >= 1


def test_reanalyse_next_refusals(ttt):
    rb = _buffer(ttt, 4, MOVES[:2])
    with pytest.raises(ValueError, match="mode"):
        rb.reanalyse_next(lambda x: x, 0, 16)
    with pytest.raises(ValueError, match="cannot hold one game"):
        rb.reanalyse_next(lambda *a: None, REAN_BY_SEARCH, ttt.conf.max_moves)
    empty = ReplayBuffer(ttt.conf, seed=1)
    assert empty.reanalyse_next(lambda x: x, REAN_BY_VALUE) == (1, 0, [], 1)
    fs = ReplayBuffer(ttt.conf, seed=1, frame_stack=4)
    with pytest.raises(ValueError, match="frame-stack env not built"):
        fs.reanalyse_next(lambda x: x, REAN_BY_VALUE)
