"""The expert opponent's host mirror (muzero_jl_amd/games/expert.py)
on the CPU: against an independent recursion written here on the env classes'
own rules, on hand-made positions, and the properties of perfect TicTacToe
play (the solved value of the env's game, Q14 included, is a draw)."""
import functools

import numpy as np
import pytest

import expert_cases as xc


# ---- the independent recursion: TicTacToe on the reference-rule env class itself,
# Connect4 on a column-list board with a table of the 69 lines of four
def _ttt_value(board, player, d):
    return _ttt_value_memo(board.tobytes(), player, d)


def _ttt_step(board, player, a):
    from muzero_jl_amd.games.tictactoe import TicTacToe
    from muzero_jl_amd.selfplay import game_winner
    env = TicTacToe()
    env.board[:] = board.astype(bool)
    env.player = player
    env(a + 1)
    done = env.is_terminated()
    w = game_winner("tictactoe", float(env.reward(player)), player) if done else 0
    return env.board.astype(np.uint8), done, w


def _ttt_scores(board, player, d):
    out = np.full(9, -128, np.int32)
    for a in np.flatnonzero(board[18:]):
        nb, done, w = _ttt_step(board, player, int(a))
        out[a] = (0 if w == 0 else d if w == player else -d) if done else -_ttt_value(nb, 3 - player, d - 1)
    return out


@functools.lru_cache(maxsize=None)
def _ttt_value_memo(key, player, d):
    if d == 0:
        return 0
    sc = _ttt_scores(np.frombuffer(key, np.uint8), player, d)
    return int(sc[sc != -128].max())


def _c4_cols(board):
    b = np.asarray(board).reshape(3, 7, 6)                   # [plane][column][row]
    return [[1 if b[0, h, w] else 2 for w in range(6) if not b[2, h, w]] for h in range(7)]


_C4_LINES = [[(h + k * dh, w + k * dw) for k in range(4)]
             for h in range(7) for w in range(6) for dh, dw in ((1, 0), (0, 1), (1, 1), (1, -1))
             if 0 <= h + 3 * dh < 7 and 0 <= w + 3 * dw < 6]                # the 69 lines of four
_C4_THROUGH = {(h, w): [l for l in _C4_LINES if (h, w) in l] for h in range(7) for w in range(6)}


def _c4_has_four(cols, p, h):
    """A line of four of p through the top stone of column h."""
    return any(all(w < len(cols[c]) and cols[c][w] == p for c, w in line)
               for line in _C4_THROUGH[(h, len(cols[h]) - 1)])


def _c4_scores(cols, p, d):
    out = [-128] * 7
    for h in range(7):
        if len(cols[h]) == 6:
            continue
        cols[h].append(p)
        if _c4_has_four(cols, p, h):
            out[h] = d
        elif all(len(c) == 6 for c in cols):
            out[h] = 0
        else:
            out[h] = 0 if d == 1 else -max(s for s in _c4_scores(cols, 3 - p, d - 1) if s != -128)
        cols[h].pop()
    return out


def independent_scores(name, board, player, d):
    if name == "tictactoe":
        return _ttt_scores(np.asarray(board, np.uint8), player, d)
    return np.array(_c4_scores(_c4_cols(board), player, d), np.int32)


@pytest.mark.parametrize("name", xc.NAMES)
def test_mirror_matches_independent_recursion(name):
    from muzero_jl_amd.games.expert import expert_scores
    pos = xc.random_positions(name)
    assert len(pos) == 200
    seen = {xc.plies(name, b) for b, _ in pos}
    assert seen >= set(range(9 if name == "tictactoe" else 20)), seen      # every ply count of a game
    for d in xc.DEPTHS[name]:
        for board, player in pos:
            assert np.array_equal(expert_scores(name, board, player, d), independent_scores(name, board, player, d)), \
                (d, board, player)


def test_hand_positions():
    from muzero_jl_amd.games.expert import expert_pick, expert_scores
    b, p = xc.C4_WIN
    s = expert_scores("connect4", b, p, 1)
    assert s[0] == 1 and (s[1:] == 0).all() and expert_pick(s, 0xFFFFFFFF) == 1
    b, p = xc.C4_BLOCK
    s1, s2 = expert_scores("connect4", b, p, 1), expert_scores("connect4", b, p, 2)
    assert (s1 == 0).all()                                   # depth 1 sees no difference: it misses the block
    assert s2[1] == 0 and (np.delete(s2, 1) == -1).all()     # depth 2: only the block does not lose
    assert expert_pick(s2, 0) == expert_pick(s2, 0xFFFFFFFF) == 2
    b, p = xc.C4_FULLCOL
    s = expert_scores("connect4", b, p, 3)
    assert s[3] == -128 and (np.delete(s, 3) != -128).all()
    b, p = xc.C4_LAST
    for d in (1, 4, 9):                                      # the depth exceeds what is left
        assert expert_scores("connect4", b, p, d).tolist() == [-128] * 6 + [0]
    b, p = xc.TTT_Q14                                        # the mover's opponent holds a line: every reply loses
    for d in (1, 2, 9):
        s = expert_scores("tictactoe", b, p, d)
        assert s.tolist() == [-128, -128, -d, -128, -128, -d, -128, -d, -d]
    for name in xc.NAMES:
        for board, player in xc.HAND[name]:
            for d in xc.DEPTHS[name]:
                assert np.array_equal(expert_scores(name, board, player, d),
                                      independent_scores(name, board, player, d))


def test_refusals():
    from muzero_jl_amd.games.expert import expert_scores
    b, p = xc.TTT_EMPTY
    for bad in xc.bad_boards("tictactoe"):
        with pytest.raises(ValueError, match="exactly one plane"):
            expert_scores("tictactoe", bad, 1, 3)
    with pytest.raises(ValueError, match="player"):
        expert_scores("tictactoe", b, 3, 3)
    with pytest.raises(ValueError, match="depth"):
        expert_scores("tictactoe", b, p, 10)
    with pytest.raises(ValueError, match="board env"):
        expert_scores("atari_synth", b, p, 3)


def test_empty_board_is_a_draw():
    from muzero_jl_amd.games.expert import expert_scores
    b, p = xc.TTT_EMPTY
    assert expert_scores("tictactoe", b, p, 9).tolist() == [0] * 9


def _play(seed, games, expert_side, rnd):
    """`games` TicTacToe games: the expert (depth 9) as expert_side (0: both
    sides), a uniform random player otherwise; returns (winners, lengths)."""
    from muzero_jl_amd.games.expert import expert_pick, expert_scores
    from muzero_jl_amd.games.tictactoe import BatchedTicTacToe
    from muzero_jl_amd.selfplay import game_winner
    env = BatchedTicTacToe(1)
    winners, lengths = [], []
    for _ in range(games):
        env.reset_all()
        n = 0
        while True:
            p = int(env.player[0])
            legal = np.flatnonzero(env.legal_mask()[0])
            if expert_side in (0, p):
                a = expert_pick(expert_scores("tictactoe", env.board[0], p, 9), int(rnd.integers(0, 2 ** 32)))
            else:
                a = int(rnd.choice(legal)) + 1
            rew, done = env.step(np.array([a], np.int32))
            n += 1
            if done[0]:
                winners.append(game_winner("tictactoe", float(rew[0]), p))
                lengths.append(n)
                break
    return winners, lengths


def test_expert_against_expert_draws():
    w, ln = _play(0, 200, 0, np.random.default_rng(3))
    assert w == [0] * 200 and ln == [9] * 200


@pytest.mark.parametrize("side", [1, 2])
def test_expert_never_loses_to_random(side):
    w, _ = _play(0, 1000, side, np.random.default_rng(10 + side))
    assert 3 - side not in w and len(w) == 1000
