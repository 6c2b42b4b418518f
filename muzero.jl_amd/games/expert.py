"""The rules-search expert opponent, host mirror of
mz_expert_move: a fixed-depth exhaustive negamax over the Python envs' own
rules (games/tictactoe.py with quirk Q14, games/connect4.py) and
selfplay.game_winner.  No network is involved and every value is a small
integer.

For a live position s with player p to move and a depth d >= 1:
  score(s, a, d) = 0 / +d / -d when a ends the game in a draw / a win of p / a
                   win of the other player, else -V(s', d - 1);
  V(s, 0) = 0,  V(s, d) = max over the legal a of score(s, a, d).
The expert plays the k-th (ascending) of the actions with the maximal score.

Also here: the solved TicTacToe table's mirror (ttt_code,
ttt_decode, solved_table) and the judge's rule for one move (§20.1: judge_move).
"""
import numpy as np

from ..rng import rng_below
from . import connect4, tictactoe

ILLEGAL = -128
DEFAULT_DEPTH = {"tictactoe": 9, "connect4": 4}
_LINES = [tuple(int(c) for c in l) for l in tictactoe.LINES]
_W, _H = connect4.W, connect4.H


def _cells(name, board):
    """[p1, p2, empty] planes -> a tuple of 0 (empty) / 1 / 2 per cell; every
    cell must be set in exactly one plane."""
    n = 9 if name == "tictactoe" else connect4.CELLS
    b = np.asarray(board).reshape(3, n) != 0
    if not (b.sum(0) == 1).all():
        raise ValueError("expert: every cell must be set in exactly one plane")
    return tuple(int(x) for x in (b[0] * 1 + b[1] * 2))


def _ttt_legal(c):
    return [a for a in range(9) if c[a] == 0]


def _ttt_step(c, p, a):
    """TicTacToe.__call__ + is_terminated + game_winner: (cells, done, winner)."""
    c = c[:a] + (p,) + c[a + 1:]
    q = p % 2 + 1                                        # the player now to move
    if any(c[i] == q and c[j] == q and c[k] == q for i, j, k in _LINES):
        return c, True, 3 - p                            # Q14: nonzero reward, winner = 3 - mover
    return c, 0 not in c, 0


def _c4_legal(c):
    return [h for h in range(_H) if c[(_W - 1) + _W * h] == 0]


def _c4_step(c, p, h):
    """BatchedConnect4.step + game_winner: (cells, done, winner)."""
    w = next(r for r in range(_W) if c[r + _W * h] == 0)
    cell = w + _W * h
    c = c[:cell] + (p,) + c[cell + 1:]
    for dw, dh in connect4._DIRS:
        n = 1
        for s in (1, -1):
            ww, hh = w + s * dw, h + s * dh
            while 0 <= ww < _W and 0 <= hh < _H and c[ww + _W * hh] == p:
                n += 1
                ww += s * dw
                hh += s * dh
        if n >= 4:
            return c, True, p
    return c, 0 not in c, 0


def _rules(name):
    if name == "tictactoe":
        return _ttt_legal, _ttt_step, 9
    if name == "connect4":
        return _c4_legal, _c4_step, _H
    raise ValueError("expert: needs a two-player board env")


_memo = {"tictactoe": {}, "connect4": {}}


def _value(name, legal, step, c, p, d):
    if d == 0:
        return 0
    memo = _memo[name]
    key = (c, p, d)
    v = memo.get(key)
    if v is None:
        v = max(_score(name, legal, step, c, p, a, d) for a in legal(c))
        if len(memo) > 2_000_000:
            memo.clear()
        memo[key] = v
    return v


def _score(name, legal, step, c, p, a, d):
    c2, done, w = step(c, p, a)
    if done:
        return 0 if w == 0 else d if w == p else -d
    return -_value(name, legal, step, c2, 3 - p, d - 1)


def expert_scores(name, board, player, depth):
    """score(s, a, depth) for the A actions of the position `board` ([p1, p2,
    empty] planes, taken as not finished) with `player` to move; ILLEGAL for
    an illegal action.  int32 (A,)."""
    legal, step, A = _rules(name)
    if player not in (1, 2):
        raise ValueError("expert: player must be 1 or 2")
    if not 1 <= depth <= 9:
        raise ValueError("expert: depth must be in 1..9")
    c = _cells(name, board)
    out = np.full(A, ILLEGAL, np.int32)
    for a in legal(c):
        out[a] = _score(name, legal, step, c, int(player), a, int(depth))
    return out


TTT_CODES = 3 ** 9
_TTT_FULL = 0x1FF
_TTT_LINE_MASKS = tuple(sum(1 << c for c in l) for l in _LINES)


def ttt_code(board, player):
    """The solved table's index of a TicTacToe position: the sum
    over the cells of 3^cell * d, d = 0 empty / 1 the mover's stone / 2 the
    other player's, cells in the planes' order."""
    c = _cells("tictactoe", board)
    if player not in (1, 2):
        raise ValueError("expert: player must be 1 or 2")
    return sum(3 ** k * (0 if x == 0 else 1 if x == player else 2) for k, x in enumerate(c))


def ttt_decode(code, player=1):
    """The [p1, p2, empty] planes (uint8 (27,)) of table index `code` with `player` to move."""
    b = np.zeros(27, np.uint8)
    for k in range(9):
        code, d = divmod(code, 3)
        b[18 + k if d == 0 else 9 * ((player if d == 1 else 3 - player) - 1) + k] = 1
    return b


_solved = {}


def _solved_value(me, opp, d):
    """V(s, d) of the mover-relative position (me, opp: cell bit masks), from the definition."""
    if d == 0:
        return 0
    key = (me, opp, d)
    v = _solved.get(key)
    if v is None:
        v = max(_solved_score(me, opp, a, d) for a in range(9) if not (me | opp) >> a & 1)
        _solved[key] = v
    return v


def _solved_score(me, opp, a, d):
    mine = me | 1 << a
    if any(opp & m == m for m in _TTT_LINE_MASKS):       # Q14: the player now to move holds a line and wins
        return -d
    if mine | opp == _TTT_FULL:
        return 0
    return -_solved_value(opp, mine, d - 1)


_table = None


def solved_table():
    """score(s, a, 9) of all 3^9 mover-relative TicTacToe boards, int8 (19683, 9), ILLEGAL for an occupied
    cell: the mirror of the device's solved table (mz_expert_table), written from the definition.  Every
    code is filled, unreachable and finished boards too, each move scored as if the game were still on."""
    global _table
    if _table is None:
        t = np.full((TTT_CODES, 9), ILLEGAL, np.int8)
        for code in range(TTT_CODES):
            me = opp = 0
            x = code
            for k in range(9):
                x, d = divmod(x, 3)
                me |= (d == 1) << k
                opp |= (d == 2) << k
            for a in range(9):
                if not (me | opp) >> a & 1:
                    t[code, a] = _solved_score(me, opp, a, 9)
        t.setflags(write=False)
        _table = t
    return _table


def judge_move(scores, action):
    """The judge's four terms of the 1-based `action` given its position's scores:
    (1, c == b, sgn(c) < sgn(b), b - c) with c the action's score and b the best legal score."""
    scores = np.asarray(scores)
    c = int(scores[action - 1])
    if c == ILLEGAL:
        raise ValueError("expert: action not legal on its board")
    b = int(scores[scores != ILLEGAL].max())
    return 1, int(c == b), int(np.sign(c) < np.sign(b)), b - c


def expert_pick(scores, r):
    """The expert's 1-based action: the k-th (ascending) of the best legal
    actions, k = rng_below(r, |best|) for the 32-bit draw r (the OPPONENT
    stream, as the random opponent's)."""
    scores = np.asarray(scores)
    best = np.flatnonzero((scores == scores.max()) & (scores != ILLEGAL))
    return int(best[rng_below(int(r), len(best))]) + 1
