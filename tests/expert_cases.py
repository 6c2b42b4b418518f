"""Positions shared by the expert-opponent tests (test_expert.py,
test_expert_rules_host.py, test_expert_gpu.py): random-play positions of both
board envs and the hand-made ones.  A position is (board uint8 planes, player)."""
import functools

import numpy as np

NAMES = ("tictactoe", "connect4")
DEPTHS = {"tictactoe": (1, 2, 9), "connect4": (1, 2, 4)}


def _env(name, G=1):
    from muzero_jl_amd.games import connect4, tictactoe
    return tictactoe.BatchedTicTacToe(G) if name == "tictactoe" else connect4.BatchedConnect4(G)


@functools.lru_cache(maxsize=None)
def random_positions(name, n=200, seed=0):
    """n live positions met by uniform random legal play from the initial
    board, whole games one after the other: every ply count a game reaches."""
    rng = np.random.default_rng(seed)
    env = _env(name)
    out = []
    while len(out) < n:
        legal = env.legal_mask()[0]
        out.append((env.board[0].astype(np.uint8), int(env.player[0])))
        a = int(rng.choice(np.flatnonzero(legal))) + 1
        _, done = env.step(np.array([a], np.int32))
        if done[0]:
            env.reset(np.array([0]))
    return tuple(out)


def plies(name, board):
    cells = 9 if name == "tictactoe" else 42
    return int(np.asarray(board)[:2 * cells].sum())


def c4_board(columns):
    """Connect4 planes from per-column strings of '1' / '2', bottom first."""
    b = np.zeros(126, np.uint8)
    b[84:] = 1
    for h, col in enumerate(columns):
        for w, ch in enumerate(col):
            b[84 + w + 6 * h] = 0
            b[(int(ch) - 1) * 42 + w + 6 * h] = 1
    return b


def ttt_board(rows):
    """TicTacToe planes from three strings of '1' / '2' / '.'; cell = row + 3 * column
    (column-major: the string index is the column)."""
    b = np.zeros(27, np.uint8)
    for r, row in enumerate(rows):
        for c, ch in enumerate(row):
            cell = r + 3 * c
            b[18 + cell if ch == "." else 9 * (int(ch) - 1) + cell] = 1
    return b


# player 1 to move holds three in column 0: dropping there wins at once
C4_WIN = (c4_board(["111", "222", "", "", "", "", ""]), 1)
# player 1 to move has no win, player 2 threatens column 1 (three stacked): depth 2 must block
C4_BLOCK = (c4_board(["1", "222", "", "1", "", "", "1"]), 1)
# column 3 is full: six legal actions
C4_FULLCOL = (c4_board(["", "", "", "121212", "", "", ""]), 1)
# one empty cell (the top of column 6), no four anywhere: any depth sees one move, a draw
C4_LAST = (c4_board(["112211", "221122", "112211", "221122", "112211", "221122", "11221"]), 2)
# Q14: player 1 (not to move) already holds the line 0,3,6 (row 0); player 2 to move: every reply ends
# the game with winner 1 = 3 - mover
TTT_Q14 = (ttt_board(["111", "22.", "..."]), 2)
TTT_EMPTY = (ttt_board(["...", "...", "..."]), 1)

HAND = {"connect4": (C4_WIN, C4_BLOCK, C4_FULLCOL, C4_LAST), "tictactoe": (TTT_Q14, TTT_EMPTY)}


def bad_boards(name):
    """Plane sets mz_expert_eval refuses: a cell in no plane, a cell in two."""
    good = HAND[name][0][0]
    cells = len(good) // 3
    none = good.copy()
    none[2 * cells + cells - 1] = 0
    none[cells - 1] = 0
    none[cells + cells - 1] = 0
    two = good.copy()
    two[cells - 1] = 1
    two[cells + cells - 1] = 1
    two[2 * cells + cells - 1] = 0
    return none, two
