"""The solved TicTacToe table and the move audit on the host (DESIGN §18.1,
§20.1): the table's index and its mirror games/expert.solved_table against the
rules-search mirror expert_scores, selfplay.evaluation_audit on hand-written
games, the binding's new signatures against include/mz.h, and the header's
index functions and a host-filled table as a stand-alone program under
AddressSanitizer + UBSan (tests/sanitize/expert_table_main.cpp).  Nothing
loaded into Python runs under a sanitizer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import expert_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "expert_table_main.cpp")


def _swap(board):
    b = np.asarray(board).reshape(3, -1)
    return np.concatenate([b[1], b[0], b[2]]).astype(np.uint8)


def test_ttt_code_round_trips():
    from muzero_jl_amd.games.expert import TTT_CODES, ttt_code, ttt_decode
    assert TTT_CODES == 19683
    assert ttt_code(xc.TTT_EMPTY[0], 1) == 0 == ttt_code(xc.TTT_EMPTY[0], 2)
    b = xc.ttt_board(["1..", "2..", "..."])                   # cell = row + 3 * column: X on cell 0, O on cell 1
    assert ttt_code(b, 1) == 1 + 2 * 3 and ttt_code(b, 2) == 2 + 1 * 3
    for code in range(TTT_CODES):
        for p in (1, 2):
            board = ttt_decode(code, p)
            assert board.reshape(3, 9).sum(0).tolist() == [1] * 9
            assert ttt_code(board, p) == code
        assert np.array_equal(ttt_decode(code, 2), _swap(ttt_decode(code, 1)))
    for bad in xc.bad_boards("tictactoe"):
        with pytest.raises(ValueError):
            ttt_code(bad, 1)
    with pytest.raises(ValueError):
        ttt_code(xc.TTT_EMPTY[0], 3)


def _playouts(n, seed):
    """Every position of n uniform random playouts, the finished last boards included."""
    from muzero_jl_amd.games.tictactoe import BatchedTicTacToe
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        env = BatchedTicTacToe(1)
        done = False
        while not done:
            out.append((env.board[0].astype(np.uint8), int(env.player[0])))
            a = int(rng.choice(np.flatnonzero(env.legal_mask()[0]))) + 1
            _, d = env.step(np.array([a], np.int32))
            done = bool(d[0])
        if env.legal_mask()[0].any():
            out.append((env.board[0].astype(np.uint8), int(env.player[0])))
    return out


def test_solved_table_matches_the_rules_search():
    from muzero_jl_amd.games.expert import ILLEGAL, expert_scores, solved_table, ttt_code, ttt_decode
    t = solved_table()
    assert t.shape == (19683, 9) and t.dtype == np.int8 and solved_table() is t
    assert t[0].tolist() == [0] * 9                            # the empty board: perfect play draws
    assert np.array_equal(expert_scores("tictactoe", xc.TTT_EMPTY[0], 1, 9), t[0])
    pos = _playouts(50, seed=3)
    assert len(pos) > 300
    for b, p in pos:
        assert np.array_equal(expert_scores("tictactoe", b, p, 9), t[ttt_code(b, p)]), (b, p)
    rng = np.random.default_rng(11)
    for code in rng.choice(19683, 300, replace=False):
        code = int(code)
        for p in (1, 2):                                       # swapped stones, the other mover: the same entry
            b = ttt_decode(code, p)
            assert ttt_code(b, p) == code
            assert np.array_equal(expert_scores("tictactoe", b, p, 9), t[code]), (code, p)
    occupied = np.array([[(c // 3 ** k) % 3 != 0 for k in range(9)] for c in range(19683)])
    assert np.array_equal(t == ILLEGAL, occupied)
    assert np.abs(t[~occupied]).max() <= 9


def _history(moves):
    """A GameHistory from (board, to_play, action) triples."""
    from muzero_jl_amd.selfplay import GameHistory
    return GameHistory(observation_history=[np.asarray(b, np.float32) for b, _, _ in moves],
                       action_history=[a for _, _, a in moves], to_play_history=[p for _, p, _ in moves],
                       reward_history=[0.0] * len(moves), child_visits=[None] * len(moves),
                       root_values=[0.0] * len(moves))


def _perfect_game():
    """Both sides play the first of the table's best moves from the empty board."""
    from muzero_jl_amd.games.expert import solved_table, ttt_code
    from muzero_jl_amd.games.tictactoe import BatchedTicTacToe
    env = BatchedTicTacToe(1)
    moves, done = [], False
    while not done:
        b, p = env.board[0].astype(np.uint8), int(env.player[0])
        a = int(np.argmax(solved_table()[ttt_code(b, p)])) + 1
        moves.append((b, p, a))
        _, d = env.step(np.array([a], np.int32))
        done = bool(d[0])
    return moves


# X (player 1) to move on cells X: 3, 4, 8, O: 0, 1, 5, empty: 2, 6, 7.  O threatens 0-1-2.  Cell 2 blocks
# and the board fills up: a draw, score 0.  Cell 6 (or 7) lets O complete the line on cell 2; X's forced
# last move then ends the game with O holding a line (Q14), three plies in: score -(9 - 2) = -7.
def _blunder_board():
    b = np.zeros(27, np.uint8)
    for c in range(9):
        b[c if c in (3, 4, 8) else 9 + c if c in (0, 1, 5) else 18 + c] = 1
    return b


def test_evaluation_audit_on_hand_written_games():
    from muzero_jl_amd.games.expert import expert_scores, judge_move
    from muzero_jl_amd.selfplay import evaluation_audit
    game = _perfect_game()
    n = len(game)
    assert n == 9                                              # perfect play fills the board
    assert evaluation_audit([_history(game)], "tictactoe", "self", 1) == (n, n, 0, 0)
    # the counting rule: against an opponent only the records with to_play == muzero_player
    assert evaluation_audit([_history(game)], "tictactoe", "random", 1) == (5, 5, 0, 0)
    assert evaluation_audit([_history(game)], "tictactoe", "expert", 2) == (4, 4, 0, 0)
    assert evaluation_audit([_history(game), _history(game)], "tictactoe", "self", 2) == (2 * n, 2 * n, 0, 0)
    # one move that turns a draw into a loss
    b = _blunder_board()
    assert expert_scores("tictactoe", b, 1, 9).tolist() == [-128, -128, 0, -128, -128, -128, -7, -7, -128]
    assert judge_move(expert_scores("tictactoe", b, 1, 9), 7) == (1, 0, 1, 7)
    lost = game[:2] + [(b, 1, 7)]
    assert evaluation_audit([_history(lost)], "tictactoe", "self", 1) == (3, 2, 1, 7)
    assert evaluation_audit([_history(lost)], "tictactoe", "random", 1) == (2, 1, 1, 7)
    assert evaluation_audit([_history(lost)], "tictactoe", "random", 2) == (1, 1, 0, 0)
    assert evaluation_audit([_history([(b, 1, 3)])], "tictactoe", "self", 1) == (1, 1, 0, 0)
    # a depth below 9 goes through the rules search, not the table: one ply sees no danger
    assert evaluation_audit([_history([(b, 1, 7)])], "tictactoe", "self", 1, depth=1) == (1, 1, 0, 0)
    with pytest.raises(ValueError, match="not legal"):
        evaluation_audit([_history([(b, 1, 1)])], "tictactoe", "self", 1)
    # Connect4 at depth 2.  C4_BLOCK: only column 1 stops the four, score 0; every other column loses
    # one ply later, -(2 - 1).  C4_WIN: column 0 wins at once, +2; column 1 blocks, 0; column 3 loses, -1.
    blk, win = xc.C4_BLOCK[0], xc.C4_WIN[0]
    assert expert_scores("connect4", blk, 1, 2).tolist() == [-1, 0, -1, -1, -1, -1, -1]
    assert expert_scores("connect4", win, 1, 2).tolist() == [2, 0, -1, -1, -1, -1, -1]
    c4 = _history([(blk, 1, 2), (blk, 1, 4), (win, 1, 1), (win, 1, 2), (win, 1, 4)])
    assert evaluation_audit([c4], "connect4", "self", 1, depth=2) == (5, 2, 3, 0 + 1 + 0 + 2 + 3)
    assert evaluation_audit([c4], "connect4", "expert", 2, depth=2) == (0, 0, 0, 0)


def test_binding_matches_the_header():
    from muzero_jl_amd import abi
    hdr = open(os.path.join(ROOT, "include", "mz.h")).read()
    vp, ci, i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32
    want = {"mz_expert_table": (ci, [vp, ci]),
            "mz_expert_table_get": (ci, [vp, vp, vp, vp]),
            "mz_expert_judge": (ci, [vp, ci, ci, vp, vp, vp, ci, vp]),
            "mz_test_audit": (ci, [vp, ci]),
            "mz_test_audit_results": (ci, [vp, vp, vp, i32])}
    ctype_of = {"int32_t": i32, "int": ci}
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    jl = open(os.path.join(ROOT, "julia", "LibMZ.jl")).read()
    for name, sig in want.items():
        assert abi.SIGNATURES[name] == sig, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", body, flags=re.M)
        assert m, name
        params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
        assert len(params) == len(sig[1]), name
        for p, t in zip(params, sig[1]):                       # scalars by type, every pointer as void*
            assert (t is vp) == ("*" in p), (name, p)
            if "*" not in p:
                assert ctype_of[p.rsplit(" ", 1)[0]] is t, (name, p)
        assert f"(:{name}, libmz)" in jl, name
    for meth in ("expert_table", "expert_table_get", "expert_judge", "test_audit", "test_audit_results"):
        assert callable(getattr(abi.Engine, meth))
    assert abi.TTT_CODES == 19683 and len(abi.TEST_AUDIT_FIELDS) == 4


def test_table_header_sanitizer_clean(tmp_path):
    from muzero_jl_amd.games.expert import solved_table
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "expert_table_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    rng = np.random.default_rng(5)
    codes = [0, 19682] + [int(c) for c in rng.choice(19683, 1998, replace=False)]
    lines = [str(c) for c in codes] + ["-1", "19683", "x"]
    path = tmp_path / "codes.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    got = r.stdout.splitlines()
    assert got[0] == "roundtrip ok" and f"{len(lines)} codes" in r.stderr
    t = solved_table()
    want = [f"{c} " + " ".join(str(int(s)) for s in t[c]) for c in codes] + ["rejected"] * 3
    assert got[1:] == want, [(g, w) for g, w in zip(got[1:], want) if g != w][:5]
