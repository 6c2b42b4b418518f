"""The solved TicTacToe table on the device (mz_expert_table): the
table against the search kernel on all 19683 codes and against the host
mirror, when the lookup is in use, evaluation play and the test worker with
the table off and on bit for bit (and against the host driver), exact resume
from a snapshot with the table on, and the refusals.  E = 5 leaves idle waves
in the last workgroup of the one-wave-per-slot kernels."""
import numpy as np
import pytest

import worker_ref as wr

pytestmark = pytest.mark.gpu


def _engines(name, G, n=1, **kw):
    import test_expert_gpu as xg
    return xg._engines(name, G, n=n, **kw)


@pytest.fixture(scope="module")
def all_codes():
    """The boards of every table code as player 1 and as player 2 (stones swapped) sees them."""
    from muzero_jl_amd.games.expert import TTT_CODES, ttt_decode
    return {p: np.stack([ttt_decode(c, p) for c in range(TTT_CODES)]) for p in (1, 2)}


def test_table_equals_the_search_and_the_mirror(all_codes):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games.expert import solved_table
    (e,) = _engines("tictactoe", 4)
    assert e.expert_table_get(scores=False) == (None, False, False)
    e.expert_table(True)
    table, built, in_use = e.expert_table_get()
    assert built and not in_use                               # no env yet: nothing would be launched
    assert table.dtype == np.int8 and table.shape == (19683, 9)
    for p in (1, 2):                                          # bit for bit the search kernel's scores, either mover
        got = e.expert_eval(abi.ENV_TICTACTOE, all_codes[p], np.full(19683, p, np.int32), 9)
        assert np.array_equal(got, table.astype(np.int32)), (p, np.argwhere(got != table)[:4])
    assert np.array_equal(table, solved_table()), np.argwhere(table != solved_table())[:4]
    e.expert_table(True)                                      # again: the same table, nothing rebuilt
    assert np.array_equal(e.expert_table_get()[0], table)
    e.close()


def test_when_the_lookup_is_in_use():
    from muzero_jl_amd import abi
    (e,) = _engines("tictactoe", 4)
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    assert e.expert_table_get(scores=False)[1:] == (False, False)
    e.expert_table(True)
    assert e.expert_table_get(scores=False)[1:] == (True, True)
    e.expert_depth(5)
    assert e.expert_table_get(scores=False)[1:] == (True, False)
    e.expert_depth(9)
    assert e.expert_table_get(scores=False)[1:] == (True, True)
    e.expert_depth(0)                                         # the env's default is 9
    e.expert_table(False)
    assert e.expert_table_get(scores=False)[1:] == (True, False)
    e.expert_table(True)
    e.selfplay_init(abi.ENV_TICTACTOE, 2, 4)                  # a handle setting: kept, the table too
    assert e.expert_table_get(scores=False)[1:] == (True, True)
    e.close()
    (c,) = _engines("connect4", 4)
    c.selfplay_init(abi.ENV_CONNECT4, 4, 8)
    with pytest.raises(abi.MzError, match="TicTacToe needs"):
        c.expert_table(True)
    c.expert_table(False)
    assert c.expert_table_get(scores=False) == (None, False, False)
    with pytest.raises(abi.MzError, match="not built"):
        c.expert_table_get()
    c.close()


def _snapshot_arrays(e, path):
    from muzero_jl_amd import checkpoint as ck
    e.snapshot_save(path, 0)
    return ck.read(path)[0]


@pytest.mark.parametrize("mzp", [1, 2])
def test_evaluation_play_table_off_and_on(mzp, tmp_path):
    """12 moves of G = 16 slots: the two engines agree after every move and in everything a snapshot
    holds (the games in progress, record for record), and with the host driver."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.games.tictactoe import BatchedTicTacToe
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    G, moves = 16, 12
    eh, off, on = _engines("tictactoe", G, n=3)
    sp = BatchedSelfPlay(eh, BatchedTicTacToe, G, game_offset=7, step0=100, opponent="expert", muzero_player=mzp)
    for e in (off, on):
        e.selfplay_init(abi.ENV_TICTACTOE, G, 64)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, mzp)
    on.expert_table(True)
    assert on.expert_table_get(scores=False)[2] and not off.expert_table_get(scores=False)[2]
    for m in range(moves):
        sp.play_move(0.0)
        for e in (off, on):
            e.selfplay_move(100 + m, game_offset=7, temperature=0.0)
        for a, b in zip(off.selfplay_slots(), on.selfplay_slots()):
            assert np.array_equal(a, b), m
    t = [0, 0, 0, 0]
    for h in sp.finished:
        w = game_winner("tictactoe", h.reward_history[-1], h.to_play_history[-1])
        t[0] += 1
        t[3 if w == 0 else 1 if w == mzp else 2] += 1
    assert t[0] >= G and t[1] == 0
    assert on.eval_results() == off.eval_results() == tuple(t)
    ln, board, player = on.selfplay_slots()
    assert np.array_equal(ln, [len(h.action_history) for h in sp.histories])
    assert np.array_equal(board, sp.env.board.astype(np.uint8)) and np.array_equal(player, sp.env.player)
    a, b = _snapshot_arrays(off, str(tmp_path / "off.safetensors")), _snapshot_arrays(on, str(tmp_path / "on.safetensors"))
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    eh.close(); off.close(); on.close()


@pytest.mark.parametrize("mzp", [1, 2])
def test_test_worker_table_off_and_on(mzp):
    from muzero_jl_amd import abi
    E = wr.E
    off, on = _engines("tictactoe", 8, n=2, max_moves=wr.MAX_MOVES)
    for e in (off, on):
        e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
        e.test_config(E, abi.OPP_EXPERT, mzp)
    on.expert_table(True)
    for e in (off, on):
        e.test_play(3, wr.STEP0, game_offset=wr.GOFF, temperature=wr.TEMP)
    (ra,), (rb,) = off.test_results(1)[1], on.test_results(1)[1]
    assert wr.same_record(ra, rb) and ra["games"] == E and ra["muzero_wins"] == 0, (ra, rb)
    for g in range(E):
        assert wr.same_history(off.test_get_game(g), on.test_get_game(g)), g
    off.close(); on.close()


def test_expert_eval_run_with_the_table_resumes_from_snapshot(tmp_path):
    from muzero_jl_amd import abi
    G, cap = 12, 20

    def start(wseed=17, cap=cap):
        (e,) = _engines("tictactoe", G, wseed=wseed)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, 2)
        e.expert_table(True)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(10 + m, 3, temperature=0.0)

    uncut = start()
    drive(uncut, 0, 24)
    first = start()
    drive(first, 0, 12)
    at_cut = first.eval_results()
    snap = str(tmp_path / "table.safetensors")
    first.snapshot_save(snap, 0)
    first.close()
    second = start(wseed=99, cap=cap + 5)                     # other weights, another shard size, other moves
    drive(second, 40, 45)
    second.snapshot_load(snap)                                # keeps the handle's switch and its table
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, 2)
    assert second.expert_table_get(scores=False)[1:] == (True, True)
    assert second.eval_results() == at_cut and at_cut[0] > 0
    drive(second, 12, 24)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    for a, b in zip(uncut.selfplay_slots(), second.selfplay_slots()):
        assert np.array_equal(a, b)
    uncut.close(); second.close()
