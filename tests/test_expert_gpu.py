"""The rules-search expert opponent on the device (mz_expert_move):
mz_expert_eval against the Python mirror (games/expert.py) bit for bit,
evaluation play with MZ_OPP_EXPERT move for move against the host driver, the
invariant that nothing beats perfect TicTacToe play, exact resume from a
snapshot, and the refusals."""
import dataclasses

import numpy as np
import pytest

import expert_cases as xc

pytestmark = pytest.mark.gpu

ENV = {"tictactoe": 0, "connect4": 1}


def _mod(name):
    from muzero_jl_amd.games import connect4, tictactoe
    return (tictactoe, tictactoe.BatchedTicTacToe) if name == "tictactoe" else (connect4, connect4.BatchedConnect4)


def _engines(name, G, n=1, seed=5, wseed=105, **kw):
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod, _ = _mod(name)
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=64, **kw)
    nets = init_nets(conf, mod.hyper, seed=wseed)
    out = []
    for _ in range(n):
        e = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=seed)
        for k, w in enumerate(nets):
            e.set_weights(k, w)
        out.append(e)
    return out


def _mirror(name, pos, d):
    from muzero_jl_amd.games.expert import expert_scores
    return np.stack([expert_scores(name, b, p, d) for b, p in pos])


@pytest.mark.parametrize("name", xc.NAMES)
def test_expert_eval_matches_mirror(name):
    """G = 1, 5, 67 (a partial last workgroup); the empty TicTacToe board has 72
    live two-ply prefixes, more than the 64 lanes."""
    (eng,) = _engines(name, 4)
    if name == "tictactoe":
        pos = (xc.TTT_EMPTY, xc.TTT_Q14) + xc.random_positions(name)
        depths = (1, 2, 9)
    else:
        pos = xc.HAND[name] + xc.random_positions(name)
        depths = (1, 2, 3, 4)
    for G in (1, 5, 67):
        boards = np.stack([b for b, _ in pos[:G]])
        players = np.array([p for _, p in pos[:G]], np.int32)
        for d in depths:
            got = eng.expert_eval(ENV[name], boards, players, d)
            want = _mirror(name, pos[:G], d)
            assert got.dtype == np.int32 and np.array_equal(got, want), (G, d, np.argwhere(got != want)[:4])
    if name == "connect4":
        deep = xc.random_positions(name)[5:8]
        got = eng.expert_eval(ENV[name], np.stack([b for b, _ in deep]), [p for _, p in deep], 6)
        assert np.array_equal(got, _mirror(name, deep, 6))
    eng.close()


def _eval_play(name, mzp, depth, moves, G=16):
    """Host driver and device side by side; returns (tally of the host's games,
    device engine, the device boards after every move)."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    _, env_cls = _mod(name)
    eh, ed = _engines(name, G, n=2)
    sp = BatchedSelfPlay(eh, env_cls, G, game_offset=7, step0=100, opponent="expert", muzero_player=mzp,
                         expert_depth=depth)
    ed.selfplay_init(ENV[name], G, 64)
    ed.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, mzp)
    if depth is not None:
        ed.expert_depth(depth)
    trace = []
    for m in range(moves):
        sp.play_move(0.0)
        ed.selfplay_move(100 + m, game_offset=7, temperature=0.0)
        trace.append(ed.selfplay_slots()[1].copy())
    t = [0, 0, 0, 0]
    for h in sp.finished:
        w = game_winner(name, h.reward_history[-1], h.to_play_history[-1])
        t[0] += 1
        t[3 if w == 0 else 1 if w == mzp else 2] += 1
    assert t[0] > 0 and ed.eval_results() == tuple(t)
    assert ed.replay_counts()[0][0] == 0                      # evaluation play saves nothing
    ln, board, player = ed.selfplay_slots()
    assert np.array_equal(ln, [len(h.action_history) for h in sp.histories])
    assert np.array_equal(board, sp.env.board.astype(np.uint8)) and np.array_equal(player, sp.env.player)
    eh.close(); ed.close()
    return tuple(t), np.stack(trace)


@pytest.mark.parametrize("name,mzp,depth,moves", [("tictactoe", 1, None, 14), ("tictactoe", 2, None, 14),
                                                  ("connect4", 2, 3, 30)])
def test_expert_evaluation_play_matches_host(name, mzp, depth, moves):
    t, trace = _eval_play(name, mzp, depth, moves)
    if name == "tictactoe":
        assert t[1] == 0                                      # perfect play is never beaten
    if name == "tictactoe" and mzp == 1:                      # the depth setting reaches the kernel
        _, shallow = _eval_play(name, mzp, 1, moves)
        assert not np.array_equal(trace, shallow)


@pytest.mark.parametrize("mzp", [1, 2])
def test_muzero_never_beats_perfect_tictactoe(mzp):
    from muzero_jl_amd import abi
    (ed,) = _engines("tictactoe", 16)
    ed.selfplay_init(abi.ENV_TICTACTOE, 16, 64)
    ed.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, mzp)
    ed.expert_depth(9)
    for m in range(40):
        ed.selfplay_move(300 + m, game_offset=2, temperature=0.0)
    r = ed.eval_results()
    assert r[0] >= 16 * 4 and r[1] == 0 and r[0] == r[2] + r[3], r
    ed.close()


def test_expert_eval_run_resumes_from_snapshot(tmp_path):
    from muzero_jl_amd import abi
    G, cap = 12, 20

    def start(wseed=17, cap=cap):
        (e,) = _engines("tictactoe", G, wseed=wseed)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, 2)
        e.expert_depth(3)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(10 + m, 3, temperature=0.0)

    uncut = start()
    drive(uncut, 0, 24)
    first = start()
    drive(first, 0, 12)
    at_cut = first.eval_results()
    snap = str(tmp_path / "expert.safetensors")
    first.snapshot_save(snap, 0)
    first.close()
    second = start(wseed=99, cap=cap + 5)                     # other weights, another shard size, other moves
    drive(second, 40, 45)
    second.snapshot_load(snap)                                # keeps the handle's expert depth
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, 2)
    assert second.eval_results() == at_cut and at_cut[0] > 0
    drive(second, 12, 24)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    for a, b in zip(uncut.selfplay_slots(), second.selfplay_slots()):
        assert np.array_equal(a, b)
    uncut.close(); second.close()


def test_expert_refusals():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth
    from muzero_jl_amd.networks import init_nets
    (e,) = _engines("tictactoe", 4)
    b, p = xc.TTT_EMPTY
    good = e.expert_eval(abi.ENV_TICTACTOE, b, [p], 9)        # needs no selfplay_init
    assert good.tolist() == [[0] * 9]
    for d in (-1, 10):
        with pytest.raises(abi.MzError, match="depth"):
            e.expert_depth(d)
    for d in (0, 10):
        with pytest.raises(abi.MzError, match="depth"):
            e.expert_eval(abi.ENV_TICTACTOE, b, [p], d)
    for bad in xc.bad_boards("tictactoe"):
        with pytest.raises(abi.MzError, match="exactly one plane"):
            e.expert_eval(abi.ENV_TICTACTOE, bad, [1], 3)
    for bad_p in (0, 3):
        with pytest.raises(abi.MzError, match="player"):
            e.expert_eval(abi.ENV_TICTACTOE, b, [bad_p], 3)
    with pytest.raises(abi.MzError, match="Connect4 needs"):  # the shape check of mz_selfplay_init
        e.expert_eval(abi.ENV_CONNECT4, xc.C4_WIN[0], [1], 3)
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    with pytest.raises(abi.MzError, match="opponent"):
        e.selfplay_mode(abi.SP_EVAL, 3, 1)
    e.close()
    conf = dataclasses.replace(atari_synth.conf, num_iters=2, max_moves=6, batch_size=4)
    a = abi.Engine(conf, atari_synth.resnet_hyper, device=0, max_games=4, rng_seed=5)
    for n, w in enumerate(init_nets(conf, atari_synth.resnet_hyper, seed=17)):
        a.set_weights(n, w)
    a.selfplay_init(abi.ENV_ATARI, 4, 8)
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        a.selfplay_mode(abi.SP_EVAL, abi.OPP_EXPERT, 1)
    with pytest.raises(abi.MzError, match="expert: needs a two-player board env"):
        a.expert_eval(abi.ENV_ATARI, np.zeros((1, 27), np.uint8), [1], 3)
    a.close()
