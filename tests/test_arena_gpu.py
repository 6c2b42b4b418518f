"""Net against net on the device (MZ_OPP_NETWORK, mz_sp_pick), bit
for bit: equal nets are self-play, evaluation play move for move against the
host driver with two engines, the three ways to fill the opponent set, the
refusals and the absence of side effects, and exact resume from a snapshot.
G = 10 and 6 leave a partial last workgroup in the one-wave-per-slot kernels."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = {"tictactoe": 0, "connect4": 1}
SEED = 5                                       # the engines' rng_seed: one Philox key space for both sides


def _mod(name):
    from muzero_jl_amd.games import connect4, tictactoe
    return (tictactoe, tictactoe.BatchedTicTacToe) if name == "tictactoe" else (connect4, connect4.BatchedConnect4)


def _conf(name, resnet=False, **kw):
    mod, _ = _mod(name)
    kw.setdefault("num_iters", 4 if resnet else 6)
    return dataclasses.replace(mod.conf, replay_buffer_size=64, **kw), (mod.resnet_hyper if resnet else mod.hyper)


def _nets(name, wseed, resnet=False, **kw):
    from muzero_jl_amd.networks import init_nets
    return init_nets(*_conf(name, resnet, **kw), seed=wseed)


def _engine(name, G, wseed, resnet=False, **kw):
    from muzero_jl_amd import abi
    conf, hyper = _conf(name, resnet, **kw)
    e = abi.Engine(conf, hyper, device=0, max_games=G, rng_seed=SEED)
    for k, w in enumerate(_nets(name, wseed, resnet, **kw)):
        e.set_weights(k, w)
    return e


def _fill(e, nets):
    for k, w in enumerate(nets):
        e.opponent_set_weights(k, w)


def _play(e, name, G, opponent, mzp, moves, temperature=0.0, step0=100, goff=7, init=True):
    """Evaluation play on the device: ([slots after every move], the tally)."""
    from muzero_jl_amd import abi
    if init:
        e.selfplay_init(ENV[name], G, 64)
    e.selfplay_mode(abi.SP_EVAL, opponent, mzp)
    trace = []
    for m in range(moves):
        e.selfplay_move(step0 + m, game_offset=goff, temperature=temperature)
        trace.append(e.selfplay_slots())
    return trace, e.eval_results()


def _same_trace(a, b):
    assert len(a) == len(b)
    for m, (x, y) in enumerate(zip(a, b)):
        for u, v, what in zip(x, y, ("lengths", "boards", "players")):
            assert np.array_equal(u, v), (m, what)


def _boards(trace):
    return np.stack([t[1] for t in trace])


@pytest.mark.parametrize("mzp", [1, 2])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_equal_nets_are_selfplay(mzp, temperature):
    """The opponent set's images equal those mz_weights_set builds, and the pick copies whole results."""
    from muzero_jl_amd import abi
    G = 10
    arena, plain = _engine("tictactoe", G, 105), _engine("tictactoe", G, 105)
    _fill(arena, _nets("tictactoe", 105))
    ta, ra = _play(arena, "tictactoe", G, abi.OPP_NETWORK, mzp, 14, temperature)
    tp, rp = _play(plain, "tictactoe", G, abi.OPP_SELF, mzp, 14, temperature)
    _same_trace(ta, tp)
    assert ra == rp and ra[0] > 0
    arena.close(); plain.close()


@pytest.mark.parametrize("name,resnet,G,mzp,moves", [("tictactoe", False, 10, 1, 14), ("tictactoe", False, 10, 2, 14),
                                                     ("connect4", False, 10, 2, 30), ("tictactoe", True, 6, 1, 12)])
def test_device_matches_host_mirror(name, resnet, G, mzp, moves):
    """A: the host side's MuZero; B: the opponent's weights; D: the device engine, A's weights and the
    opponent set = B's."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    _, env_cls = _mod(name)
    ea, eb, ed = _engine(name, G, 105, resnet), _engine(name, G, 211, resnet), _engine(name, G, 105, resnet)
    _fill(ed, _nets(name, 211, resnet))
    sp = BatchedSelfPlay(ea, env_cls, G, opponent="network", opponent_engine=eb, muzero_player=mzp, game_offset=7,
                         step0=100)
    ed.selfplay_init(ENV[name], G, 64)
    ed.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, mzp)
    trace = []
    for m in range(moves):
        sp.play_move(0.0)
        ed.selfplay_move(100 + m, game_offset=7, temperature=0.0)
        trace.append(ed.selfplay_slots())
        assert np.array_equal(trace[-1][1], sp.env.board.astype(np.uint8)), m   # (both restart finished slots)
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
    if name == "tictactoe" and not resnet:                    # the pick fires: A alone plays another match
        alone, _ = _play(ea, name, G, abi.OPP_SELF, mzp, moves)
        assert not np.array_equal(_boards(alone), _boards(trace))
    ea.close(); eb.close(); ed.close()


def test_three_ways_to_fill_the_set_agree(tmp_path):
    from muzero_jl_amd import abi
    G, name = 10, "tictactoe"
    src = _nets(name, 211)

    def check(e):
        for k in range(3):
            assert np.array_equal(e.opponent_get_weights(k), src[k]), k
        return _play(e, name, G, abi.OPP_NETWORK, 1, 8)

    by_set = _engine(name, G, 105)
    _fill(by_set, src)
    want, tally = check(by_set)

    saver = _engine(name, G, 211)
    ckpt = str(tmp_path / "opp.safetensors")
    saver.checkpoint_save(ckpt, 4321)
    saver.close()
    by_load = _engine(name, G, 105)
    mine = [by_load.get_weights(k) for k in range(3)]
    assert by_load.opponent_load(ckpt) == 4321
    for k in range(3):                                         # the learner's nets are not touched
        assert np.array_equal(by_load.get_weights(k), mine[k])
    got, t2 = check(by_load)
    _same_trace(got, want)
    assert t2 == tally

    by_from = _engine(name, G, 211)                            # its own nets are the opponent's ...
    by_from.opponent_from(abi.TRAIN_LEARNER)
    for k, w in enumerate(_nets(name, 105)):                   # ... and its playing nets are then replaced
        by_from.set_weights(k, w)
    got, t3 = check(by_from)
    _same_trace(got, want)
    assert t3 == tally
    # the differing nets matter: equal nets play another match
    _fill(by_set, _nets(name, 105))
    other, _ = _play(by_set, name, G, abi.OPP_NETWORK, 1, 8)
    assert not np.array_equal(_boards(other), _boards(want))
    by_set.close(); by_load.close(); by_from.close()


def test_opponent_from_the_train_loops_sets():
    from muzero_jl_amd import abi
    G = 10
    e = _engine("tictactoe", G, 105, batch_size=4, checkpoint_interval=3, training_steps=10000)
    e.selfplay_init(abi.ENV_TICTACTOE, G, 64)
    e.train_init(4)
    st = e.train_run(12, move0=30, game_offset=2)
    assert st[2] >= 2                                          # refreshes: the three sets differ
    sets = {w: [e.train_weights(w, k) for k in range(3)]
            for w in (abi.TRAIN_LEARNER, abi.TRAIN_ACTOR, abi.TRAIN_QUEUED)}
    assert not np.array_equal(sets[abi.TRAIN_ACTOR][0], sets[abi.TRAIN_QUEUED][0])
    assert not np.array_equal(sets[abi.TRAIN_LEARNER][0], sets[abi.TRAIN_ACTOR][0])
    for which, want in sets.items():
        e.opponent_from(which)
        for k in range(3):
            assert np.array_equal(e.opponent_get_weights(k), want[k]), (which, k)
            assert np.array_equal(e.train_weights(which, k), want[k])
    e.close()


def test_refusals_and_no_side_effects(tmp_path):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth, tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    G, name = 10, "tictactoe"
    e = _engine(name, G, 105)
    e.selfplay_init(abi.ENV_TICTACTOE, G, 64)
    src = _nets(name, 211)
    with pytest.raises(abi.MzError, match="opponent"):         # no set at all
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 1)
    with pytest.raises(abi.MzError, match="mz_train_init first"):
        e.opponent_from(abi.TRAIN_ACTOR)
    with pytest.raises(abi.MzError, match="wrong parameter count"):
        e.opponent_set_weights(0, src[0][:-1])
    e.opponent_set_weights(0, src[0])
    e.opponent_set_weights(2, src[2])
    with pytest.raises(abi.MzError, match="opponent"):         # two of the three nets
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 1)
    with pytest.raises(abi.MzError, match="never given"):
        e.opponent_get_weights(1)
    e.opponent_set_weights(1, src[1])
    e.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 1)
    e.selfplay_mode(abi.SP_TRAIN, abi.OPP_SELF, 1)

    # refused files leave the set and the learner's nets as they were
    rn, shp = str(tmp_path / "resnet.safetensors"), str(tmp_path / "narrow.safetensors")
    for path, hyper in ((rn, ttt.resnet_hyper), (shp, dataclasses.replace(ttt.hyper, width_hidden=32))):
        other = abi.Engine(_conf(name)[0], hyper, device=0, max_games=2, rng_seed=SEED)
        other.checkpoint_save(path, 1)
        other.close()
    for path, msg in ((rn, "network"), (shp, "shape"), (str(tmp_path / "none.safetensors"), "cannot open")):
        with pytest.raises(abi.MzError, match=msg):
            e.opponent_load(path)
        for k in range(3):
            assert np.array_equal(e.opponent_get_weights(k), src[k]), (path, k)
            assert np.array_equal(e.get_weights(k), _nets(name, 105)[k]), (path, k)

    # an engine that holds a set but plays another mode is the engine without one
    bare = _engine(name, G, 105)
    for opp in (abi.OPP_SELF, abi.OPP_RANDOM, abi.OPP_EXPERT):
        with_set, r1 = _play(e, name, G, opp, 2, 8)
        without, r2 = _play(bare, name, G, opp, 2, 8)
        _same_trace(with_set, without)
        assert r1 == r2
    e.close(); bare.close()

    conf = dataclasses.replace(atari_synth.conf, num_iters=2, max_moves=6, batch_size=4)
    a = abi.Engine(conf, atari_synth.resnet_hyper, device=0, max_games=4, rng_seed=5)
    for n, w in enumerate(init_nets(conf, atari_synth.resnet_hyper, seed=17)):
        a.set_weights(n, w)
    a.selfplay_init(abi.ENV_ATARI, 4, 8)
    a.opponent_from(abi.TRAIN_LEARNER)
    with pytest.raises(abi.MzError, match="opponent network: needs a two-player board env"):
        a.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 1)
    a.close()


def test_arena_run_resumes_from_snapshot(tmp_path):
    from muzero_jl_amd import abi
    G, cap, name = 10, 20, "tictactoe"
    opp = _nets(name, 211)

    def start(wseed=105, cap=cap):
        e = _engine(name, G, wseed)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        _fill(e, opp)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 2)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(10 + m, 3, temperature=0.0)

    uncut = start()
    drive(uncut, 0, 20)
    first = start()
    drive(first, 0, 10)
    at_cut = first.eval_results()
    snap = str(tmp_path / "arena.safetensors")
    first.snapshot_save(snap, 0)
    first.close()
    second = _engine(name, G, 99)                              # other weights, another shard size, no set yet
    second.selfplay_init(abi.ENV_TICTACTOE, G, cap + 5)
    drive(second, 40, 43)
    second.snapshot_load(snap)                                 # the learner's nets come from the file ...
    _fill(second, opp)                                         # ... the opponent's and the mode from the host
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_NETWORK, 2)
    assert second.eval_results() == at_cut and at_cut[0] > 0
    drive(second, 10, 20)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    for a, b in zip(uncut.selfplay_slots(), second.selfplay_slots()):
        assert np.array_equal(a, b)
    # a loader that was already in the mode keeps its set and its mode across the load
    third = start(wseed=99, cap=cap + 5)
    drive(third, 40, 43)
    third.snapshot_load(snap)
    drive(third, 10, 20)
    assert third.eval_results() == uncut.eval_results()
    uncut.close(); second.close(); third.close()
