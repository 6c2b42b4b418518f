"""The network-only player on the device (mz_prior_fc / mz_prior_pick,
mz_eval_players), bit for bit: mz_prior_eval against the Python
mirror (selfplay.prior_move) and the engine's own net_forward pair on FC,
BatchNorm, ResNet and downsampler engines, the keys, the opponent weight set,
evaluation play with every pair of player kinds move for move against the host
driver and through the test worker with its record and audit, the launches a
move issues, exact resume from a snapshot, the refusals, and that the setting
changes nothing outside evaluation play."""
import dataclasses

import numpy as np
import pytest

import prior_cases as pc
import weight_regimes as wrg
import worker_ref as wr

pytestmark = pytest.mark.gpu

INF = float("inf")
KIND = {"search": 0, "prior": 1}
OPP = {"self": 0, "random": 1, "expert": 2, "network": 3}


def _game(name):
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth, connect4, tictactoe
    return {"ttt": (tictactoe, tictactoe.BatchedTicTacToe, abi.ENV_TICTACTOE),
            "c4": (connect4, connect4.BatchedConnect4, abi.ENV_CONNECT4),
            "atari": (atari_synth, atari_synth.BatchedAtariSynth, abi.ENV_ATARI)}[name]


def _setup(name, resnet=False, bn=False, **conf_kw):
    mod = _game(name)[0]
    hyper = mod.resnet_hyper if (resnet or name == "atari") else mod.hyper
    if bn:
        hyper = dataclasses.replace(hyper, use_batch_norm=True)
    conf_kw.setdefault("num_iters", 4)
    return dataclasses.replace(mod.conf, replay_buffer_size=64, **conf_kw), hyper


def _engine(conf, hyper, nets, max_games, seed=wr.SEED):
    from muzero_jl_amd import abi
    e = abi.Engine(conf, hyper, device=0, max_games=max_games, rng_seed=seed)
    for k, w in enumerate(nets):
        e.set_weights(k, w)
    return e


def _nets(conf, hyper, wseed=wr.WSEED):
    from muzero_jl_amd.networks import init_nets
    return init_nets(conf, hyper, seed=wseed)


def _rows(conf, G, kind, seed):
    """G observation rows and their legal masks: "full", "single" (one action) or "random"."""
    from muzero_jl_amd.config import stacked_features
    rng = np.random.default_rng(seed)
    A = len(conf.action_space)
    obs = (rng.random((G, stacked_features(conf))) < 0.4).astype(np.float32)
    if kind == "full":
        legal = np.ones((G, A), bool)
    elif kind == "single":
        legal = np.zeros((G, A), bool)
        legal[np.arange(G), rng.integers(0, A, G)] = True
    else:
        legal = rng.random((G, A)) < 0.5
        legal[np.arange(G), rng.integers(0, A, G)] = True
    return obs, legal


def _same_move(got, want, what):
    (pol, val, act), (wpol, wval, wact) = got, want
    assert pol.dtype == np.float32 and val.dtype == np.float32 and act.dtype == np.int32, what
    assert np.array_equal(pol.view(np.uint32), wpol.view(np.uint32)), (what, "policy", np.argwhere(pol != wpol)[:4])
    assert np.array_equal(val.view(np.uint32), wval.view(np.uint32)), (what, "value")
    assert np.array_equal(act, wact), (what, "action", act, wact)


def _check_rows(eng, conf, Gs, temps, masks, dm, seed=0):
    """mz_prior_eval against the mirror on the same engine's net_forward pair, every combination."""
    from muzero_jl_amd.selfplay import prior_move
    n = 0
    for G in Gs:
        for kind in masks:
            obs, legal = _rows(conf, G, kind, seed + 17 * G)
            for T in temps:
                step, goff = 5 + n, 3 + 2 * n
                got = eng.prior_eval(obs, legal, rng_step=step, game_offset=goff, temperature=T)
                want = prior_move(eng, obs, legal, T, eng.rng_seed, goff, step, dm)
                _same_move(got, want, (G, kind, T))
                assert np.all(got[0][~legal] == 0) and np.all(legal[np.arange(G), got[2] - 1])
                n += 1
    return n


@pytest.mark.parametrize("regime", ["init", "biased", "peaked", "underflow"])
def test_prior_eval_fc_tictactoe(regime):
    """G = 1, 5 (a partial tile) and 17 (a second tile with one row), four temperatures, three kinds of mask,
    on init_nets and three head regimes; one case also against the CPU oracle's forward."""
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from muzero_jl_amd.selfplay import prior_policy
    from oracle import Oracle
    conf, hyper = _setup("ttt")
    nets = _nets(conf, hyper)
    if regime != "init":
        nets = wrg.named(conf, hyper, nets, regime)
    eng = _engine(conf, hyper, nets, 17)
    assert _check_rows(eng, conf, (1, 5, 17), (0.0, 1.0, INF, 0.5), ("full", "single", "random"), pc.OracleMath()) == 36
    ora = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=wr.SEED)
    for k, w in enumerate(nets):
        ora.set_weights(k, w)
    obs, legal = _rows(conf, 17, "random", 99)
    pol, val, _ = eng.prior_eval(obs, legal, rng_step=1, temperature=1.0)
    v, p = ora.forward(1, ora.forward(0, obs))
    assert np.array_equal(val, v[:, 0])
    assert all(np.array_equal(pol[g], prior_policy(p[g], legal[g])) for g in range(17))
    if regime == "underflow":                                  # zeros in p: the regime reaches them
        assert (p == 0).any()
    eng.close()


@pytest.mark.parametrize("name,bn", [("c4", False), ("ttt", True)])
def test_prior_eval_fc_connect4_and_batchnorm(name, bn):
    conf, hyper = _setup(name, bn=bn)
    nets = _nets(conf, hyper)
    if bn:
        from test_fc_bn import _bn_nets
        nets = _bn_nets(conf, hyper)
    eng = _engine(conf, hyper, nets, 8)
    _check_rows(eng, conf, (5,), (0.0, 1.0, INF, 0.5), ("full", "random"), pc.OracleMath())
    eng.close()


def test_prior_eval_resnet_past_one_tile():
    conf, hyper = _setup("ttt", resnet=True)
    eng = _engine(conf, hyper, _nets(conf, hyper), 64)
    G = eng.resnet_tile_games() + 1
    assert 1 < G <= 64
    _check_rows(eng, conf, (G,), (0.0, 1.0, INF, 0.5), ("full", "random"), pc.OracleMath())
    eng.close()


def test_prior_eval_downsampler_engine():
    """The Atari-like engine: the downsampler in front of the representation, 18 actions (the 32-lane group)."""
    conf, hyper = _setup("atari", num_iters=2, max_moves=6)
    assert len(conf.action_space) > 16
    eng = _engine(conf, hyper, _nets(conf, hyper, 17), 4)
    _check_rows(eng, conf, (3,), (0.0, 1.0, INF, 0.5), ("full", "random"), pc.OracleMath())
    eng.close()


def test_keys_reach_the_draw():
    """Two (game_offset, rng_step) pairs at T = 1: each equals its own mirror, and the mirrors differ."""
    from muzero_jl_amd.selfplay import prior_move
    conf, hyper = _setup("ttt")
    eng = _engine(conf, hyper, _nets(conf, hyper), 17)
    obs, legal = _rows(conf, 17, "full", 4)
    wants = []
    for goff, step in ((0, 5), (100, 6)):
        want = prior_move(eng, obs, legal, 1.0, eng.rng_seed, goff, step)
        _same_move(eng.prior_eval(obs, legal, rng_step=step, game_offset=goff, temperature=1.0), want, (goff, step))
        wants.append(want)
    assert np.array_equal(wants[0][0], wants[1][0]) and not np.array_equal(wants[0][2], wants[1][2])
    eng.close()


def test_opponent_set():
    from muzero_jl_amd import abi
    conf, hyper = _setup("ttt")
    mine, theirs = _nets(conf, hyper), _nets(conf, hyper, 211)
    eng, other = _engine(conf, hyper, mine, 8), _engine(conf, hyper, theirs, 8)
    obs, legal = _rows(conf, 5, "random", 8)
    with pytest.raises(abi.MzError, match="MZ_OPP_NETWORK needs the opponent's nets"):
        eng.prior_eval(obs, legal, opponent_set=1)
    for k, w in enumerate(theirs):
        eng.opponent_set_weights(k, w)
    own = eng.prior_eval(obs, legal, rng_step=3, game_offset=2, temperature=1.0)
    got = eng.prior_eval(obs, legal, opponent_set=1, rng_step=3, game_offset=2, temperature=1.0)
    _same_move(got, other.prior_eval(obs, legal, rng_step=3, game_offset=2, temperature=1.0), "set 1")
    assert not np.array_equal(got[0], own[0])
    _same_move(eng.prior_eval(obs, legal, rng_step=3, game_offset=2, temperature=1.0), own, "set 0 again")
    with pytest.raises(abi.MzError, match="opponent_set must be 0 or 1"):
        eng.prior_eval(obs, legal, opponent_set=2)
    eng.close(); other.close()


# ---- evaluation play: (env, slots, opponent, muzero_player, (muzero_kind, other_kind), temperature, threshold)
PLAY = [("ttt", 5, "random", 2, ("prior", "prior"), 0.0, None),
        ("ttt", 5, "expert", 2, ("prior", "prior"), 1.0, None),
        ("ttt", 5, "self", 2, ("search", "prior"), 1.0, None),
        ("ttt", 5, "self", 1, ("prior", "search"), 1.0, 2),
        ("ttt", 5, "network", 1, ("search", "prior"), 0.5, None),
        ("c4", 3, "network", 2, ("prior", "prior"), 1.0, None),
        ("c4", 3, "random", 2, ("prior", "prior"), 1.0, None),
        ("c4", 3, "self", 2, ("prior", "search"), 0.0, None)]


def _play_engines(name, G, opponent, thr, **kw):
    """(device engine, mirror engine, the opponent's mirror engine or None); NETWORK: other weights in the set."""
    ckw = dict(kw)
    if thr is not None:
        ckw["temperature_threshold"] = thr
    conf, hyper = _setup(name, **ckw)
    nets = _nets(conf, hyper)
    ed, eh, eo = _engine(conf, hyper, nets, G), _engine(conf, hyper, nets, G), None
    if opponent == "network":
        theirs = _nets(conf, hyper, 211)
        eo = _engine(conf, hyper, theirs, G)
        for k, w in enumerate(theirs):
            ed.opponent_set_weights(k, w)
    return ed, eh, eo


@pytest.mark.parametrize("name,G,opponent,mzp,kinds,temp,thr", PLAY)
def test_evaluation_play_matches_host(name, G, opponent, mzp, kinds, temp, thr):
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import BatchedSelfPlay, game_winner
    _, env_cls, env = _game(name)
    ed, eh, eo = _play_engines(name, G, opponent, thr)
    sp = BatchedSelfPlay(eh, env_cls, G, game_offset=7, step0=100, opponent=opponent, muzero_player=mzp,
                         opponent_engine=eo, muzero_kind=kinds[0], other_kind=kinds[1], detmath=pc.OracleMath())
    ed.selfplay_init(env, G, 64)
    if mzp == 1:                                               # the setting before the mode, and after it
        ed.eval_players(KIND[kinds[0]], KIND[kinds[1]])
    ed.selfplay_mode(abi.SP_EVAL, OPP[opponent], mzp)
    if mzp == 2:
        ed.eval_players(KIND[kinds[0]], KIND[kinds[1]])
    for m in range(14 if name == "ttt" else 24):
        sp.play_move(temp)
        ed.selfplay_move(100 + m, game_offset=7, temperature=temp)
        ln, board, player = ed.selfplay_slots()
        assert np.array_equal(ln, [len(h.action_history) for h in sp.histories]), m
        assert np.array_equal(board, sp.env.board.astype(np.uint8)) and np.array_equal(player, sp.env.player), m
    t = [0, 0, 0, 0]
    for h in sp.finished:
        w = game_winner("tictactoe" if name == "ttt" else "connect4", h.reward_history[-1], h.to_play_history[-1])
        t[0] += 1
        t[3 if w == 0 else 1 if w == mzp else 2] += 1
    assert t[0] > 0 and ed.eval_results() == tuple(t)
    for e in (ed, eh, eo):
        if e is not None:
            e.close()


@pytest.mark.parametrize("name,E,opponent,mzp,kinds,temp,thr", PLAY)
def test_through_the_test_worker(name, E, opponent, mzp, kinds, temp, thr):
    """mz_test_play: every slot's game (actions, rewards, child visits = π, root values = v) and the record
    against evaluate / evaluation_record; with (prior, prior) on TicTacToe also the audit."""
    from muzero_jl_amd.selfplay import evaluate
    _, env_cls, env = _game(name)
    kw = dict(max_moves=wr.MAX_MOVES) if name == "ttt" else {}
    ed, eh, eo = _play_engines(name, E, opponent, thr, **kw)
    audit = kinds == ("prior", "prior") and name == "ttt"
    ed.selfplay_init(env, E, E)
    ed.eval_players(KIND[kinds[0]], KIND[kinds[1]])
    ed.test_config(E, OPP[opponent], mzp)
    ed.test_audit(audit)
    out = evaluate(eh, env_cls, E, opponent=opponent, muzero_player=mzp, rng_step0=300, game_offset=11,
                   temperature=temp, training_step=17, opponent_engine=eo, audit=audit, muzero_kind=kinds[0],
                   other_kind=kinds[1], detmath=pc.OracleMath())
    hs, want = out[0], out[1]
    ed.test_play(17, 300, game_offset=11, temperature=temp)
    total, recs = ed.test_results(max_records=1)
    assert total == 1 and len(recs) == 1
    print(name, opponent, mzp, kinds, "device", recs[0], "mirror", want)
    for g in range(E):
        assert wr.same_history(ed.test_get_game(g), hs[g]), (name, opponent, mzp, g)
    assert wr.same_record(recs[0], want), (recs[0], want)
    assert want["games"] == E
    if audit:
        _, rows = ed.test_audit_results(max_records=1)
        assert tuple(int(x) for x in rows[0]) == out[2] and out[2][0] > 0
    for e in (ed, eh, eo):
        if e is not None:
            e.close()


def test_launches_per_move():
    """mz_debug_enable(2) counts the ResNet search's network launches, num_iters a search: (prior, prior) against
    the random mover searches nothing, (search, prior) with itself once a move, (search, search) as ever."""
    from muzero_jl_amd import abi
    S, G, moves = 4, 5, 6
    conf, hyper = _setup("ttt", resnet=True, num_iters=S)
    nets = _nets(conf, hyper)
    counts = {}
    for what, opp, kinds in (("none", abi.OPP_RANDOM, (1, 1)), ("none-self", abi.OPP_SELF, (1, 1)),
                             ("one", abi.OPP_SELF, (0, 1)), ("one-flipped", abi.OPP_SELF, (1, 0)),
                             ("parent-self", abi.OPP_SELF, (0, 0)), ("parent-random", abi.OPP_RANDOM, (0, 0)),
                             ("parent-network", abi.OPP_NETWORK, (0, 0)), ("network-prior", abi.OPP_NETWORK, (0, 1)),
                             ("train", None, (1, 1))):
        e = _engine(conf, hyper, nets, G)
        for k, w in enumerate(nets):
            e.opponent_set_weights(k, w)
        e.selfplay_init(abi.ENV_TICTACTOE, G, 16)
        e.eval_players(*kinds)
        if opp is not None:
            e.selfplay_mode(abi.SP_EVAL, opp, 1)
        e.debug_enable(2)
        for m in range(moves):
            e.selfplay_move(20 + m, game_offset=1, temperature=0.0)
        counts[what] = e.debug_kernel_time()[1]
        e.close()
    assert counts == {"none": 0, "none-self": 0, "one": moves * S, "one-flipped": moves * S,
                      "parent-self": moves * S, "parent-random": moves * S, "parent-network": 2 * moves * S,
                      "network-prior": moves * S, "train": moves * S}, counts


def _slots_equal(a, b, what):
    for x, y in zip(a.selfplay_slots(), b.selfplay_slots()):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("mode", ["train", "eval-reset"])
def test_setting_changes_nothing_outside_evaluation_play(mode):
    """A TRAIN-mode run with the setting at (prior, prior), and an EVAL run after setting it and resetting it to
    the default: the same games as on an engine that never heard of it."""
    from muzero_jl_amd import abi
    G = 5
    conf, hyper = _setup("ttt", num_iters=6)
    nets = _nets(conf, hyper)
    plain, tuned = _engine(conf, hyper, nets, G), _engine(conf, hyper, nets, G)
    tuned.eval_players(abi.PLAYER_PRIOR, abi.PLAYER_PRIOR)
    for e in (plain, tuned):
        e.selfplay_init(abi.ENV_TICTACTOE, G, 64)
        if mode != "train":
            e.selfplay_mode(abi.SP_EVAL, abi.OPP_SELF, 2)
    if mode != "train":
        tuned.selfplay_mode(abi.SP_EVAL, abi.OPP_SELF, 2)
        tuned.eval_players(abi.PLAYER_SEARCH, abi.PLAYER_PRIOR)            # allocates the second outputs
        tuned.eval_players()                                               # back to the default
    for m in range(14):
        for e in (plain, tuned):
            e.selfplay_move(50 + m, game_offset=2, temperature=1.0)
        _slots_equal(plain, tuned, m)
    if mode == "train":
        (counts, held), (counts2, held2) = plain.replay_counts(), tuned.replay_counts()
        assert held == held2 and held > 0 and np.array_equal(counts, counts2)
        for i in range(held):
            assert wr.same_history(plain.replay_get_game(i), tuned.replay_get_game(i)), i
    else:
        assert plain.eval_results() == tuned.eval_results() and plain.eval_results()[0] > 0
    plain.close(); tuned.close()


def test_train_run_with_a_prior_test_worker(tmp_path):
    """The same job with a test worker that plays (prior, prior) and without one: equal in every public
    read-out; the worker's records are the mirror's on the learner's weights of that moment."""
    import test_snapshot_gpu as snap
    from muzero_jl_amd import abi
    from muzero_jl_amd.selfplay import evaluate
    G_TR, CAP, B, MOVES, MOVE0, GOFF = 8, 32, 8, 16, 30, 2
    TEST_GOFF, INTERVAL, E, T = 500, 4, 5, 10
    conf, hyper = _setup("ttt", num_iters=8, batch_size=B, checkpoint_interval=3, training_steps=10000)
    nets = _nets(conf, hyper, 17)

    def start():
        e = _engine(conf, hyper, nets, 16)
        e.selfplay_init(abi.ENV_TICTACTOE, G_TR, CAP)
        e.train_init(B)
        return e

    on, off = start(), start()
    third = _engine(conf, hyper, _nets(conf, hyper, 99), 16)
    on.eval_players(abi.PLAYER_PRIOR, abi.PLAYER_PRIOR)
    on.test_config(E, abi.OPP_RANDOM, 2)
    on.train_set_test(INTERVAL, TEST_GOFF, 1.0)
    t0, want = 0, []
    for m in range(MOVES):
        s_on = on.train_run(1, move0=MOVE0 + m, game_offset=GOFF)
        s_off = off.train_run(1, move0=MOVE0 + m, game_offset=GOFF)
        assert s_on == s_off, m
        t1 = s_off[0]
        if t1 // INTERVAL > t0 // INTERVAL:
            for k in range(3):
                third.set_weights(k, off.train_weights(abi.TRAIN_LEARNER, k))
            want.append(evaluate(third, _game("ttt")[1], E, opponent="random", muzero_player=2,
                                 rng_step0=(t1 * T) & 0xffffffff, game_offset=TEST_GOFF, temperature=1.0,
                                 training_step=t1, muzero_kind="prior", other_kind="prior")[1])
        t0 = t1
    assert len(want) >= 2
    snap._same(snap._readout(on, tmp_path, "on"), snap._readout(off, tmp_path, "off"))
    total, recs = on.test_results()
    assert total == len(want)
    for a, b in zip(recs, want):
        assert wr.same_record(a, b), (a, b)
    assert off.test_results() == (0, [])
    on.close(); off.close(); third.close()


def test_eval_run_resumes_from_snapshot(tmp_path):
    from muzero_jl_amd import abi
    G, cap = 6, 12
    conf, hyper = _setup("ttt", num_iters=6)

    def start(wseed=17, cap=cap):
        e = _engine(conf, hyper, _nets(conf, hyper, wseed), G)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        e.eval_players(abi.PLAYER_PRIOR, abi.PLAYER_SEARCH)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_SELF, 2)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(10 + m, 3, temperature=1.0)

    uncut = start()
    drive(uncut, 0, 24)
    first = start()
    drive(first, 0, 11)                                        # games are in progress at the cut
    assert first.selfplay_slots()[0].any()
    at_cut = first.eval_results()
    path = str(tmp_path / "prior.safetensors")
    first.snapshot_save(path, 0)
    first.close()
    second = start(wseed=99, cap=cap + 5)                      # other weights, another shard size, other moves
    drive(second, 40, 45)
    second.snapshot_load(path)                                 # keeps the handle's kinds
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_SELF, 2)
    assert second.eval_results() == at_cut
    drive(second, 11, 24)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    _slots_equal(uncut, second, "resumed")
    uncut.close(); second.close()


def test_refusals():
    from muzero_jl_amd import abi
    conf, hyper = _setup("ttt")
    e = _engine(conf, hyper, _nets(conf, hyper), 4)
    for kinds in ((2, 0), (0, 2), (-1, 1), (1, 7)):
        with pytest.raises(abi.MzError, match="^.*eval players:"):
            e.eval_players(*kinds)
    e.eval_players(abi.PLAYER_PRIOR, abi.PLAYER_SEARCH)        # needs no selfplay_init
    obs, legal = _rows(conf, 5, "full", 1)
    with pytest.raises(abi.MzError, match="G exceeds max_games"):
        e.prior_eval(obs, legal)
    obs, legal = obs[:3], legal[:3].copy()
    assert e.prior_eval(obs[:0], legal[:0])[2].shape == (0,)   # G = 0
    legal[1] = False
    with pytest.raises(abi.MzError, match=r"Legal actions should not be an empty array \(game 1\)"):
        e.prior_eval(obs, legal)
    legal[1, 4] = True
    for T in (-1.0, float("nan")):
        with pytest.raises(abi.MzError, match="temperature must be >= 0"):
            e.prior_eval(obs, legal, temperature=T)
    assert e.prior_eval(obs, legal, temperature=INF)[2][1] == 5
    e.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    for opp in (5, 7, -1):                                     # no new opponent id
        with pytest.raises(abi.MzError, match="opponent must be"):
            e.selfplay_mode(abi.SP_EVAL, opp, 1)
    e.close()
