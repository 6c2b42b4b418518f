"""Snapshots (mz_snapshot_save / _load): a run cut in two by save ->
another engine -> load equals the uncut run bit for bit.

Every comparison is between two engines, the uncut run and the cut run, through
public read-outs only (_readout): the replay counters, every held game with its
reanalysed values / policies and priorities, the Reanalyse cursor, the games in
progress, the three weight sets, the ADAM state (through checkpoint_save), the
loop's state_out, the last losses and the evaluation tally — all with
np.array_equal.  The engine that loads was created with DIFFERENT initial
weights and has already played on a shard of another size, so a pass proves
that load replaces the state.  The reference has no counterpart (its buffer is
never written to disk, games/tictactoe/main.jl:21)."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, CAP, B = 12, 20, 8
MOVE0, GOFF = 10, 3


def _game(name):
    from muzero_jl_amd.games import atari_synth, connect4, tictactoe
    return {"ttt": tictactoe, "c4": connect4, "atari": atari_synth}[name]


def _env(name):
    from muzero_jl_amd import abi
    return {"ttt": abi.ENV_TICTACTOE, "c4": abi.ENV_CONNECT4, "atari": abi.ENV_ATARI}[name]


def _engine(game="ttt", resnet=False, wseed=17, seed=5, max_games=G, **kw):
    """(conf, hyper, engine) with init_nets(wseed) weights."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    g = _game(game)
    hyper = g.resnet_hyper if (resnet or game == "atari") else g.hyper
    kw.setdefault("num_iters", 5 if resnet else 8)
    kw.setdefault("batch_size", B)
    kw.setdefault("checkpoint_interval", 3)
    kw.setdefault("training_steps", 10000)
    conf = dataclasses.replace(g.conf, **kw)
    eng = abi.Engine(conf, hyper, device=0, max_games=max_games, rng_seed=seed)
    for n, w in enumerate(init_nets(conf, hyper, seed=wseed)):
        eng.set_weights(n, w)
    return conf, hyper, eng


def _readout(eng, tmp_path, tag, train=True, per=False):
    """Everything the public read-outs show, as a dict of arrays."""
    from muzero_jl_amd import abi
    from muzero_jl_amd import checkpoint as ck
    d = {}
    counts, held = eng.replay_counts()
    d["counts"], d["held"] = counts, np.array(held)
    for i in range(held):
        for k, v in eng.replay_get_game(i).as_arrays().items():
            d[f"game{i}.{k}"] = v
        rr, rp = eng.replay_get_reanalysed(i), eng.replay_get_reanalysed_policies(i)
        d[f"game{i}.rean"] = np.array([rr is not None, rp is not None])
        if rr is not None:
            d[f"game{i}.rrv"] = rr
        if rp is not None:
            d[f"game{i}.rcv"] = rp
        if per:
            pr, gp = eng.replay_get_priorities(i)
            d[f"game{i}.prio"], d[f"game{i}.gprio"] = pr, np.array(gp)
    cur, rnd = eng.replay_reanalyse_cursor()
    d["cursor"] = np.array([cur, *rnd])
    d["reanalysed_games"] = np.array(eng.replay_reanalysed_count())
    try:
        d["slot_len"], d["slot_board"], d["slot_player"] = eng.selfplay_slots()
    except abi.MzError:                               # the Atari-like env before its first move
        d["slot_len"] = np.array("pending")
    for n in range(3):
        d[f"learner{n}"] = eng.train_weights(abi.TRAIN_LEARNER, n)
        if train:
            d[f"actor{n}"] = eng.train_weights(abi.TRAIN_ACTOR, n)
            d[f"queued{n}"] = eng.train_weights(abi.TRAIN_QUEUED, n)
    path = str(tmp_path / f"adam_{tag}.safetensors")
    eng.checkpoint_save(path, 0)
    t, _ = ck.read(path)
    for k in ("adam.m", "adam.v", "adam.beta_pow"):
        d[k] = t[k]
    d["eval"] = np.array(eng.eval_results())
    return d


def _same(a, b):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _loader(game, conf_kw, resnet=False, per_moves=2, max_games=G, g=G, cap=CAP + 3, train=True):
    """The engine that loads: other weights, a shard of another size, a few moves played."""
    _, _, eng = _engine(game, resnet=resnet, wseed=99, max_games=max_games, **conf_kw)
    eng.selfplay_init(_env(game), g, cap)
    if train:
        eng.train_init(B)
        eng.train_run(per_moves, move0=77, game_offset=1)
    else:
        for m in range(per_moves):
            eng.selfplay_move(50 + m, 1)
    return eng


CASES = {
    "ttt_fc": dict(),
    "ttt_fc_small_staging": dict(stage=4096),
    "ttt_resnet": dict(resnet=True),
    "c4_fc": dict(game="c4"),
    "per": dict(conf=dict(PER=True)),
    "temperature_threshold": dict(conf=dict(temperature_threshold=3)),
    "training_steps_9": dict(conf=dict(training_steps=9)),
    "rean_search": dict(rean="search"),
    "rean_value": dict(rean="value"),
    "cut_after_1": dict(cut=1),
    "cut_after_0": dict(cut=0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_exact_resume_of_train_run(case, tmp_path, monkeypatch):
    import torch
    from muzero_jl_amd import abi
    c = CASES[case]
    game, resnet, conf_kw = c.get("game", "ttt"), c.get("resnet", False), c.get("conf", {})
    moves, cut = 26, c.get("cut", 13)
    per = bool(conf_kw.get("PER"))
    if "stage" in c:                                  # several record ranges through the staging buffer
        monkeypatch.setenv("MZ_SNAP_STAGE_BYTES", str(c["stage"]))

    def settings(e):
        if c.get("rean") == "search":
            e.train_set_reanalyse(abi.REAN_BY_SEARCH, 1)
        elif c.get("rean") == "value":
            e.train_set_reanalyse(abi.REAN_BY_VALUE, 1)

    def start():
        _, _, e = _engine(game, resnet=resnet, **conf_kw)
        e.selfplay_init(_env(game), G, CAP)
        e.train_init(B)
        settings(e)
        return e, torch.zeros(8, dtype=torch.float32, device="cuda")

    def leg(e, losses, first):
        n, m0 = (cut, MOVE0) if first else (moves - cut, MOVE0 + cut)
        return e.train_run(n, move0=m0, game_offset=GOFF, losses_ptr=losses.data_ptr())

    uncut, l_uncut = start()
    leg(uncut, l_uncut, True)
    st_uncut = leg(uncut, l_uncut, False)

    first, l_cut = start()
    leg(first, l_cut, True)
    snap = str(tmp_path / "cut.safetensors")
    first.snapshot_save(snap, 1234)
    first.close()
    assert os.listdir(tmp_path) == ["cut.safetensors"]                # no .tmp left behind
    second = _loader(game, conf_kw, resnet=resnet)
    settings(second)                                  # handle settings are the loading host's
    assert second.snapshot_load(snap) == 1234
    st_cut = leg(second, l_cut, False)

    assert st_cut == st_uncut and st_uncut[0] > 0
    uncut.sync()                                      # train_run returns with its last learner steps in flight
    second.sync()
    assert np.array_equal(l_cut.cpu().numpy(), l_uncut.cpu().numpy())
    a, b = _readout(uncut, tmp_path, "uncut", per=per), _readout(second, tmp_path, "cut", per=per)
    _same(a, b)
    if game == "ttt":
        assert a["counts"][0] > CAP                   # the ring wrapped
    if c.get("rean"):
        assert a["reanalysed_games"] > 0 and a["cursor"][0] > 1
        assert any(a[f"game{i}.rean"][0] for i in range(int(a["held"])))
    if c.get("rean") == "search":
        assert any(a[f"game{i}.rean"][1] for i in range(int(a["held"])))
    uncut.close()
    second.close()


def test_host_driven_loop_without_train_init(tmp_path):
    """selfplay_move x k interleaved with learner_train_dev, cut in the middle: the snapshot has no
    train section, and after the load train_run is still refused."""
    from muzero_jl_amd import abi
    from muzero_jl_amd import checkpoint as ck

    def start():
        _, _, e = _engine()
        e.selfplay_init(abi.ENV_TICTACTOE, G, CAP)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(MOVE0 + m, GOFF)
            if m >= 9:                                # every slot has finished a game by then
                e.learner_train_dev(B, m, 1e-3 * (1 + m % 3))

    uncut = start()
    drive(uncut, 0, 22)
    first = start()
    drive(first, 0, 14)
    snap = str(tmp_path / "host.safetensors")
    first.snapshot_save(snap, 14)
    first.close()
    assert "train.state" not in ck.read(snap)[0] and ck.read_metadata(snap)["train"] == "0"
    second = _loader("ttt", {})                       # had a train loop of its own
    assert second.snapshot_load(snap) == 14
    with pytest.raises(abi.MzError, match="mz_train_init first"):
        second.train_run(1)
    drive(second, 14, 22)
    _same(_readout(uncut, tmp_path, "uncut", train=False), _readout(second, tmp_path, "cut", train=False))
    uncut.close()
    second.close()


@pytest.mark.parametrize("cut", [0, 11])
def test_atari_like_env(cut, tmp_path):
    """Frames, keys and the pending initial reset: cut before the first move and mid-run."""
    from muzero_jl_amd import abi
    g, cap, moves, kw = 4, 8, 24, dict(num_iters=2, max_moves=6, batch_size=4)

    def start():
        _, _, e = _engine("atari", max_games=g, **kw)
        e.selfplay_init(abi.ENV_ATARI, g, cap)
        e.train_init(4)
        return e

    uncut = start()
    uncut.train_run(cut, move0=MOVE0, game_offset=GOFF)
    st_uncut = uncut.train_run(moves - cut, move0=MOVE0 + cut, game_offset=GOFF)
    first = start()
    first.train_run(cut, move0=MOVE0, game_offset=GOFF)
    snap = str(tmp_path / "atari.safetensors")
    first.snapshot_save(snap, 5)
    first.close()
    _, _, second = _engine("atari", wseed=99, max_games=g, **kw)
    second.selfplay_init(abi.ENV_ATARI, g, cap + 1)
    second.train_init(4)
    second.train_run(2, move0=70, game_offset=9)
    assert second.snapshot_load(snap) == 5
    st_cut = second.train_run(moves - cut, move0=MOVE0 + cut, game_offset=GOFF)
    assert st_cut == st_uncut
    a, b = _readout(uncut, tmp_path, "uncut"), _readout(second, tmp_path, "cut")
    _same(a, b)
    assert a["counts"][0] > cap and a["game0.observation"].shape[1] == 84 * 84
    ba, _ = uncut.replay_sample(4, 3)
    ha = uncut.batch_to_host(ba)
    bb, _ = second.replay_sample(4, 3)
    hb = second.batch_to_host(bb)
    _same(ha, hb)
    uncut.close()
    second.close()


def test_eval_mode_tally_carries_over(tmp_path):
    from muzero_jl_amd import abi

    def start(wseed=17, cap=CAP):
        _, _, e = _engine(wseed=wseed)
        e.selfplay_init(abi.ENV_TICTACTOE, G, cap)
        e.selfplay_mode(abi.SP_EVAL, abi.OPP_RANDOM, 2)
        return e

    def drive(e, m0, m1):
        for m in range(m0, m1):
            e.selfplay_move(MOVE0 + m, GOFF, temperature=0.0)

    uncut = start()
    drive(uncut, 0, 24)
    first = start()
    drive(first, 0, 12)
    at_cut = first.eval_results()
    snap = str(tmp_path / "eval.safetensors")
    first.snapshot_save(snap, 0)
    first.close()
    second = start(wseed=99, cap=CAP + 5)
    drive(second, 40, 45)
    second.snapshot_load(snap)
    second.selfplay_mode(abi.SP_EVAL, abi.OPP_RANDOM, 2)
    assert second.eval_results() == at_cut and at_cut[0] > 0
    drive(second, 12, 24)
    assert second.eval_results() == uncut.eval_results() and uncut.eval_results()[0] > at_cut[0]
    _same(_readout(uncut, tmp_path, "uncut", train=False), _readout(second, tmp_path, "cut", train=False))
    uncut.close()
    second.close()


@pytest.fixture(scope="module")
def base_snapshot(tmp_path_factory):
    """A snapshot of the TicTacToe FC loop after 16 moves with the Reanalyse worker searching (PER off):
    (path, conf, hyper, the engine's read-outs as the file's truth)."""
    from muzero_jl_amd import abi
    d = tmp_path_factory.mktemp("snap")
    conf, hyper, e = _engine()
    e.selfplay_init(abi.ENV_TICTACTOE, G, CAP)
    e.train_init(B)
    e.train_set_reanalyse(abi.REAN_BY_SEARCH, 1)
    st = e.train_run(16, move0=MOVE0, game_offset=GOFF)
    path = str(d / "base.safetensors")
    e.snapshot_save(path, st[0])
    truth = dict(st=st, held=e.replay_counts()[1], counts=e.replay_counts()[0],
                 games=[e.replay_get_game(i).as_arrays() for i in range(e.replay_counts()[1])],
                 rrv=[e.replay_get_reanalysed(i) for i in range(e.replay_counts()[1])],
                 rcv=[e.replay_get_reanalysed_policies(i) for i in range(e.replay_counts()[1])],
                 slots=e.selfplay_slots(), cursor=e.replay_reanalyse_cursor(),
                 sets=[[e.train_weights(w, n) for n in range(3)] for w in range(3)])
    e.close()
    assert sorted(os.listdir(d)) == ["base.safetensors"]
    return path, conf, hyper, truth


def test_file_contents(base_snapshot, tmp_path):
    from muzero_jl_amd import abi
    from muzero_jl_amd import checkpoint as ck
    path, conf, hyper, truth = base_snapshot
    s = ck.read_snapshot(path)
    assert s["meta"]["format"] == "libmz-snapshot-1" and s["meta"]["rng_seed"] == "5"
    assert 0 < len(s["games"]) == truth["held"] <= CAP
    assert np.array_equal(s["counters"][:3], truth["counts"])
    assert int(s["counters"][4]) == truth["cursor"][0] and tuple(s["counters"][5:8]) == truth["cursor"][1]
    rows = 0
    for i, g in enumerate(s["games"]):
        a = g.as_arrays()
        for k, v in truth["games"][i].items():
            assert np.array_equal(a[k], v), (i, k)
        rows += len(g.action_history)
        for got, want in ((g.reanalysed_predicted_root_values, truth["rrv"][i]),
                          (g.reanalysed_child_visits, truth["rcv"][i])):
            assert (got is None) == (want is None), i
            if want is not None:
                assert np.array_equal(np.array(got, np.float32), want), i
    assert any(r is not None for r in truth["rcv"])
    # live rows only: Σ len rows, not cap · T
    T = conf.max_moves + 1
    assert rows == truth["counts"][2] < CAP * T
    for k in ("obs", "act", "rew", "tp", "cv", "rv", "rrv", "rcv"):
        assert s["tensors"]["shard." + k].shape[0] == rows, k
    assert s["tensors"]["shard.obs"].shape == (rows, 27) and s["tensors"]["shard.cv"].shape == (rows, 9)
    ln, board, player = truth["slots"]
    assert np.array_equal(s["slots"]["len"], ln) and np.array_equal(s["slots"]["board"], board)
    assert np.array_equal(s["slots"]["player"], player) and not s["slots"]["reset_pending"]
    assert s["tensors"]["slots.obs"].shape == (int(ln.sum()), 27)
    assert [len(g.action_history) for g in s["slots"]["games"]] == list(ln)
    tr = s["train"]
    assert (tr["batch_size"], tr["t"], tr["refreshes"]) == (B, truth["st"][0], truth["st"][2])
    assert np.array_equal(tr["actor"], np.concatenate(truth["sets"][abi.TRAIN_ACTOR]))
    assert np.array_equal(tr["queued"], np.concatenate(truth["sets"][abi.TRAIN_QUEUED]))
    # a snapshot is a checkpoint too
    for n, flat in enumerate(ck.nets_from(s["tensors"], conf, hyper)):
        assert np.array_equal(flat, truth["sets"][abi.TRAIN_LEARNER][n])
    _, _, fresh = _engine(wseed=99)
    assert fresh.checkpoint_load(path) == truth["st"][0]
    for n in range(3):
        assert np.array_equal(fresh.get_weights(n), truth["sets"][abi.TRAIN_LEARNER][n])
    fresh.close()


def _rewrite(src, dst, edit):
    """The snapshot rewritten in Python with `edit(tensors, meta)` applied."""
    from safetensors.numpy import save_file
    from muzero_jl_amd import checkpoint as ck
    tensors, meta = ck.read(src)
    tensors = {k: v.copy() for k, v in tensors.items()}
    edit(tensors, meta)
    save_file(tensors, dst, metadata=meta)


def _len_T_plus_1(t, m):
    t["shard.len"][3] = int(m["T"]) + 1


def _len_negative(t, m):
    t["shard.len"][3] = -2


def _len_sum(t, m):                                   # one row fewer than the row tensors hold ...
    t["shard.len"][3] -= 1


def _len_sum_counters_agree(t, m):                    # ... also with the counters adjusted to agree
    t["shard.len"][3] -= 1
    t["shard.counters"][1] -= 1
    t["shard.counters"][2] -= 1


def _n_over_cap(t, m):
    m["cap"] = str(len(t["shard.len"]) - 1)


def _identity(t, m):
    pass


FILE_EDITS = {"len_T_plus_1": _len_T_plus_1, "len_negative": _len_negative, "len_sum": _len_sum,
              "len_sum_counters_agree": _len_sum_counters_agree, "n_over_cap": _n_over_cap}
ENGINES = {"other_network_kind": dict(resnet=True), "other_env": dict(game="c4"),
           "other_max_moves": dict(max_moves=7), "other_PER": dict(PER=True), "other_seed": dict(seed=6),
           "G_over_max_games": dict(max_games=G - 1)}


@pytest.mark.parametrize("case", list(ENGINES) + list(FILE_EDITS) + ["truncated", "rewritten_unchanged"])
def test_refusals_leave_the_engine_as_it_was(case, base_snapshot, tmp_path):
    from muzero_jl_amd import abi
    path, conf, hyper, truth = base_snapshot
    ekw = dict(ENGINES.get(case, {}))
    game, max_games = ekw.pop("game", "ttt"), ekw.pop("max_games", G)
    resnet, seed = ekw.pop("resnet", False), ekw.pop("seed", 5)
    g = min(G, max_games)

    def start():
        _, _, e = _engine(game, resnet=resnet, seed=seed, wseed=23, max_games=max_games, **ekw)
        e.selfplay_init(_env(game), g, CAP)
        e.train_init(B)
        e.train_run(11, move0=4, game_offset=2)
        return e

    bad = path
    if case in FILE_EDITS or case == "rewritten_unchanged":
        bad = str(tmp_path / "bad.safetensors")
        _rewrite(path, bad, FILE_EDITS.get(case, _identity))
    elif case == "truncated":
        bad = str(tmp_path / "bad.safetensors")
        data = open(path, "rb").read()
        open(bad, "wb").write(data[:len(data) * 3 // 5])
    victim, twin = start(), start()
    per = bool(ekw.get("PER"))
    if case == "rewritten_unchanged":                 # the control: the rewriting itself is not what is refused
        assert victim.snapshot_load(bad) == truth["st"][0]
        assert victim.replay_counts()[1] == truth["held"]
        assert np.array_equal(victim.train_weights(abi.TRAIN_ACTOR, 0), truth["sets"][abi.TRAIN_ACTOR][0])
    else:
        with pytest.raises(abi.MzError):
            victim.snapshot_load(bad)
        assert victim.train_run(5, move0=15, game_offset=2) == twin.train_run(5, move0=15, game_offset=2)
        _same(_readout(victim, tmp_path, "victim", per=per), _readout(twin, tmp_path, "twin", per=per))
    victim.close()
    twin.close()
