"""The run log on the device (mz_train_set_log), bit for bit.

Every record a logged job commits is compared, every int64 and every float64
bit, with learning.run_log_record fed from a CONTROL engine: the same conf and
seed with the log off, driven as the split loop (train_move, then one
train_learn(1, losses) per saved game, which yields each step's six losses),
its games read with replay_get_game and its counters with replay_counts.  The
logged job is also the unlogged job in every public read-out, mz_train_run and
the split loop give the same records, and the learner paths (FC multi, ResNet
multi, the one-launch-per-step fallback of PER / corrected mode / the
downsampler nets, the n == 1 step, two chunks in one call), the one-player
frame-stack env, the ring's wrap, host-saved games with evictions, the
lifetimes across snapshots and mz_selfplay_init and the refusals each have a
case.  Shapes are the smallest that reach the path."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, WSEED, MOVE0, GOFF = 5, 17, 30, 2
ENV_NAME = {"ttt": "tictactoe", "c4": "connect4", "atari": "atari"}


def _mod(game):
    from muzero_jl_amd.games import atari_synth, connect4, tictactoe
    return {"ttt": tictactoe, "c4": connect4, "atari": atari_synth}[game]


def _env(game):
    from muzero_jl_amd import abi
    return {"ttt": abi.ENV_TICTACTOE, "c4": abi.ENV_CONNECT4, "atari": abi.ENV_ATARI}[game]


def _engine(game="ttt", resnet=False, G=8, cap=64, max_games=None, corrected=False, init=True, wseed=WSEED, **kw):
    """An engine of the base job (TicTacToe FC, G = 8, 8 simulations, a shard of 64 games, batches of 4, an
    actor refresh every 2 steps) with the changes asked for, after selfplay_init and train_init."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod = _mod(game)
    hyper = mod.resnet_hyper if (resnet or game == "atari") else mod.hyper
    kw.setdefault("num_iters", 8)
    kw.setdefault("batch_size", 4)
    kw.setdefault("checkpoint_interval", 2)
    kw.setdefault("training_steps", 100000)
    conf = dataclasses.replace(mod.conf, **kw)
    e = abi.Engine(conf, hyper, device=0, max_games=max_games or G, rng_seed=SEED)
    for k, w in enumerate(init_nets(conf, hyper, seed=wseed)):
        e.set_weights(k, w)
    if corrected:
        e.learner_set_mode(abi.LEARN_CORRECTED)
    if init:
        e.selfplay_init(_env(game), G, cap)
        e.train_init(conf.batch_size)
    return e


def _same_record(got, want):
    from muzero_jl_amd.abi import LOG_COUNT_FIELDS, LOG_SUM_FIELDS
    bad = [k for k in LOG_COUNT_FIELDS if int(got[k]) != int(want[k])]
    bad += [k for k in LOG_SUM_FIELDS if np.float64(got[k]).tobytes() != np.float64(want[k]).tobytes()]
    return bad


def _assert_records(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        print(what, "record", i, "device", g, "mirror", w)
        assert _same_record(g, w) == [], (what, i, _same_record(g, w))


class Control:
    """The log-off engine driven as the split loop, with the mirror of the log's bookkeeping beside it."""

    def __init__(self, eng, game, interval):
        import torch
        self.eng, self.env_name, self.iv = eng, ENV_NAME[game], interval
        self.losses = torch.zeros(8, dtype=torch.float32, device="cuda")
        self.rows, self.games, self.missed, self.upto = [], [], 0, 0
        self.t, self.refreshes, self.records, self.nfin = 0, 0, [], []

    def fold_games(self):                                      # mz_log_games
        counts, held = self.eng.replay_counts()
        played = int(counts[0])
        if self.upto < played:
            oldest = played - held
            first = max(self.upto, oldest) + 1
            self.missed += first - 1 - self.upto
            self.games += [self.eng.replay_get_game(num - oldest - 1) for num in range(first, played + 1)]
        self.upto = played

    def commit(self):                                          # mz_log_commit
        from muzero_jl_amd.config import cos_schedule
        from muzero_jl_amd.learning import run_log_record
        counts, held = self.eng.replay_counts()
        counters = (counts[0], counts[1], counts[2], held, self.eng.replay_reanalysed_count())
        self.records.append(run_log_record(np.array(self.rows, np.float32).reshape(-1, 6), self.games, counters, self.t,
                                           cos_schedule(self.t), self.refreshes, self.missed, self.env_name))
        self.rows, self.games, self.missed = [], [], 0

    def learn(self, n):                                        # n single steps, then the commit rule
        t0 = self.t
        for _ in range(n):
            st = self.eng.train_learn(1, losses_ptr=self.losses.data_ptr())
            assert st[3] == 1
            self.eng.sync()                                    # the engine's own stream: torch does not wait for it
            self.rows.append(self.losses.cpu().numpy()[:6].copy())
            self.t, self.refreshes = st[0], st[2]
        if self.t // self.iv > t0 // self.iv:
            self.commit()

    def move(self, m):
        n = self.eng.train_move(m, game_offset=GOFF)
        self.nfin.append(n)
        self.fold_games()
        self.learn(n)


def _pair(interval, game="ttt", **kw):
    on, off = _engine(game, **kw), _engine(game, **kw)
    on.train_set_log(interval)
    return on, Control(off, game, interval)


def _finish(on, ctl, what, min_records=2):
    """Flush both, compare every record, close."""
    on.train_log_flush()
    ctl.commit()
    total, recs = on.train_log_results()
    assert total == len(recs) >= min_records
    _assert_records(recs, ctl.records, what)
    assert ctl.eng.train_log_results() == (0, [])
    on.close(); ctl.eng.close()
    return recs


# ---- 1. the records are the mirror's
def test_records_equal_the_mirror(tmp_path):
    import test_snapshot_gpu as snap
    moves, interval = 14, 5
    on, ctl = _pair(interval)
    st = on.train_run(moves, move0=MOVE0, game_offset=GOFF)
    for m in range(moves):
        ctl.move(MOVE0 + m)
    assert st[0] == ctl.t >= 8 and st[1] >= 8 and st[2] == ctl.refreshes >= 2
    assert on.train_log_results()[0] == len(ctl.records) >= 1  # the commit rule fired where the mirror's did
    snap._same(snap._readout(on, tmp_path, "on"), snap._readout(ctl.eng, tmp_path, "off"))
    recs = _finish(on, ctl, "base")
    assert sum(r["steps"] for r in recs) == st[0] and sum(r["games"] for r in recs) == st[1]
    assert sum(r["moves"] for r in recs) >= 5 * st[1] and all(r["missed"] == 0 for r in recs)
    assert any(r["wins_p1"] + r["wins_p2"] for r in recs) and recs[-1]["training_step"] == st[0]
    assert all(r["value"] > 0 and r["l2_repr"] > 0 for r in recs if r["steps"])


# ---- 2. the logged job is the unlogged job
@pytest.mark.parametrize("workers", [False, True])
def test_the_logged_job_is_the_unlogged_job(workers, tmp_path):
    import test_snapshot_gpu as snap
    import torch
    from muzero_jl_amd import abi
    on, off = _engine(max_games=16), _engine(max_games=16)
    for e in (on, off):
        if workers:
            e.test_config(5, abi.OPP_RANDOM, 2)
            e.train_set_test(4, 500, 0.0)
            e.train_set_reanalyse(abi.REAN_BY_SEARCH, 1)
    on.train_set_log(5)
    la, lb = (torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(2))
    for m in range(14):
        sa = on.train_run(1, move0=MOVE0 + m, game_offset=GOFF, losses_ptr=la.data_ptr())
        sb = off.train_run(1, move0=MOVE0 + m, game_offset=GOFF, losses_ptr=lb.data_ptr())
        assert sa == sb, m
        on.sync(); off.sync()
        assert np.array_equal(la.cpu().numpy().view(np.uint32), lb.cpu().numpy().view(np.uint32)), m
    assert sa[0] >= 8 and on.train_log_results()[0] >= 1 and off.train_log_results() == (0, [])
    snap._same(snap._readout(on, tmp_path, "on"), snap._readout(off, tmp_path, "off"))
    ta, tb = on.test_results(), off.test_results()
    assert ta == tb and (ta[0] >= 2) == workers
    if workers:
        assert on.replay_reanalysed_count() > 0 and on.train_log_results()[1][-1]["reanalysed"] > 0
    on.close(); off.close()


# ---- 3. mz_train_run and the split loop
def test_train_run_and_the_split_loop_give_the_same_records():
    run, split = _engine(), _engine()
    for e in (run, split):
        e.train_set_log(5)
    st = run.train_run(14, move0=MOVE0, game_offset=GOFF)
    for m in range(14):
        st2 = split.train_learn(split.train_move(MOVE0 + m, game_offset=GOFF))
    assert st[:3] == st2[:3]
    for e in (run, split):
        e.train_log_flush()
    (ta, ra), (tb, rb) = run.train_log_results(), split.train_log_results()
    assert ta == tb >= 2
    _assert_records(ra, rb, "run vs split")
    run.close(); split.close()


# ---- 4. the learner paths
def _drive(moves, interval, what, game="ttt", **kw):
    on, ctl = _pair(interval, game, **kw)
    st = on.train_run(moves, move0=MOVE0, game_offset=GOFF)
    for m in range(moves):
        ctl.move(MOVE0 + m)
    assert st[0] == ctl.t and st[0] >= 1, (what, st)
    return on, ctl, st


def test_connect4_resnet():
    """max_moves = 8: the four lockstep games all end by length on move 9, so move 9's chunk has four
    steps on the ResNet multi-step path (12 moves: one more game each cannot end)."""
    on, ctl, st = _drive(12, 3, "c4 resnet", game="c4", resnet=True, G=4, cap=8, num_iters=4, batch_size=2, max_moves=8)
    assert max(ctl.nfin) >= 2 and on.learner_variant() != "none"
    _finish(on, ctl, "c4 resnet")


def test_per():
    on, ctl, st = _drive(12, 5, "PER", PER=True)
    assert st[0] >= 8
    _finish(on, ctl, "PER")


def test_corrected_mode():
    on, ctl, st = _drive(12, 5, "corrected", corrected=True)
    assert st[0] >= 8
    _finish(on, ctl, "corrected")


def test_single_step_chunks_and_batch_size_one():
    """G = 1: every move that saves a game saves exactly one, the n == 1 path of the loop."""
    on, ctl, st = _drive(20, 2, "n == 1", G=1, cap=4, max_games=4, batch_size=1)
    assert st[0] >= 2 and set(ctl.nfin) == {0, 1}
    _finish(on, ctl, "n == 1")


def test_two_chunks_in_one_call():
    """train_learn(300) on a filled shard: chunks of 256 and 44 steps, one record for the call."""
    on, ctl, st = _drive(9, 200, "two chunks")
    assert on.train_log_results()[0] == 0
    st = on.train_learn(300)
    ctl.learn(300)
    assert st[3] == 300 and st[0] == ctl.t and on.train_log_results()[0] == len(ctl.records) == 1
    recs = _finish(on, ctl, "two chunks")
    assert recs[0]["steps"] == st[0] and recs[0]["games"] >= 8 and recs[1]["steps"] == 0 == recs[1]["games"]


# ---- 5. the one-player frame-stack env
def test_atari_like_env():
    """max_moves = 6: every game ends by length on move 7 at the latest; the downsampler nets take the
    one-launch-per-step learner."""
    on, ctl, st = _drive(8, 3, "atari", game="atari", G=4, cap=8, num_iters=2, batch_size=2, num_unroll_steps=2,
                         max_moves=6)
    assert st[0] >= 4
    recs = _finish(on, ctl, "atari")
    assert all(r["wins_p2"] == 0 for r in recs) and sum(r["games"] for r in recs) == st[1]


# ---- 6. the ring
def test_ring_wrap_and_clear():
    from muzero_jl_amd import abi
    e = _engine()
    e.train_set_log(1000)
    e.train_run(9, move0=MOVE0, game_offset=GOFF)              # a TicTacToe game has at most 9 moves: the shard has games
    e.train_log_flush()
    e.train_log_clear()
    assert e.train_log_results() == (0, [])
    t0 = e.train_learn(0)[0]
    n, at = abi.LOG_RECORDS + 6, (5, 6, abi.LOG_RECORDS + 3)
    want = []
    for i in range(n):
        if i in at:
            e.train_learn(1)
        e.train_log_flush()
        want.append((t0 + sum(i >= a for a in at), int(i in at)))
    total, recs = e.train_log_results()
    assert total == n and len(recs) == abi.LOG_RECORDS
    assert [(r["training_step"], r["steps"]) for r in recs] == want[6:]         # the newest 1024, oldest first
    assert all(r["games"] == 0 and r["moves"] == 0 and r["missed"] == 0 for r in recs)
    total, recs3 = e.train_log_results(3)
    assert total == n and recs3 == recs[-3:] and [r["steps"] for r in recs3] == [1, 0, 0]
    assert e.train_log_results(0) == (n, [])
    e.train_log_clear()
    assert e.train_log_results() == (0, [])
    e.train_log_flush()
    assert e.train_log_results()[0] == 1
    e.close()


# ---- 7. games a host saves, and the ones the shard loses before a fold
def test_host_saved_games_and_the_missed_count():
    cap = 16
    e = _engine(cap=cap)
    e.train_set_log(1000)
    e.train_run(9, move0=MOVE0, game_offset=GOFF)
    e.train_log_flush()
    game = e.replay_get_game(0)
    played0 = int(e.replay_counts()[0][0])
    for _ in range(cap + 3):
        e.replay_save_game(game)
    played1 = int(e.replay_counts()[0][0])
    assert played1 == played0 + cap + 3
    e.train_run(1, move0=MOVE0 + 9, game_offset=GOFF)
    counts, held = e.replay_counts()
    played2 = int(counts[0])
    e.train_log_flush()
    total, recs = e.train_log_results(1)
    r = recs[0]
    print("host-saved", played0, played1, played2, r)
    assert total == 2 and held == cap
    assert r["games"] + r["missed"] == played2 - played0        # every game that entered is accounted for
    assert r["missed"] == 3 + (played2 - played1) and r["games"] == cap
    assert r["num_played_games"] == played2 and r["games_held"] == cap and r["positions_held"] == counts[2]
    e.close()


# ---- 8. lifetimes
def test_snapshot_and_reinit(tmp_path):
    from muzero_jl_amd import abi
    a = _engine()
    a.train_set_log(1000)
    a.train_run(10, move0=MOVE0, game_offset=GOFF)             # mid-interval: steps and games accumulated
    path = str(tmp_path / "snap.safetensors")
    a.snapshot_save(path, 3)
    a.train_log_flush()                                        # a's accumulators start over here
    assert a.train_log_results(1)[1][0]["steps"] >= 8
    b = _engine(wseed=99, G=4, cap=8, max_games=8, init=False)
    b.train_set_log(1000)                                      # set before any shard exists
    b.selfplay_init(abi.ENV_TICTACTOE, 4, 8)
    b.train_init(4)
    b.train_run(9, move0=77, game_offset=1)                    # its own games and steps, never committed
    assert b.snapshot_load(path) == 3
    for e in (a, b):
        st = e.train_run(6, move0=MOVE0 + 10, game_offset=GOFF)
        e.train_log_flush()
    (ta, ra), (tb, rb) = a.train_log_results(1), b.train_log_results(1)
    assert (ta, tb) == (2, 1)
    _assert_records(rb, ra, "after the load")                  # only the steps and games after the load
    assert ra[0]["steps"] == st[3] >= 1 and ra[0]["games"] >= 1 and ra[0]["num_played_games"] == st[1]
    counts, held = b.replay_counts()
    assert [rb[0][k] for k in ("num_played_games", "num_played_steps", "positions_held", "games_held")] == \
        [counts[0], counts[1], counts[2], held]
    # mz_selfplay_init again: the accumulators are zeroed, the ring and the setting are kept
    b.train_run(9, move0=MOVE0 + 16, game_offset=GOFF)
    b.selfplay_init(abi.ENV_TICTACTOE, 8, 64)
    b.train_init(4)
    assert b.train_log_results() == (tb, rb)
    b.train_log_flush()
    total, recs = b.train_log_results()
    assert total == 2 and _same_record(recs[0], rb[0]) == []
    assert [recs[1][k] for k in abi.LOG_COUNT_FIELDS] == [0] * 16
    assert all(recs[1][k] == 0.0 for k in abi.LOG_SUM_FIELDS if k != "eta")
    st = b.train_run(9, move0=MOVE0, game_offset=GOFF)         # and the log goes on with the new shard
    b.train_log_flush()
    r = b.train_log_results(1)[1][0]
    assert r["games"] == st[1] >= 8 and r["steps"] == st[0] and r["missed"] == 0
    a.close(); b.close()


# ---- 9. refusals, each followed by a working call
def test_refusals():
    from muzero_jl_amd import abi
    e = _engine(init=False)
    with pytest.raises(abi.MzError, match="interval must be >= 0"):
        e.train_set_log(-1)
    e.train_set_log(3)
    with pytest.raises(abi.MzError, match="mz_train_init first"):
        e.train_log_flush()
    e.selfplay_init(abi.ENV_TICTACTOE, 8, 64)
    with pytest.raises(abi.MzError, match="mz_train_init first"):
        e.train_log_flush()
    e.train_init(4)
    e.train_log_flush()
    e.train_set_log(0)
    with pytest.raises(abi.MzError, match="the run log is off"):
        e.train_log_flush()
    e.train_set_log(3)
    e.train_log_flush()
    with pytest.raises(abi.MzError, match="max_records must be >= 0"):
        e.train_log_results(-1)
    total, recs = e.train_log_results()
    assert total == 2 and all(r["steps"] == 0 and r["games"] == 0 and r["training_step"] == 0 for r in recs)
    e.close()
