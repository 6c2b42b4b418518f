"""The Reanalyse worker on the device shard (mz_replay_reanalyse_next, kernel
mz_reanalyse_pack, the row list of the five reanalyse kernels) and its switch in
mz_train_run (mz_train_set_reanalyse).  Every round's selection against
pack_round on the lengths read back, search rounds against one mcts_search of
the host-built max_games rows, value rounds against an explicit
mz_replay_reanalyse on a twin engine, the targets against the host ReplayBuffer
driven by reanalyse_next, and mz_train_run against the hand-written split loop.
The shards are small (cap 8, max_games 16: one to three games per search round)
and come from device self-play, as in tests/test_reanalyse_search_gpu.py."""
import dataclasses
import os

import numpy as np
import pytest

from test_reanalyse_search_gpu import _mod, _same_batches, _stacked, _train

pytestmark = pytest.mark.gpu

MG, STEP, OFF = 16, 900, 3


def _engines(n, kind="ttt", cap=8, slots=8, min_games=8, seed=5, max_games=MG, **conf_kw):
    """n twin engines whose shards hold the same >= min_games self-played games (at most cap of them held)."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.networks import init_nets
    mod, env_kind, hyper = _mod(kind)
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=cap, td_steps=2, batch_size=40, **conf_kw)
    nets = init_nets(conf, hyper, seed=seed + 100)
    out, moves = [], None
    for _ in range(n):
        e = abi.Engine(conf, hyper, device=0, max_games=max_games, rng_seed=seed)
        for k, w in enumerate(nets):
            e.set_weights(k, w)
        e.selfplay_init(env_kind, slots, cap)
        m = 0
        while (m < moves) if moves is not None else (int(e.replay_counts()[0][0]) < min_games and m < 400):
            e.selfplay_move(100 + m, game_offset=7)
            m += 1
        moves = m
        out.append(e)
    assert int(out[0].replay_counts()[0][0]) >= min_games
    return conf, out


def _held(eng):
    """{game number: GameHistory} of the held games, and num_played_games."""
    counts, held = eng.replay_counts()
    played = int(counts[0])
    return {played - held + 1 + i: eng.replay_get_game(i) for i in range(held)}, played


def _state(eng, n):
    """Per held game (values or None, policies or None)."""
    return [(eng.replay_get_reanalysed(i), eng.replay_get_reanalysed_policies(i)) for i in range(n)]


def _nothing(t):
    return t[0] is None and t[1] is None


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def _round_rows(conf, games, rows, G):
    """The G rows of a search round as the engine builds them: the packed rows, then the dummy rows (zero
    observation, every action legal, to_play 1), which also stand in for a row with no legal action."""
    from muzero_jl_amd.replay_buffer import stored_legal_mask
    A = len(conf.action_space)
    stacked = {g: _stacked(conf, games[g]) for g in {g for g, _ in rows}}
    x = np.zeros((G, next(iter(stacked.values())).shape[1] if stacked else 1), np.float32)
    legal, tp, live = np.ones((G, A), np.uint8), np.ones(G, np.int32), np.zeros(G, bool)
    for i, (g, pos) in enumerate(rows):
        h = games[g]
        lm = stored_legal_mask(conf, h.observation_history[pos], h.to_play_history[pos])
        if lm.any():
            x[i], legal[i], tp[i], live[i] = stacked[g][pos], lm, h.to_play_history[pos], True
    return x, legal, tp, live


def _search_round(eng, conf, cap, exploration, rng_step=STEP, game_offset=OFF, G=MG):
    """One search round, checked: header and cursor against pack_round, the taken games against one
    mcts_search of the host-built G rows, the others untouched, the counter.  Returns pack_round's tuple."""
    from muzero_jl_amd import abi
    from muzero_jl_amd.replay_buffer import pack_round
    games, played = _held(eng)
    nums = sorted(games)
    lens = {g: len(h.root_values) for g, h in games.items()}
    cursor, _ = eng.replay_reanalyse_cursor()
    before, n0 = _state(eng, len(nums)), eng.replay_reanalysed_count()
    want = pack_round(lens, cursor, played, cap, G)
    first, ngames, rows, new_cursor = want
    eng.replay_reanalyse_next(abi.REAN_BY_SEARCH, exploration=exploration, rng_step=rng_step, game_offset=game_offset)
    assert eng.replay_reanalyse_cursor() == (new_cursor, (first, ngames, len(rows)))
    assert eng.replay_reanalysed_count() == n0 + ngames
    after = _state(eng, len(nums))
    if ngames:
        x, legal, tp, live = _round_rows(conf, games, rows, G)
        cv, rv, _ = eng.mcts_search(x, legal, tp, exploration=exploration, rng_step=rng_step,
                                    game_offset=game_offset, temperature=0.0)
    for i, g in enumerate(nums):
        if first <= g < first + ngames:
            r0 = rows.index((g, 0))
            r = slice(r0, r0 + lens[g])
            h = games[g]
            want_p = np.where(live[r, None], cv[r], np.array(h.child_visits, np.float32))
            want_v = np.where(live[r], rv[r], np.array(h.root_values, np.float32))
            assert np.array_equal(after[i][1], want_p), (g, exploration)
            assert np.array_equal(after[i][0], want_v), (g, exploration)
        else:
            assert _same(after[i][0], before[i][0]) and _same(after[i][1], before[i][1]), g
    return want


def _lap(eng, conf, cap, exploration, limit=40):
    """Rounds to the end of the lap (the round that reaches num_played_games); the games taken, in order."""
    taken = []
    for k in range(limit):
        first, n, rows, cur = _search_round(eng, conf, cap, exploration, rng_step=STEP + k, game_offset=OFF + 5 * k)
        taken += list(range(first, first + n))
        assert n >= 1 and len(rows) <= MG
        if cur == int(eng.replay_counts()[0][0]) + 1:
            return taken
    raise AssertionError("the lap did not end")


@pytest.mark.parametrize("exploration", [False, True])
def test_search_rounds_two_laps(exploration):
    cap = 8
    conf, (eng,) = _engines(1, cap=cap)
    _train(eng, (1, 2, 3))                                  # the networks move on: the new searches differ
    games, played = _held(eng)
    assert len(games) == cap
    assert _lap(eng, conf, cap, exploration) == sorted(games)           # cursor 1: before or at the oldest game
    # lap two starts with a wrap (the cursor is past the last game) ...
    first, n, _, cur = _search_round(eng, conf, cap, exploration)
    assert first == min(games) and cur == first + n
    # ... and self-play evicts the games under the cursor: the next round has to skip to the oldest held
    m = 1000
    while int(eng.replay_counts()[0][0]) < played + n + 1 and m < 1040:
        for _ in range(4):
            eng.selfplay_move(m, game_offset=7)
            m += 1
    games2, played2 = _held(eng)
    assert cur < min(games2)
    fresh = [g for g in games2 if g > played]
    st = _state(eng, cap)
    assert fresh and all(_nothing(st[sorted(games2).index(g)]) for g in fresh)  # stored into reanalysed slots
    assert _lap(eng, conf, cap, exploration) == sorted(games2)
    assert all(v is not None and p is not None for v, p in _state(eng, cap))
    eng.close()


@pytest.mark.parametrize("kind", ["ttt", "ttt-rn"])
def test_value_round_equals_explicit_call(kind):
    from muzero_jl_amd import abi
    cap = 8
    conf, (e1, e2) = _engines(2, kind, cap=cap)
    _train(e1, (1, 2)); _train(e2, (1, 2))
    games, played = _held(e1)
    nums, rows = sorted(games), sum(len(h.root_values) for h in games.values())
    assert len(nums) == cap and rows <= 4096
    # a value round holds 4096 rows: the whole shard goes in one round
    e1.replay_reanalyse_next(abi.REAN_BY_VALUE)
    assert e1.replay_reanalyse_cursor() == (played + 1, (nums[0], cap, rows))
    e2.replay_reanalyse()
    for i in range(cap):
        v1, v2 = e1.replay_get_reanalysed(i), e2.replay_get_reanalysed(i)
        assert v1 is not None and np.array_equal(v1, v2), (kind, i)
        if kind == "ttt":
            want = e1.forward(1, e1.forward(0, _stacked(conf, games[nums[i]])))[0][:, 0]
            assert np.array_equal(v1, want)
        assert e1.replay_get_reanalysed_policies(i) is None
    assert e1.replay_reanalysed_count() == e2.replay_reanalysed_count() == cap
    # from the middle of the shard, after another learner step: games 3.. only
    for e in (e1, e2):
        _train(e, (3,))
    old = [e1.replay_get_reanalysed(i) for i in range(cap)]
    e1.replay_reanalyse_seek(nums[3])
    e1.replay_reanalyse_next(abi.REAN_BY_VALUE)
    assert e1.replay_reanalyse_cursor() == (played + 1, (nums[3], cap - 3, sum(len(games[g].root_values) for g in nums[3:])))
    e2.replay_reanalyse(first=3, count=cap - 3)
    for i in range(cap):
        v1 = e1.replay_get_reanalysed(i)
        assert np.array_equal(v1, e2.replay_get_reanalysed(i)), (kind, i)
        assert np.array_equal(v1, old[i]) == (i < 3)
    assert e1.replay_reanalysed_count() == e2.replay_reanalysed_count() == 2 * cap - 3
    e1.close(); e2.close()


def test_resnet_search_round():
    cap = 8
    conf, (eng,) = _engines(1, "ttt-rn", cap=cap)
    _train(eng, (1, 2))
    for e in (False, True):
        first, n, rows, _ = _search_round(eng, conf, cap, e)
        assert n >= 1 and len(rows) > MG - 10
    eng.close()


def test_connect4_round_capacity():
    from muzero_jl_amd import abi
    conf, (small,) = _engines(1, "c4", cap=8, slots=8, min_games=3, max_games=16)
    n = small.replay_counts()[1]
    counts0, st0, cur0 = small.replay_counts(), _state(small, n), small.replay_reanalyse_cursor()
    with pytest.raises(abi.MzError, match="cannot hold one game of max_moves \\+ 1 positions"):
        small.replay_reanalyse_next(abi.REAN_BY_SEARCH, rng_step=STEP, game_offset=OFF)
    with pytest.raises(abi.MzError, match="cannot hold one game of max_moves \\+ 1 positions"):
        small.train_set_reanalyse(abi.REAN_BY_SEARCH, 1)
    counts1 = small.replay_counts()
    assert np.array_equal(counts0[0], counts1[0]) and counts0[1] == counts1[1]
    assert small.replay_reanalysed_count() == 0 and small.replay_reanalyse_cursor() == cur0 == (1, (0, 0, 0))
    assert all(_nothing(a) for a in _state(small, n)) and all(_nothing(a) for a in st0)
    small.close()
    conf, (eng,) = _engines(1, "c4", cap=8, slots=8, min_games=3, max_games=48)
    assert conf.max_moves + 1 == 43
    _train(eng, (1, 2))
    first, n, rows, _ = _search_round(eng, conf, 8, True, G=48)
    assert n >= 1 and len(rows) <= 48
    eng.close()


def test_seek():
    cap = 8
    conf, (eng,) = _engines(1, cap=cap, min_games=12)       # games have been evicted: the oldest is not game 1
    games, played = _held(eng)
    nums = sorted(games)
    assert nums[0] > 1
    for target, start in ((nums[0] - 1, nums[0]), (0, nums[0]), (-7, nums[0]), (nums[4], nums[4]),
                          (played, played), (played + 1, nums[0]), (played + 100, nums[0])):
        eng.replay_reanalyse_seek(target)
        assert eng.replay_reanalyse_cursor()[0] == target
        first, n, rows, cur = _search_round(eng, conf, cap, False)
        assert first == start and n >= 1 and cur == first + n
    eng.close()


def test_empty_shard_and_refusals():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import atari_synth as at
    from muzero_jl_amd.games import tictactoe as mod
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=8)
    eng = abi.Engine(conf, mod.hyper, device=0, max_games=MG, rng_seed=5)
    with pytest.raises(abi.MzError, match="mz_selfplay_init first"):
        eng.replay_reanalyse_next(abi.REAN_BY_VALUE)
    eng.selfplay_init(abi.ENV_TICTACTOE, 8, 8)
    assert eng.replay_reanalyse_cursor() == (1, (0, 0, 0))
    for mode in (abi.REAN_BY_VALUE, abi.REAN_BY_SEARCH):
        eng.replay_reanalyse_next(mode, rng_step=STEP, game_offset=OFF)
        assert eng.replay_reanalyse_cursor() == (1, (1, 0, 0))
        assert eng.replay_reanalysed_count() == 0 and eng.replay_counts()[1] == 0
    eng.replay_reanalyse_seek(5)
    eng.replay_reanalyse_next(abi.REAN_BY_SEARCH)
    assert eng.replay_reanalyse_cursor() == (5, (5, 0, 0))              # nothing played: the cursor stays
    with pytest.raises(abi.MzError, match="mode"):
        eng.replay_reanalyse_next(abi.REAN_OFF)
    with pytest.raises(abi.MzError, match="mode"):
        eng.train_set_reanalyse(3, 1)
    with pytest.raises(abi.MzError, match="rounds_per_move"):
        eng.train_set_reanalyse(abi.REAN_BY_VALUE, -1)
    eng.close()
    conf = dataclasses.replace(at.conf, num_iters=2)
    eng = abi.Engine(conf, at.resnet_hyper, device=0, max_games=4, rng_seed=1)
    eng.selfplay_init(abi.ENV_ATARI, 4, 8)
    for mode in (abi.REAN_BY_VALUE, abi.REAN_BY_SEARCH):
        with pytest.raises(abi.MzError, match="reanalyse: frame-stack env not built"):
            eng.replay_reanalyse_next(mode)
    assert eng.replay_reanalysed_count() == 0 and eng.replay_reanalyse_cursor() == (1, (0, 0, 0))
    eng.close()


def _host_mirror(eng, conf, cap):
    """The host ReplayBuffer holding the shard's games (none reanalysed yet) with the device's cursor."""
    from muzero_jl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(dataclasses.replace(conf, replay_buffer_size=cap), seed=5)
    games, played = _held(eng)
    for g in sorted(games):
        rb.save_game(games[g])
    shift = played - len(games)
    rb.reanalyse_cursor = eng.replay_reanalyse_cursor()[0] - shift
    return rb, shift


def test_targets_match_host_buffer_driven_by_reanalyse_next():
    from muzero_jl_amd import abi
    from muzero_jl_amd.replay_buffer import REAN_BY_SEARCH, REAN_BY_VALUE
    cap = 8
    conf, (eng,) = _engines(1, cap=cap, min_games=12)
    _train(eng, (1, 2, 3))
    rb, shift = _host_mirror(eng, conf, cap)
    assert shift > 0
    plain = {s: rb.get_batch(s) for s in (1, 2, 77)}
    key = {}

    def search_fn(x, legal, tp, p0):                        # rows p0.. of the round keyed (rng_step, game_offset)
        cv, rv, _ = eng.mcts_search(x, legal, tp, exploration=True, rng_step=key["step"],
                                    game_offset=key["off"] + p0, temperature=0.0)
        return cv, rv

    def value_fn(x):
        return eng.forward(1, eng.forward(0, x))[0][:, 0]

    for k in range(2):                                      # search rounds: at most six of the eight games
        key.update(step=STEP + k, off=OFF + 7 * k)
        eng.replay_reanalyse_next(abi.REAN_BY_SEARCH, exploration=True, rng_step=key["step"], game_offset=key["off"])
        first, n, rows, cur = rb.reanalyse_next(search_fn, REAN_BY_SEARCH, MG)
        assert eng.replay_reanalyse_cursor() == (cur + shift, (first + shift, n, len(rows)))
    assert 0 < sum(h.reanalysed_child_visits is not None for h in rb.buffer.values()) < cap
    _same_batches(eng, rb, shift, (1, 2, 77))
    eng.replay_reanalyse_next(abi.REAN_BY_VALUE)            # the value round: from the cursor to the last game
    first, n, rows, cur = rb.reanalyse_next(value_fn, REAN_BY_VALUE)
    assert eng.replay_reanalyse_cursor() == (cur + shift, (first + shift, n, len(rows))) and 0 < n < cap
    _same_batches(eng, rb, shift, (1, 2, 77))
    moved = set()
    for s in (1, 2, 77):
        idx, b = rb.get_batch(s)
        assert idx == plain[s][0]
        moved |= {k for k in b if not np.array_equal(b[k], plain[s][1][k])}
    assert moved == {"target_policies", "target_values"}
    eng.close()


def test_learner_paths_after_a_round():
    """train_dev == replay_sample + grad_dev + apply after rounds, and the batch train_dev(s) drew ahead for
    s + 1 is not used after a round (e2: prefetch off).  e0 is never reanalysed."""
    import torch
    from muzero_jl_amd import abi
    from muzero_jl_amd.config import cos_schedule
    B = 32
    conf, (e0, e1, e2) = _engines(3, cap=8)
    grad = torch.empty(e1.grad_count(), dtype=torch.float32, device="cuda")
    ls = [torch.zeros(8, dtype=torch.float32, device="cuda") for _ in range(3)]

    def losses(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()[:6].copy()

    def rounds(e, mode, k):
        for r in range(k):
            e.replay_reanalyse_next(mode, exploration=True, rng_step=STEP + r, game_offset=OFF + r * MG)

    for e in (e1, e2):
        rounds(e, abi.REAN_BY_SEARCH, 3)
    s = 1
    e0.learner_train_dev(B, s, cos_schedule(s), ls[0].data_ptr())
    e1.learner_train_dev(B, s, cos_schedule(s), ls[1].data_ptr())
    b, _ = e2.replay_sample(B, s)
    e2.learner_grad_dev([b.observation, b.actions, b.target_values, b.target_rewards, b.target_policies,
                         b.gradient_scale], B, grad.data_ptr(), ls[2].data_ptr())
    e2.learner_apply_dev(grad.data_ptr(), 1.0, cos_schedule(s))
    for e in (e0, e1, e2):
        e.sync()
    assert e1.learner_variant().startswith("mz_learn_small")            # the fused one-launch path
    assert np.array_equal(losses(ls[1]), losses(ls[2]))
    assert not np.array_equal(losses(ls[1]), losses(ls[0]))
    for mode in (abi.REAN_BY_VALUE, abi.REAN_BY_SEARCH):
        s += 2
        e0.learner_train_dev(B, s, cos_schedule(s), ls[0].data_ptr())
        e0.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[0].data_ptr())
        e1.learner_train_dev(B, s, cos_schedule(s), ls[1].data_ptr())
        rounds(e1, mode, 2)
        e1.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[1].data_ptr())
        os.environ["MZ_NO_BATCH_PREFETCH"] = "1"
        try:
            e2.learner_train_dev(B, s, cos_schedule(s), ls[2].data_ptr())
            rounds(e2, mode, 2)
            e2.learner_train_dev(B, s + 1, cos_schedule(s + 1), ls[2].data_ptr())
        finally:
            del os.environ["MZ_NO_BATCH_PREFETCH"]
        for e in (e0, e1, e2):
            e.sync()
        assert np.array_equal(losses(ls[1]), losses(ls[2])), mode
        assert not np.array_equal(losses(ls[1]), losses(ls[0])), mode
    assert e1.replay_reanalyse_cursor() == e2.replay_reanalyse_cursor()
    for e in (e0, e1, e2):
        e.close()


# ---- mz_train_run with the worker on
TG, TCAP, TB, TMOVES, MOVE0, TOFF = 16, 32, 8, 12, 50, 7


def _train_engine():
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import tictactoe as mod
    from muzero_jl_amd.networks import init_nets
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=TCAP, td_steps=2, batch_size=TB,
                               checkpoint_interval=4, training_steps=1000)
    eng = abi.Engine(conf, mod.hyper, device=0, max_games=TG, rng_seed=5)
    for k, w in enumerate(init_nets(conf, mod.hyper, seed=105)):
        eng.set_weights(k, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, TG, TCAP)
    eng.train_init(TB)
    return eng


def _snapshot(eng):
    from muzero_jl_amd import abi
    counts, held = eng.replay_counts()
    sets = [eng.train_weights(w, n) for w in (abi.TRAIN_LEARNER, abi.TRAIN_ACTOR, abi.TRAIN_QUEUED) for n in range(3)]
    games = []
    for i in range(held):
        h = eng.replay_get_game(i)
        games.append((np.array(h.action_history), np.array(h.root_values, np.float32), np.array(h.child_visits)))
    return dict(counts=counts, held=held, sets=sets, games=games, rean=_state(eng, held),
                count=eng.replay_reanalysed_count(), cursor=eng.replay_reanalyse_cursor())


def _assert_same(a, b, rean=True):
    assert np.array_equal(a["counts"], b["counts"]) and a["held"] == b["held"]
    for x, y in zip(a["sets"], b["sets"]):
        assert np.array_equal(x, y)
    for ga, gb in zip(a["games"], b["games"]):
        for x, y in zip(ga, gb):
            assert np.array_equal(x, y)
    if rean:
        assert a["count"] == b["count"] and a["cursor"] == b["cursor"]
        for (va, pa), (vb, pb) in zip(a["rean"], b["rean"]):
            assert _same(va, vb) and _same(pa, pb)


@pytest.mark.parametrize("mode,rounds", [("search", 2), ("value", 1)])
def test_train_run_equals_the_split_loop(mode, rounds):
    from muzero_jl_amd import abi
    mode = abi.REAN_BY_SEARCH if mode == "search" else abi.REAN_BY_VALUE
    one, two = _train_engine(), _train_engine()
    one.train_set_reanalyse(mode, rounds, exploration=False)
    st1 = one.train_run(TMOVES, move0=MOVE0, game_offset=TOFF)
    tot = 0
    for m in range(TMOVES):
        nfin = two.train_move(MOVE0 + m, game_offset=TOFF)
        for r in range(rounds):
            two.replay_reanalyse_next(mode, exploration=False, rng_step=MOVE0 + m, game_offset=TOFF + r * TG)
        st2 = two.train_learn(nfin)
        tot += st2[3]
    assert st1 == st2[:3] + (tot,) and st1[3] > 0 and st1[2] > 0
    a, b = _snapshot(one), _snapshot(two)
    _assert_same(a, b)
    assert a["count"] > 0 and any(v is not None for v, _ in a["rean"])
    assert any(p is not None for _, p in a["rean"]) == (mode == abi.REAN_BY_SEARCH)
    one.close(); two.close()


def test_train_run_off_again_equals_never_on():
    from muzero_jl_amd import abi
    ON, OFF_MOVES = 11, 4
    on, never = _train_engine(), _train_engine()
    on.train_set_reanalyse(abi.REAN_BY_SEARCH, 2, exploration=True)
    on.train_run(ON, move0=MOVE0, game_offset=TOFF)     # long enough for the first games to end and be taken
    mid = _snapshot(on)
    assert mid["count"] > 0
    on.train_set_reanalyse(abi.REAN_OFF, 2)
    st_on = on.train_run(OFF_MOVES, move0=MOVE0 + ON, game_offset=TOFF)
    never.train_run(ON, move0=MOVE0, game_offset=TOFF)
    st_never = never.train_run(OFF_MOVES, move0=MOVE0 + ON, game_offset=TOFF)
    assert st_on == st_never and st_on[3] > 0             # learner steps ran after the switch
    a, b = _snapshot(on), _snapshot(never)
    _assert_same(a, b, rean=False)                          # the games, the counters and all three weight sets
    assert a["count"] == mid["count"] and a["cursor"] == mid["cursor"]  # no round ran after the switch
    assert b["count"] == 0 and b["cursor"] == (1, (0, 0, 0)) and all(_nothing(x) for x in b["rean"])
    on.close(); never.close()
