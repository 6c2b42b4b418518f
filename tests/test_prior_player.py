"""The network-only player on the CPU: the Python mirror
(selfplay.prior_policy / prior_pick / prior_move) against a naive restatement
of the definition and its invariants on the shared cases, BatchedSelfPlay's
player kinds with stub engines, and the bindings against the header."""
import os
import re

import numpy as np
import pytest

import prior_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _naive(p, legal, T, r, dm):
    """The definition restated on arrays: (π, 0-based action)."""
    idx = np.flatnonzero(legal)
    s = np.add.accumulate(np.where(legal, p, F(0)).astype(F))[-1]              # ascending float32 sum
    pi = np.zeros(len(p), F)
    pi[idx] = F(1) / F(len(idx)) if s == 0 else (p[idx] / s).astype(F)
    if T == 0:
        return pi, int(idx[np.argmax(pi[idx])])                               # argmax: the first maximum
    if np.isinf(T):
        return pi, int(idx[(r * len(idx)) >> 32])
    if T == 1:
        w = pi[idx]
    else:
        inv = float(F(1) / F(T))
        w = np.array([F(dm.det_exp(dm.det_log(float(x)) * inv)) if x > 0 else F(0) for x in pi[idx]], F)
    c = np.add.accumulate(w)
    u = F(F(F(r >> 8) * F(2.0 ** -24)) * c[-1])
    hit = np.flatnonzero(c > u)
    return pi, int(idx[hit[0]] if len(hit) else idx[-1])


def test_mirror_equals_the_naive_restatement():
    from muzero_jl_amd.selfplay import prior_pick, prior_policy
    dm = pc.OracleMath()
    seen = set()
    for name, p, legal, T, r in pc.cases():
        pi = prior_policy(p, legal)
        act = prior_pick(pi, legal, T, r, dm)
        want_pi, want_act = _naive(p, legal, T, r, dm)
        assert pi.dtype == np.float32 and np.array_equal(pi.view(np.uint32), want_pi.view(np.uint32)), name
        assert act == want_act, (name, T, r, act, want_act)
        seen.add((name, act))
    assert len({a for n, a in seen if n == "A9-all-legal"}) > 2               # the draws and temperatures matter


def test_invariants():
    from muzero_jl_amd.rng import rng_below
    from muzero_jl_amd.selfplay import prior_pick, prior_policy
    dm = pc.OracleMath()
    last_hit = n_far = 0
    for name, p, legal, T, r in pc.cases():
        pi = prior_policy(p, legal)
        idx = np.flatnonzero(legal)
        assert np.all(pi[~legal] == 0) and np.all(pi[legal] >= 0), name      # 0 exactly on illegal actions
        if "legal-all-zero" in name:
            assert np.all(pi[legal] == F(1) / F(len(idx))), name              # the uniform fallback
        else:
            assert abs(float(pi.sum()) - 1.0) < 1e-5, name
        act = prior_pick(pi, legal, T, r, dm)
        assert legal[act], name
        if T == 0:
            assert act == idx[np.argmax(pi[idx])] and pi[act] == pi[idx].max(), name
            assert not np.any(pi[idx[idx < act]] == pi[act]), name            # the first of equal maxima
        if np.isinf(T):
            assert act == idx[rng_below(r, len(idx))], name
        if T not in (0.0, float("inf")):
            if r == 0 and T == 1:                                             # u = 0: the first legal action with weight
                assert act == idx[np.flatnonzero(pi[idx] > 0)[0]], name
            if r == 0xFFFFFFFF:                                               # u = (1 - 2^-24) S: the far end
                n_far += 1
                last_hit += act == idx[-1]
                assert not np.any(pi[idx[idx > act]] >= F(2.0 ** -20)), name  # nothing of weight lies behind it
    assert last_hit > n_far // 2
    _, p, legal = pc.rows()[0]
    two = next(c for c in pc.rows() if c[0] == "A9-two-maxima")
    assert prior_pick(prior_policy(two[1], two[2]), two[2], 0.0, 7) == 2     # 2 and 5 tie, 3 is larger but illegal
    with pytest.raises(AssertionError):
        prior_policy(p, np.zeros(len(p), bool))
    with pytest.raises(AssertionError):
        prior_pick(prior_policy(p, legal), legal, -1.0, 0)
    with pytest.raises(AssertionError):
        prior_pick(prior_policy(p, legal), legal, float("nan"), 0)
    with pytest.raises(AssertionError, match="detmath"):
        prior_pick(prior_policy(p, legal), legal, 0.5, 0)


def test_last_legal_fallback_is_reached():
    """Weights whose running float32 sum never exceeds u = (1 - 2^-24) S: with S = 1 + 2^-24-sized tails
    rounding away, the scan ends without a hit and the last legal action is played."""
    from muzero_jl_amd.selfplay import prior_pick
    pi = np.array([1.0, 2.0 ** -26, 0.0, 2.0 ** -26], F)                      # S = 1 (the tails round away), u < 1
    legal = np.array([True, True, False, True])
    assert prior_pick(pi, legal, 1.0, 0xFFFFFFFF) == 0                        # 1 > u: the first action
    pi = np.array([0.0, 0.0, 0.0, 0.0], F)                                    # S = 0, u = 0: no running sum exceeds it
    assert prior_pick(pi, legal, 1.0, 0xFFFFFFFF) == 3
    assert prior_pick(pi, legal, 1.0, 0) == 3


class _Stub:
    """An engine whose players return its own tag everywhere.  The search: child visits tag + slot / 100, root
    value -tag, the tag-th legal action.  The nets: representation = the observation's first columns + tag,
    value -(10 + tag), a policy that puts most of its mass on action 9 - tag."""

    def __init__(self, conf, tag):
        self.conf, self.tag, self.rng_seed, self.calls, self.fwd = conf, tag, 5, [], []

    def mcts_search(self, obs, legal, tp, exploration=True, rng_step=0, game_offset=0, temperature=1.0):
        self.calls.append((rng_step, game_offset, temperature))
        G, A = legal.shape
        cv = F(self.tag) + np.tile(np.arange(A, dtype=F) / 100, (G, 1))
        rv = np.full(G, -float(self.tag), F)
        act = np.array([np.flatnonzero(legal[g])[self.tag - 1] + 1 for g in range(G)], np.int32)
        return cv, rv, act

    def policy(self, A=9):
        p = np.full(A, 0.02, F)
        p[8 - self.tag] = F(1.0) - F(0.02) * F(A - 1)
        return p

    def forward(self, net, x):
        self.fwd.append(net)
        if net == 0:
            return np.asarray(x[:, :4], F) + F(self.tag)
        assert np.all(x[:, 0] >= self.tag)                                   # the prediction sees this engine's h
        return np.full((len(x), 1), -(10.0 + self.tag), F), np.tile(self.policy(), (len(x), 1))


KINDS = [("search", "search"), ("search", "prior"), ("prior", "search"), ("prior", "prior")]


@pytest.mark.parametrize("opponent", ["self", "network"])
@pytest.mark.parametrize("kinds", KINDS)
def test_host_mirror_takes_each_row_from_the_right_player(kinds, opponent):
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay, prior_policy
    a, b = _Stub(ttt.conf, 1), _Stub(ttt.conf, 2)
    mzp = 2
    sp = BatchedSelfPlay(a, ttt.BatchedTicTacToe, 4, game_offset=7, step0=100, opponent=opponent,
                         opponent_engine=b if opponent == "network" else None, muzero_player=mzp,
                         muzero_kind=kinds[0], other_kind=kinds[1])
    for m in range(4):
        mover = m % 2 + 1
        kind = kinds[0] if mover == mzp else kinds[1]
        eng = a if mover == mzp or opponent == "self" else b
        legal = sp.env.legal_mask().copy()
        assert not len(sp.play_move(0.0))
        for g, h in enumerate(sp.histories):
            if kind == "search":
                assert h.root_values[-1] == -float(eng.tag)
                assert np.array_equal(h.child_visits[-1], F(eng.tag) + np.arange(9, dtype=F) / 100)
                assert h.action_history[-1] == np.flatnonzero(legal[g])[eng.tag - 1] + 1
            else:
                pi = prior_policy(eng.policy(), legal[g])
                assert h.root_values[-1] == -(10.0 + eng.tag)
                assert np.array_equal(h.child_visits[-1], pi)
                assert h.action_history[-1] == int(np.argmax(pi)) + 1        # temperature 0
    # a player is run only where it produces rows: the primary always, the secondary where it differs
    second = opponent == "network" or kinds[0] != kinds[1]
    eng2 = b if opponent == "network" else a
    n_search = {id(a): 0, id(b): 0}
    n_prior = {id(a): 0, id(b): 0}
    (n_search if kinds[0] == "search" else n_prior)[id(a)] += 4
    if second:
        (n_search if kinds[1] == "search" else n_prior)[id(eng2)] += 4
    for e in (a, b):
        assert len(e.calls) == n_search[id(e)] and len(e.fwd) == 2 * n_prior[id(e)], (kinds, opponent, e.tag)
    for e in (a, b):                                                         # every search carries the move's keys
        per_move = max(1, len(e.calls) // 4)
        assert all(c[:2] == (100 + k // per_move, 7) for k, c in enumerate(e.calls))


@pytest.mark.parametrize("opponent", ["random", "expert", "mcts"])
def test_rules_opponents_ignore_other_kind(opponent):
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    runs = []
    for other in ("search", "prior"):
        a = _Stub(ttt.conf, 1)
        sp = BatchedSelfPlay(a, ttt.BatchedTicTacToe, 3, game_offset=2, step0=40, opponent=opponent, muzero_player=1,
                             muzero_kind="prior", other_kind=other, mcts_sims=4, mcts_rollouts=2)
        for _ in range(4):
            sp.play_move(0.0)
        assert not a.calls and len(a.fwd) == 8                               # no search at all, one prior per move
        runs.append([(h.action_history, h.root_values) for h in sp.histories + sp.finished])
    assert runs[0] == runs[1]
    assert all(rv[0] == -11.0 for _, rv in runs[0])                          # every record holds the prior's value


def test_temperature_threshold_picks_cold_games_at_zero():
    import dataclasses
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    conf = dataclasses.replace(ttt.conf, temperature_threshold=2)
    a = _Stub(conf, 1)
    sp = BatchedSelfPlay(a, ttt.BatchedTicTacToe, 6, opponent="self", muzero_kind="prior", other_kind="prior")
    for m in range(4):
        legal = sp.env.legal_mask().copy()
        sp.play_move(float("inf"))                                           # warm games: the r-th legal action
        acts = [h.action_history[-1] for h in sp.histories]
        if m >= 2:                                                           # cold: the argmax of π
            assert all(x == int(np.argmax(np.where(legal[g], a.policy(), 0))) + 1 for g, x in enumerate(acts))
        else:
            assert len(set(acts)) > 1


def test_host_mirror_argument_checks():
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    a = _Stub(ttt.conf, 1)
    for kw in (dict(muzero_kind="value"), dict(other_kind=1), dict(muzero_kind=None)):
        with pytest.raises(AssertionError, match="eval players"):
            BatchedSelfPlay(a, ttt.BatchedTicTacToe, 2, **kw)
    with pytest.raises(AssertionError):                                      # "network" still needs its engine
        BatchedSelfPlay(a, ttt.BatchedTicTacToe, 2, opponent="network", other_kind="prior")


def test_binding_matches_the_header():
    import ctypes
    from muzero_jl_amd import abi
    hdr = open(os.path.join(ROOT, "include", "mz.h")).read()
    jl = open(os.path.join(ROOT, "julia", "LibMZ.jl")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(MZ_PLAYER_\w+)\s*=\s*(\d+)", hdr))
    assert enum == {"MZ_PLAYER_SEARCH": abi.PLAYER_SEARCH, "MZ_PLAYER_PRIOR": abi.PLAYER_PRIOR}
    assert (abi.PLAYER_SEARCH, abi.PLAYER_PRIOR) == (0, 1)
    assert re.search(r"const PLAYER_SEARCH, PLAYER_PRIOR = Cint\(0\), Cint\(1\)", jl)
    # the opponent ids stay as they are: no new one
    opp = dict((k, v) for k, v in re.findall(r"\b(MZ_OPP_\w+)\s*=\s*([^,}\s]+(?: \+ 1)?)", hdr))
    assert opp == {"MZ_OPP_SELF": "0", "MZ_OPP_RANDOM": "1", "MZ_OPP_EXPERT": "2", "MZ_OPP_NETWORK": "3",
                   "MZ_OPP_MCTS": "MZ_OPP_NETWORK + 1"}
    assert (abi.OPP_SELF, abi.OPP_RANDOM, abi.OPP_EXPERT, abi.OPP_NETWORK, abi.OPP_MCTS) == (0, 1, 2, 3, 4)
    vp, ci, u32, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_float
    want = {"mz_eval_players": (ci, [vp, ci, ci]),
            "mz_prior_eval": (ci, [vp, ci, vp, vp, ci, u32, u32, cf, vp, vp, vp]),
            "mz_prior_eval_dev": (ci, [vp, ci, vp, vp, ci, u32, u32, cf, vp, vp, vp, vp])}
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in want.items():
        assert abi.SIGNATURES[name] == sig, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", body, flags=re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
    for name, arity in (("mz_eval_players", 3), ("mz_prior_eval", 11)):
        m = re.search(r"ccall\(\(:" + name + r", libmz\), Cint,\s*\(([^)]*)\)", jl)
        assert m and len([t for t in m.group(1).split(",") if t.strip()]) == arity, name
    for meth in ("eval_players", "prior_eval"):
        assert callable(getattr(abi.Engine, meth))
    assert "eval_players!" in jl and "function prior_eval(" in jl
