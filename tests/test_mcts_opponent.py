"""The rules-MCTS opponent's host mirror (games/mcts_rules.py) on the
CPU: against an independent, naive, recursive restatement of the definition
written here, the invariants of the root statistics, and the strength floor
(it beats the uniform random mover from both sides)."""
import math

import numpy as np
import pytest

import mcts_cases as mc

ROLLOUT, OPPONENT = 10, 7                                 # the Philox purposes (include/mz_detmath.h)


# ---- the restatement: its own rules on plain lists, scalar Philox draws, recursion for the backup
def _ttt_play(c, p, a):
    from muzero_jl_amd.games.tictactoe import LINES
    c = list(c)
    c[a] = p
    q = 3 - p
    if any(all(c[k] == q for k in line) for line in LINES):      # Q14: the player now to move holds a line
        return c, q
    return c, (0 if 0 not in c else None)


def _c4_play(c, p, h):
    from muzero_jl_amd.games.connect4 import _wins
    c = list(c)
    w = [c[r + 6 * h] for r in range(6)].index(0)
    c[w + 6 * h] = p
    if _wins(np.array(c) == p, w, h):
        return c, p
    return c, (0 if 0 not in c else None)


def _naive(name, board, player, S, R, seed, ident, step):
    from muzero_jl_amd.rng import rng_below, rng_u32
    play = _ttt_play if name == "tictactoe" else _c4_play
    A = 9 if name == "tictactoe" else 7

    def legal(c):
        return [a for a in range(A) if (c[a] if name == "tictactoe" else c[5 + 6 * a]) == 0]

    def rollout(c, p, i, j):
        first, ply = p, 0
        while True:
            acts = legal(c)
            r = rng_u32(seed, ROLLOUT, ident, step, (i * 64 + j) * 64 + ply)
            c, winner = play(c, p, acts[rng_below(r, len(acts))])
            if winner is not None:
                return 0 if winner == 0 else 1 if winner == first else -1
            p, ply = 3 - p, ply + 1

    def simulate(node, c, p, i):
        """One simulation from `node` (position c, p to move): its outcome for p, in rollouts."""
        N, L = sum(e["n"] for e in node.values()), len(node)
        score = {a: (e["w"] / (e["n"] * R) if e["n"] else 0.0) + math.sqrt(N) / ((1 + e["n"]) * L)
                 for a, e in node.items()}
        a = min(node, key=lambda a: (-score[a], a))
        e = node[a]
        c2, winner = play(c, p, a)
        if winner is not None:
            z = R * (0 if winner == 0 else 1 if winner == p else -1)
        elif e["child"] is not None:
            z = -simulate(e["child"], c2, 3 - p, i)
        else:
            e["child"] = {b: dict(n=0, w=0, child=None) for b in legal(c2)}
            z = -sum(rollout(c2, 3 - p, i, j) for j in range(R))
        e["n"] += 1
        e["w"] += z
        return z

    planes = np.asarray(board).reshape(3, -1)
    c0 = [int(x) for x in planes[0] * 1 + planes[1] * 2]
    root = {a: dict(n=0, w=0, child=None) for a in legal(c0)}
    for i in range(S):
        simulate(root, c0, player, i)
    n, w = np.full(A, -1, np.int32), np.zeros(A, np.int32)
    for a, e in root.items():
        n[a], w[a] = e["n"], e["w"]
    return n, w


@pytest.mark.parametrize("name", mc.NAMES)
def test_mirror_equals_the_naive_restatement(name):
    pos = mc.positions(name)
    for k, (b, p) in enumerate(pos[::2] + pos[-3:]):
        for S, R in ((1, 1), (7, 3), (40, 2)):
            got = mc.mirror(name, (b, p), S, R, ident=k, rng_step=S + 1)
            want = _naive(name, b, p, S, R, mc.SEED, k, S + 1)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, S, R, got, want)


@pytest.mark.parametrize("name", mc.NAMES)
def test_root_statistics_invariants(name):
    A = 9 if name == "tictactoe" else 7
    for k, (b, p) in enumerate(mc.positions(name)):
        planes = np.asarray(b).reshape(3, -1)
        empty = planes[2] != 0
        legal = empty if name == "tictactoe" else empty[5 + 6 * np.arange(7)]
        for S, R in mc.SETTINGS:
            n, w = mc.mirror(name, (b, p), S, R, 3 + k, 5 + S)
            assert n.shape == (A,) and np.array_equal(n >= 0, legal), (k, S, R)
            assert n[legal].sum() == S and (np.abs(w) <= np.maximum(n, 0) * R).all(), (k, S, R, n, w)
            assert not w[~legal].any()
            if S == 1:                                       # every score is 0: the lowest legal action
                assert n[np.flatnonzero(legal)[0]] == 1
    if name == "connect4":                                   # a root move that wins at once: every outcome +R
        b, p = mc.xc.C4_WIN
        n, w = mc.mirror(name, (b, p), 64, 16, 1, 1)
        assert n[0] > 32 and w[0] == n[0] * 16
    else:                                                    # Q14: every reply loses at once
        b, p = mc.xc.TTT_Q14
        n, w = mc.mirror(name, (b, p), 64, 16, 1, 1)
        assert np.array_equal(w[n >= 0], -16 * n[n >= 0])


def test_arguments_are_checked():
    from muzero_jl_amd.games.mcts_rules import mcts_pick, mcts_root_stats
    b, p = mc.xc.TTT_EMPTY
    for kw in (dict(player=0), dict(sims=0), dict(sims=1025), dict(rollouts=0), dict(rollouts=65)):
        args = dict(player=p, sims=4, rollouts=2)
        args.update(kw)
        with pytest.raises(ValueError):
            mcts_root_stats("tictactoe", b, **args)
    with pytest.raises(ValueError):
        mcts_root_stats("atari", b, 1, 4, 2)
    for bad in mc.xc.bad_boards("tictactoe"):
        with pytest.raises(ValueError):
            mcts_root_stats("tictactoe", bad, 1, 4, 2)
    n = np.array([3, -1, 5, 5, 0, 5, -1, 1, 1], np.int32)
    assert [mcts_pick(n, r) for r in (0, 0x55555556, 0xAAAAAAAB, 0xFFFFFFFF)] == [3, 4, 6, 6]


def test_constants_match_the_header():
    """MZ_OPP_MCTS = 4 (written as the id after MZ_OPP_NETWORK = 3) and MZ_RNG_ROLLOUT = 10 in the C headers, the
    Python binding, the Julia binding and rng.py; the two new prototypes are bound with the header's arity."""
    import os
    import re
    from muzero_jl_amd import abi, rng
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mz.h")).read()
    det = open(os.path.join(root, "include", "mz_detmath.h")).read()
    jl = open(os.path.join(root, "julia", "LibMZ.jl")).read()
    assert re.search(r"\bMZ_OPP_NETWORK = 3\b", hdr) and re.search(r"\bMZ_OPP_MCTS = MZ_OPP_NETWORK \+ 1\b", hdr)
    assert re.search(r"\bOPP_NETWORK = Cint\(3\)", jl) and re.search(r"\bOPP_MCTS = OPP_NETWORK \+ Cint\(1\)", jl)
    assert abi.OPP_MCTS == 4 == abi.OPP_NETWORK + 1
    assert int(re.search(r"\bMZ_RNG_ROLLOUT = (\d+)", det).group(1)) == rng.MZ_RNG_ROLLOUT == ROLLOUT
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mz_mcts_opponent", "mz_mcts_eval"):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", body, flags=re.M)
        assert m and len(m.group(1).split(",")) == len(abi.SIGNATURES[name][1]), name
        assert f"(:{name}, libmz)" in jl, name


def _play_match(name, games, S, R):
    """`games` seeded games of the mirror at (S, R) against the uniform random mover, MCTS as player 1 in the
    even games and as player 2 in the odd ones; (MCTS wins, random's wins, draws)."""
    from muzero_jl_amd.games.expert import _rules
    from muzero_jl_amd.games.mcts_rules import mcts_pick, mcts_root_stats
    from muzero_jl_amd.rng import rng_u32
    legal, step, _ = _rules(name)
    cells = 9 if name == "tictactoe" else 42
    rng = np.random.default_rng(2024)
    tally = [0, 0, 0]
    for g in range(games):
        me, c, p, move = 1 + g % 2, (0,) * cells, 1, 0
        while True:
            if p == me:
                planes = np.array([[x == 1 for x in c], [x == 2 for x in c], [x == 0 for x in c]], np.uint8)
                n, _ = mcts_root_stats(name, planes.reshape(-1), p, S, R, mc.SEED, g, move)
                a = mcts_pick(n, rng_u32(mc.SEED, OPPONENT, g, move, 0)) - 1
            else:
                a = int(rng.choice(legal(c)))
            c, done, winner = step(c, p, a)
            if done:
                tally[2 if winner == 0 else 0 if winner == me else 1] += 1
                break
            p, move = 3 - p, move + 1
    return tally


@pytest.mark.parametrize("name,games", [("tictactoe", 200), ("connect4", 100)])
def test_mcts_beats_the_random_mover(name, games):
    """The strength floor at (16, 8), both sides: more wins than losses.  A floor, not a measurement."""
    wins, losses, draws = _play_match(name, games, 16, 8)
    print(name, "mcts wins", wins, "random wins", losses, "draws", draws)
    assert wins + losses + draws == games and wins > losses
