"""Net against net (MZ_OPP_NETWORK) on the CPU: the host mirror's
pick rule with stub engines, and the Python binding against the header."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub:
    """An engine whose search returns its own tag everywhere: child visits
    tag + action slot / 100, root value -tag, and the tag-th legal action."""

    def __init__(self, conf, tag):
        self.conf, self.tag, self.rng_seed, self.calls = conf, tag, 5, []

    def mcts_search(self, obs, legal, tp, exploration=True, rng_step=0, game_offset=0, temperature=1.0):
        self.calls.append((obs.copy(), legal.copy(), tp.copy(), exploration, rng_step, game_offset, temperature))
        G, A = legal.shape
        cv = np.float32(self.tag) + np.tile(np.arange(A, dtype=np.float32) / 100, (G, 1))
        rv = np.full(G, -float(self.tag), np.float32)
        act = np.array([np.flatnonzero(legal[g])[self.tag - 1] + 1 for g in range(G)], np.int32)
        return cv, rv, act


@pytest.mark.parametrize("mzp", [1, 2])
def test_host_mirror_takes_each_result_from_the_movers_engine(mzp):
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    G = 5
    a, b = _Stub(ttt.conf, 1), _Stub(ttt.conf, 2)
    sp = BatchedSelfPlay(a, ttt.BatchedTicTacToe, G, game_offset=7, step0=100, opponent="network",
                         opponent_engine=b, muzero_player=mzp)
    for m in range(4):                                   # no line before move 5: every slot moves in lockstep
        mover = m % 2 + 1
        tag = 1 if mover == mzp else 2
        assert not len(sp.play_move(0.0))
        for h in sp.histories:
            assert h.to_play_history[-1] == mover
            assert np.array_equal(h.child_visits[-1], np.float32(tag) + np.arange(9, dtype=np.float32) / 100)
            assert h.root_values[-1] == -float(tag)
        # the tag-th legal action: engine 1 takes the first empty cell, engine 2 the second
        want = [a1 for a1 in range(1, 10) if a1 not in sp.histories[0].action_history[:-1]][tag - 1]
        assert all(h.action_history[-1] == want for h in sp.histories)
    assert len(a.calls) == len(b.calls) == 4             # both engines search every move ...
    for ca, cb in zip(a.calls, b.calls):                 # ... with identical arguments
        assert all(np.array_equal(x, y) for x, y in zip(ca, cb))
    assert [c[4] for c in a.calls] == [100, 101, 102, 103] and a.calls[0][5] == 7


def test_host_mirror_mixes_per_game():
    """Slots whose movers differ inside one move: each takes its own mover's engine."""
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    a, b = _Stub(ttt.conf, 1), _Stub(ttt.conf, 2)
    sp = BatchedSelfPlay(a, ttt.BatchedTicTacToe, 4, opponent="network", opponent_engine=b, muzero_player=1)
    sp.env.player[:] = [1, 2, 2, 1]
    sp.play_move(0.0)
    assert [h.root_values[-1] for h in sp.histories] == [-1.0, -2.0, -2.0, -1.0]
    assert [h.action_history[-1] for h in sp.histories] == [1, 2, 2, 1]
    assert [float(h.child_visits[-1][0]) for h in sp.histories] == [1.0, 2.0, 2.0, 1.0]


def test_host_mirror_argument_checks():
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.selfplay import BatchedSelfPlay
    a = _Stub(ttt.conf, 1)
    with pytest.raises(AssertionError):
        BatchedSelfPlay(a, ttt.BatchedTicTacToe, 2, opponent="network")
    with pytest.raises(AssertionError):
        BatchedSelfPlay(a, ttt.BatchedTicTacToe, 2, opponent="self", opponent_engine=a)


def test_binding_matches_the_header():
    import ctypes
    from muzero_jl_amd import abi
    hdr = open(os.path.join(ROOT, "include", "mz.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(MZ_OPP_\w+)\s*=\s*(\d+)", hdr))
    assert enum == {"MZ_OPP_SELF": abi.OPP_SELF, "MZ_OPP_RANDOM": abi.OPP_RANDOM, "MZ_OPP_EXPERT": abi.OPP_EXPERT,
                    "MZ_OPP_NETWORK": abi.OPP_NETWORK} and abi.OPP_NETWORK == 3
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    want = {"mz_opponent_weights_set": (ci, [vp, ci, vp, sz]), "mz_opponent_weights_get": (ci, [vp, ci, vp, sz]),
            "mz_opponent_from": (ci, [vp, ci, vp]), "mz_opponent_load": (ci, [vp, ctypes.c_char_p, vp])}
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in want.items():
        assert abi.SIGNATURES[name] == sig, name
        m = re.search(r"^int " + name + r"\(([^;]*)\);", body, flags=re.M)
        assert m and len(m.group(1).split(",")) == len(sig[1]), name
    for meth in ("opponent_set_weights", "opponent_get_weights", "opponent_from", "opponent_load"):
        assert callable(getattr(abi.Engine, meth))
