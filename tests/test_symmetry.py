"""Board-symmetry augmentation of get_batch, on the CPU: the group tables, their equivariance
with the host envs and the expert, and the host mirror (ReplayBuffer.get_batch(step, symmetry=True) against
apply_symmetry of the plain batch)."""
import dataclasses
import os
import re

import numpy as np
import pytest

from muzero_jl_amd import rng
from muzero_jl_amd.games import connect4, symmetry, tictactoe
from muzero_jl_amd.games.expert import ILLEGAL, expert_scores
from muzero_jl_amd.replay_buffer import ReplayBuffer, apply_symmetry, symmetry_ids
from muzero_jl_amd.selfplay import GameHistory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the issue's table: row s, column c = the cell that cell c moves to
TTT_TABLE = [[0, 1, 2, 3, 4, 5, 6, 7, 8], [6, 3, 0, 7, 4, 1, 8, 5, 2], [8, 7, 6, 5, 4, 3, 2, 1, 0],
             [2, 5, 8, 1, 4, 7, 0, 3, 6], [0, 3, 6, 1, 4, 7, 2, 5, 8], [6, 7, 8, 3, 4, 5, 0, 1, 2],
             [8, 5, 2, 7, 4, 1, 6, 3, 0], [2, 1, 0, 5, 4, 3, 8, 7, 6]]

ENVS = {"tictactoe": (tictactoe, tictactoe.BatchedTicTacToe), "connect4": (connect4, connect4.BatchedConnect4)}


def _tables(name):
    return symmetry.tables(name, ENVS[name][0].conf.observation_shape)


def random_game(name, gen):
    """One game of uniformly random legal moves on the host env: (GameHistory with random child visits and
    root values, boards after each move, legal masks before each move)."""
    mod, env_cls = ENVS[name]
    A = len(mod.conf.action_space)
    env = env_cls(1)
    h, after, masks = GameHistory(), [], []
    while True:
        mask = env.legal_mask()[0].copy()
        a = int(gen.choice(np.flatnonzero(mask))) + 1
        cv = (gen.random(A) * mask).astype(np.float32)
        h.observation_history.append(env.board[0].astype(np.float32))
        h.to_play_history.append(int(env.player[0]))
        r, done = env.step(np.array([a]))
        h.action_history.append(a)
        h.reward_history.append(float(r[0]))
        h.child_visits.append(cv / cv.sum())
        h.root_values.append(float(np.float32(gen.normal())))
        masks.append(mask)
        after.append(env.board[0].copy())
        if done[0]:
            return h, after, masks


@pytest.mark.parametrize("name", ["tictactoe", "connect4"])
def test_tables_are_a_group(name):
    t = _tables(name)
    P, A = t.cell.shape[1], t.action.shape[1]
    assert t.n == (8 if name == "tictactoe" else 2) and t.planes == 3
    for tab, m in ((t.cell, P), (t.action, A)):
        assert all(sorted(row) == list(range(m)) for row in tab.tolist())
        assert tab[0].tolist() == list(range(m))
        assert len({tuple(r) for r in tab.tolist()}) == t.n
    pairs = {(tuple(t.cell[s]), tuple(t.action[s])) for s in range(t.n)}
    for s in range(t.n):
        for r in range(t.n):                            # s, then r, on the cells and on the actions: one element
            assert (tuple(t.cell[r][t.cell[s]]), tuple(t.action[r][t.action[s]])) in pairs
        assert np.array_equal(t.cell[symmetry.inverse(t, s)][t.cell[s]], np.arange(P))


def test_tictactoe_table_is_the_printed_one():
    t = _tables("tictactoe")
    assert t.cell.tolist() == TTT_TABLE and t.action.tolist() == TTT_TABLE
    lines = {frozenset(l) for l in tictactoe.LINES.tolist()}
    for s in range(8):
        assert {frozenset(t.cell[s][l].tolist()) for l in tictactoe.LINES} == lines


def test_connect4_table_is_the_mirror():
    t = _tables("connect4")
    W, H = connect4.W, connect4.H
    for h in range(H):
        assert t.action[1][h] == H - 1 - h
        for w in range(W):
            assert t.cell[1][w + W * h] == w + W * (H - 1 - h)


def test_for_conf_and_refusals():
    assert symmetry.for_conf(tictactoe.conf).n == 8 and symmetry.for_conf(connect4.conf).n == 2
    from muzero_jl_amd.games import atari_synth
    with pytest.raises(ValueError, match="symmetry"):
        symmetry.for_conf(atari_synth.conf)
    with pytest.raises(ValueError, match="no symmetry group"):
        symmetry.tables("atari", (84, 84, 4))


@pytest.mark.parametrize("name", ["tictactoe", "connect4"])
def test_env_is_equivariant(name):
    """Stepping the permuted actions on a fresh env gives, at every move, the permuted board, the same mover,
    reward and termination, and the permuted legal mask: what a table on the wrong axis breaks."""
    t = _tables(name)
    env_cls = ENVS[name][1]
    gen = np.random.default_rng(3)
    for _ in range(50):
        h, after, masks = random_game(name, gen)
        for s in range(t.n):
            cp, ap = t.cell[s], t.action[s]
            env = env_cls(1)
            for m, a in enumerate(h.action_history):
                want = np.empty_like(masks[m])
                want[ap] = masks[m]
                assert np.array_equal(env.legal_mask()[0], want)
                assert int(env.player[0]) == h.to_play_history[m]
                r, done = env.step(np.array([ap[a - 1] + 1]))
                b = after[m].reshape(3, -1)
                pb = np.empty_like(b)
                pb[:, cp] = b
                assert np.array_equal(env.board[0].reshape(3, -1), pb)
                assert float(r[0]) == h.reward_history[m]
                assert bool(done[0]) == (m == len(h.action_history) - 1)


@pytest.mark.parametrize("name,depth,moves", [("tictactoe", 9, (0, 2, 3, 5)), ("connect4", 2, (1, 6, 11))])
def test_expert_is_invariant(name, depth, moves):
    """score(s·board, s·a) = score(board, a) for every element s."""
    t = _tables(name)
    gen = np.random.default_rng(9)
    seen = 0
    for _ in range(3):
        h, _, _ = random_game(name, gen)
        for m in moves:
            if m >= len(h.action_history):
                continue
            board, player = h.observation_history[m], h.to_play_history[m]
            base = expert_scores(name, board, player, depth)
            for s in range(t.n):
                pb = np.empty((3, t.cell.shape[1]), np.float32)
                pb[:, t.cell[s]] = board.reshape(3, -1)
                want = np.empty_like(base)
                want[t.action[s]] = base
                assert np.array_equal(expert_scores(name, pb.reshape(-1), player, depth), want)
            seen += int((base != ILLEGAL).any())
    assert seen >= 3


def _buffer(name, games, seed, **conf_kw):
    mod = ENVS[name][0]
    conf = dataclasses.replace(mod.conf, replay_buffer_size=games, **conf_kw)
    rb = ReplayBuffer(conf, seed=seed)
    gen = np.random.default_rng(seed)
    for _ in range(games):
        rb.save_game(random_game(name, gen)[0])
    return conf, rb


@pytest.mark.parametrize("name,kw", [("tictactoe", {}), ("connect4", {}), ("tictactoe", {"stacked_observations": 2}),
                                     ("tictactoe", {"PER": True, "PER_alpha": 1})])
def test_mirror_get_batch_is_the_transformed_plain_batch(name, kw):
    """get_batch(step, symmetry=True) replays each sampled game in its drawn orientation and samples that;
    apply_symmetry transforms the finished plain batch.  The two agree array for array."""
    conf, rb = _buffer(name, 24, 5, batch_size=64, **kw)
    t = symmetry.for_conf(conf)
    K = conf.num_unroll_steps
    for step in (1, 2, 7):
        idx_p, plain = rb.get_batch(step)
        idx_s, sym = rb.get_batch(step, symmetry=True)
        ids = rb.last_symmetry_ids
        assert np.array_equal(ids, symmetry_ids(rb.seed, step, conf.batch_size, t.n))
        assert set(ids.tolist()) == set(range(t.n))
        lens = {g: len(h.root_values) for g, h in rb.buffer.items()}
        assert any(pos == 1 for _, pos in idx_p)                       # the all-zero history block
        assert any(pos + K > lens[g] for g, pos in idx_p)              # absorbing-state actions
        assert idx_s == idx_p
        want = apply_symmetry(plain, ids, t)
        assert set(want) == set(sym) and ("weights" in sym) == bool(conf.PER)
        for k in sym:
            assert np.array_equal(sym[k], want[k]), (step, k)
        for k in ("target_values", "target_rewards", "gradient_scale"):
            assert np.array_equal(sym[k], plain[k]), k
        for k in ("observation", "actions", "target_policies"):
            assert not np.array_equal(sym[k], plain[k]), k


def test_apply_symmetry_identity_out_of_range_and_inverse():
    conf, rb = _buffer("tictactoe", 12, 2, batch_size=16)
    t = symmetry.for_conf(conf)
    _, plain = rb.get_batch(3)
    for ids in (np.zeros(16, np.int32), np.full(16, 8, np.int32), np.full(16, -1, np.int32)):
        out = apply_symmetry(plain, ids, t)
        assert all(np.array_equal(out[k], plain[k]) for k in plain)
    ids = np.arange(16, dtype=np.int32) % 8
    back = apply_symmetry(apply_symmetry(plain, ids, t), np.array([symmetry.inverse(t, s) for s in ids]), t)
    assert all(np.array_equal(back[k], plain[k]) for k in plain)


def test_frame_stack_buffer_refuses_symmetry():
    from muzero_jl_amd.games import atari_synth
    rb = ReplayBuffer(atari_synth.conf, seed=1, frame_stack=4)
    with pytest.raises(ValueError, match="Atari-like"):
        rb.get_batch(1, symmetry=True)


def test_rng_stream_constant():
    det = open(os.path.join(ROOT, "include", "mz_detmath.h")).read()
    assert int(re.search(r"\bMZ_RNG_SYMMETRY = (\d+)", det).group(1)) == rng.MZ_RNG_SYMMETRY == 11
