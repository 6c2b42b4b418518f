"""Replay buffer and targets — host mirror of src/ReplayBuffer.jl.

FIFO buffer of GameHistory keyed by game id (save_game, :133-161; the
RemoteBufferChannel Dict semantics, src/RemoteBufferChannel.jl), uniform
or prioritized (PER, :73-107, 133-145, 168-183) sampling with the engine's Philox streams instead of
Julia's global RNG (quirk Q6), n-step value targets with the reference's
exact indexing (quirk Q9), and batch assembly in the reference's column-major
tuple layout (get_batch, :188-217).  One buffer per GPU shard.
"""
import math
from collections import OrderedDict

import numpy as np

from .selfplay import GameHistory, frame_stack_obs, get_stacked_observations

MZ_RNG_GAME, MZ_RNG_POS, MZ_RNG_ABSORB = 4, 5, 6
from .rng import MZ_RNG_SYMMETRY, _M, _philox, rng_below, rng_u32  # noqa: F401  (re-exported)


def disc_pow(g, n):
    """discount^n as Julia's Float32^Int (llvm.pow.f32) ≈ f32(pow(f64))."""
    return np.float32(math.pow(float(np.float32(g)), float(n)))


def compute_target_value(conf, h, index):
    """ReplayBuffer.jl:5-20 (Q9); index is 1-based.  Float32 arithmetic.  The
    bootstrap value is the reanalysed one unless that field is None (:8)."""
    f32 = np.float32
    T = len(h.root_values)
    bi = index + conf.td_steps
    if bi < T:
        rvs = h.root_values if h.reanalysed_predicted_root_values is None else h.reanalysed_predicted_root_values
        rv = f32(rvs[bi - 1])
        last = rv if h.to_play_history[bi - 1] == h.to_play_history[index - 1] else -rv
        value = f32(last * disc_pow(conf.discount, conf.td_steps))
        for i in range(1, conf.td_steps + 2):
            r = f32(h.reward_history[index + i - 2])
            sr = r if h.to_play_history[index - 1] == h.to_play_history[index + i - 1] else -r
            value = f32(value + f32(sr * disc_pow(conf.discount, i)))
    else:
        value = f32(0.0)
    return value


def make_target(conf, h, state_index, seed=0, sample=0, step=0, action_perm=None):
    """ReplayBuffer.jl:25-50 -> (values (K+1,), rewards (K+1,), policies (K+1, A), actions (K+1,)).
    action_perm (symmetric get_batch, h already permuted): the 0-based action table row that the
    absorbing-state actions, drawn as ever, go through."""
    K, A = conf.num_unroll_steps, len(conf.action_space)
    T = len(h.root_values)
    tv = np.zeros(K + 1, np.float32)
    tr = np.zeros(K + 1, np.float32)
    tp = np.zeros((K + 1, A), np.float32)
    ta = np.zeros(K + 1, np.float32)
    uni = np.float32(1.0) / np.float32(A)
    # the policy targets: the reanalyse search's child_visits unless that field is None
    cvs = h.child_visits if h.reanalysed_child_visits is None else h.reanalysed_child_visits
    for k in range(K + 1):
        ci = state_index + k
        if ci < T:
            tv[k] = compute_target_value(conf, h, ci)
            tr[k] = h.reward_history[ci - 1]
            tp[k] = cvs[ci - 1]
            ta[k] = h.action_history[ci - 1]
        elif ci == T:
            tr[k] = h.reward_history[ci - 1]
            tp[k] = uni
            ta[k] = h.action_history[ci - 1]
        else:                                              # absorbing states
            tp[k] = uni
            ta[k] = rng_below(rng_u32(seed, MZ_RNG_ABSORB, sample, step, k), A) + 1
            if action_perm is not None:
                ta[k] = action_perm[int(ta[k]) - 1] + 1
    return tv, tr, tp, ta


def symmetry_ids(seed, step, B, n):
    """s_b of samples 0..B-1 of learner step `step` in a group of order n: keyed like the
    sample's GAME and POS draws."""
    return np.array([rng_below(rng_u32(seed, MZ_RNG_SYMMETRY, b, step, 0), n) for b in range(B)], np.int32)


def apply_symmetry(batch, ids, tables):
    """The batch dict (get_batch's layout) with row b under element ids[b] of `tables`
    (games/symmetry.SymmetryTables); a new dict.  Board planes are permuted by the cell table, the
    constant action planes and `actions` hold the permuted id, target_policies moves with the action
    table; everything else is copied.  An id outside 0..n-1 leaves its row as it is."""
    cp, ap, C = tables.cell, tables.action, tables.planes
    P = cp.shape[1]
    out = {k: np.array(v, copy=True) for k, v in batch.items()}
    obs, acts, tpol = batch["observation"], batch["actions"], batch["target_policies"]
    for b, s in enumerate(np.asarray(ids).reshape(-1)):
        if not 0 <= s < tables.n:
            continue
        x = obs[b].reshape(-1, P)
        y = np.empty_like(x)
        y[:, cp[s]] = x
        for pl in range(C, x.shape[0], C + 1):                 # the stacked action planes (Q15)
            if x[pl, 0] != 0:                                  # (the zero block before move 1 stays)
                y[pl, :] = ap[s][int(x[pl, 0]) - 1] + 1
        out["observation"][b] = y.reshape(-1)
        out["actions"][b] = ap[s][acts[b].astype(np.int64) - 1] + 1
        out["target_policies"][b][:, ap[s]] = tpol[b]
    return out


def _permuted_history(h, cp, ap, C):
    """GameHistory h played in another orientation: boards through the cell table row cp, actions and
    child visits through the action table row ap."""
    def board(o):
        x = np.asarray(o, np.float32).reshape(C, -1)
        y = np.empty_like(x)
        y[:, cp] = x
        return y.reshape(-1)

    def visits(cv):
        out = np.empty(len(ap), np.float32)
        out[ap] = np.asarray(cv, np.float32)
        return out
    return GameHistory(observation_history=[board(o) for o in h.observation_history],
                       action_history=[int(ap[a - 1]) + 1 for a in h.action_history],
                       reward_history=h.reward_history, to_play_history=h.to_play_history,
                       child_visits=[visits(c) for c in h.child_visits], root_values=h.root_values,
                       reanalysed_predicted_root_values=h.reanalysed_predicted_root_values,
                       priorities=h.priorities, game_priority=h.game_priority,
                       reanalysed_child_visits=None if h.reanalysed_child_visits is None else
                       [visits(c) for c in h.reanalysed_child_visits])


_TTT_LINES = np.array([[0, 3, 6], [1, 4, 7], [2, 5, 8], [0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 4, 8], [6, 4, 2]])


def stored_legal_mask(conf, obs, to_play):
    """Legal actions (A,) uint8 of `to_play` on a stored board (planes [p1, p2,
    empty], col-major cells) — env_legal_board of the kernels with over = 0:
    TicTacToe (3, 3, 3): the empty cells, none if to_play holds a line (Q14);
    Connect4 (6, 7, 3): the top cell of each column.  A to_play outside the
    players gives the empty mask."""
    W, H, C = conf.observation_shape
    b = np.asarray(obs).reshape(-1) != 0
    if C != 3 or (W, H) not in ((3, 3), (6, 7)):
        raise ValueError("stored_legal_mask: a TicTacToe or Connect4 board is needed")
    if to_play not in conf.players:
        return np.zeros(len(conf.action_space), np.uint8)
    cells = W * H
    if (W, H) == (3, 3):
        if b[9 * (to_play - 1): 9 * to_play][_TTT_LINES].all(axis=1).any():
            return np.zeros(9, np.uint8)
        return b[18:27].astype(np.uint8)
    return b[2 * cells + (W - 1) + W * np.arange(H)].astype(np.uint8)


def per_priority(x, alpha):
    """|x|^PER_alpha as Julia's Float32^Int, restated as f64 repeated
    multiplication rounded once to f32 (the kernels' per_priority)."""
    ax = abs(float(np.float32(x)))
    r = 1.0
    for _ in range(alpha):
        r = r * ax
    return np.float32(r)


def per_uniform(r):
    """uniform in [0, 1) from a Philox draw (24 bits, exact)."""
    return (r >> 8) * 5.9604644775390625e-08


def per_categorical(w, u):
    """Categorical over p_i = w_i / S (S = ascending f32 sum): the first index
    whose ascending f32 running sum of p is > u (else the last; Distributions
    0.25 advances while cp <= draw, so zero-probability entries are never
    drawn); returns
    (index, p_index).  The restatement of rand(rng, Categorical(p)) used by
    sample_n_games / sample_position with PER (ReplayBuffer.jl:75-78, 96-103)."""
    f32 = np.float32
    S = f32(0.0)
    for x in w:
        S = f32(S + f32(x))
    i = 0
    p = f32(f32(w[0]) / S)
    c = p
    while float(c) <= u and i < len(w) - 1:
        i += 1
        p = f32(f32(w[i]) / S)
        c = f32(c + p)
    return i, p


REAN_BY_VALUE, REAN_BY_SEARCH = 1, 2        # abi.REAN_BY_VALUE / REAN_BY_SEARCH
REAN_VALUE_ROWS = 4096                      # a value round's capacity (the engine's position chunk)


def pack_round(lens_by_game_number, cursor, played, cap, R):
    """One round of the Reanalyse worker (kernel mz_reanalyse_pack), restated: which games a round of
    capacity R rows takes from `cursor`, the game number (save_game's 1-based numbering) of the next game
    to reanalyse.  lens_by_game_number[g] = stored positions of held game g; played = num_played_games;
    cap = the shard's capacity.  With n = min(played, cap) and oldest = played - n + 1: nothing if
    played == 0 (the cursor stays); else a cursor outside [oldest, played] goes to oldest, and games
    cursor, cursor + 1, ... are taken while they are <= played and their lengths sum to <= R — whole
    games, no wrap inside a round.  Returns (first, games, rows, new_cursor): the first game number
    taken, how many, the live rows [(game number, 0-based pos)] in (game, pos) order, and the first game
    not taken."""
    if played <= 0:
        return cursor, 0, [], cursor
    n = min(played, cap)
    oldest = played - n + 1
    first = oldest if (cursor < oldest or cursor > played) else cursor
    rows, g = [], first
    while g <= played and len(rows) + lens_by_game_number[g] <= R:
        rows.extend((g, pos) for pos in range(lens_by_game_number[g]))
        g += 1
    return first, g - first, rows, g


class ReplayBuffer:
    """Per-GPU buffer: Dict{game_id => GameHistory} with FIFO eviction."""

    def __init__(self, conf, seed=0, frame_stack=0):
        """frame_stack: the env's own frame stacking (games/atari_synth.py,
        observation_history holds one frame per move), 0 for board games."""
        self.conf = conf
        self.seed = seed
        self.frame_stack = frame_stack
        self.buffer = OrderedDict()
        self.num_played_games = 0
        self.num_played_steps = 0
        self.total_samples = 0
        self.num_reanalysed_games = 0
        self.reanalyse_cursor = 1                               # reanalyse_next: the next game number

    def __len__(self):
        return len(self.buffer)

    def save_game(self, history: GameHistory):                  # :133-161
        n = len(history.root_values)
        if self.conf.PER:                                       # initial priorities :136-143
            history.priorities = np.array([per_priority(np.float32(history.root_values[i]) -
                                                        compute_target_value(self.conf, history, i + 1),
                                                        self.conf.PER_alpha) for i in range(n)], np.float32)
            history.game_priority = np.float32(history.priorities.max())
        self.num_played_games += 1
        self.num_played_steps += n
        self.total_samples += n
        self.buffer[self.num_played_games] = history
        if self.conf.replay_buffer_size < self.num_played_games:
            del_id = self.num_played_games - self.conf.replay_buffer_size
            removed = self.buffer.pop(del_id)
            self.total_samples -= len(removed.root_values)

    def get_batch(self, step, symmetry=False):
        """:188-217 with uniform sampling keyed by the learner step.
        Returns (index_batch, batch dict in the engine's layout).  symmetry (mz_replay_set_symmetry,
        DESIGN §23): sample b is the stored game replayed under element s_b of the env's symmetry
        group, s_b from the SYMMETRY stream; the ids drawn are kept in self.last_symmetry_ids."""
        c = self.conf
        sym = None
        if symmetry:
            if self.frame_stack:
                raise ValueError("symmetry: the Atari-like env has no symmetry group")
            from .games import symmetry as _symmetry
            sym = _symmetry.for_conf(c)
            self.last_symmetry_ids = symmetry_ids(self.seed, step, c.batch_size, sym.n)
        B, K, A = c.batch_size, c.num_unroll_steps, len(c.action_space)
        ids = list(self.buffer.keys())
        n = len(ids)
        if n == 0:
            raise ValueError("replay buffer is empty")
        plane = c.observation_shape[0] * c.observation_shape[1]
        feat = plane * (c.observation_shape[2] * (c.stacked_observations + 1) + c.stacked_observations)
        obs = np.zeros((B, feat), np.float32)
        acts = np.zeros((B, K + 1), np.float32)
        tv = np.zeros((B, K + 1), np.float32)
        tr = np.zeros((B, K + 1), np.float32)
        tp = np.zeros((B, K + 1, A), np.float32)
        gs = np.zeros(B, np.float32)
        index_batch = []
        per = bool(c.PER)
        if per:                                                 # :190, :91-99
            total = sum(len(h.root_values) for h in self.buffer.values())
            gprio = [self.buffer[i].game_priority for i in ids]
            wts = np.zeros(B, np.float32)
        for b in range(B):
            rg = rng_u32(self.seed, MZ_RNG_GAME, b, step, 0)
            rp = rng_u32(self.seed, MZ_RNG_POS, b, step, 0)
            if per:
                gi, gprob = per_categorical(gprio, per_uniform(rg))                # sample_n_games :96-103
            else:
                gi = rng_below(rg, n)                                              # sample_n_games :102
            h = self.buffer[ids[gi]]
            T = len(h.root_values)
            if per:                                                                # sample_position :75-78
                pi, pprob = per_categorical(h.priorities, per_uniform(rp))
                pos = pi + 1
                wts[b] = np.float32(1.0) / np.float32(np.float32(np.float32(total) * gprob) * pprob)   # :213
            else:
                pos = rng_below(rp, T) + 1                                         # sample_position :80
            ap = None
            if sym is not None:
                s = self.last_symmetry_ids[b]
                ap = sym.action[s]
                h = _permuted_history(h, sym.cell[s], ap, sym.planes)
            tv[b], tr[b], tp[b], acts[b] = make_target(c, h, pos, self.seed, b, step, ap)
            if self.frame_stack:
                obs[b] = frame_stack_obs(h.observation_history, pos, self.frame_stack)
            else:
                obs[b] = get_stacked_observations(h.observation_history, h.action_history, pos,
                                                  c.stacked_observations, plane)
            gs[b] = min(K, len(h.action_history) + 1 - pos)                        # :212
            index_batch.append((ids[gi], pos))
        out = dict(observation=obs, actions=acts, target_values=tv, target_rewards=tr,
                   target_policies=tp, gradient_scale=gs)
        if per:
            out["weights"] = (wts / wts.max()).astype(np.float32)                 # :215
        return index_batch, out

    def reanalyse(self, value_fn, game_ids=None):
        """Reanalyze (ReplayBuffer.jl:8, 56-67; the worker muzero.jl:15-19 leaves
        unbuilt): reanalysed_predicted_root_values of each game = value_fn(stacked
        observations (T, feat)) -> (T,) values of the current networks.  game_ids
        None = every held game; an id that has left the buffer since it was
        chosen is skipped (update_history!'s check).  Returns the ids updated."""
        c = self.conf
        plane = c.observation_shape[0] * c.observation_shape[1]
        done = []
        for gid in (list(self.buffer.keys()) if game_ids is None else game_ids):
            h = self.buffer.get(gid)
            if h is None:
                continue
            T = len(h.root_values)
            if self.frame_stack:
                x = np.stack([frame_stack_obs(h.observation_history, i, self.frame_stack) for i in range(1, T + 1)])
            else:
                x = np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                                       c.stacked_observations, plane) for i in range(1, T + 1)])
            v = np.asarray(value_fn(x), np.float32).reshape(-1)
            if v.shape[0] != T:
                raise ValueError(f"value_fn returned {v.shape[0]} values for {T} positions")
            h.reanalysed_predicted_root_values = [np.float32(t) for t in v]
            self.num_reanalysed_games += 1
            done.append(gid)
        return done

    def reanalyse_search(self, search_fn, game_ids=None):
        """The other half of Reanalyze (mz_replay_reanalyse_search's mirror): every
        stored position of each game is searched again.  search_fn(obs (T, feat),
        legal (T, A) uint8, to_play (T,), p0) -> (child_visits (T, A), root_values
        (T,)); p0 = gi * (max_moves + 1) is the game's first row in the flattened
        selection (gi counts the ids as given, skipped ones included), the offset
        of its Philox game ids.  legal comes from the stored board: the empty
        plane's cells (TicTacToe, none if the player to move holds a line, Q14)
        or the top cell of each column (Connect4).  A position with no legal
        action is not searched and keeps its stored child_visits / root_values.
        An id that has left the buffer is skipped (update_history!'s check).
        Returns the ids updated."""
        if self.frame_stack:
            raise ValueError("reanalyse: frame-stack env not built")
        done = []
        for gi, gid in enumerate(list(self.buffer.keys()) if game_ids is None else game_ids):
            h = self.buffer.get(gid)
            if h is None:
                continue
            self._search_game(h, search_fn, gi * (self.conf.max_moves + 1))
            done.append(gid)
        return done

    def _search_game(self, h, search_fn, p0):
        """Game h's positions searched again as rows p0 .. p0 + T - 1 of the selection (reanalyse_search)."""
        c = self.conf
        plane = c.observation_shape[0] * c.observation_shape[1]
        T = len(h.root_values)
        x = np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                               c.stacked_observations, plane) for i in range(1, T + 1)])
        legal = np.stack([stored_legal_mask(c, h.observation_history[i], h.to_play_history[i]) for i in range(T)])
        live = legal.any(axis=1)
        cv = np.array(h.child_visits, np.float32)
        rv = np.array(h.root_values, np.float32)
        if live.any():
            # unsearched rows go to search_fn as the dummy: zero observation, all legal, to_play 1
            xs, ls = np.where(live[:, None], x, np.float32(0)), np.where(live[:, None], legal, np.uint8(1))
            tps = np.where(live, np.array(h.to_play_history, np.int32), 1).astype(np.int32)
            ncv, nrv = search_fn(xs, ls, tps, p0)
            ncv, nrv = np.asarray(ncv, np.float32), np.asarray(nrv, np.float32).reshape(-1)
            if ncv.shape != cv.shape or nrv.shape != rv.shape:
                raise ValueError(f"search_fn returned {ncv.shape}, {nrv.shape} for {T} positions")
            cv[live], rv[live] = ncv[live], nrv[live]
        h.reanalysed_child_visits = [r for r in cv]
        h.reanalysed_predicted_root_values = [np.float32(t) for t in rv]
        self.num_reanalysed_games += 1

    def reanalyse_next(self, fn, mode, R=None):
        """One round of the Reanalyse worker (mz_replay_reanalyse_next's mirror): pack_round from this
        buffer's cursor, then the taken games through reanalyse (mode REAN_BY_VALUE, fn = its value_fn) or
        the search of reanalyse_search (REAN_BY_SEARCH, fn = its search_fn; p0 = the game's first row in the
        packed round, so row i has Philox id game_offset + i).  R: the round's capacity in rows (the
        engine's: max_games in search mode, REAN_VALUE_ROWS in value mode, the default there).  Returns
        (first, games, rows, new_cursor) of pack_round."""
        if self.frame_stack:
            raise ValueError("reanalyse: frame-stack env not built")
        if mode not in (REAN_BY_VALUE, REAN_BY_SEARCH):
            raise ValueError("reanalyse: mode must be REAN_BY_VALUE or REAN_BY_SEARCH")
        if R is None:
            if mode == REAN_BY_SEARCH:
                raise ValueError("reanalyse: a search round needs its capacity R (the engine's max_games)")
            R = REAN_VALUE_ROWS
        if R < self.conf.max_moves + 1:
            raise ValueError("reanalyse: a round of R rows cannot hold one game of max_moves + 1 positions")
        lens = {g: len(h.root_values) for g, h in self.buffer.items()}
        first, games, rows, cur = pack_round(lens, self.reanalyse_cursor, self.num_played_games,
                                             self.conf.replay_buffer_size, R)
        self.reanalyse_cursor = cur
        ids = list(range(first, first + games))
        if mode == REAN_BY_VALUE:
            self.reanalyse(fn, ids)
        else:
            p0 = 0
            for g in ids:
                self._search_game(self.buffer[g], fn, p0)
                p0 += lens[g]
        return first, games, rows, cur

    def update_priorities(self, index_batch, predicted_values, target_values):
        """update_priorities! (ReplayBuffer.jl:168-183, Learning.jl:400-404) in its
        intended reading: sample i (batch order) sets positions pos..min(pos+K, len)
        of its game, if still held, to |v̂ − v|^alpha of steps 0.., then the game
        priority to their max.  predicted / target values: (B, K+1)."""
        K, alpha = self.conf.num_unroll_steps, self.conf.PER_alpha
        for i, (gid, pos) in enumerate(index_batch):
            if gid not in self.buffer:
                continue
            h = self.buffer[gid]
            end = min(pos + K, len(h.priorities))
            for k in range(pos, end + 1):
                h.priorities[k - 1] = per_priority(np.float32(predicted_values[i][k - pos]) -
                                                   np.float32(target_values[i][k - pos]), alpha)
            h.game_priority = np.float32(h.priorities.max())
