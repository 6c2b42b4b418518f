"""Self-play host driver — the Python mirror of src/SelfPlay.jl over libmz.

The search itself (run_mcts + select_action + store_search_stats!,
SelfPlay.jl:115-306) runs as one HIP kernel per move for the whole batch of
games; this module keeps the reference's game loop (play_game, :330-382),
the stacked observations (:128-149) and the GameHistory records
(Constructors.jl:6-16).  Games advance in lockstep; a finished slot is reset
and starts a new game (continuous batched self-play).  RNG step keys: the
global move counter `step` (unique per move across the run), game id = slot.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .config import stacked_features
from .games.expert import DEFAULT_DEPTH, expert_pick, expert_scores, judge_move, solved_table, ttt_code
from .games.mcts_rules import DEFAULT_ROLLOUTS, DEFAULT_SIMS, mcts_pick, mcts_root_stats
from .rng import rng_below, rng_u32

MZ_RNG_OPPONENT = 7                                               # include/mz_detmath.h
MZ_RNG_ACTION = 3
NET_REPR, NET_PRED = 0, 1


def game_winner(env_name, last_reward, last_mover):
    """Winner of a finished game from its last move (0 = draw).  TicTacToe with
    Q14: the win test after a move looks at the plane of the player then to
    move, so a nonzero reward means 3 - mover holds a line; Connect4: the mover."""
    if last_reward == 0.0:
        return 0
    return 3 - last_mover if env_name == "tictactoe" else last_mover


def visit_softmax_temperature_fn(trained_steps: int) -> float:   # SelfPlay.jl:48-56
    if trained_steps < 500e3:
        return 1.0
    elif trained_steps < 750e3:
        return 0.5
    return 0.25


@dataclass
class GameHistory:                                               # Constructors.jl:6-16
    observation_history: List[np.ndarray] = field(default_factory=list)   # (W*H*C,) per move
    action_history: List[int] = field(default_factory=list)
    reward_history: List[float] = field(default_factory=list)
    to_play_history: List[int] = field(default_factory=list)
    child_visits: List[np.ndarray] = field(default_factory=list)          # (A,) per move
    root_values: List[float] = field(default_factory=list)
    reanalysed_predicted_root_values: Optional[list] = None
    priorities: Optional[np.ndarray] = None
    game_priority: Optional[float] = None
    reanalysed_child_visits: Optional[list] = None            # (A,) per move, from the reanalyse search

    def as_arrays(self):
        return dict(observation=np.array(self.observation_history, np.float32),
                    action=np.array(self.action_history, np.int32),
                    reward=np.array(self.reward_history, np.float32),
                    to_play=np.array(self.to_play_history, np.int32),
                    child_visits=np.array(self.child_visits, np.float32),
                    root_values=np.array(self.root_values, np.float32))


def frame_stack_obs(frames, index, n):
    """The frame-stacked observation at 1-based move `index` (games/atari_synth.py):
    frames index-n+1 .. index as the channels, zeros before move 1, bytes x f32(1/255)."""
    plane = np.asarray(frames[0]).size
    out = np.zeros(n * plane, np.float32)
    scale = np.float32(1.0) / np.float32(255.0)
    for c in range(n):
        s = index - n + 1 + c
        if s >= 1:
            out[c * plane:(c + 1) * plane] = np.asarray(frames[s - 1], np.uint8).astype(np.float32) * scale
    return out


def get_stacked_observations(obs_hist, action_hist, index, num_stacked, plane):
    """SelfPlay.jl:128-149 (Q15): [obs_t, (action plane, obs_{t-1}) ...], zeros before
    the first move; the action plane holds the raw action id.  `index` is 1-based."""
    parts = [np.asarray(obs_hist[index - 1], np.float32)]
    osz = parts[0].size
    for past in range(index - 1, index - num_stacked - 1, -1):
        if past >= 1:
            parts.append(np.full(plane, float(action_hist[past - 1]), np.float32))
            parts.append(np.asarray(obs_hist[past - 1], np.float32))
        else:
            parts.append(np.zeros(plane + osz, np.float32))
    return np.concatenate(parts)


# ---- the network-only player (csrc/mz_prior_rules.h): every operation in float32, in the
# header's order
def prior_policy(p, legal):
    """π of one row: the policy head's softmax p (A,) renormalised over the legal actions — s = the ascending
    float32 sum of the legal p (an illegal action adds +0), π = p / s on legal actions and 0 elsewhere; with
    s == 0 (every legal p underflowed) π = 1 / n_legal on legal actions."""
    p = np.asarray(p, np.float32)
    legal = np.asarray(legal).astype(bool)
    assert p.ndim == 1 and legal.shape == p.shape and legal.any(), "prior: one row with a legal action"
    s = np.float32(0.0)
    for a in range(p.size):
        s = np.float32(s + (p[a] if legal[a] else np.float32(0.0)))
    pi = np.zeros(p.size, np.float32)
    n = int(legal.sum())
    for a in np.flatnonzero(legal):
        pi[a] = np.float32(1.0) / np.float32(n) if s == 0 else np.float32(p[a] / s)
    return pi


def prior_pick(pi, legal, temperature, r, detmath=None):
    """The 0-based action the network-only player draws from π with the row's ACTION draw r (the rule of
    select_action): temperature 0 the first maximum over the legal actions, +inf the rng_below(r, n_legal)-th
    legal action, else weights w = π (temperature 1) or float32(det_exp(det_log(float64(π)) * float64(
    float32(1) / temperature))) where π > 0 (0 elsewhere; detmath supplies det_exp / det_log, the engine's
    deterministic float64 exp / log), S = their ascending float32 sum over the legal actions, u =
    float32(r >> 8) * 2^-24 * S, the first legal action whose running float32 sum exceeds u, else the last."""
    pi = np.asarray(pi, np.float32)
    acts = np.flatnonzero(np.asarray(legal).astype(bool))
    T = np.float32(temperature)
    assert len(acts) and T >= 0, "prior: a legal action and a temperature >= 0"
    if T == 0:
        best = acts[0]
        for a in acts[1:]:
            if pi[a] > pi[best]:
                best = a
        return int(best)
    if np.isinf(T):
        return int(acts[rng_below(r, len(acts))])
    if T == 1:
        w = pi
    else:
        assert detmath is not None, "prior: a temperature outside {0, 1, inf} needs detmath (det_exp, det_log)"
        inv = np.float64(np.float32(1.0) / T)
        w = np.zeros(pi.size, np.float32)
        for a in acts:
            if pi[a] > 0:
                w[a] = np.float32(detmath.det_exp(np.float64(detmath.det_log(np.float64(pi[a]))) * inv))
    S = np.float32(0.0)
    for a in acts:
        S = np.float32(S + w[a])
    u = np.float32(np.float32(np.float32(r >> 8) * np.float32(5.9604644775390625e-08)) * S)
    cum = np.float32(0.0)
    for a in acts:
        cum = np.float32(cum + w[a])
        if cum > u:
            return int(a)
    return int(acts[-1])


def prior_move(engine, obs, legal, temperature, seed, game_offset, step, detmath=None):
    """The network-only player's result of G rows on `engine`'s nets: (π (G, A), v (G,), 1-based actions (G,)),
    where a search has (child visits, root values, actions).  (v, p) = prediction(representation(obs)) from the
    engine's batched forward; row g draws with the ACTION stream's key (game_offset + g, step).  temperature:
    one value or one per row."""
    obs = np.ascontiguousarray(obs, np.float32)
    legal = np.asarray(legal).astype(bool)
    G = obs.shape[0]
    h = engine.forward(NET_REPR, obs)
    v, p = engine.forward(NET_PRED, h)
    temps = np.broadcast_to(np.asarray(temperature, np.float32), (G,))
    pi = np.zeros((G, legal.shape[1]), np.float32)
    act = np.zeros(G, np.int32)
    for g in range(G):
        pi[g] = prior_policy(p[g], legal[g])
        r = rng_u32(seed, MZ_RNG_ACTION, game_offset + g, step, 0)
        act[g] = prior_pick(pi[g], legal[g], temps[g], r, detmath) + 1
    return pi, np.asarray(v, np.float32).reshape(G).copy(), act


KINDS = ("search", "prior")


class BatchedSelfPlay:
    """G TicTacToe games played in lockstep on one engine (one GPU)."""

    def __init__(self, engine, env_cls, G, game_offset=0, step0=0, opponent="self", muzero_player=1,
                 expert_depth=None, opponent_engine=None, mcts_sims=None, mcts_rollouts=None,
                 muzero_kind="search", other_kind="search", detmath=None):
        """opponent "self" (self_play!, SelfPlay.jl:384-419) or "random": the
        player != muzero_player plays a uniform legal action
        (select_opponent_action, :311-325) — competitive_play! (:421-435);
        "expert": that player plays the rules search of games/expert.py to
        expert_depth plies (None: the env's default); "network": that player's
        moves are the same search on opponent_engine (another set of weights
        under the same config and rng_seed), and the history holds the mover's
        own search statistics; "mcts": that player plays the rules MCTS of
        games/mcts_rules.py with mcts_sims simulations of mcts_rollouts
        rollouts (None: the defaults).
        muzero_kind / other_kind (mz_eval_players): "search" or "prior" (the network-only player,
        prior_move) for the turns of muzero_player on `engine` and for the other turns where the other side is
        a network player ("self": the same engine, "network": opponent_engine); the rules opponents ignore
        other_kind.  detmath: prior_pick's, for temperatures outside {0, 1, inf}."""
        assert opponent in ("self", "random", "expert", "network", "mcts") and muzero_player in (1, 2)
        assert muzero_kind in KINDS and other_kind in KINDS, "eval players: a kind must be \"search\" or \"prior\""
        self.muzero_kind, self.other_kind, self.detmath = muzero_kind, other_kind, detmath
        assert (opponent == "network") == (opponent_engine is not None), "network: needs opponent_engine (only)"
        self.opponent = opponent
        self.opponent_engine = opponent_engine
        self.expert_depth = expert_depth
        self.mcts_sims, self.mcts_rollouts = mcts_sims or DEFAULT_SIMS, mcts_rollouts or DEFAULT_ROLLOUTS
        self.muzero_player = muzero_player
        self.eng = engine
        self.conf = engine.conf
        self.G = G
        # keyed envs (games/atari_synth.py) draw from the engine's Philox streams
        self.env = (env_cls(G, seed=engine.rng_seed, game_offset=game_offset) if getattr(env_cls, "KEYED", False)
                    else env_cls(G))
        self.frame_stack = getattr(env_cls, "FRAME_STACK", 0)
        assert not (opponent == "expert" and self.frame_stack), "expert: needs a two-player board env"
        assert not (opponent == "network" and self.frame_stack), "opponent network: needs a two-player board env"
        assert not (opponent == "mcts" and self.frame_stack), "mcts opponent: needs a two-player board env"
        self.game_offset = game_offset
        self.step = step0
        self.plane = self.conf.observation_shape[0] * self.conf.observation_shape[1]
        self.histories = [GameHistory() for _ in range(G)]
        self.finished: List[GameHistory] = []

    def _stacked(self):
        c = self.conf
        out = np.empty((self.G, stacked_features(c)), np.float32)
        for g, h in enumerate(self.histories):
            if self.frame_stack:                         # the env's own frame stack (atari_synth)
                out[g] = frame_stack_obs(h.observation_history, len(h.observation_history), self.frame_stack)
                continue
            out[g] = get_stacked_observations(h.observation_history, h.action_history,
                                              len(h.observation_history), c.stacked_observations, self.plane)
        return out

    def _search(self, eng, obs, legal, tp, temperature):
        """The move's batched search on `eng`: (child visits, root values, actions)."""
        c = self.conf
        cv, rv, act = eng.mcts_search(obs, legal, tp, exploration=True, rng_step=self.step,
                                      game_offset=self.game_offset, temperature=temperature)  # :359-360
        if c.temperature_threshold is not None:
            # :344-346: a game with >= temperature_threshold moves plays at temperature 0.
            # A game's search depends only on its own inputs and Philox keys (game id,
            # step), so the batch is searched again at 0 and those games take that action.
            moves = np.array([len(h.action_history) for h in self.histories])
            cold = moves >= c.temperature_threshold
            if cold.any() and temperature != 0.0:
                _, _, act0 = eng.mcts_search(obs, legal, tp, exploration=True, rng_step=self.step,
                                             game_offset=self.game_offset, temperature=0.0)
                act = np.where(cold, act0, act)
        return cv, rv, act

    def _player(self, kind, eng, obs, legal, tp, temperature):
        """One side's result of the move's rows on `eng`: the search, or the network-only player with the
        rows' own temperatures (a game with >= temperature_threshold moves picks at 0, as _search's does)."""
        if kind == "search":
            return self._search(eng, obs, legal, tp, temperature)
        temps = np.full(self.G, temperature, np.float32)
        if self.conf.temperature_threshold is not None:
            moves = np.array([len(h.action_history) for h in self.histories])
            temps[moves >= self.conf.temperature_threshold] = 0.0
        return prior_move(eng, obs, legal, temps, self.eng.rng_seed, self.game_offset, self.step, self.detmath)

    def play_move(self, temperature=1.0):
        """One move of every game (play_game's loop body, SelfPlay.jl:343-380)."""
        c = self.conf
        tp = self.env.player.copy()                                           # :351
        for g, h in enumerate(self.histories):
            h.observation_history.append(self.env.board[g].copy() if self.frame_stack else
                                         self.env.board[g].astype(np.float32))   # :352
        obs = self._stacked()                                                 # :355
        legal = self.env.legal_mask()
        cv, rv, act = self._player(self.muzero_kind, self.eng, obs, legal, tp, temperature)
        # the other side's own player where it differs in weights ("network") or in kind ("self"): its turns
        # take that whole result (mz_sp_pick)
        if self.opponent == "network" or (self.opponent == "self" and self.other_kind != self.muzero_kind):
            theirs = tp != self.muzero_player
            cv2, rv2, act2 = self._player(self.other_kind, self.opponent_engine or self.eng, obs, legal, tp,
                                          temperature)
            cv = np.where(theirs[:, None], cv2, cv)
            rv = np.where(theirs, rv2, rv)
            act = np.where(theirs, act2, act)
        if self.opponent == "random":                                         # :357-362, :321
            for g in np.flatnonzero(tp != self.muzero_player):
                acts = np.flatnonzero(legal[g])
                if len(acts):
                    r = rng_u32(self.eng.rng_seed, MZ_RNG_OPPONENT, self.game_offset + int(g), self.step, 0)
                    act[g] = acts[rng_below(r, len(acts))] + 1
        if self.opponent == "expert":                                         # the same turns, the same stream
            name = "tictactoe" if self.env.board.shape[1] == 27 else "connect4"
            depth = self.expert_depth or DEFAULT_DEPTH[name]
            for g in np.flatnonzero(tp != self.muzero_player):
                if legal[g].any():
                    r = rng_u32(self.eng.rng_seed, MZ_RNG_OPPONENT, self.game_offset + int(g), self.step, 0)
                    act[g] = expert_pick(expert_scores(name, self.env.board[g], int(tp[g]), depth), r)
        if self.opponent == "mcts":                                           # the same turns, its own ROLLOUT stream
            name = "tictactoe" if self.env.board.shape[1] == 27 else "connect4"
            for g in np.flatnonzero(tp != self.muzero_player):
                if legal[g].any():
                    gid = self.game_offset + int(g)
                    n, _ = mcts_root_stats(name, self.env.board[g], int(tp[g]), self.mcts_sims, self.mcts_rollouts,
                                           self.eng.rng_seed, gid, self.step)
                    act[g] = mcts_pick(n, rng_u32(self.eng.rng_seed, MZ_RNG_OPPONENT, gid, self.step, 0))
        reward, done = self.env.step(act)                                     # :366-368
        for g, h in enumerate(self.histories):                                # :375-379
            h.child_visits.append(cv[g])
            h.root_values.append(float(rv[g]))
            h.action_history.append(int(act[g]))
            h.reward_history.append(float(reward[g]))
            h.to_play_history.append(int(tp[g]))
        too_long = np.array([len(h.action_history) > c.max_moves for h in self.histories])
        ended = np.flatnonzero(done | too_long)
        for g in ended:
            self.finished.append(self.histories[g])
            self.histories[g] = GameHistory()
        if len(ended):
            if getattr(self.env, "KEYED", False):
                self.env.reset(ended, step=self.step)
            else:
                self.env.reset(ended)
        self.step += 1
        return ended

    def play_games(self, temperature=1.0):
        """Play every slot's current game to the end (no new games started);
        returns the histories in slot order."""
        results: List[Optional[GameHistory]] = [None] * self.G
        active = np.ones(self.G, bool)
        while active.any():
            n0 = len(self.finished)
            ended = self.play_move(temperature)
            for k, g in enumerate(ended):
                if active[g]:
                    results[g] = self.finished[n0 + k]
                    active[g] = False
        return results


def evaluation_record(histories, env_name, opponent, muzero_player, players, training_step=0, rng_step0=0):
    """The test worker's record of one evaluation (mz_test_play) from its games, one finished
    GameHistory per slot in slot order: the exact mirror of mz_test_tally, integers and float64 bits.
    Each game's three sums are float64, start at +0 and add float64(x) in record order; the record adds
    the games' sums in (move on which the game ended, ascending slot) order.  MuZero's moves are the
    records with to_play == muzero_player, every record when the opponent is "self" or players == 1."""
    every = opponent == "self" or players == 1
    rec = dict(training_step=int(training_step), games=0, muzero_wins=0, opponent_wins=0, draws=0, moves=0,
               value_moves=0, rng_step0=int(rng_step0) & 0xffffffff, reward_muzero=np.float64(0.0),
               reward_opponent=np.float64(0.0), value_sum=np.float64(0.0))
    for g in sorted(range(len(histories)), key=lambda g: (len(histories[g].action_history), g)):
        h = histories[g]
        mine, theirs, values, vm = np.float64(0.0), np.float64(0.0), np.float64(0.0), 0
        for rew, tp, rv in zip(h.reward_history, h.to_play_history, h.root_values):
            if every or tp == muzero_player:
                mine = mine + np.float64(np.float32(rew))
                values = values + np.float64(np.float32(rv))
                vm += 1
            else:
                theirs = theirs + np.float64(np.float32(rew))
        w = game_winner(env_name, h.reward_history[-1], h.to_play_history[-1])
        rec["games"] += 1
        rec["draws" if w == 0 else "muzero_wins" if w == muzero_player else "opponent_wins"] += 1
        rec["moves"] += len(h.action_history)
        rec["value_moves"] += vm
        rec["reward_muzero"] = rec["reward_muzero"] + mine
        rec["reward_opponent"] = rec["reward_opponent"] + theirs
        rec["value_sum"] = rec["value_sum"] + values
    return rec


def evaluation_audit(histories, env_name, opponent, muzero_player, depth=None):
    """The audit row of one evaluation (mz_test_audit) from its games: MuZero's moves (the
    records with to_play == muzero_player, every record when the opponent is "self"), each judged on the
    board it was made on by the expert's scores at `depth` (None: the env's default).  With c the
    move's score and b the best legal score a move adds (1, c == b, sgn(c) < sgn(b), b - c) to (moves
    judged, in the expert's best set, win or draw given away, score deficit).  Integers: exact."""
    depth = depth or DEFAULT_DEPTH[env_name]
    table = solved_table() if env_name == "tictactoe" and depth == 9 else None
    out = [0, 0, 0, 0]
    for h in histories:
        for board, tp, a in zip(h.observation_history, h.to_play_history, h.action_history):
            if opponent != "self" and tp != muzero_player:
                continue
            scores = table[ttt_code(board, tp)] if table is not None else expert_scores(env_name, board, tp, depth)
            for k, x in enumerate(judge_move(scores, a)):
                out[k] += x
    return tuple(out)


def env_name_of(env_cls):
    """game_winner's name of a batched env class: "tictactoe", "connect4" or "atari"."""
    if getattr(env_cls, "FRAME_STACK", 0):
        return "atari"
    return "tictactoe" if env_cls(1).board.shape[1] == 27 else "connect4"


def evaluate(engine, env_cls, E, opponent="self", muzero_player=1, rng_step0=0, game_offset=0, temperature=0.0,
             training_step=0, expert_depth=None, opponent_engine=None, audit=False, mcts_sims=None,
             mcts_rollouts=None, muzero_kind="search", other_kind="search", detmath=None):
    """One evaluation of the test worker on the host: E slots play one game each (move m keyed
    rng_step0 + m, game_offset); returns (the histories in slot order, their evaluation_record), and
    with audit=True their evaluation_audit at expert_depth as a third item.  muzero_kind / other_kind:
    BatchedSelfPlay's (mz_eval_players)."""
    sp = BatchedSelfPlay(engine, env_cls, E, game_offset=game_offset, step0=rng_step0, opponent=opponent,
                         muzero_player=muzero_player, expert_depth=expert_depth, opponent_engine=opponent_engine,
                         mcts_sims=mcts_sims, mcts_rollouts=mcts_rollouts, muzero_kind=muzero_kind,
                         other_kind=other_kind, detmath=detmath)
    histories = sp.play_games(temperature)
    players = engine.conf.players                      # Config.players lists the player ids
    name = env_name_of(env_cls)
    rec = evaluation_record(histories, name, opponent, muzero_player,
                            players if isinstance(players, int) else len(players), training_step, rng_step0)
    if audit:
        return histories, rec, evaluation_audit(histories, name, opponent, muzero_player, expert_depth)
    return histories, rec


def random_positions(env_cls, G, seed=0, max_plies=6):
    """Real positions for benchmarking (any env with [p1, p2, empty] board
    planes, stacked_observations = 1): random legal play from the initial
    board for 0..max_plies plies; returns stacked observations (G, F), legal
    masks (G, A) and to_play (G,).  Positions that ended are replaced by the
    initial board."""
    rng = np.random.default_rng(seed)
    env = env_cls(G)
    osz = env.board.shape[1]
    plane = osz // 3
    prev_obs = np.zeros((G, osz), np.float32)
    prev_act = np.zeros(G, np.int32)
    plies = rng.integers(0, max_plies + 1, G)
    alive = np.ones(G, bool)
    for t in range(max_plies):
        legal = env.legal_mask()
        go = (plies > t) & alive & legal.any(1)
        if not go.any():
            break
        # games not playing this ply take their first legal move and are restored below
        choice = np.array([rng.choice(np.flatnonzero(legal[g])) + 1 if go[g] else int(np.argmax(legal[g])) + 1
                           for g in range(G)], np.int32)
        before = env.board.astype(np.float32)
        saved = {k: v.copy() for k, v in vars(env).items() if isinstance(v, np.ndarray)}
        _, done = env.step(choice)
        for k, v in saved.items():                       # games not playing this ply keep their state
            getattr(env, k)[~go] = v[~go]
        prev_obs[go] = before[go]
        prev_act[go] = choice[go]
        ended = go & done
        if ended.any():
            env.reset(np.flatnonzero(ended))
            prev_obs[ended] = 0
            prev_act[ended] = 0
            alive &= ~ended
    cur = env.board.astype(np.float32)
    planes = np.repeat(prev_act[:, None].astype(np.float32), plane, axis=1)
    obs = np.concatenate([cur, planes, prev_obs], axis=1)
    return obs, env.legal_mask(), env.player.copy()
