"""Learner driver — host mirror of learning! (src/Learning.jl:306-438).

Each step: get_batch from the (per-GPU) replay buffer, then one
ref_semantics learner step on the GPU (mz_learner_step: K-step unroll,
losses, gradient 2θ per quirk Q11, Flux ADAM with the Cos(λ0=1e-4,
λ1=1e-1, period=10) learning rate, Learning.jl:318-319,382).  Data-parallel
training splits the step: the gradient's data term -> RCCL
all-reduce (sum) of the flat bucket -> ADAM on data·(1/world) + 2θ, so every
replica applies the same update, equal to the single-GPU one in ref_semantics
at any world size.
"""
import numpy as np

from .config import cos_schedule
from .networks import NET_DYN, NET_PRED, NET_REPR


class Learner:
    def __init__(self, engine, buffer, process_group=None):
        self.eng = engine
        self.buffer = buffer
        self.conf = engine.conf
        self.training_step = 0
        self.losses = None
        self.pg = process_group

    def step(self):
        """One iteration of Learning.jl:327-413 (single GPU)."""
        _, batch = self.buffer.get_batch(self.training_step)
        eta = cos_schedule(self.training_step + 1)              # next!(schedule), :382
        l = self.eng.learner_step(batch, eta)
        self.training_step += 1
        # the three reported losses (:385-393) differ only in their L2 term
        data = float(l[0]) + float(l[1]) + float(l[2])
        self.losses = dict(representation=data + float(l[3]), prediction=data + float(l[4]),
                           dynamics=data + float(l[5]), value=float(l[0]), policy=float(l[2]))
        return self.losses

    def nets(self):
        return [self.eng.get_weights(n) for n in (NET_REPR, NET_PRED, NET_DYN)]


def allreduce_step(engine, dev_batch_ptrs, B, grad, losses, step, world, all_reduce, stream=None):
    """Data-parallel learner step on device buffers: the DATA TERM of the
    gradient into `grad` (a device tensor of engine.grad_count() floats; zero
    in ref_semantics, where only Σθ² depends on θ, Q11), `all_reduce(grad)`
    (sum over ranks; RCCL via torch.distributed on GPU, gloo in CPU tests),
    then ADAM on ∇ = Σ·(1/world) + 2θ.  The rank-invariant 2θ is added after
    the exchange (mz_adam_kernel), so every replica's update equals the
    single-GPU update bit for bit at EVERY world size in ref_semantics — an
    exchange of the full 2θ would not: a sequential f32 sum of eight equal
    terms differs from 8x for ~44 % of inputs (dp_gradient)."""
    engine.learner_grad_dev(dev_batch_ptrs, B, grad.data_ptr(), losses.data_ptr(), stream=stream)
    if world > 1:
        all_reduce(grad)
    engine.learner_apply_dev(grad.data_ptr(), 1.0 / world, cos_schedule(step + 1), stream=stream)


def dp_gradient(data_grad, theta, world, all_reduce):
    """Host reference of the data-parallel gradient mz_adam_kernel applies:
    ∇ = (Σ_ranks data_grad) · f32(1/world) + 2θ, in f32 with the device's
    operation order (the data term's product rounded, then the sum).
    data_grad is summed in place by all_reduce (world > 1)."""
    if world > 1:
        all_reduce(data_grad)
    d = np.asarray(data_grad, dtype=np.float32) * np.float32(1.0 / world)
    return (d + np.asarray(theta, dtype=np.float32) * np.float32(2)).astype(np.float32)


# ---- the run log (mz_train_set_log)
def run_log_record(step_losses, games, counters, t1, eta, refreshes, missed=0, env_name="tictactoe"):
    """One record of the run log from what went into it: the exact host mirror of mz_log_steps,
    mz_log_games and mz_log_commit, integers and float64 bits.  step_losses: (n, 6) float32, the six
    losses {value, reward, policy, l2_repr, l2_pred, l2_dyn} of the folded steps in ascending step;
    games: the folded GameHistory in game-number order; counters: the shard's {num_played_games,
    num_played_steps, positions held, games held, reanalysed count} at the commit.  The loss sums add
    float64(x) in ascending step; a game's three sums start at +0 and add float64(x) in record order
    (the sharpness term is the float32 maximum of the move's child_visits); the record adds the
    games' sums in the order given.  Sums and counts, never means."""
    from .abi import LOG_COUNT_FIELDS, LOG_SUM_FIELDS
    from .selfplay import game_winner
    rows = np.asarray(step_losses, np.float32).reshape(-1, 6)
    loss = [np.float64(0.0)] * 6
    for row in rows:
        loss = [s + np.float64(x) for s, x in zip(loss, row)]
    last = [np.float64(x) for x in rows[-1]] if len(rows) else [np.float64(0.0)] * 6
    wins = [0, 0, 0]
    moves = 0
    gsum = [np.float64(0.0)] * 3
    for h in games:
        a = [np.float64(0.0)] * 3
        for rew, rv, cv in zip(h.reward_history, h.root_values, h.child_visits):
            a[0] = a[0] + np.float64(np.float32(rew))
            a[1] = a[1] + np.float64(np.float32(rv))
            a[2] = a[2] + np.float64(np.max(np.asarray(cv, np.float32)))
        w = game_winner(env_name, h.reward_history[-1], h.to_play_history[-1])
        wins[0 if w == 1 else 1 if w == 2 else 2] += 1
        moves += len(h.action_history)
        gsum = [s + x for s, x in zip(gsum, a)]
    counts = [int(t1), len(rows)] + [int(c) for c in counters] + [len(games), moves] + wins + \
             [int(refreshes), int(missed), 0, 0]
    assert len(counts) == 16, "counters: five shard words"
    rec = dict(zip(LOG_COUNT_FIELDS, counts))
    rec.update(zip(LOG_SUM_FIELDS, loss + last + [np.float64(eta)] + gsum))
    return rec


def run_log_derived(rec):
    """What a reader wants from one record: the means the device never takes.  A quotient with a zero
    count is None."""
    def div(x, n):
        return float(x) / n if n else None
    steps, games, moves = rec["steps"], rec["games"], rec["moves"]
    out = dict(training_step=rec["training_step"], steps=steps, games=games, eta=float(rec["eta"]),
               num_played_games=rec["num_played_games"], games_held=rec["games_held"],
               positions_held=rec["positions_held"], reanalysed=rec["reanalysed"], refreshes=rec["refreshes"],
               missed=rec["missed"])
    for k in ("value", "reward", "policy", "l2_repr", "l2_pred", "l2_dyn"):
        out["mean_" + k + "_loss"] = div(rec[k], steps)
        out["last_" + k + "_loss"] = float(rec["last_" + k])
    out["win_p1_fraction"] = div(rec["wins_p1"], games)
    out["win_p2_fraction"] = div(rec["wins_p2"], games)
    out["draw_fraction"] = div(rec["draws"], games)
    out["mean_game_length"] = div(moves, games)
    out["mean_game_reward"] = div(rec["reward_sum"], games)
    out["mean_root_value"] = div(rec["root_value_sum"], moves)
    out["mean_sharpness"] = div(rec["sharpness_sum"], moves)
    return out


def run_log_jsonl(path, records):
    """Append one JSON object per record (Engine.train_log_results' dicts, or run_log_record's) to
    `path`: the derived values of run_log_derived.  Plain json, one line each."""
    import json
    with open(path, "a") as f:
        for rec in records:
            f.write(json.dumps(run_log_derived(rec)) + "\n")
