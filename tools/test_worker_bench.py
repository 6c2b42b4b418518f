"""What the test worker costs, on the configs[1] engine (TicTacToe
FC, G = 512, 50 sims) with E = 512 test slots, in one process.

1. One evaluation against T self-play moves.  --rounds times: a leg of
   mz_selfplay_move (MZ_SP_TRAIN; --warmup untimed, then --moves timed moves),
   then a leg of mz_test_play (--eval-warmup untimed, then --evals timed
   evaluations, opponent self, temperature 0), device events around every call
   on the launch stream.  The prediction: an evaluation is T = max_moves + 1
   search launches plus T small launches (mz_test_tally in place of mz_sp_order
   / mz_sp_store), the frozen rows still searched, so ms per evaluation is
   about T x the self-play move.
2. mz_train_run with the worker off and on.  Two engines of the same weights run
   the same job; --train-rounds times each runs --train-moves moves, the engine
   with mz_train_set_test(--interval) and the one without taking turns, host
   wall clock around each call (mz_train_run hands back to the host every
   move).  extra_ms_per_evaluation = the on - off difference spread over the
   evaluations that ran.

Prints ONE JSON line (and writes it to --out).
"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime)
import _mzpkg  # noqa: E402

_mzpkg.load()
from muzero_jl_amd import abi  # noqa: E402
from muzero_jl_amd.games import tictactoe  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402


def timed(stream, n, call):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i, (a, b) in enumerate(evs):
        a.record(stream)
        call(i)
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def stats(ms):
    ms = np.asarray(ms)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_mean": round(float(ms.mean()), 4),
            "ms_max": round(float(ms.max()), 4)}


def engine(conf, G):
    eng = abi.Engine(conf, tictactoe.hyper, device=0, max_games=G, rng_seed=7)
    for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=3)):
        eng.set_weights(n, w)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--test-games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--moves", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--eval-warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-moves", type=int, default=300)
    ap.add_argument("--train-rounds", type=int, default=3)
    ap.add_argument("--interval", type=int, default=1000, help="learner steps between two evaluations")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G, E = args.games, args.test_games
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    conf = dataclasses.replace(tictactoe.conf, num_iters=args.sims, replay_buffer_size=4 * G,
                               training_steps=10 ** 7)        # the loop's learner never runs out of steps
    T = conf.max_moves + 1

    # ---- 1. an evaluation against T self-play moves
    eng = engine(conf, max(G, E))
    eng.selfplay_init(abi.ENV_TICTACTOE, G, 4 * G)
    eng.test_config(E, abi.OPP_SELF, 1)
    ms = {"move": [], "evaluation": []}
    rounds = {"move": [], "evaluation": []}
    step = 0
    for _ in range(args.rounds):
        for i in range(args.warmup):
            eng.selfplay_move(step + i, temperature=1.0, stream=sp)
        step += args.warmup
        t = timed(stream, args.moves, lambda i: eng.selfplay_move(step + i, temperature=1.0, stream=sp))
        step += args.moves
        ms["move"] += t
        rounds["move"].append(round(float(np.median(t)), 4))
        for i in range(args.eval_warmup):
            eng.test_play(0, step + i * T, temperature=0.0, stream=sp)
        step += args.eval_warmup * T
        t = timed(stream, args.evals, lambda i: eng.test_play(i, step + i * T, temperature=0.0, stream=sp))
        step += args.evals * T
        ms["evaluation"] += t
        rounds["evaluation"].append(round(float(np.median(t)), 4))
    total, recs = eng.test_results(1)
    res = {"tool": "test_worker_bench", "games": G, "test_games": E, "num_iters": conf.num_iters, "T": T,
           "moves": args.moves, "evals": args.evals, "rounds": args.rounds, "search_variant": eng.search_variant(),
           "evaluations_run": total, "last_record_games": recs[0]["games"], "last_record_moves": recs[0]["moves"],
           "selfplay_move": {**stats(ms["move"]), "round_medians": rounds["move"]},
           "evaluation": {**stats(ms["evaluation"]), "round_medians": rounds["evaluation"]}}
    res["T_moves_ms"] = round(T * res["selfplay_move"]["ms_median"], 4)
    res["evaluation_over_T_moves"] = round(res["evaluation"]["ms_median"] / res["T_moves_ms"], 4)
    res["ms_per_evaluation_move"] = round(res["evaluation"]["ms_median"] / T, 4)
    eng.close()

    # ---- 2. mz_train_run with the worker off and on
    B = conf.batch_size
    run = {}
    for tag in ("off", "on"):
        e = engine(conf, max(G, E))
        e.selfplay_init(abi.ENV_TICTACTOE, G, 4 * G)
        e.train_init(B)
        if tag == "on":
            e.test_config(E, abi.OPP_SELF, 1)
            e.train_set_test(args.interval, game_offset=1 << 20, temperature=0.0)
        e.train_run(5, move0=0, stream=sp)                    # allocations and the first launches
        torch.cuda.synchronize()
        run[tag] = {"eng": e, "s": [], "state": None, "evals0": e.test_results(0)[0]}
    mv = 5
    for _ in range(args.train_rounds):
        for tag in ("off", "on"):
            e = run[tag]["eng"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = e.train_run(args.train_moves, move0=mv, stream=sp)
            torch.cuda.synchronize()
            run[tag]["s"].append(time.perf_counter() - t0)
            run[tag]["state"] = st
        mv += args.train_moves
    n_moves = args.train_moves * args.train_rounds
    evals = run["on"]["eng"].test_results(0)[0] - run["on"]["evals0"]
    tr = {"moves_per_round": args.train_moves, "rounds": args.train_rounds, "interval": args.interval, "batch_size": B,
          "same_state": run["on"]["state"] == run["off"]["state"], "learner_step": run["on"]["state"][0],
          "games_played": run["on"]["state"][1], "evaluations": evals}
    for tag in ("off", "on"):
        s = run[tag]["s"]
        tr[tag] = {"ms_per_move": round(sum(s) / n_moves * 1e3, 4),
                   "round_ms_per_move": [round(x / args.train_moves * 1e3, 4) for x in s]}
        run[tag]["eng"].close()
    tr["extra_ms_per_move"] = round(tr["on"]["ms_per_move"] - tr["off"]["ms_per_move"], 4)
    tr["extra_ms_per_evaluation"] = round(tr["extra_ms_per_move"] * n_moves / evals, 4) if evals else None
    res["train_run"] = tr
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
