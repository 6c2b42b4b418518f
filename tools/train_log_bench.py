"""What the run log costs, on the configs[1] engine (TicTacToe FC,
G = 512, 50 sims): mz_train_run ms per move with the log off and with
mz_train_set_log(checkpoint_interval), in one process.

Two engines of the same weights run the same job; --rounds times each runs
--moves moves, the engine with the log and the one without taking turns, host
wall clock around each call (mz_train_run hands back to the host every move).
The prediction: one launch of mz_log_games per move, one of mz_log_steps (and
one small device copy when losses_dev is given) per learner chunk, one of
mz_log_commit per record, nothing read back.

--baseline-lib PATH: the same log-off leg on another build of the library (the
parent commit's, tools/build_rev_lib.sh <rev> <name>), in a child process of
its own started before this one touches the device (one library per process,
MZ_LIB).  Prints ONE JSON line (and writes it to --out).
"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def legs(args, tags):
    """ms per move of mz_train_run for each tag ("off", "on"), the engines taking turns."""
    import torch  # (one HIP runtime)
    import _mzpkg
    _mzpkg.load()
    from muzero_jl_amd import abi
    from muzero_jl_amd.games import tictactoe
    from muzero_jl_amd.networks import init_nets
    G = args.games
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    conf = dataclasses.replace(tictactoe.conf, num_iters=args.sims, replay_buffer_size=4 * G,
                               training_steps=10 ** 7)        # the loop's learner never runs out of steps
    interval = args.interval or conf.checkpoint_interval
    run = {}
    for tag in tags:
        e = abi.Engine(conf, tictactoe.hyper, device=0, max_games=G, rng_seed=7)
        for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=3)):
            e.set_weights(n, w)
        e.selfplay_init(abi.ENV_TICTACTOE, G, 4 * G)
        e.train_init(conf.batch_size)
        if tag == "on":
            e.train_set_log(interval)
        e.train_run(5, move0=0, stream=sp)                    # allocations and the first launches
        torch.cuda.synchronize()
        run[tag] = {"eng": e, "s": [], "state": None}
    mv = 5
    for _ in range(args.rounds):
        for tag in tags:
            e = run[tag]["eng"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = e.train_run(args.moves, move0=mv, stream=sp)
            torch.cuda.synchronize()
            run[tag]["s"].append(time.perf_counter() - t0)
            run[tag]["state"] = st
        mv += args.moves
    n_moves = args.moves * args.rounds
    out = {"games": G, "num_iters": conf.num_iters, "batch_size": conf.batch_size, "interval": interval,
           "moves_per_round": args.moves, "rounds": args.rounds}
    for tag in tags:
        s = run[tag]["s"]
        out[tag] = {"ms_per_move": round(sum(s) / n_moves * 1e3, 4),
                    "round_ms_per_move": [round(x / args.moves * 1e3, 4) for x in s],
                    "state": list(run[tag]["state"])}
    if "on" in tags:
        total, recs = run["on"]["eng"].train_log_results(1)
        out["records"] = total
        out["last_record"] = {k: (int(v) if isinstance(v, int) else float(v)) for k, v in recs[0].items()} if recs else None
        out["same_state"] = run["on"]["state"] == run["off"]["state"]
        out["extra_ms_per_move"] = round(out["on"]["ms_per_move"] - out["off"]["ms_per_move"], 4)
    for tag in tags:
        run[tag]["eng"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--moves", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--interval", type=int, default=0, help="learner steps between two records (0: checkpoint_interval)")
    ap.add_argument("--baseline-lib", default="", help="another build of libmz.so for a log-off leg of its own")
    ap.add_argument("--off-only", action="store_true", help="(the baseline child) the log-off leg alone")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.off_only:
        print(json.dumps(legs(args, ("off",))))
        return
    res = {"tool": "train_log_bench"}
    if args.baseline_lib:                                     # before this process opens the device
        cmd = [sys.executable, os.path.abspath(__file__), "--off-only", "--games", str(args.games), "--sims",
               str(args.sims), "--moves", str(args.moves), "--rounds", str(args.rounds)]
        env = dict(os.environ, MZ_LIB=os.path.abspath(args.baseline_lib))
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"the baseline leg failed ({p.returncode}):\n{p.stderr[-2000:]}")
        res["baseline"] = dict(json.loads(p.stdout.strip().splitlines()[-1]), lib=os.path.basename(args.baseline_lib))
    res.update(legs(args, ("off", "on")))
    if "baseline" in res:
        res["off_minus_baseline_ms_per_move"] = round(res["off"]["ms_per_move"] - res["baseline"]["off"]["ms_per_move"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
