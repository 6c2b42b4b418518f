"""What the expert opponent costs per evaluation move: ms per
mz_selfplay_move in MZ_SP_EVAL at G = 512 on the FC engines, MZ_OPP_RANDOM
against MZ_OPP_EXPERT in one process; the difference is the mz_expert_move
launch.  Device events around every move on the launch stream.

Legs (each: --warmup moves untimed, then --moves timed ones, mean and median):
  tictactoe  steady state (muzero_player 1): random, expert D = 9;
             first move from all-empty boards with the opponent to move
             (muzero_player 2, a fresh mz_selfplay_init before every timed
             move): random, expert D = 9 — the expert's worst case, 72 live
             two-ply prefixes with 7-ply subtrees on every row;
  connect4   steady state: random, expert D = 4, expert D = 8.
Prints ONE JSON line (and writes it to --out): per leg ms_mean / ms_median,
and for each expert leg the extra time over the same env's random leg as a
fraction of that random move.  Run it once more under
`rocprofv3 --kernel-trace --stats -- python tools/expert_bench.py --moves 50`
for mz_expert_move's own kernel time.

--table adds, in the same job: the build of the solved TicTacToe
table (mz_expert_table(1) on fresh handles: the first call, then the median of
5 more; host wall clock around the host-synchronous call, the device idle
before it) and the two TicTacToe expert legs again with the table on
(expert_d9_steady_table, expert_d9_first_move_table), each with its ratio to
the same job's table-off leg.  Without the flag the output is what it was.
"""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime)
import _mzpkg  # noqa: E402

_mzpkg.load()
from muzero_jl_amd import abi  # noqa: E402
from muzero_jl_amd.games import connect4, tictactoe  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402


def leg(eng, env_kind, G, stream, opponent, depth, mzp, warmup, moves, fresh, table=False):
    sp = stream.cuda_stream

    def init():
        eng.selfplay_init(env_kind, G, G)
        eng.selfplay_mode(abi.SP_EVAL, opponent, mzp)

    init()
    eng.expert_depth(depth)
    if env_kind == abi.ENV_TICTACTOE:
        eng.expert_table(table)                       # off: the flag only, the launches are the search kernel's
    step = 0
    for _ in range(warmup):
        if fresh:
            init()
        eng.selfplay_move(step, temperature=0.0, stream=sp)
        step += 1
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(moves)]
    for a, b in evs:
        if fresh:
            torch.cuda.synchronize()
            init()
        a.record(stream)
        eng.selfplay_move(step, temperature=0.0, stream=sp)
        b.record(stream)
        step += 1
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    return {"ms_mean": round(float(ms.mean()), 4), "ms_median": round(float(np.median(ms)), 4),
            "ms_max": round(float(ms.max()), 4), "games": eng.eval_results()[0]}


def table_build(conf, hyper, G, fresh=6):
    """mz_expert_table(1) on fresh handles: ms of the first call and the median of the others."""
    import time
    ms = []
    for _ in range(fresh):
        eng = abi.Engine(conf, hyper, device=0, max_games=G, rng_seed=7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.expert_table(True)
        ms.append((time.perf_counter() - t0) * 1e3)
        eng.close()
    return {"first_ms": round(ms[0], 3), "median_ms": round(float(np.median(ms[1:])), 3),
            "all_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--table", action="store_true", help="also: the solved table's build time and the table-on legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G = args.games
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    res = {"tool": "expert_bench", "games": G, "moves": args.moves, "warmup": args.warmup, "legs": {}}
    plan = [("tictactoe", tictactoe, abi.ENV_TICTACTOE,
             [("random_steady", abi.OPP_RANDOM, 0, 1, False), ("expert_d9_steady", abi.OPP_EXPERT, 9, 1, False),
              ("random_first_move", abi.OPP_RANDOM, 0, 2, True), ("expert_d9_first_move", abi.OPP_EXPERT, 9, 2, True)]),
            ("connect4", connect4, abi.ENV_CONNECT4,
             [("random_steady", abi.OPP_RANDOM, 0, 1, False), ("expert_d4_steady", abi.OPP_EXPERT, 4, 1, False),
              ("expert_d8_steady", abi.OPP_EXPERT, 8, 1, False)])]
    for name, mod, env_kind, legs in plan:
        conf = dataclasses.replace(mod.conf, replay_buffer_size=G)
        eng = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=7)
        for n, w in enumerate(init_nets(conf, mod.hyper, seed=3)):
            eng.set_weights(n, w)
        out = {}
        for tag, opp, depth, mzp, fresh in legs:
            out[tag] = leg(eng, env_kind, G, stream, opp, depth, mzp, args.warmup, args.moves, fresh)
        if args.table and name == "tictactoe":
            for tag, opp, depth, mzp, fresh in legs:
                if opp == abi.OPP_EXPERT:
                    r = leg(eng, env_kind, G, stream, opp, depth, mzp, args.warmup, args.moves, fresh, table=True)
                    r["over_table_off"] = round(r["ms_median"] / out[tag]["ms_median"], 4)
                    out[tag + "_table"] = r
            out["table_build"] = table_build(conf, mod.hyper, G)
        for tag, r in out.items():
            if tag.startswith("expert"):
                base = out["random_first_move" if "first_move" in tag else "random_steady"]["ms_median"]
                r["extra_ms"] = round(r["ms_median"] - base, 4)
                r["extra_over_random_move"] = round((r["ms_median"] - base) / base, 4)
        res["legs"][name] = {"num_iters": conf.num_iters, **out}
        eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
