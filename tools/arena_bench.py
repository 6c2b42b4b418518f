"""What net against net costs per evaluation move: ms per
mz_selfplay_move in MZ_SP_EVAL on the configs[1] engine (TicTacToe FC,
G = 512, 50 sims) with MZ_OPP_SELF and with MZ_OPP_NETWORK, alternating in
one process on one engine whose opponent set holds other weights.  Device
events around every move on the launch stream.  The prediction: the
difference is one more search launch plus mz_sp_pick.

--rounds times: a leg of MZ_OPP_SELF, then a leg of MZ_OPP_NETWORK (each:
--warmup moves untimed, then --moves timed ones; the games in progress carry
over, mz_selfplay_mode only switches the opponent).  Prints ONE JSON line (and
writes it to --out): per mode the median / mean / max over all timed moves and
the per-round medians, extra_ms = network - self (medians), and, with
--parent-bench FILE (the JSON line of a plain `bench.py` run of the parent
commit's library in the same job; its ms_per_step is one search launch of this
workload), gap_ms = extra_ms - that launch.
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
from muzero_jl_amd.games import tictactoe  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402


def leg(eng, stream, opponent, step, warmup, moves):
    sp = stream.cuda_stream
    eng.selfplay_mode(abi.SP_EVAL, opponent, 1)
    for _ in range(warmup):
        eng.selfplay_move(step, temperature=0.0, stream=sp)
        step += 1
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(moves)]
    for a, b in evs:
        a.record(stream)
        eng.selfplay_move(step, temperature=0.0, stream=sp)
        b.record(stream)
        step += 1
    torch.cuda.synchronize()
    return step, [a.elapsed_time(b) for a, b in evs]


def stats(ms):
    ms = np.asarray(ms)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_mean": round(float(ms.mean()), 4),
            "ms_max": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--moves", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-bench", default="", help="file with the JSON line of the parent's plain bench.py run")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G = args.games
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    conf = dataclasses.replace(tictactoe.conf, num_iters=args.sims, replay_buffer_size=G)
    eng = abi.Engine(conf, tictactoe.hyper, device=0, max_games=G, rng_seed=7)
    for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=3)):
        eng.set_weights(n, w)
    for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=4)):
        eng.opponent_set_weights(n, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, G, G)
    ms = {"self": [], "network": []}
    rounds = {"self": [], "network": []}
    step = 0
    for _ in range(args.rounds):
        for tag, opp in (("self", abi.OPP_SELF), ("network", abi.OPP_NETWORK)):
            step, t = leg(eng, stream, opp, step, args.warmup, args.moves)
            ms[tag] += t
            rounds[tag].append(round(float(np.median(t)), 4))
    res = {"tool": "arena_bench", "games": G, "num_iters": conf.num_iters, "moves": args.moves, "warmup": args.warmup,
           "rounds": args.rounds, "search_variant": eng.search_variant(), "games_finished": eng.eval_results()[0],
           "self": {**stats(ms["self"]), "round_medians": rounds["self"]},
           "network": {**stats(ms["network"]), "round_medians": rounds["network"]}}
    res["extra_ms"] = round(res["network"]["ms_median"] - res["self"]["ms_median"], 4)
    if args.parent_bench:
        with open(args.parent_bench) as f:
            parent = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
        res["parent_search_ms_per_launch"] = parent["ms_per_step"]
        res["gap_ms"] = round(res["extra_ms"] - parent["ms_per_step"], 4)
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
