"""What the rules-MCTS opponent costs per evaluation move: ms per
mz_selfplay_move in MZ_SP_EVAL at G = 512 on the FC engines, MZ_OPP_RANDOM
against MZ_OPP_MCTS in one process; the difference is the mz_mcts_move launch.
Device events around every move on the launch stream.

Legs (each: --warmup moves untimed, then --moves timed ones, mean and median),
steady state with muzero_player 1, for TicTacToe and Connect4:
  random          the random opponent;
  mcts_default    (S, R) = the defaults (64, 16);
  mcts_256x64     (S, R) = (256, 64).
Prints ONE JSON line (and writes it to --out): per leg ms_mean / ms_median /
ms_max, and for each MCTS leg the extra time over the same env's random leg,
in ms, as a fraction of that random move and per simulation.  About half the
rows of a steady-state move are the opponent's turns.  Run it once more under
`rocprofv3 --kernel-trace --stats -- python tools/mcts_opponent_bench.py --moves 50`
for mz_mcts_move's own kernel time.
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


def leg(eng, env_kind, G, stream, opponent, sims, rollouts, warmup, moves):
    sp = stream.cuda_stream
    eng.selfplay_init(env_kind, G, G)
    eng.mcts_opponent(sims, rollouts)
    eng.selfplay_mode(abi.SP_EVAL, opponent, 1)
    step = 0
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
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    return {"ms_mean": round(float(ms.mean()), 4), "ms_median": round(float(np.median(ms)), 4),
            "ms_max": round(float(ms.max()), 4), "games": eng.eval_results()[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G = args.games
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    res = {"tool": "mcts_opponent_bench", "games": G, "moves": args.moves, "warmup": args.warmup, "legs": {}}
    legs = [("random", abi.OPP_RANDOM, 0, 0), ("mcts_default", abi.OPP_MCTS, 0, 0),
            ("mcts_256x64", abi.OPP_MCTS, 256, 64)]
    for name, mod, env_kind in (("tictactoe", tictactoe, abi.ENV_TICTACTOE), ("connect4", connect4, abi.ENV_CONNECT4)):
        conf = dataclasses.replace(mod.conf, replay_buffer_size=G)
        eng = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=7)
        for n, w in enumerate(init_nets(conf, mod.hyper, seed=3)):
            eng.set_weights(n, w)
        out = {}
        for tag, opp, sims, rollouts in legs:
            out[tag] = leg(eng, env_kind, G, stream, opp, sims, rollouts, args.warmup, args.moves)
            if opp == abi.OPP_MCTS:
                r, base = out[tag], out["random"]["ms_median"]
                r["sims"], r["rollouts"] = sims or 64, rollouts or 16
                r["extra_ms"] = round(r["ms_median"] - base, 4)
                r["extra_over_random_move"] = round((r["ms_median"] - base) / base, 4)
                r["extra_us_per_sim"] = round((r["ms_median"] - base) * 1e3 / r["sims"], 3)
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
