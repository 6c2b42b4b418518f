"""What the solved table and judging do to one evaluation of the test worker
(DESIGN §18.1, §20.1), on the configs[1] engine (TicTacToe FC, G = 512, 50
sims) with E = 512 test slots, in one process.  The companion of
tools/test_worker_bench.py (what the worker itself costs), whose engine and
evaluation loop this follows.

Legs, taking turns --rounds times in one engine (each: --eval-warmup untimed,
then --evals timed mz_test_play at temperature 0, device events around every
call on the launch stream):
  expert_table_off / expert_table_on   against the expert, which moves first
                                       (muzero_player 2: its worst case), by
                                       the search kernel and by the lookup;
  self_judging_off                     against self, as today;
  self_judging_on_search / _on_table   the same with mz_test_audit on, judged
                                       by the search kernel and by the lookup.
Prints ONE JSON line (and writes it to --out): per leg ms_median / ms_mean /
ms_max, the table-on over table-off ratio, each judging leg's extra ms per
evaluation and per move over self_judging_off, and its audit row.
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

# leg -> (opponent, solved table on, judging on)
LEGS = {"expert_table_off": (abi.OPP_EXPERT, False, False), "expert_table_on": (abi.OPP_EXPERT, True, False),
        "self_judging_off": (abi.OPP_SELF, False, False), "self_judging_on_search": (abi.OPP_SELF, False, True),
        "self_judging_on_table": (abi.OPP_SELF, True, True)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--test-games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--eval-warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G, E = args.games, args.test_games
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    conf = dataclasses.replace(tictactoe.conf, num_iters=args.sims, replay_buffer_size=4 * G)
    T = conf.max_moves + 1
    eng = abi.Engine(conf, tictactoe.hyper, device=0, max_games=max(G, E), rng_seed=7)
    for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=3)):
        eng.set_weights(n, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, G, 4 * G)
    ms = {k: [] for k in LEGS}
    rows = {}
    for _ in range(args.rounds):
        for tag, (opp, table, judge) in LEGS.items():
            eng.test_config(E, opp, 2 if opp == abi.OPP_EXPERT else 1)
            eng.expert_table(table)
            eng.test_audit(judge)
            for i in range(args.eval_warmup):
                eng.test_play(0, i * T, temperature=0.0, stream=sp)
            ms[tag] += timed(stream, args.evals, lambda i: eng.test_play(i, 1000 + i * T, temperature=0.0, stream=sp))
            if judge:
                rows[tag] = eng.test_audit_results(1)[1][0].tolist()
    legs = {tag: stats(v) for tag, v in ms.items()}
    for tag, row in rows.items():
        legs[tag]["audit_row"] = row
    legs["expert_table_on_over_off"] = round(legs["expert_table_on"]["ms_median"] /
                                             legs["expert_table_off"]["ms_median"], 4)
    for tag in ("self_judging_on_search", "self_judging_on_table"):
        legs[tag]["extra_ms"] = round(legs[tag]["ms_median"] - legs["self_judging_off"]["ms_median"], 4)
        legs[tag]["extra_ms_per_move"] = round(legs[tag]["extra_ms"] / T, 4)
    eng.close()
    res = {"tool": "audit_bench", "games": G, "test_games": E, "num_iters": conf.num_iters, "T": T,
           "evals": args.evals, "eval_warmup": args.eval_warmup, "rounds": args.rounds, "legs": legs}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
