"""What the network-only player costs, on the configs[1] engine
(TicTacToe FC, 50 sims) with G = E = 512, in one process.  Device events
around every call on the launch stream; each leg --warmup untimed calls, then
--moves timed ones, medians.

Legs:
  eval_random_search_search   mz_selfplay_move, MZ_SP_EVAL against MZ_OPP_RANDOM with the default kinds;
  eval_random_prior_prior     the same with (prior, prior): no search is launched;
  eval_self_search_prior      MZ_OPP_SELF with (search, prior): one search, one prior launch, mz_sp_pick;
  evaluation_search / _prior  one mz_test_play evaluation of E games, opponent self, both ways;
  prior_eval_dev              the bare mz_prior_eval_dev launch at G rows.
A library without mz_eval_players (the parent commit's) runs the legs it has,
so the two trees can be timed by the same file in one job.  Prints ONE JSON
line (and writes it to --out).  The two mz_forward_kernel launches that
mz_prior_fc fuses have no device entry point of their own: run
`rocprofv3 --kernel-trace --stats -- python tools/prior_bench.py --forward 50`
once more for their kernel times beside mz_prior_fc's.
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
from muzero_jl_amd.config import stacked_features  # noqa: E402
from muzero_jl_amd.games import tictactoe  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402

HAS_PRIOR = hasattr(abi.Engine, "eval_players")


def timed(stream, warmup, n, call):
    for i in range(warmup):
        call(i)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i, (a, b) in enumerate(evs):
        a.record(stream)
        call(warmup + i)
        b.record(stream)
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in evs])
    return {"ms_median": round(float(np.median(ms)), 4), "ms_mean": round(float(ms.mean()), 4),
            "ms_max": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--moves", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--forward", type=int, default=0, help="also N host-synchronous net_forward pairs (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    G = args.games
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    conf = dataclasses.replace(tictactoe.conf, num_iters=args.sims, replay_buffer_size=G)
    T = conf.max_moves + 1
    eng = abi.Engine(conf, tictactoe.hyper, device=0, max_games=G, rng_seed=7)
    for n, w in enumerate(init_nets(conf, tictactoe.hyper, seed=3)):
        eng.set_weights(n, w)
    res = {"tool": "prior_bench", "games": G, "num_iters": conf.num_iters, "T": T, "moves": args.moves,
           "warmup": args.warmup, "evals": args.evals, "has_prior": HAS_PRIOR, "legs": {}}
    legs = [("eval_random_search_search", abi.OPP_RANDOM, (0, 0))]
    if HAS_PRIOR:
        legs += [("eval_random_prior_prior", abi.OPP_RANDOM, (1, 1)), ("eval_self_search_prior", abi.OPP_SELF, (0, 1))]
    step = [0]

    def move(_):
        eng.selfplay_move(step[0], temperature=0.0, stream=sp)
        step[0] += 1

    def evaluation(i):
        eng.test_play(i, step[0], temperature=0.0, stream=sp)
        step[0] += T

    for tag, opp, kinds in legs:
        eng.selfplay_init(abi.ENV_TICTACTOE, G, G)
        if HAS_PRIOR:
            eng.eval_players(*kinds)
        eng.selfplay_mode(abi.SP_EVAL, opp, 1)
        res["legs"][tag] = {**timed(stream, args.warmup, args.moves, move), "games": eng.eval_results()[0]}
    for tag, kinds in (("evaluation_search", (0, 0)), ("evaluation_prior", (1, 1))):
        if kinds != (0, 0) and not HAS_PRIOR:
            continue
        eng.selfplay_init(abi.ENV_TICTACTOE, G, G)
        if HAS_PRIOR:
            eng.eval_players(*kinds)
        eng.test_config(G, abi.OPP_SELF, 1)
        res["legs"][tag] = {**timed(stream, 3, args.evals, evaluation), "games": eng.test_results(1)[1][0]["games"]}
    if HAS_PRIOR:
        eng.eval_players()
        rng = np.random.default_rng(0)
        F = stacked_features(conf)
        obs = torch.from_numpy((rng.random((G, F)) < 0.4).astype(np.float32)).to(dev)
        legal = torch.ones((G, 9), dtype=torch.uint8, device=dev)
        pol = torch.empty((G, 9), dtype=torch.float32, device=dev)
        val = torch.empty(G, dtype=torch.float32, device=dev)
        act = torch.empty(G, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def bare(i):
            rc = eng.lib.mz_prior_eval_dev(eng.h, G, obs.data_ptr(), legal.data_ptr(), 0, i, 0, 1.0, pol.data_ptr(),
                                           val.data_ptr(), act.data_ptr(), sp)
            assert rc == 0

        res["legs"]["prior_eval_dev"] = timed(stream, args.warmup, args.moves, bare)
        ss, pp = res["legs"]["eval_random_search_search"], res["legs"]["eval_random_prior_prior"]
        res["prior_over_search_move"] = round(pp["ms_median"] / ss["ms_median"], 4)
        res["evaluation_prior_over_search"] = round(res["legs"]["evaluation_prior"]["ms_median"] /
                                                    res["legs"]["evaluation_search"]["ms_median"], 4)
        host_obs = obs.cpu().numpy()
        for _ in range(args.forward):
            eng.forward(1, eng.forward(0, host_obs))
            eng.prior_eval(host_obs, np.ones((G, 9), bool))
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
