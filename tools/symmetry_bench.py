"""What the board-symmetry augmentation costs: on the configs[1] (TicTacToe) and configs[3]
(Connect4) FC engines, the same calls with mz_replay_set_symmetry off and on in one process, alternating,
device events around every call on the launch stream:

  sample       mz_replay_sample(B) — the mz_rp_sample launch;
  train_ref    mz_learner_train_dev in ref_semantics (the one-launch learner with its prefetch), steps/s;
  train_corr   mz_learner_train_dev in MZ_LEARN_CORRECTED (sample, backprop, ADAM), steps/s;
  batch_sym    mz_batch_symmetry at B = 32 and B = 2048 (ids drawn uniformly), no off leg.

Each leg: --warmup calls untimed, then --calls timed, --rounds rounds of (off, on); medians per round.
Prints ONE JSON line and writes it to --out.  There is no threshold: the expectation is a few table bytes out
of cache per row.
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
from muzero_jl_amd.config import cos_schedule  # noqa: E402
from muzero_jl_amd.games import connect4, tictactoe  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402


def timed(stream, fn, warmup, calls):
    for i in range(warmup):
        fn(i)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i, (a, b) in enumerate(evs):
        a.record(stream)
        fn(warmup + i)
        b.record(stream)
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in evs]))


def engine(mod, env_kind, G, moves, corrected):
    conf = dataclasses.replace(mod.conf, num_iters=6, replay_buffer_size=4 * G)
    eng = abi.Engine(conf, mod.hyper, device=0, max_games=G, rng_seed=7)
    for n, w in enumerate(init_nets(conf, mod.hyper, seed=3)):
        eng.set_weights(n, w)
    if corrected:
        eng.learner_set_mode(abi.LEARN_CORRECTED)
    eng.selfplay_init(env_kind, G, 4 * G)
    for m in range(moves):
        eng.selfplay_move(100 + m, game_offset=7)
    eng.sync()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    B = args.batch
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    torch.cuda.set_stream(stream)
    sp = stream.cuda_stream
    res = {"tool": "symmetry_bench", "batch": B, "calls": args.calls, "warmup": args.warmup, "rounds": args.rounds,
           "legs": {}}
    for name, mod, env_kind, moves in (("tictactoe", tictactoe, abi.ENV_TICTACTOE, 20),
                                       ("connect4", connect4, abi.ENV_CONNECT4, 60)):
        out = {}
        ref, corr = engine(mod, env_kind, 64, moves, False), engine(mod, env_kind, 64, moves, True)
        losses = torch.empty(8, dtype=torch.float32, device="cuda")
        step = [1]

        def train(eng):
            def f(i):
                eng.learner_train_dev(B, step[0], cos_schedule(step[0]), losses.data_ptr(), stream=sp)
                step[0] += 1
            return f
        legs = {"sample": (ref, lambda i: ref.replay_sample(B, 1 + i, stream=sp)),
                "train_ref": (ref, train(ref)), "train_corr": (corr, train(corr))}
        for tag, (eng, fn) in legs.items():
            rounds = {"off": [], "on": []}
            for _ in range(args.rounds):
                for on in (False, True):
                    eng.replay_set_symmetry(on)
                    rounds["on" if on else "off"].append(round(timed(stream, fn, args.warmup, args.calls), 5))
            off, on = float(np.median(rounds["off"])), float(np.median(rounds["on"]))
            out[tag] = {"ms_off": rounds["off"], "ms_on": rounds["on"], "on_over_off": round(on / off, 4)}
            if tag != "sample":
                out[tag]["steps_per_s_off"] = round(1e3 / off, 1)
                out[tag]["steps_per_s_on"] = round(1e3 / on, 1)
        ref.replay_set_symmetry(False)
        n = ref.replay_symmetry_get()[0].n
        K1, A = mod.conf.num_unroll_steps + 1, len(mod.conf.action_space)
        for Bs in (32, 2048):
            src, _ = ref.replay_sample(Bs, 5, stream=sp)
            ids = torch.randint(0, n, (Bs,), dtype=torch.int32, device="cuda")
            bufs = [torch.empty(Bs * k, dtype=torch.float32, device="cuda")
                    for k in (ref.obs_feat, K1, K1, K1, K1 * A, 1)]
            dst = abi.MzBatch(Bs, *(t.data_ptr() for t in bufs), None)
            torch.cuda.synchronize()

            def f(i):
                ref._check(ref.lib.mz_batch_symmetry(ref.h, src, ids.data_ptr(), dst, sp), "mz_batch_symmetry")
            out[f"batch_sym_B{Bs}"] = {"ms": [round(timed(stream, f, args.warmup, args.calls), 5)
                                              for _ in range(args.rounds)]}
        res["legs"][name] = out
        ref.close(); corr.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
