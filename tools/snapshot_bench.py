"""Snapshot cost (mz_snapshot_save / _load) at two shards:

  configs1   the TicTacToe FC engine, the shard filled by device self-play
             (512 slots x 50 simulations, 4096 games held), the train loop on;
  configs4   the configs[4] shape: the synthetic Atari-like env, 512 slots,
             max_moves 1000 (T = 1001 rows of 7,056 frame bytes per record), a
             512-game shard filled through mz_replay_save_game with games whose
             lengths follow the env's own rule (an episode ends with p = 1/128
             per move), then a few self-play moves so the slots hold rows too.

Per case ONE JSON line: the packed tensors' bytes against the raw arrays' bytes (cap·T and
G·T rows of every saved field), save and load seconds (wall clock around the
host-synchronous calls, median of --repeats), the staging size, and the
yardstick: a plain hipMemcpy device-to-host of as many bytes as the packed shard
and slot tensors hold, into pageable and into pinned host memory, in the same
process (and, for the file system's share, a plain write of the file's bytes).  The loaded
engine's held games are compared with the saved engine's (first, last and a
middle game) so a timing of a wrong result is not reported.
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (one HIP runtime)
import _mzpkg  # noqa: E402

_mzpkg.load()
from muzero_jl_amd import abi  # noqa: E402
from muzero_jl_amd.networks import init_nets  # noqa: E402

STAGE_DEFAULT = 64 << 20


def build_configs1(a):
    from muzero_jl_amd.games import tictactoe as g
    conf = dataclasses.replace(g.conf, num_iters=50, replay_buffer_size=4096, batch_size=64)
    eng = abi.Engine(conf, g.hyper, device=0, max_games=512, rng_seed=1)
    for n, w in enumerate(init_nets(conf, g.hyper, seed=1234)):
        eng.set_weights(n, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, 512, 4096)
    eng.train_init(64)
    eng.train_run(80, move0=0, game_offset=0)
    fresh = abi.Engine(conf, g.hyper, device=0, max_games=512, rng_seed=1)
    return conf, eng, fresh, abi.ENV_TICTACTOE, 512, 4096


def build_configs4(a):
    from muzero_jl_amd.games import atari_synth as g
    G = cap = a.atari_games
    conf = dataclasses.replace(g.conf, num_iters=2, batch_size=8)
    eng = abi.Engine(conf, g.resnet_hyper, device=0, max_games=G, rng_seed=1)
    for n, w in enumerate(init_nets(conf, g.resnet_hyper, seed=1234)):
        eng.set_weights(n, w)
    eng.selfplay_init(abi.ENV_ATARI, G, cap)
    rng = np.random.default_rng(7)
    T, osz, A = conf.max_moves + 1, 84 * 84, 18
    p = abi._p
    for _ in range(cap):                              # episodes end with p = 1/128 per move, or at max_moves
        n = int(min(rng.geometric(1.0 / 128.0), T))
        obs = rng.integers(0, 256, (n, osz), dtype=np.uint8)
        act = rng.integers(1, A + 1, n).astype(np.int32)
        rew = (rng.random(n) < 1.0 / A).astype(np.float32)
        tp = np.ones(n, np.int32)
        cv = rng.random((n, A)).astype(np.float32)
        cv /= cv.sum(1, keepdims=True)
        rv = rng.normal(0, 1, n).astype(np.float32)
        eng._check(eng.lib.mz_replay_save_game(eng.h, n, p(obs), p(act), p(rew), p(tp), p(cv), p(rv)),
                   "mz_replay_save_game")
    for m in range(a.atari_moves):
        eng.selfplay_move(m, game_offset=0)
    eng.sync()
    fresh = abi.Engine(conf, g.resnet_hyper, device=0, max_games=G, rng_seed=1)
    return conf, eng, fresh, abi.ENV_ATARI, G, cap


def memcpy_yardstick(nbytes, repeats):
    d = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d.fill_(3)
    torch.cuda.synchronize()
    pageable = np.empty(nbytes, np.uint8)
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    tp, tq = [], []
    for _ in range(repeats + 1):                      # the first touches the pages
        t0 = time.perf_counter()
        abi._copy_d2h(pageable, d.data_ptr())
        tp.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        pinned.copy_(d)
        torch.cuda.synchronize()
        tq.append(time.perf_counter() - t0)
    return float(np.median(tp[1:])), float(np.median(tq[1:]))


def same_game(x, y):
    x, y = x.as_arrays(), y.as_arrays()
    return all(np.array_equal(x[k], y[k]) for k in x)


def run(name, a, out_dir):
    conf, eng, fresh, env, G, cap = (build_configs1 if name == "configs1" else build_configs4)(a)
    counts, held = eng.replay_counts()
    ln, _, _ = eng.selfplay_slots()
    T, A, osz = conf.max_moves + 1, len(conf.action_space), eng.osz
    path = os.path.join(out_dir, name + ".safetensors")
    save_s, load_s = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        eng.snapshot_save(path, 1)
        save_s.append(time.perf_counter() - t0)
    file_bytes = os.path.getsize(path)
    with open(path, "rb") as f:                       # the packed part: the shard's and the slots' tensors
        hdr = json.loads(f.read(int.from_bytes(f.read(8), "little")))
    packed = sum(v["data_offsets"][1] - v["data_offsets"][0] for k, v in hdr.items()
                 if k.startswith(("shard.", "slots.")))
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fresh.snapshot_load(path)
        load_s.append(time.perf_counter() - t0)
    assert fresh.replay_counts()[1] == held
    ok = all(same_game(eng.replay_get_game(i), fresh.replay_get_game(i)) for i in {0, held // 2, held - 1})
    ring_row = osz + 4 * 5 + 4 * A                    # obs, act, rew, tp, rv, rrv, cv (rcv / prio: not allocated here)
    hist_row = osz + 4 * 4 + 4 * A
    raw = cap * T * ring_row + G * T * hist_row + G * osz
    pageable_s, pinned_s = memcpy_yardstick(packed, a.repeats)
    buf, write_s = np.zeros(file_bytes, np.uint8), []
    for _ in range(a.repeats):                        # the file system's share: the same bytes from host memory
        t0 = time.perf_counter()
        with open(path + ".w", "wb") as f:
            f.write(buf)
        write_s.append(time.perf_counter() - t0)
    os.remove(path + ".w")
    s, l = float(np.median(save_s)), float(np.median(load_s))
    print(json.dumps({
        "tool": "snapshot_bench", "case": name, "games_held": int(held), "slots": G, "cap": cap, "T": T,
        "live_rows_shard": int(counts[2]), "live_rows_slots": int(ln.sum()), "live_fraction_shard": round(int(counts[2]) / (cap * T), 6),
        "file_bytes": file_bytes, "packed_bytes": packed, "raw_array_bytes": raw, "packed_over_raw": round(packed / raw, 6),
        "plain_file_write_s": round(float(np.median(write_s)), 6),
        "staging_bytes": int(os.environ.get("MZ_SNAP_STAGE_BYTES", STAGE_DEFAULT)), "repeats": a.repeats,
        "save_s": round(s, 6), "save_s_all": [round(x, 6) for x in save_s],
        "load_s": round(l, 6), "load_s_all": [round(x, 6) for x in load_s],
        "save_GBps": round(file_bytes / s / 1e9, 3), "load_GBps": round(file_bytes / l / 1e9, 3),
        "hipMemcpy_d2h_pageable_s": round(pageable_s, 6), "hipMemcpy_d2h_pinned_s": round(pinned_s, 6),
        "save_over_pageable_memcpy": round(s / pageable_s, 2), "save_over_pinned_memcpy": round(s / pinned_s, 2),
        "loaded_games_equal": bool(ok)}), flush=True)
    eng.close()
    fresh.close()
    os.remove(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="configs1,configs4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--atari-games", type=int, default=512)
    ap.add_argument("--atari-moves", type=int, default=8)
    ap.add_argument("--dir", default=None, help="where the snapshot files go (default: a temporary directory)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for name in a.cases.split(","):
            run(name, a, d)


if __name__ == "__main__":
    main()
