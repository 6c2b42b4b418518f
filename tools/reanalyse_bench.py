"""Reanalyse throughput at the configs[1] shard: the TicTacToe FC engine, the
shard filled by device self-play (512 slots, 50 simulations per move).

Two routes to reanalysed_predicted_root_values of every held game, timed
alternately in one process:
  device  mz_replay_reanalyse over all held games (one mz_reanalyse_fc
          launch), device events around enough repeats to run >= 0.5 s (the
          host's issue time of the same passes is reported next to it: a pass
          is not launch-bound while it is the smaller);
  host    what there was before it: replay_get_game for every game, the
          stacked observations in numpy, two net_forward calls (wall clock,
          synchronised; the values then have nowhere to go on the device).
Prints ONE JSON line: positions/s of both routes, the kernel's FLOP per
position from the layer shapes (2 x MACs of representation + prediction, the
policy head included: the root plan runs it) and the share of the f32 peak.

--search times the other half, mz_replay_reanalyse_search over all held games
(ceil(rows / games) rounds of gather -> batched search -> scatter, rows = cap x
(max_moves + 1): dead rows are searched too), against its host route:
replay_get_game + one mcts_search per game (wall clock, over the first
--host-games games; the results stay on the host).  Its JSON line carries the
fraction of searched rows that were live and, given --search-ms (ms_per_step
of a plain bench.py run of the parent commit on the same machine, i.e. one
batched search of `games` games), the figure to judge the pass against:
rounds x that launch time, and the gap to it.

--next times the worker, mz_replay_reanalyse_next in search mode, on the same
shard: rounds of whole games from the device cursor, only their live rows
packed into the `games` rows of one batched search.  One untimed lap with the
cursor read back after every round counts the rounds of a lap and their live
rows (no game arrives in between, so every lap is the same); the timed laps
then run from a seek to the oldest game with device events around them and no
read-back.  Its JSON line carries rounds, live rows per round, device seconds
per round, positions/s and, given --search-ms, the gap per round above that
launch.
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
from muzero_jl_amd.games import tictactoe as ttt  # noqa: E402
from muzero_jl_amd.networks import init_nets, net_macs  # noqa: E402
from muzero_jl_amd.selfplay import get_stacked_observations  # noqa: E402

PEAK_F32 = 157.3                     # TFLOP/s, as bench.py


def host_route(eng, conf, held):
    plane = conf.observation_shape[0] * conf.observation_shape[1]
    t0 = time.perf_counter()
    games = [eng.replay_get_game(i) for i in range(held)]
    x = np.stack([get_stacked_observations(h.observation_history, h.action_history, i, conf.stacked_observations, plane)
                  for h in games for i in range(1, len(h.root_values) + 1)])
    v = eng.forward(1, eng.forward(0, x))[0][:, 0]
    return time.perf_counter() - t0, v, games


def host_search_route(eng, conf, n_games):
    """replay_get_game + mcts_search per game; returns (seconds, positions, [(child_visits, root_values)])."""
    plane = conf.observation_shape[0] * conf.observation_shape[1]
    Tm = conf.max_moves + 1
    t0 = time.perf_counter()
    out, positions = [], 0
    for gi in range(n_games):
        h = eng.replay_get_game(gi)
        T = len(h.root_values)
        x = np.stack([get_stacked_observations(h.observation_history, h.action_history, i, conf.stacked_observations,
                                               plane) for i in range(1, T + 1)])
        legal = np.stack(h.observation_history)[:, 2 * plane:].astype(np.uint8)
        cv, rv, _ = eng.mcts_search(x, legal, np.array(h.to_play_history, np.int32), exploration=False, rng_step=0,
                                    game_offset=gi * Tm, temperature=0.0)
        out.append((cv, rv))
        positions += T
    return time.perf_counter() - t0, positions, out


def search_mode(a, eng, conf, held, ts, st):
    Tm = conf.max_moves + 1
    rows = a.cap * Tm                       # the selection clipped to the capacity: what the pass searches
    rounds_per_pass = -(-rows // a.games)
    for _ in range(2):                                        # warm-up (the first call allocates)
        eng.replay_reanalyse_search(stream=st)
    torch.cuda.synchronize()
    dev_s, issue_s, reps = [], [], 2
    for r in range(a.rounds):
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            t_issue = time.perf_counter()
            for _ in range(reps):
                eng.replay_reanalyse_search(stream=st)
            issued = time.perf_counter() - t_issue
            e1.record(ts)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            print(f"round {r}: {reps} passes, {ms:.3f} ms on the device, issued in {issued * 1e3:.3f} ms", file=sys.stderr)
            if ms >= 500.0:
                break
            reps = int(reps * min(100.0, max(2.0, 650.0 / max(ms, 1e-3))))
        dev_s.append(ms * 1e-3 / reps)
        issue_s.append(issued / reps)
    n_host = min(a.host_games, held)
    host_t, host_pos, host_out = host_search_route(eng, conf, n_host)
    agree = all(np.array_equal(eng.replay_get_reanalysed_policies(gi), cv) and
                np.array_equal(eng.replay_get_reanalysed(gi), rv) for gi, (cv, rv) in enumerate(host_out))
    positions = sum(len(eng.replay_get_game(i).root_values) for i in range(held))
    d = float(np.median(dev_s))
    out = {
        "tool": "reanalyse_bench", "mode": "search", "engine": "tictactoe fc", "games_held": int(held),
        "sims_per_move": conf.num_iters, "rows_per_round": a.games, "positions": positions, "rows_searched": rows,
        "live_fraction": round(positions / rows, 6), "rounds_per_pass": rounds_per_pass, "repeats": reps,
        "rounds": a.rounds, "device_s_per_pass": round(d, 9), "device_positions_per_s": round(positions / d, 1),
        "device_s_per_round": round(d / rounds_per_pass, 9),
        "host_issue_s_per_pass": round(float(np.median(issue_s)), 9),
        "host_games": n_host, "host_positions": host_pos, "host_s": round(host_t, 6),
        "host_positions_per_s": round(host_pos / host_t, 1),
        "speedup": round((host_t / host_pos) / (d / positions), 1), "routes_agree": bool(agree)}
    if a.search_ms:
        ref = rounds_per_pass * a.search_ms * 1e-3
        out.update({"parent_search_ms_per_launch": a.search_ms, "reference_s_per_pass": round(ref, 9),
                    "gap_s_per_pass": round(d - ref, 9), "gap_us_per_round": round((d - ref) / rounds_per_pass * 1e6, 3)})
    print(json.dumps(out))


def next_mode(a, eng, conf, held, ts, st):
    counts, _ = eng.replay_counts()
    played = int(counts[0])
    oldest = played - held + 1

    def lap(read_back):
        eng.replay_reanalyse_seek(oldest, stream=st)
        live = []
        for _ in range(rounds_per_lap if not read_back else held):
            eng.replay_reanalyse_next(abi.REAN_BY_SEARCH, exploration=False, rng_step=0, game_offset=0, stream=st)
            if read_back:
                cur, (first, n, rows) = eng.replay_reanalyse_cursor()
                live.append(rows)
                if cur == played + 1:
                    break
        return live

    rounds_per_lap = 0
    live = lap(True)                                          # warm-up (the first call allocates) and the count
    rounds_per_lap = len(live)
    positions = sum(live)
    assert positions == sum(len(eng.replay_get_game(i).root_values) for i in range(held))
    assert eng.replay_reanalysed_count() == held
    torch.cuda.synchronize()
    dev_s, issue_s, reps = [], [], 1
    for r in range(a.rounds):
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            t_issue = time.perf_counter()
            for _ in range(reps):
                lap(False)
            issued = time.perf_counter() - t_issue
            e1.record(ts)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            print(f"round {r}: {reps} laps, {ms:.3f} ms on the device, issued in {issued * 1e3:.3f} ms", file=sys.stderr)
            if ms >= 500.0:
                break
            reps = int(reps * min(100.0, max(2.0, 650.0 / max(ms, 1e-3))))
        dev_s.append(ms * 1e-3 / reps)
        issue_s.append(issued / reps)
    cur, last = eng.replay_reanalyse_cursor()
    assert cur == played + 1, "a timed lap did not end at the last game"
    d = float(np.median(dev_s))
    out = {
        "tool": "reanalyse_bench", "mode": "next", "engine": "tictactoe fc", "games_held": int(held),
        "sims_per_move": conf.num_iters, "rows_per_round": a.games, "positions": positions,
        "rounds_per_lap": rounds_per_lap, "live_rows_per_round_mean": round(positions / rounds_per_lap, 3),
        "live_rows_per_round_min": int(min(live)), "live_rows_per_round_max": int(max(live)),
        "live_fraction": round(positions / (rounds_per_lap * a.games), 6), "repeats": reps, "rounds": a.rounds,
        "device_s_per_lap": round(d, 9), "device_s_per_round": round(d / rounds_per_lap, 9),
        "device_positions_per_s": round(positions / d, 1),
        "host_issue_s_per_lap": round(float(np.median(issue_s)), 9)}
    if a.search_ms:
        gap = d / rounds_per_lap - a.search_ms * 1e-3
        out.update({"parent_search_ms_per_launch": a.search_ms, "gap_us_per_round": round(gap * 1e6, 3)})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--next", action="store_true", help="time rounds of mz_replay_reanalyse_next (search mode) over one lap")
    ap.add_argument("--search", action="store_true", help="time mz_replay_reanalyse_search instead of the value pass")
    ap.add_argument("--host-games", type=int, default=512, help="--search: games of the host route")
    ap.add_argument("--search-ms", type=float, default=None,
                    help="--search / --next: the parent commit's ms_per_step of a plain bench.py run on the same machine")
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sims", type=int, default=None,
                    help="simulations per move of the self-play that fills the shard and of the reanalyse search "
                         "(default: the game's num_iters; --search: 50, bench.py's configs[1])")
    a = ap.parse_args()
    conf = dataclasses.replace(ttt.conf, replay_buffer_size=a.cap)
    if a.sims or a.search or a.next:
        conf = dataclasses.replace(conf, num_iters=a.sims or 50)
    eng = abi.Engine(conf, ttt.hyper, device=0, max_games=a.games, rng_seed=1)
    for n, w in enumerate(init_nets(conf, ttt.hyper, seed=1234)):
        eng.set_weights(n, w)
    eng.selfplay_init(abi.ENV_TICTACTOE, a.games, a.cap)
    for m in range(a.moves):
        eng.selfplay_move(m, game_offset=0)
    counts, held = eng.replay_counts()
    eng.sync()
    ts = torch.cuda.Stream()              # its own stream: the events and the launches share it (a null handle
    st = ts.cuda_stream                   # would send the launches to the engine's stream, past the events)
    if a.search or a.next:
        (next_mode if a.next else search_mode)(a, eng, conf, held, ts, st)
        eng.close()
        return
    for _ in range(5):                                        # warm-up
        eng.replay_reanalyse(stream=st)
    torch.cuda.synchronize()
    dev_s, host_s, issue_s, reps = [], [], [], 10
    positions = None
    for r in range(a.rounds):
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            t_issue = time.perf_counter()
            for _ in range(reps):
                eng.replay_reanalyse(stream=st)
            issued = time.perf_counter() - t_issue
            e1.record(ts)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            print(f"round {r}: {reps} passes, {ms:.3f} ms on the device, issued in {issued * 1e3:.3f} ms", file=sys.stderr)
            if ms >= 500.0:
                break
            reps = int(reps * min(100.0, max(2.0, 650.0 / max(ms, 1e-3))))
        dev_s.append(ms * 1e-3 / reps)
        issue_s.append(issued / reps)
        t, v, games = host_route(eng, conf, held)
        host_s.append(t)
        positions = int(v.shape[0])
        got = np.concatenate([eng.replay_get_reanalysed(i) for i in range(held)])
        assert np.array_equal(got, v), "the two routes disagree"
    flop = 2 * (net_macs(conf, ttt.hyper, 0) + net_macs(conf, ttt.hyper, 1))
    d, h = float(np.median(dev_s)), float(np.median(host_s))
    print(json.dumps({
        "tool": "reanalyse_bench", "engine": "tictactoe fc", "games_held": int(held), "positions": positions,
        "ring_rows": int(held) * (conf.max_moves + 1), "repeats": reps, "rounds": a.rounds,
        "device_s_per_pass": round(d, 9), "device_positions_per_s": round(positions / d, 1),
        "host_issue_s_per_pass": round(float(np.median(issue_s)), 9),
        "host_s_per_pass": round(h, 6), "host_positions_per_s": round(positions / h, 1),
        "speedup": round(h / d, 1), "flop_per_position": flop,
        "device_tflops": round(positions * flop / d / 1e12, 5),
        "frac_f32_peak": round(positions * flop / d / 1e12 / PEAK_F32, 6)}))
    eng.close()


if __name__ == "__main__":
    main()
