"""bench.py's plain run and --dump-outputs.

A plain run (no --full) times the searches only: its JSON line carries the
headline fields and none of the --full legs.  --dump-outputs DIR writes what
the last timed search returned — child visits, root values and the 1-based
actions, float32 — as DIR/<name>.npy.  The bench's inputs are seeded (nets
`init_nets(conf, hyper, seed=1234)`, positions `random_positions(env, G,
seed=100, max_plies=6)`, engine RNG seed 1) and the last timed step's RNG key
is warmup + steps - 1, so the dump is compared bit for bit with the C oracle's
search of the same inputs.  One small run (40 games x 16 sims, 2 steps).
"""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_timed_search(tmp_path):
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from muzero_jl_amd.games import tictactoe as ttt
    from muzero_jl_amd.networks import init_nets
    from muzero_jl_amd.selfplay import random_positions
    from oracle import Oracle

    G, S, steps, warmup = 40, 16, 2, 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--games", str(G), "--sims", str(S),
                        "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["unit"] == "node-expansions/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value = G * S / step time; the line rounds ms_per_step to 4 decimals (<= 5e-5 ms off) and value to 1
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - G * S) <= G * S * (5.1e-5 / d["ms_per_step"] + 1e-6)
    for k in ("cpu_baseline", "roofline", "learner_steps_per_s", "selfplay_pipeline", "train_loop"):
        assert k not in d, f"{k}: a --full leg in the plain line"

    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("child_visits", "root_values", "actions")}
    assert sorted(os.listdir(tmp_path)) == ["actions.npy", "child_visits.npy", "root_values.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["child_visits"].shape == (G, 9) and got["root_values"].shape == (G,) and got["actions"].shape == (G,)

    conf = dataclasses.replace(ttt.conf, num_iters=S)
    ora = Oracle(to_c_config(conf), to_c_ffhp(ttt.hyper), seed=1)
    for n, w in enumerate(init_nets(conf, ttt.hyper, seed=1234)):
        ora.set_weights(n, w)
    obs, legal, tp = random_positions(ttt.BatchedTicTacToe, G, seed=100, max_plies=6)
    cv, rv, act = ora.mcts_search(obs, legal, tp, exploration=True, rng_step=warmup + steps - 1, game_offset=0,
                                  temperature=1.0)
    assert np.array_equal(got["child_visits"], cv), "child visits differ from the oracle"
    assert np.array_equal(got["root_values"], rv), "root values differ from the oracle"
    assert np.array_equal(got["actions"], act.astype(np.float32)), "actions differ from the oracle"
