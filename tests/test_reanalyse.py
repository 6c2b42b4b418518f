"""Reanalyse on the host mirror (replay_buffer.py; ReplayBuffer.jl:8, 56-67):
compute_target_value bootstraps from reanalysed_predicted_root_values unless
the field is None, and ReplayBuffer.reanalyse fills the field from the
current networks.  CPU only; the device shard is checked against this mirror
in tests/test_reanalyse_gpu.py."""
import ctypes
import dataclasses

import numpy as np

from muzero_jl_amd.replay_buffer import ReplayBuffer, compute_target_value
from muzero_jl_amd.selfplay import GameHistory, get_stacked_observations


def rand_history(rng, T, osz=27, A=9):
    """A two-player history of T moves: 0/1 observation planes, alternating to_play."""
    h = GameHistory()
    for t in range(T):
        h.observation_history.append((rng.random(osz) < 0.4).astype(np.float32))
        h.action_history.append(int(rng.integers(1, A + 1)))
        h.reward_history.append(float(rng.choice([0.0, 0.0, 1.0, -1.0])))
        h.to_play_history.append(1 + t % 2)
        cv = rng.random(A).astype(np.float32)
        h.child_visits.append(cv / cv.sum())
        h.root_values.append(float(np.float32(rng.uniform(-1, 1))))
    return h


def _oracle(conf, hyper, nets, seed=0):
    from muzero_jl_amd.config import to_c_config, to_c_ffhp
    from oracle import Oracle
    o = Oracle(to_c_config(conf), to_c_ffhp(hyper), seed=seed)
    for n, w in enumerate(nets):
        o.set_weights(n, w)
    return o


def test_host_targets_use_the_reanalysed_values(ttt):
    from muzero_jl_amd.config import to_c_config
    from oracle import histories_to_c, lib
    conf = dataclasses.replace(ttt.conf, td_steps=2)
    cc = to_c_config(conf)
    L = lib()
    rng = np.random.default_rng(21)
    for T in (1, 2, 3, 4, 7, 10):
        h = rand_history(rng, T)
        plain = [compute_target_value(conf, h, i) for i in range(1, T + 1)]
        arr, keep = histories_to_c([h.as_arrays()])
        for i in range(1, T + 1):                           # the field None: root_values, as before
            assert plain[i - 1] == np.float32(L.ora_compute_target_value(ctypes.byref(cc), ctypes.byref(arr[0]), i))
        rean = rng.uniform(-1, 1, T).astype(np.float32)
        h.reanalysed_predicted_root_values = [np.float32(x) for x in rean]
        d = h.as_arrays()
        d["root_values"] = rean                             # the oracle's view: root_values replaced
        arr, keep = histories_to_c([d])
        got = [compute_target_value(conf, h, i) for i in range(1, T + 1)]
        for i in range(1, T + 1):
            assert got[i - 1] == np.float32(L.ora_compute_target_value(ctypes.byref(cc), ctypes.byref(arr[0]), i)), (T, i)
        if T > conf.td_steps + 1:                           # some index bootstraps: the targets moved
            assert got != plain
        h.reanalysed_predicted_root_values = None
        assert [compute_target_value(conf, h, i) for i in range(1, T + 1)] == plain


def test_host_reanalyse_fills_the_field_from_the_networks(ttt, nets):
    conf = dataclasses.replace(ttt.conf, td_steps=2, replay_buffer_size=4, batch_size=40)
    o = _oracle(conf, ttt.hyper, nets)
    rng = np.random.default_rng(22)
    rb = ReplayBuffer(conf, seed=9)
    for T in (3, 9, 1, 6, 8, 5):                            # ids 1..6, the FIFO holds 3..6
        rb.save_game(rand_history(rng, T))
    assert list(rb.buffer.keys()) == [3, 4, 5, 6]
    _, plain = rb.get_batch(step=4)

    def value_fn(x):
        return o.forward(1, o.forward(0, x))[0][:, 0]

    done = rb.reanalyse(value_fn, game_ids=[2, 4, 6])       # 2 was evicted: skipped
    assert done == [4, 6] and rb.num_reanalysed_games == 2
    assert rb.buffer[3].reanalysed_predicted_root_values is None
    assert rb.buffer[5].reanalysed_predicted_root_values is None
    for gid in (4, 6):
        h = rb.buffer[gid]
        T = len(h.root_values)
        x = np.stack([get_stacked_observations(h.observation_history, h.action_history, i,
                                               conf.stacked_observations, 9) for i in range(1, T + 1)])
        want = o.forward(1, o.forward(0, x))[0][:, 0]
        assert np.array_equal(np.array(h.reanalysed_predicted_root_values, np.float32), want)
    _, after = rb.get_batch(step=4)
    for k in plain:
        if k == "target_values":
            assert not np.array_equal(after[k], plain[k])
        else:
            assert np.array_equal(after[k], plain[k]), k
    assert rb.reanalyse(value_fn) == [3, 4, 5, 6] and rb.num_reanalysed_games == 6
