"""ctypes binding of libmz (include/mz.h) — the Python side of the drop-in
boundary.  The Julia side a maintainer would add is in INTEGRATION.md.

The product path has no fallback: if libmz.so is missing or no HIP device is
present, `Engine(...)` raises.  Arrays crossing the ABI are numpy arrays in the
reference's column-major shapes, stored here as C-contiguous arrays whose LAST
axis is Julia's FIRST (e.g. Julia (A, G) == numpy (G, A)).
"""
import ctypes
import os

import numpy as np

from . import LIB_PATH
from .config import (MzConfig, MzFFHP, MzResNetHP, ResNetHP, hidden_size, stacked_features, to_c_config,
                     to_c_ffhp, to_c_resnet_hp)

NET_REPR, NET_PRED, NET_DYN = 0, 1, 2
ENV_TICTACTOE, ENV_CONNECT4, ENV_ATARI = 0, 1, 2
SP_TRAIN, SP_EVAL = 0, 1
TRAIN_LEARNER, TRAIN_ACTOR, TRAIN_QUEUED = 0, 1, 2
LEARN_REF_SEMANTICS, LEARN_CORRECTED = 0, 1
# mz_debug_bp_plan's values, in order (include/mz.h)
BP_PLAN_FIELDS = ("n_app", "fwd_levels", "bwd_levels", "slot_floats", "nslot", "lds_bytes", "arena_reads",
                  "unslotted_outputs", "arena_accumulations", "fwd_flagged", "bwd_flagged")
OPP_SELF, OPP_RANDOM, OPP_EXPERT, OPP_NETWORK, OPP_MCTS = 0, 1, 2, 3, 4
PLAYER_SEARCH, PLAYER_PRIOR = 0, 1               # mz_eval_players: the search, the network-only player
REAN_OFF, REAN_BY_VALUE, REAN_BY_SEARCH = 0, 1, 2
TEST_RECORDS = 1024                              # MZ_TEST_RECORDS: the test worker's record ring
# one record of the test worker (mz_test_results): counts[8] then sums[3]
TEST_COUNT_FIELDS = ("training_step", "games", "muzero_wins", "opponent_wins", "draws", "moves", "value_moves",
                     "rng_step0")
TEST_SUM_FIELDS = ("reward_muzero", "reward_opponent", "value_sum")
# one audit row (mz_test_audit_results, mz_expert_judge); judged == -1: the evaluation ran with judging off
TEST_AUDIT_FIELDS = ("judged", "best", "blunders", "deficit")
# the run log (mz_train_log_results): counts[16] then sums[16]; sums and counts, never means
LOG_RECORDS = 1024                               # MZ_LOG_RECORDS: the run log's record ring
LOG_COUNT_FIELDS = ("training_step", "steps", "num_played_games", "num_played_steps", "positions_held", "games_held",
                    "reanalysed", "games", "moves", "wins_p1", "wins_p2", "draws", "refreshes", "missed",
                    "reserved14", "reserved15")
LOG_SUM_FIELDS = ("value", "reward", "policy", "l2_repr", "l2_pred", "l2_dyn", "last_value", "last_reward",
                  "last_policy", "last_l2_repr", "last_l2_pred", "last_l2_dyn", "eta", "reward_sum", "root_value_sum",
                  "sharpness_sum")
TTT_CODES = 19683                                # the solved TicTacToe table's entries (mz_expert_table)

_lib = None

_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int32)
_U8 = ctypes.POINTER(ctypes.c_uint8)
_VP = ctypes.c_void_p


class MzBatch(ctypes.Structure):
    _fields_ = [("batch_size", ctypes.c_int32), ("observation", _VP), ("actions", _VP),
                ("target_values", _VP), ("target_rewards", _VP), ("target_policies", _VP),
                ("gradient_scale", _VP), ("weights", _VP)]


# exported symbol -> (restype, argtypes); tests check every one is present
SIGNATURES = {
    "mz_engine_create": (ctypes.c_int, [ctypes.POINTER(MzConfig), ctypes.POINTER(MzFFHP), ctypes.c_int,
                                        ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(_VP)]),
    "mz_engine_create_resnet": (ctypes.c_int, [ctypes.POINTER(MzConfig), ctypes.POINTER(MzResNetHP), ctypes.c_int,
                                               ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(_VP)]),
    "mz_engine_destroy": (None, [_VP]),
    "mz_last_error": (ctypes.c_char_p, [_VP]),
    "mz_create_error": (ctypes.c_char_p, []),
    "mz_net_param_count": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]),
    "mz_weights_set": (ctypes.c_int, [_VP, ctypes.c_int, _VP, ctypes.c_size_t]),
    "mz_weights_get": (ctypes.c_int, [_VP, ctypes.c_int, _VP, ctypes.c_size_t]),
    "mz_net_forward": (ctypes.c_int, [_VP, ctypes.c_int, _VP, ctypes.c_int, _VP, _VP]),
    "mz_mcts_search": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, _VP, ctypes.c_int, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_float, _VP, _VP, _VP]),
    "mz_mcts_search_dev": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, _VP, ctypes.c_int, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.c_float, _VP, _VP, _VP, _VP]),
    "mz_debug_enable": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_set_sync_stream": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    "mz_debug_tree": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mz_debug_unroll": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, _VP]),
    "mz_debug_select_stats": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP]),
    "mz_debug_kernel_time": (ctypes.c_int, [_VP, _VP, _VP]),
    "mz_learner_step": (ctypes.c_int, [_VP, ctypes.POINTER(MzBatch), ctypes.c_double, _VP]),
    "mz_grad_count": (ctypes.c_int, [_VP, ctypes.POINTER(ctypes.c_size_t)]),
    "mz_learner_grad_dev": (ctypes.c_int, [_VP, ctypes.POINTER(MzBatch), _VP, _VP, _VP]),
    "mz_learner_apply_dev": (ctypes.c_int, [_VP, _VP, ctypes.c_float, ctypes.c_double, _VP]),
    "mz_selfplay_init": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mz_selfplay_move": (ctypes.c_int, [_VP, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, _VP]),
    "mz_dp_unique_id": (ctypes.c_int, [_VP]),
    "mz_dp_init": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP]),
    "mz_dp_allreduce": (ctypes.c_int, [_VP, _VP, _VP]),
    "mz_learner_train_dp": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, ctypes.c_double, _VP, _VP]),
    "mz_selfplay_mode": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mz_expert_depth": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_expert_eval": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, _VP]),
    "mz_expert_table": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_expert_table_get": (ctypes.c_int, [_VP, _VP, _VP, _VP]),
    "mz_expert_judge": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP, ctypes.c_int, _VP]),
    "mz_mcts_opponent": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int]),
    "mz_mcts_eval": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_uint32, ctypes.c_uint32, _VP, _VP]),
    "mz_eval_players": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int]),
    "mz_prior_eval": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_float, _VP, _VP, _VP]),
    "mz_prior_eval_dev": (ctypes.c_int, [_VP, ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_float, _VP, _VP, _VP, _VP]),
    "mz_opponent_weights_set": (ctypes.c_int, [_VP, ctypes.c_int, _VP, ctypes.c_size_t]),
    "mz_opponent_weights_get": (ctypes.c_int, [_VP, ctypes.c_int, _VP, ctypes.c_size_t]),
    "mz_opponent_from": (ctypes.c_int, [_VP, ctypes.c_int, _VP]),
    "mz_opponent_load": (ctypes.c_int, [_VP, ctypes.c_char_p, _VP]),
    "mz_eval_results": (ctypes.c_int, [_VP, _VP]),
    "mz_test_config": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int, ctypes.c_int]),
    "mz_test_play": (ctypes.c_int, [_VP, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, _VP]),
    "mz_test_results": (ctypes.c_int, [_VP, _VP, _VP, _VP, ctypes.c_int32]),
    "mz_test_clear": (ctypes.c_int, [_VP]),
    "mz_test_audit": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_test_audit_results": (ctypes.c_int, [_VP, _VP, _VP, ctypes.c_int32]),
    "mz_test_get_game": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mz_train_set_test": (ctypes.c_int, [_VP, ctypes.c_int64, ctypes.c_uint32, ctypes.c_float]),
    "mz_train_set_log": (ctypes.c_int, [_VP, ctypes.c_int64]),
    "mz_train_log_flush": (ctypes.c_int, [_VP, _VP]),
    "mz_train_log_results": (ctypes.c_int, [_VP, _VP, _VP, _VP, ctypes.c_int32]),
    "mz_train_log_clear": (ctypes.c_int, [_VP]),
    "mz_replay_counts": (ctypes.c_int, [_VP, _VP, _VP]),
    "mz_replay_save_game": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mz_replay_sample": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(MzBatch), _VP, _VP]),
    "mz_replay_set_symmetry": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_replay_symmetry_get": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "mz_batch_symmetry": (ctypes.c_int, [_VP, ctypes.POINTER(MzBatch), _VP, ctypes.POINTER(MzBatch), _VP]),
    "mz_learner_grad_sampled_dev": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, _VP, _VP, _VP]),
    "mz_learner_train_dev": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, ctypes.c_double, _VP, _VP]),
    "mz_learner_train_multi_dev": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_double), _VP, _VP, _VP]),
    "mz_debug_unroll_step": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, _VP, _VP]),
    "mz_debug_bp_plan": (ctypes.c_int, [_VP, _VP, ctypes.c_int]),
    "mz_replay_update_priorities": (ctypes.c_int, [_VP, _VP]),
    "mz_replay_get_priorities": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP]),
    "mz_replay_get_game": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "mz_selfplay_slots": (ctypes.c_int, [_VP, _VP, _VP, _VP]),
    "mz_replay_reanalyse": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int32, _VP]),
    "mz_replay_clear_reanalysed": (ctypes.c_int, [_VP, _VP]),
    "mz_replay_reanalysed_count": (ctypes.c_int, [_VP, _VP]),
    "mz_replay_get_reanalysed": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP]),
    "mz_replay_reanalyse_search": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_uint32,
                                                  ctypes.c_uint32, _VP]),
    "mz_replay_get_reanalysed_policies": (ctypes.c_int, [_VP, ctypes.c_int32, _VP, _VP]),
    "mz_replay_reanalyse_next": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _VP]),
    "mz_replay_reanalyse_cursor": (ctypes.c_int, [_VP, _VP, _VP]),
    "mz_replay_reanalyse_seek": (ctypes.c_int, [_VP, ctypes.c_int64, _VP]),
    "mz_train_set_reanalyse": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mz_learner_set_mode": (ctypes.c_int, [_VP, ctypes.c_int]),
    "mz_train_init": (ctypes.c_int, [_VP, ctypes.c_int32]),
    "mz_train_init_at": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_int64]),
    "mz_train_set_networks_path": (ctypes.c_int, [_VP, ctypes.c_char_p]),
    "mz_train_run": (ctypes.c_int, [_VP, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, _VP, _VP, _VP]),
    "mz_train_move": (ctypes.c_int, [_VP, ctypes.c_uint32, ctypes.c_uint32, _VP, _VP]),
    "mz_train_learn": (ctypes.c_int, [_VP, ctypes.c_int64, _VP, _VP, _VP]),
    "mz_train_weights_get": (ctypes.c_int, [_VP, ctypes.c_int, ctypes.c_int, _VP, ctypes.c_size_t]),
    "mz_checkpoint_save": (ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int64]),
    "mz_checkpoint_load": (ctypes.c_int, [_VP, ctypes.c_char_p, _VP]),
    "mz_snapshot_save": (ctypes.c_int, [_VP, ctypes.c_char_p, ctypes.c_int64]),
    "mz_snapshot_load": (ctypes.c_int, [_VP, ctypes.c_char_p, _VP]),
    "mz_search_variant": (ctypes.c_char_p, [_VP]),
    "mz_learner_variant": (ctypes.c_char_p, [_VP]),
    "mz_resnet_tile_games": (ctypes.c_int, [_VP]),
    "mz_downsample_staged": (ctypes.c_int, [_VP]),
    "mz_sync": (ctypes.c_int, [_VP]),
}


def load_library(path=LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libmz.so not built at {path}: run __graft_entry__.build() "
                           "(there is no CPU fallback for the engine)")
    # torch's wheel ships its own libamdhip64.so.7 with the same soname as
    # /opt/rocm's: whichever loads first serves the whole process.  Loading
    # torch first (when present) makes libmz bind to torch's copy, so the
    # engine and torch streams / device tensors share one HIP runtime in any
    # import order; torch cannot initialise on the other copy.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    variant = bool(os.environ.get("MZ_LIB")) and path == os.environ.get("MZ_LIB")
    for name, (res, args) in SIGNATURES.items():
        if variant and not hasattr(lib, name):
            continue                 # an older A/B variant library (MZ_LIB) without this entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_VP)


_hip = None


def _copy_d2h(dst, src_ptr):
    """hipMemcpy device -> host (the HIP runtime libmz is linked against)."""
    global _hip
    if _hip is None:
        # by soname: the copy already loaded for libmz (torch's or /opt/rocm's,
        # whichever came first); a plain "libamdhip64.so" can load a second runtime
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpy.restype = ctypes.c_int
        _hip.hipMemcpy.argtypes = [_VP, _VP, ctypes.c_size_t, ctypes.c_int]
    rc = _hip.hipMemcpy(dst.ctypes.data_as(_VP), ctypes.c_void_p(src_ptr), dst.nbytes, 2)   # DeviceToHost
    if rc != 0:
        raise MzError(f"hipMemcpy failed ({rc})")


class MzError(RuntimeError):
    pass


class Engine:
    """One libmz handle = one GPU (SURVEY §8b conventions)."""

    def __init__(self, conf, hyper, device=0, max_games=512, rng_seed=0):
        lib = load_library()
        self.lib = lib
        self.conf = conf
        self.hyper = hyper
        self._cconf = to_c_config(conf)
        h = _VP()
        if isinstance(hyper, ResNetHP):        # row a14: the ResNet networks
            self._chp = to_c_resnet_hp(hyper)
            rc = lib.mz_engine_create_resnet(ctypes.byref(self._cconf), ctypes.byref(self._chp), device, max_games,
                                             rng_seed, ctypes.byref(h))
        else:
            self._chp = to_c_ffhp(hyper)
            rc = lib.mz_engine_create(ctypes.byref(self._cconf), ctypes.byref(self._chp), device, max_games,
                                      rng_seed, ctypes.byref(h))
        if rc != 0:
            raise MzError(f"mz_engine_create: {lib.mz_create_error().decode()}")
        self.h = h
        self.rng_seed = rng_seed
        self.max_games = max_games
        self.A = len(conf.action_space)
        self.H = hidden_size(conf, hyper)
        self.obs_feat = stacked_features(conf)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mz_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise MzError(f"{what}: {self.lib.mz_last_error(self.h).decode()}")

    # ---- weights (Flux order per net)
    def param_count(self, net):
        n = ctypes.c_size_t()
        self._check(self.lib.mz_net_param_count(self.h, net, ctypes.byref(n)), "mz_net_param_count")
        return n.value

    def set_weights(self, net, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        self._check(self.lib.mz_weights_set(self.h, net, _p(flat), flat.size), "mz_weights_set")

    def get_weights(self, net):
        out = np.empty(self.param_count(net), dtype=np.float32)
        self._check(self.lib.mz_weights_get(self.h, net, _p(out), out.size), "mz_weights_get")
        return out

    # ---- batched net forward (Flux Chain call)
    def forward(self, net, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        if net == NET_PRED:
            o0 = np.empty((n, 1), np.float32)
            o1 = np.empty((n, self.A), np.float32)
        elif net == NET_DYN:
            o0 = np.empty((n, self.H), np.float32)
            o1 = np.empty((n, 1), np.float32)
        else:
            o0 = np.empty((n, self.H), np.float32)
            o1 = None
        self._check(self.lib.mz_net_forward(self.h, net, _p(x), n, _p(o0), _p(o1)), "mz_net_forward")
        return (o0, o1) if o1 is not None else o0

    # ---- batched run_mcts
    def mcts_search(self, obs, legal_mask, to_play, exploration=True, rng_step=0, game_offset=0,
                    temperature=1.0):
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        G = obs.shape[0]
        legal = np.ascontiguousarray(legal_mask, dtype=np.uint8)
        tp = np.ascontiguousarray(to_play, dtype=np.int32)
        cv = np.empty((G, self.A), np.float32)
        rv = np.empty(G, np.float32)
        act = np.empty(G, np.int32)
        self._check(self.lib.mz_mcts_search(self.h, G, _p(obs), _p(legal), _p(tp), int(exploration),
                                            rng_step & 0xffffffff, game_offset, temperature,
                                            _p(cv), _p(rv), _p(act)), "mz_mcts_search")
        return cv, rv, act

    def mcts_search_dev(self, G, obs_ptr, legal_ptr, tp_ptr, cv_ptr, rv_ptr, act_ptr, exploration=True,
                        rng_step=0, game_offset=0, temperature=1.0, stream=None):
        self._check(self.lib.mz_mcts_search_dev(self.h, G, obs_ptr, legal_ptr, tp_ptr, int(exploration),
                                                rng_step & 0xffffffff, game_offset, temperature, cv_ptr,
                                                rv_ptr, act_ptr, stream), "mz_mcts_search_dev")

    def set_sync_stream(self, stream, narrow=True):
        """Narrow the host-synchronous calls' wait to `stream` + the handle's own (mz_set_sync_stream)."""
        self._check(self.lib.mz_set_sync_stream(self.h, stream, int(narrow)), "mz_set_sync_stream")

    def debug_enable(self, flags=1):
        self._check(self.lib.mz_debug_enable(self.h, flags), "mz_debug_enable")

    def debug_tree(self, G):
        S, A = self.conf.num_iters, self.A
        eN = np.empty((G, S + 1, A), np.int32)
        eW = np.empty((G, S + 1, A), np.float32)
        eP = np.empty((G, S + 1, A), np.float32)
        eR = np.empty((G, S + 1, A), np.float32)
        eC = np.empty((G, S + 1, A), np.int32)
        ntp = np.empty((G, S + 1), np.int32)
        self._check(self.lib.mz_debug_tree(self.h, G, _p(eN), _p(eW), _p(eP), _p(eR), _p(eC), _p(ntp)),
                    "mz_debug_tree")
        return dict(N=eN, W=eW, P=eP, R=eR, C=eC, to_play=ntp)

    def debug_select_stats(self, G):
        """Per game of the last small-kernel search: (simulations whose leaf the
        ballot select found, simulations that entered the serial walk)."""
        fast = np.empty(G, np.int32)
        walked = np.empty(G, np.int32)
        self._check(self.lib.mz_debug_select_stats(self.h, G, _p(fast), _p(walked)), "mz_debug_select_stats")
        return fast, walked

    def debug_kernel_time(self):
        """(summed ms, launches) of the timed network launches since the last call."""
        t, n = ctypes.c_double(), ctypes.c_int()
        self._check(self.lib.mz_debug_kernel_time(self.h, ctypes.byref(t), ctypes.byref(n)), "mz_debug_kernel_time")
        return t.value, n.value

    def debug_unroll(self, B):
        """Read-outs of the last learner unroll: values (B, K+1), policies
        (B, K+1, A) as probabilities, rewards (B, K+1)."""
        K1 = self.conf.num_unroll_steps + 1
        pv = np.empty((B, K1), np.float32)
        pp = np.empty((B, K1, self.A), np.float32)
        pr = np.empty((B, K1), np.float32)
        self._check(self.lib.mz_debug_unroll(self.h, B, _p(pv), _p(pp), _p(pr)), "mz_debug_unroll")
        return pv, pp, pr

    def debug_unroll_step(self, i, B):
        """debug_unroll of step step0 + i of the last learner_train_multi_dev."""
        K1 = self.conf.num_unroll_steps + 1
        pv = np.empty((B, K1), np.float32)
        pp = np.empty((B, K1, self.A), np.float32)
        pr = np.empty((B, K1), np.float32)
        self._check(self.lib.mz_debug_unroll_step(self.h, i, B, _p(pv), _p(pp), _p(pr)), "mz_debug_unroll_step")
        return pv, pp, pr

    def debug_bp_plan(self):
        """The FC corrected learner's plan (mz_debug_bp_plan; built if needed, nothing launched) as a
        dict of BP_PLAN_FIELDS; a plan the engine refuses raises MzError."""
        out = np.zeros(len(BP_PLAN_FIELDS), np.int32)
        self._check(self.lib.mz_debug_bp_plan(self.h, _p(out), out.size), "mz_debug_bp_plan")
        return dict(zip(BP_PLAN_FIELDS, (int(x) for x in out)))

    # ---- learner
    def learner_step(self, batch, eta):
        """batch: dict with observation (B, F), actions (B, K+1), target_values (B, K+1),
        target_rewards (B, K+1), target_policies (B, K+1, A), gradient_scale (B) and,
        with PER, weights (B)."""
        arrs = {k: np.ascontiguousarray(batch[k], dtype=np.float32) for k in
                ("observation", "actions", "target_values", "target_rewards", "target_policies", "gradient_scale")}
        w = batch.get("weights")
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
        b = MzBatch(arrs["observation"].shape[0], _p(arrs["observation"]), _p(arrs["actions"]),
                    _p(arrs["target_values"]), _p(arrs["target_rewards"]), _p(arrs["target_policies"]),
                    _p(arrs["gradient_scale"]), _p(w))
        losses = np.empty(6, np.float32)
        self._check(self.lib.mz_learner_step(self.h, ctypes.byref(b), float(eta), _p(losses)), "mz_learner_step")
        return losses

    def grad_count(self):
        n = ctypes.c_size_t()
        self._check(self.lib.mz_grad_count(self.h, ctypes.byref(n)), "mz_grad_count")
        return n.value

    def learner_grad_dev(self, dev_batch_ptrs, B, grad_ptr, losses_ptr=None, stream=None):
        b = MzBatch(B, *dev_batch_ptrs)
        self._check(self.lib.mz_learner_grad_dev(self.h, ctypes.byref(b), grad_ptr, losses_ptr, stream),
                    "mz_learner_grad_dev")

    def learner_apply_dev(self, grad_ptr, grad_scale, eta, stream=None):
        self._check(self.lib.mz_learner_apply_dev(self.h, grad_ptr, grad_scale, float(eta), stream),
                    "mz_learner_apply_dev")

    # ---- device self-play + replay shard
    def selfplay_init(self, env_kind, G, replay_games):
        self._check(self.lib.mz_selfplay_init(self.h, env_kind, G, replay_games), "mz_selfplay_init")
        self.sp_G = G
        self.osz = int(np.prod(self.conf.observation_shape))
        if env_kind == ENV_ATARI:                      # one 84x84 frame per move in the records
            self.osz = int(self.conf.observation_shape[0] * self.conf.observation_shape[1])

    def selfplay_move(self, rng_step, game_offset=0, temperature=1.0, stream=None):
        self._check(self.lib.mz_selfplay_move(self.h, rng_step, game_offset, temperature, stream),
                    "mz_selfplay_move")

    def learner_set_mode(self, mode):
        """LEARN_REF_SEMANTICS (∇ = 2θ, quirk Q11) or LEARN_CORRECTED (backprop)."""
        self._check(self.lib.mz_learner_set_mode(self.h, mode), "mz_learner_set_mode")

    def train_init(self, batch_size, t0=0):
        """Actor–learner loop (self_play! ‖ learning!, Q16): actors and the
        queued nets start from the current weights (mz_train_init_at; t0 = the
        learner step to continue from, e.g. a loaded checkpoint's)."""
        self._check(self.lib.mz_train_init_at(self.h, batch_size, int(t0)), "mz_train_init_at")

    def train_set_networks_path(self, path):
        """conf.networks_path: periodic checkpoints <path>/<t>.safetensors past
        0.9 training_steps (Learning.jl:416-432); None = none."""
        self._check(self.lib.mz_train_set_networks_path(self.h, path.encode() if path else None),
                    "mz_train_set_networks_path")

    def train_set_reanalyse(self, mode, rounds_per_move=1, exploration=False):
        """The Reanalyse worker inside train_run: `rounds_per_move` rounds of replay_reanalyse_next(mode)
        every move, after its self-play and before its learner steps (round r of move key m: rng_step m,
        game_offset + r * max_games).  REAN_OFF (the default): none."""
        self._check(self.lib.mz_train_set_reanalyse(self.h, mode, rounds_per_move, int(exploration)),
                    "mz_train_set_reanalyse")

    def train_run(self, moves, move0=0, game_offset=0, losses_ptr=None, stream=None):
        """`moves` self-play moves with the actors' nets, one learner step per
        finished game, actor refresh every checkpoint_interval steps; returns
        (t, num_played_games, actor refreshes, learner steps of this call)."""
        st = np.zeros(4, np.int64)
        self._check(self.lib.mz_train_run(self.h, moves, move0, game_offset, _p(st), losses_ptr, stream),
                    "mz_train_run")
        return tuple(int(x) for x in st)

    def train_move(self, move, game_offset=0, stream=None):
        """One self-play move of the actor-learner loop with the actors' nets; returns the games it saved
        (this rank's shard).  A data-parallel host sums that over the ranks and passes it to train_learn."""
        n = np.zeros(1, np.int64)
        self._check(self.lib.mz_train_move(self.h, move, game_offset, _p(n), stream), "mz_train_move")
        return int(n[0])

    def train_learn(self, steps, losses_ptr=None, stream=None):
        """`steps` learner steps (capped at training_steps) with the actor refreshes; returns
        (t, num_played_games, actor refreshes, learner steps of this call)."""
        st = np.zeros(4, np.int64)
        self._check(self.lib.mz_train_learn(self.h, int(steps), losses_ptr, _p(st), stream), "mz_train_learn")
        return tuple(int(x) for x in st)

    def train_weights(self, which, net):
        """Flux-order weights of the learner / actors / queued nets."""
        out = np.empty(self.param_count(net), np.float32)
        self._check(self.lib.mz_train_weights_get(self.h, which, net, _p(out), out.size), "mz_train_weights_get")
        return out

    def selfplay_mode(self, mode, opponent=OPP_SELF, muzero_player=1):
        """SP_TRAIN (self_play!) or SP_EVAL (competitive_play!: games tallied, not saved)."""
        self._check(self.lib.mz_selfplay_mode(self.h, mode, opponent, muzero_player), "mz_selfplay_mode")

    def expert_depth(self, depth=0):
        """Depth of the OPP_EXPERT rules search, 1..9 (0: the env's default, TicTacToe 9, Connect4 4)."""
        self._check(self.lib.mz_expert_depth(self.h, depth), "mz_expert_depth")

    def expert_eval(self, env_kind, boards, players, depth):
        """The expert's score(s, a, depth) of the positions boards (G, W*H*3) ([p1, p2, empty] planes)
        with players (G,) to move: int32 (G, A), -128 for an illegal action."""
        b = np.ascontiguousarray(boards, np.uint8)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        p = np.ascontiguousarray(players, np.int32).reshape(-1)
        want = {ENV_TICTACTOE: 27, ENV_CONNECT4: 126}.get(env_kind)     # any other env: the library refuses it
        if want is not None and (b.shape[1] != want or p.size != b.shape[0]):
            raise MzError(f"mz_expert_eval: boards must be (G, {want}) with G players")
        out = np.zeros((b.shape[0], self.A), np.int32)
        self._check(self.lib.mz_expert_eval(self.h, env_kind, b.shape[0], _p(b), _p(p), depth, _p(out)),
                    "mz_expert_eval")
        return out

    def expert_table(self, on=True):
        """The solved TicTacToe table: a handle setting, default off.  on: the table is built
        if the handle has none (host-synchronous), and the depth-9 TicTacToe expert's move becomes a lookup."""
        self._check(self.lib.mz_expert_table(self.h, int(bool(on))), "mz_expert_table")

    def expert_table_get(self, scores=True):
        """(table int8 (19683, 9) or None, built, in_use): entry code = sum of 3^cell * d (d = 0 empty, 1 the
        mover's stone, 2 the other's) holds score(s, a, 9), -128 for an illegal action; in_use: the lookup
        would be launched for the current env and depth.  scores=False: the flags only (table None); asking
        for the scores of a handle that has built no table is refused."""
        built, in_use = ctypes.c_int32(), ctypes.c_int32()
        table = np.zeros((TTT_CODES, 9), np.int8) if scores else None
        self._check(self.lib.mz_expert_table_get(self.h, _p(table), ctypes.byref(built), ctypes.byref(in_use)),
                    "mz_expert_table_get")
        return table, bool(built.value), bool(in_use.value)

    def expert_judge(self, env_kind, boards, players, actions, depth):
        """The judge's rule on given moves (boards (G, W*H*3), players (G,), 1-based actions (G,)) at `depth`:
        (moves judged, in the expert's best set, win or draw given away, score deficit) as ints."""
        b = np.ascontiguousarray(boards, np.uint8)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        p = np.ascontiguousarray(players, np.int32).reshape(-1)
        a = np.ascontiguousarray(actions, np.int32).reshape(-1)
        want = {ENV_TICTACTOE: 27, ENV_CONNECT4: 126}.get(env_kind)     # any other env: the library refuses it
        if want is not None and (b.shape[1] != want or p.size != b.shape[0] or a.size != b.shape[0]):
            raise MzError(f"mz_expert_judge: boards must be (G, {want}) with G players and G actions")
        out = np.zeros(4, np.int64)
        self._check(self.lib.mz_expert_judge(self.h, env_kind, b.shape[0], _p(b), _p(p), _p(a), depth, _p(out)),
                    "mz_expert_judge")
        return tuple(int(x) for x in out)

    def eval_players(self, muzero_kind=PLAYER_SEARCH, other_kind=PLAYER_SEARCH):
        """Which player produces a network side's rows in evaluation play: PLAYER_SEARCH or
        PLAYER_PRIOR (the policy head's move, no tree) for MuZero's turns and for the other turns where the other
        side is a network player (OPP_SELF, OPP_NETWORK).  A handle setting like expert_depth; training
        self-play never consults it."""
        self._check(self.lib.mz_eval_players(self.h, muzero_kind, other_kind), "mz_eval_players")

    def prior_eval(self, obs, legal_mask, opponent_set=0, rng_step=0, game_offset=0, temperature=0.0):
        """The network-only player on G rows (mz_prior_eval): (policy (G, A) = the policy head's softmax
        renormalised over the legal actions, value (G,), action (G,) 1-based).  opponent_set 1: the opponent
        weight set's nets."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        G = obs.shape[0]
        legal = np.ascontiguousarray(legal_mask, dtype=np.uint8)
        assert obs.ndim == 2 and legal.shape == (G, self.A), "prior_eval: obs (G, features), legal_mask (G, A)"
        pol = np.empty((G, self.A), np.float32)
        val = np.empty(G, np.float32)
        act = np.empty(G, np.int32)
        self._check(self.lib.mz_prior_eval(self.h, G, _p(obs), _p(legal), opponent_set, rng_step & 0xffffffff,
                                           game_offset, temperature, _p(pol), _p(val), _p(act)), "mz_prior_eval")
        return pol, val, act

    def mcts_opponent(self, sims=0, rollouts=0):
        """Budget of the OPP_MCTS rules MCTS: sims 1..1024 simulations a move, rollouts 1..64 random
        playouts per simulation; 0: the default (64, 16).  A handle setting like expert_depth."""
        self._check(self.lib.mz_mcts_opponent(self.h, sims, rollouts), "mz_mcts_opponent")

    def mcts_eval(self, env_kind, boards, players, sims, rollouts, rng_step=0, game_offset=0):
        """The rules MCTS's root statistics of the positions boards (G, W*H*3) ([p1, p2, empty] planes) with
        players (G,) to move, row g keyed (game_offset + g, rng_step): (n, w) int32 (G, A) each, the simulations
        through every root action and the sum of their outcomes for the mover in rollouts; n = -1 for an illegal
        action."""
        b = np.ascontiguousarray(boards, np.uint8)
        b = b.reshape(1, -1) if b.ndim == 1 else b
        p = np.ascontiguousarray(players, np.int32).reshape(-1)
        want = {ENV_TICTACTOE: 27, ENV_CONNECT4: 126}.get(env_kind)     # any other env: the library refuses it
        if want is not None and (b.shape[1] != want or p.size != b.shape[0]):
            raise MzError(f"mz_mcts_eval: boards must be (G, {want}) with G players")
        n = np.zeros((b.shape[0], self.A), np.int32)
        w = np.zeros((b.shape[0], self.A), np.int32)
        self._check(self.lib.mz_mcts_eval(self.h, env_kind, b.shape[0], _p(b), _p(p), sims, rollouts, rng_step,
                                          game_offset, _p(n), _p(w)), "mz_mcts_eval")
        return n, w

    # ---- the opponent's weight set of OPP_NETWORK: a handle setting
    def opponent_set_weights(self, net, flat):
        """One net of the opponent set (Flux order, as set_weights); complete after all three."""
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        self._check(self.lib.mz_opponent_weights_set(self.h, net, _p(flat), flat.size), "mz_opponent_weights_set")

    def opponent_get_weights(self, net):
        out = np.empty(self.param_count(net), dtype=np.float32)
        self._check(self.lib.mz_opponent_weights_get(self.h, net, _p(out), out.size), "mz_opponent_weights_get")
        return out

    def opponent_from(self, which, stream=None):
        """The opponent set := the engine's current nets (TRAIN_LEARNER) or the actor-learner loop's
        TRAIN_ACTOR / TRAIN_QUEUED set: a stream-ordered device copy, no host synchronisation."""
        self._check(self.lib.mz_opponent_from(self.h, which, stream), "mz_opponent_from")

    def opponent_load(self, path):
        """The opponent set := the three nets of a checkpoint or snapshot file (the learner is not
        touched; a refused file leaves the set as it was); returns the file's training step."""
        step = ctypes.c_int64()
        self._check(self.lib.mz_opponent_load(self.h, os.fsencode(path), ctypes.byref(step)), "mz_opponent_load")
        return step.value

    def eval_results(self):
        """(games finished, MuZero wins, opponent wins, draws) since selfplay_init."""
        out = np.zeros(4, np.int64)
        self._check(self.lib.mz_eval_results(self.h, _p(out)), "mz_eval_results")
        return tuple(int(x) for x in out)

    # ---- the test worker: evaluation games on their own slots
    def test_config(self, games, opponent=OPP_SELF, muzero_player=1):
        """E = games test slots (0 = off), the opponent and MuZero's side: a handle setting."""
        self._check(self.lib.mz_test_config(self.h, games, opponent, muzero_player), "mz_test_config")

    def test_play(self, training_step, rng_step0, game_offset=0, temperature=0.0, stream=None):
        """One evaluation: every test slot plays one game with the current nets (moves keyed rng_step0 + m,
        game_offset); appends one record.  Stream-ordered, no host synchronisation."""
        self._check(self.lib.mz_test_play(self.h, int(training_step), rng_step0 & 0xffffffff,
                                          game_offset & 0xffffffff, temperature, stream), "mz_test_play")

    def test_results(self, max_records=TEST_RECORDS):
        """(evaluations since create / test_clear, the latest records oldest first): each record a dict of
        TEST_COUNT_FIELDS (int) and TEST_SUM_FIELDS (np.float64).  Synchronises."""
        total = ctypes.c_int64()
        counts = np.zeros((max(max_records, 1), 8), np.int64)
        sums = np.zeros((max(max_records, 1), 3), np.float64)
        self._check(self.lib.mz_test_results(self.h, ctypes.byref(total), _p(counts), _p(sums), max_records),
                    "mz_test_results")
        n = min(max_records, total.value, TEST_RECORDS)
        recs = []
        for c, s in zip(counts[:n], sums[:n]):
            r = {k: int(v) for k, v in zip(TEST_COUNT_FIELDS, c)}
            r.update({k: np.float64(v) for k, v in zip(TEST_SUM_FIELDS, s)})
            recs.append(r)
        return int(total.value), recs

    def test_clear(self):
        self._check(self.lib.mz_test_clear(self.h), "mz_test_clear")

    def test_audit(self, on=True):
        """Judge MuZero's moves of the following evaluations by the expert's scores: a handle
        setting, default off."""
        self._check(self.lib.mz_test_audit(self.h, int(bool(on))), "mz_test_audit")

    def test_audit_results(self, max_records=TEST_RECORDS):
        """(evaluations since create / test_clear, int64 (n, 4) audit rows TEST_AUDIT_FIELDS of the records
        test_results returns, in its order; (-1, 0, 0, 0): that evaluation ran with judging off)."""
        total = ctypes.c_int64()
        audit = np.zeros((max(max_records, 1), 4), np.int64)
        self._check(self.lib.mz_test_audit_results(self.h, ctypes.byref(total), _p(audit), max_records),
                    "mz_test_audit_results")
        return int(total.value), audit[:min(max_records, total.value, TEST_RECORDS)].copy()

    def test_get_game(self, slot):
        """Test slot `slot`'s game of the last evaluation as a selfplay.GameHistory."""
        from .selfplay import GameHistory
        Tm = self.conf.max_moves + 1
        T = ctypes.c_int32()
        obs = np.zeros((Tm, self.osz), np.uint8)
        act = np.zeros(Tm, np.int32)
        rew = np.zeros(Tm, np.float32)
        tp = np.zeros(Tm, np.int32)
        cv = np.zeros((Tm, self.A), np.float32)
        rv = np.zeros(Tm, np.float32)
        self._check(self.lib.mz_test_get_game(self.h, slot, ctypes.byref(T), _p(obs), _p(act), _p(rew), _p(tp),
                                              _p(cv), _p(rv)), "mz_test_get_game")
        n = T.value
        return GameHistory(observation_history=[o.astype(np.float32) for o in obs[:n]],
                           action_history=[int(x) for x in act[:n]], reward_history=[float(x) for x in rew[:n]],
                           to_play_history=[int(x) for x in tp[:n]], child_visits=[c for c in cv[:n]],
                           root_values=[float(x) for x in rv[:n]])

    def train_set_test(self, interval, game_offset=0, temperature=0.0):
        """The test worker inside train_run: one evaluation after every move whose learner steps crossed a
        multiple of `interval` (test_play(t1, t1 * (max_moves + 1), game_offset, temperature)); 0 = off."""
        self._check(self.lib.mz_train_set_test(self.h, int(interval), game_offset & 0xffffffff, temperature),
                    "mz_train_set_test")

    # ---- the run log: per-interval loss and self-play records kept on the device
    def train_set_log(self, interval):
        """One record after every move (train_run) or call (train_learn) whose learner steps crossed a
        multiple of `interval`; 0 = off.  A handle setting."""
        self._check(self.lib.mz_train_set_log(self.h, int(interval)), "mz_train_set_log")

    def train_log_flush(self, stream=None):
        """One record now from whatever is accumulated.  Stream-ordered, no host synchronisation."""
        self._check(self.lib.mz_train_log_flush(self.h, stream), "mz_train_log_flush")

    def train_log_results(self, max_records=LOG_RECORDS):
        """(records since create / train_log_clear, the latest records oldest first): each record a dict of
        LOG_COUNT_FIELDS (int) and LOG_SUM_FIELDS (np.float64).  Synchronises."""
        total = ctypes.c_int64()
        counts = np.zeros((max(max_records, 1), 16), np.int64)
        sums = np.zeros((max(max_records, 1), 16), np.float64)
        self._check(self.lib.mz_train_log_results(self.h, ctypes.byref(total), _p(counts), _p(sums), max_records),
                    "mz_train_log_results")
        n = min(max_records, total.value, LOG_RECORDS)
        recs = []
        for c, s in zip(counts[:n], sums[:n]):
            r = {k: int(v) for k, v in zip(LOG_COUNT_FIELDS, c)}
            r.update({k: np.float64(v) for k, v in zip(LOG_SUM_FIELDS, s)})
            recs.append(r)
        return int(total.value), recs

    def train_log_clear(self):
        self._check(self.lib.mz_train_log_clear(self.h), "mz_train_log_clear")

    def replay_counts(self):
        """({num_played_games, num_played_steps, total_samples}, games held)."""
        c = np.zeros(3, np.int64)
        n = ctypes.c_int32()
        self._check(self.lib.mz_replay_counts(self.h, _p(c), ctypes.byref(n)), "mz_replay_counts")
        return c, n.value

    def replay_save_game(self, hist):
        """save_game of a host GameHistory (selfplay.GameHistory)."""
        a = hist.as_arrays()
        obs = np.ascontiguousarray(a["observation"], np.uint8)      # 0/1 planes, or frame bytes
        self._check(self.lib.mz_replay_save_game(
            self.h, len(a["action"]), _p(obs), _p(np.ascontiguousarray(a["action"], np.int32)),
            _p(np.ascontiguousarray(a["reward"], np.float32)), _p(np.ascontiguousarray(a["to_play"], np.int32)),
            _p(np.ascontiguousarray(a["child_visits"], np.float32)),
            _p(np.ascontiguousarray(a["root_values"], np.float32))), "mz_replay_save_game")

    def replay_get_game(self, i):
        """Game i of the shard (0 = oldest held) as a selfplay.GameHistory."""
        from .selfplay import GameHistory
        Tm = self.conf.max_moves + 1
        T = ctypes.c_int32()
        obs = np.zeros((Tm, self.osz), np.uint8)
        act = np.zeros(Tm, np.int32)
        rew = np.zeros(Tm, np.float32)
        tp = np.zeros(Tm, np.int32)
        cv = np.zeros((Tm, self.A), np.float32)
        rv = np.zeros(Tm, np.float32)
        self._check(self.lib.mz_replay_get_game(self.h, i, ctypes.byref(T), _p(obs), _p(act), _p(rew), _p(tp),
                                                _p(cv), _p(rv)), "mz_replay_get_game")
        n = T.value
        return GameHistory(observation_history=[o.astype(np.float32) for o in obs[:n]],
                           action_history=[int(x) for x in act[:n]], reward_history=[float(x) for x in rew[:n]],
                           to_play_history=[int(x) for x in tp[:n]], child_visits=[c for c in cv[:n]],
                           root_values=[float(x) for x in rv[:n]])

    def replay_sample(self, B, step, stream=None, index=False):
        """Device get_batch: returns (MzBatch of device pointers, index_batch (B, 2) or None)."""
        b = MzBatch()
        idx = np.zeros((B, 2), np.int32) if index else None
        self._check(self.lib.mz_replay_sample(self.h, B, step, ctypes.byref(b), _p(idx) if index else None, stream),
                    "mz_replay_sample")
        return b, idx

    def replay_set_symmetry(self, on=True):
        """Board-symmetry augmentation of every device get_batch: sample b at learner step
        `step` is drawn under element rng_below(rng_u32(seed, MZ_RNG_SYMMETRY, b, step, 0), n) of the
        env's group.  A handle setting like expert_depth; off by default."""
        self._check(self.lib.mz_replay_set_symmetry(self.h, int(on)), "mz_replay_set_symmetry")

    def replay_symmetry_get(self):
        """(games.symmetry.SymmetryTables as the device holds them, the setting)."""
        from .games.symmetry import SymmetryTables
        n, on = ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.mz_replay_symmetry_get(self.h, ctypes.byref(n), None, None, ctypes.byref(on)),
                    "mz_replay_symmetry_get")
        P = self.conf.observation_shape[0] * self.conf.observation_shape[1]
        cell, act = np.zeros((n.value, P), np.int32), np.zeros((n.value, self.A), np.int32)
        self._check(self.lib.mz_replay_symmetry_get(self.h, None, _p(cell), _p(act), None), "mz_replay_symmetry_get")
        return SymmetryTables(cell, act, self.conf.observation_shape[2]), bool(on.value)

    def batch_symmetry(self, batch, ids, stream=None):
        """mz_batch_symmetry: row b of `batch` under element ids[b] of the env's group.  batch: a device
        MzBatch (replay_sample's) or a host dict in get_batch's layout; ids: (B,) int32.  Returns a
        device MzBatch in torch tensors the result keeps alive (out._keep)."""
        import torch
        K1 = self.conf.num_unroll_steps + 1
        keep = []

        def dev(a, dtype):
            t = torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()
            keep.append(t)
            return t.data_ptr()
        if isinstance(batch, dict):
            B = batch["observation"].shape[0]
            src = MzBatch(B, *(dev(batch[k], np.float32) for k in (
                "observation", "actions", "target_values", "target_rewards", "target_policies", "gradient_scale")),
                dev(batch["weights"], np.float32) if "weights" in batch else None)
        else:
            src, B = batch, batch.batch_size
        out = MzBatch(B)
        for name, size in (("observation", B * self.obs_feat), ("actions", B * K1), ("target_values", B * K1),
                           ("target_rewards", B * K1), ("target_policies", B * K1 * self.A), ("gradient_scale", B),
                           ("weights", B if src.weights else 0)):
            if size:
                t = torch.empty(size, dtype=torch.float32, device="cuda")
                keep.append(t)
                setattr(out, name, t.data_ptr())
        self._check(self.lib.mz_batch_symmetry(self.h, ctypes.byref(src), dev(ids, np.int32), ctypes.byref(out), stream),
                    "mz_batch_symmetry")
        self.sync()
        out._keep = keep
        return out

    def learner_grad_sampled_dev(self, B, step, grad_ptr, losses_ptr=None, stream=None):
        """replay_sample(B, step) + learner_grad_dev, the sampling fused into the unroll kernel."""
        self._check(self.lib.mz_learner_grad_sampled_dev(self.h, B, step, grad_ptr, losses_ptr, stream),
                    "mz_learner_grad_sampled_dev")

    def learner_train_dev(self, B, step, eta, losses_ptr=None, stream=None):
        """One GPU: replay_sample + learner_grad_dev + learner_apply_dev(scale 1) in two launches."""
        self._check(self.lib.mz_learner_train_dev(self.h, B, step, float(eta), losses_ptr, stream),
                    "mz_learner_train_dev")

    def learner_train_multi_dev(self, B, step0, etas, losses_ptr=None, theta_ptr=None, stream=None):
        """len(etas) consecutive learner_train_dev steps step0 .. step0+L-1 (ref_semantics FC: the ADAM
        chain in one launch, the L unrolls + losses side by side in a second); losses_ptr: [L][8] floats,
        theta_ptr: [L][nflat] floats (the parameters after each step), both optional device pointers."""
        e = np.ascontiguousarray(etas, dtype=np.float64)
        self._check(self.lib.mz_learner_train_multi_dev(self.h, B, step0, e.size,
                                                        e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                        losses_ptr, theta_ptr, stream), "mz_learner_train_multi_dev")

    # ---- data-parallel learner over RCCL through the C ABI
    @staticmethod
    def dp_unique_id():
        """128-byte RCCL id (rank 0; hand it to every rank out of band)."""
        lib = load_library()
        buf = (ctypes.c_uint8 * 128)()
        if lib.mz_dp_unique_id(buf) != 0:
            raise MzError("mz_dp_unique_id failed (librccl.so.1)")
        return bytes(buf)

    def dp_init(self, rank, world, uid):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.mz_dp_init(self.h, rank, world, buf), "mz_dp_init")

    def dp_allreduce(self, grad_ptr=None, stream=None):
        self._check(self.lib.mz_dp_allreduce(self.h, grad_ptr, stream), "mz_dp_allreduce")

    def learner_train_dp(self, B, step, eta, losses_ptr=None, stream=None):
        """grad_sampled_dev + RCCL all-reduce + apply(1/world) in one call."""
        self._check(self.lib.mz_learner_train_dp(self.h, B, step, float(eta), losses_ptr, stream),
                    "mz_learner_train_dp")

    def batch_to_host(self, b):
        """Copy a device MzBatch (from replay_sample) into the host dict layout of ReplayBuffer.get_batch."""
        B, K1, A = b.batch_size, self.conf.num_unroll_steps + 1, self.A
        self.sync()
        out = {}
        for name, shape in (("observation", (B, self.obs_feat)), ("actions", (B, K1)), ("target_values", (B, K1)),
                            ("target_rewards", (B, K1)), ("target_policies", (B, K1, A)), ("gradient_scale", (B,))):
            a = np.empty(shape, np.float32)
            _copy_d2h(a, getattr(b, name))
            out[name] = a
        if b.weights:                                   # PER importance weights
            a = np.empty(B, np.float32)
            _copy_d2h(a, b.weights)
            out["weights"] = a
        return out

    def replay_update_priorities(self, stream=None):
        """PER update_priorities! of the last sampled batch from the last unroll's values."""
        self._check(self.lib.mz_replay_update_priorities(self.h, stream), "mz_replay_update_priorities")

    def replay_get_priorities(self, i):
        """(priorities (T,), game priority) of shard game i (0 = oldest held)."""
        T = self.replay_get_game(i).as_arrays()["action"].shape[0]
        pr = np.zeros(T, np.float32)
        gp = np.zeros(1, np.float32)
        self._check(self.lib.mz_replay_get_priorities(self.h, i, _p(pr), _p(gp)), "mz_replay_get_priorities")
        return pr, float(gp[0])

    # ---- Reanalyse (ReplayBuffer.jl:8, 56-67) on the device shard
    def replay_reanalyse(self, first=0, count=-1, stream=None):
        """reanalysed_predicted_root_values of shard games first .. first+count-1 (0 = oldest held,
        count < 0 = all held) from the current weights; stream-ordered, no host synchronisation.
        Targets sampled afterwards bootstrap from them."""
        self._check(self.lib.mz_replay_reanalyse(self.h, first, count, stream), "mz_replay_reanalyse")

    def replay_clear_reanalysed(self, stream=None):
        """Every held game back to `nothing` (targets bootstrap from root_values again)."""
        self._check(self.lib.mz_replay_clear_reanalysed(self.h, stream), "mz_replay_clear_reanalysed")

    def replay_reanalysed_count(self):
        """num_reanalysed_games: one per game per replay_reanalyse since selfplay_init."""
        n = ctypes.c_int64()
        self._check(self.lib.mz_replay_reanalysed_count(self.h, ctypes.byref(n)), "mz_replay_reanalysed_count")
        return int(n.value)

    def replay_get_reanalysed(self, i):
        """Shard game i (0 = oldest held): its reanalysed values (T,) float32, or None if `nothing`."""
        v = np.zeros(self.conf.max_moves + 1, np.float32)
        s = ctypes.c_int32()
        self._check(self.lib.mz_replay_get_reanalysed(self.h, i, ctypes.byref(s), _p(v)), "mz_replay_get_reanalysed")
        if not s.value:
            return None
        return v[:len(self.replay_get_game(i).action_history)].copy()

    def replay_reanalyse_search(self, first=0, count=-1, exploration=False, rng_step=0, game_offset=0, stream=None):
        """The stored positions of shard games first .. first+count-1 searched again with the current
        networks (position pos of selected game gi as mcts_search's game with Philox id
        game_offset + gi*(max_moves+1) + pos); stream-ordered, no host synchronisation.  Targets sampled
        afterwards take their policies from the new child_visits and bootstrap from the new root values."""
        self._check(self.lib.mz_replay_reanalyse_search(self.h, first, count, int(exploration),
                                                        rng_step & 0xffffffff, game_offset & 0xffffffff, stream),
                    "mz_replay_reanalyse_search")

    def replay_get_reanalysed_policies(self, i):
        """Shard game i (0 = oldest held): its reanalysed child_visits (T, A) float32, or None if unset."""
        cv = np.zeros((self.conf.max_moves + 1, self.A), np.float32)
        s = ctypes.c_int32()
        self._check(self.lib.mz_replay_get_reanalysed_policies(self.h, i, ctypes.byref(s), _p(cv)),
                    "mz_replay_get_reanalysed_policies")
        if not s.value:
            return None
        return cv[:len(self.replay_get_game(i).action_history)].copy()

    def replay_reanalyse_next(self, mode, exploration=False, rng_step=0, game_offset=0, stream=None):
        """One round of the Reanalyse worker: the device takes whole games from the shard's cursor while
        their stored positions fit the round (max_games rows with REAN_BY_SEARCH, 4096 with REAN_BY_VALUE)
        and reanalyses exactly those positions; stream-ordered, no host synchronisation.  Search mode: row i
        of the round as mcts_search's game with Philox id game_offset + i of a max_games batch."""
        self._check(self.lib.mz_replay_reanalyse_next(self.h, mode, int(exploration), rng_step & 0xffffffff,
                                                      game_offset & 0xffffffff, stream),
                    "mz_replay_reanalyse_next")

    def replay_reanalyse_cursor(self):
        """(the next game number to reanalyse, (first game number, games, rows) of the last round); synchronises."""
        c = ctypes.c_int64()
        r = np.zeros(3, np.int64)
        self._check(self.lib.mz_replay_reanalyse_cursor(self.h, ctypes.byref(c), _p(r)), "mz_replay_reanalyse_cursor")
        return int(c.value), tuple(int(x) for x in r)

    def replay_reanalyse_seek(self, game_number, stream=None):
        """Stream-ordered: the cursor := game_number (any value; the next round normalises it)."""
        self._check(self.lib.mz_replay_reanalyse_seek(self.h, int(game_number), stream), "mz_replay_reanalyse_seek")

    def selfplay_slots(self):
        G = self.sp_G
        ln = np.zeros(G, np.int32)
        board = np.zeros((G, self.osz), np.uint8)
        pl = np.zeros(G, np.int32)
        self._check(self.lib.mz_selfplay_slots(self.h, _p(ln), _p(board), _p(pl)), "mz_selfplay_slots")
        return ln, board, pl

    # ---- checkpoints
    def checkpoint_save(self, path, training_step):
        self._check(self.lib.mz_checkpoint_save(self.h, os.fsencode(path), int(training_step)), "mz_checkpoint_save")

    def checkpoint_load(self, path):
        """Restores weights + ADAM state; returns the checkpoint's training step."""
        step = ctypes.c_int64()
        self._check(self.lib.mz_checkpoint_load(self.h, os.fsencode(path), ctypes.byref(step)), "mz_checkpoint_load")
        return step.value

    # ---- snapshots: the shard, the games in progress and the train loop as well
    def snapshot_save(self, path, training_step):
        self._check(self.lib.mz_snapshot_save(self.h, os.fsencode(path), int(training_step)), "mz_snapshot_save")

    def snapshot_load(self, path):
        """Exact resume: replaces the learner, the shard, the slots and the train loop with the file's
        (a refused file leaves the engine as it was); returns the snapshot's training step."""
        from . import checkpoint as ck
        step = ctypes.c_int64()
        self._check(self.lib.mz_snapshot_load(self.h, os.fsencode(path), ctypes.byref(step)), "mz_snapshot_load")
        meta = ck.read_metadata(path)                  # the shard geometry the read-outs use
        self.sp_G, self.osz = int(meta["G"]), int(meta["osz"])
        return step.value

    def search_variant(self):
        return self.lib.mz_search_variant(self.h).decode()

    def learner_variant(self):
        return self.lib.mz_learner_variant(self.h).decode()

    def resnet_tile_games(self):
        """Games per tile of the ResNet network kernels (0 for the FC nets)."""
        return self.lib.mz_resnet_tile_games(self.h)

    def downsample_staged(self):
        """1 / 0: the downsampler stages the observation in LDS or reads it from HBM; -1 without one."""
        return self.lib.mz_downsample_staged(self.h)

    def sync(self):
        self._check(self.lib.mz_sync(self.h), "mz_sync")
