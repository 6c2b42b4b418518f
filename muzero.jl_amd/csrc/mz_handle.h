// mz_handle.h — what the host files of libmz share: the handle (one engine, one GPU), the
// layer / plan description types it holds, the error and allocation helpers, and the prototypes
// of the helpers that one host file defines and another calls.  Host only: no kernel file
// includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "mz_internal.h"
#include "mz_small_params.h"
#include "mz_resnet_params.h"
#include "mz_backprop_params.h"
#include "mz_selfplay_params.h"

static const size_t kLdsMax = 160 * 1024;   // LDS per workgroup on gfx950

// The FC layer / plan description (hidden, like the helpers below: no inline member becomes an export)
#pragma GCC visibility push(hidden)
enum { CH_TRUNK = 0, CH_HEAD1 = 1, CH_HEAD2 = 2 };

struct LayerSpec {
    int net, chain, in, out, act;
    size_t flux_w, flux_b;     // offsets in the global flat parameter vector
    int bn = 0;                // make_dense with use_batch_norm: BatchNorm β at flux_be, γ at flux_be + out
    size_t flux_be = 0;
    int nq, n_ob;
    int packed_w, packed_b;    // offsets in the packed images
};

struct PlanBuild {
    std::vector<std::vector<std::pair<int, int>>> stages;
    std::vector<LayerDesc> layers;
    void ensure(int n) { if ((int)stages.size() < n) stages.resize(n); }
    std::vector<int> image() const {
        std::vector<int> v;
        int nt = 0;
        for (auto& s : stages) nt += (int)s.size();
        v.push_back((int)stages.size()); v.push_back((int)layers.size()); v.push_back(nt);
        int acc = 0;
        for (auto& s : stages) { v.push_back(acc); acc += (int)s.size(); }
        v.push_back(acc);
        for (auto& s : stages) for (auto& t : s) { v.push_back(t.first); v.push_back(t.second); }
        for (auto& L : layers) {
            const int* p = reinterpret_cast<const int*>(&L);
            for (size_t i = 0; i < sizeof(LayerDesc) / sizeof(int); ++i) v.push_back(p[i]);
        }
        return v;
    }
};
#pragma GCC visibility pop

struct RSpec {
    int chain, conv, cin, cout, kw, kh, act, bn, res_save, res_add;
    size_t woff, boff, bnoff;               // local to the net
};

struct mz_handle {
    // ---- the engine: configuration, device, stream, error text, allocation lists (mz_engine.hip)
    mz_config conf;
    mz_ffhp hp;
    int kind = 0;                           // 0 FeedForwardHP, 1 ResNetHP
    mz_resnet_hp rhp{};
    int device = 0, max_games = 0;
    uint64_t seed = 0;
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t sync_stream = nullptr; bool sync_narrow = false;   // mz_set_sync_stream
    std::vector<void*> sp_allocs;
    std::vector<void*> allocs;
    // ---- FC networks: layer specs, plans, weight images, ADAM's inverse image maps (mz_engine.hip)
    std::vector<LayerSpec> layers;
    std::vector<int> chains[3][3];          // [net][chain] -> layer indices
    size_t nparams[3] = {0, 0, 0}, flat_off[3] = {0, 0, 0}, nflat = 0;
    size_t packed_w_n = 0, packed_b_n = 0;
    int obs_feat = 0, plane = 0, H = 0, A = 0, S = 0;
    ActLayout lay{};
    int chain_buf[3][3][2];                 // LDS ping-pong buffers per chain
    float* d_flat = nullptr; float* d_Wp = nullptr; float* d_Bp = nullptr;
    int* d_srcW = nullptr; int* d_srcB = nullptr;
    int* d_plan[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // repr, pred, dyn, root, sim
    int* d_plan_sim_res = nullptr;          // register-resident image of the sim plan (or null)
    double* d_pbc = nullptr; double* d_sqrt = nullptr; float* d_aval = nullptr;
    double* d_pbterm = nullptr;             // pbc(Np) * (sqrt(Np) / (Nc + 1)), triangle
    // inverse image maps, one code per flat parameter: >= 0 position in the
    // weight image, <= -2 position -code-2 in the bias image, -1 none.  ADAM
    // scatters every update into the images through them (no repack).
    std::vector<int> inv_tile, inv_small;
    int* d_inv_tile = nullptr; int* d_inv_small = nullptr;
    // ---- search: trees, io buffers, kernel choice, the small-batch kernel's schedule (mz_engine.hip)
    char* d_tree = nullptr; size_t tree_game_bytes = 0; bool lds_tree = false; int dump_tree = 0;
    bool use_res = false;                   // register-resident sim-plan kernel
    // small-batch kernel (mz_small.hip): schedule images + LDS layout
    bool small_ok = false;
    int n_cu = 256;
    int sm_n_sim = 0, sm_n_root = 0;
    float* d_sm_w = nullptr;                // [n_sim + n_root][2][256][16] weight image (sim then root)
    float* d_sm_bias = nullptr;             // [n_sim + n_root][2][64]
    // FC engines: a second image set (tile16 W/B, small W/bias) that the one-launch
    // learner step (mz_learn_small*) writes while its unroll reads the current set;
    // the host swaps the sets after the launch
    float* d_Wp2 = nullptr; float* d_Bp2 = nullptr; float* d_sm_w2 = nullptr; float* d_sm_bias2 = nullptr;
    int* d_sm_srcw = nullptr; int* d_sm_srcb = nullptr;
    size_t sm_w_n = 0, sm_b_n = 0;
    int* d_sm_rec[3] = {nullptr, nullptr, nullptr};   // per T in {1,2,4}
    int sm_lay[3][8];                       // per T: act_total, x_rep, x_pred, x_dyn, h_out, v_out, p_out, r_out
    size_t sm_lds[3] = {0, 0, 0};
    std::vector<uint32_t> sm_nzm;           // nonzero-chunk masks of the register images (SM_NZM_N)
    bool sm_bn = false;                     // BatchNorm FC layers: the bias image carries γ, β sections
    float* d_zero16 = nullptr;              // 64 zero bytes (sm_load's skipped chunks)
    int force_kernel = 0;                   // 0 auto, 1 tile16, 2 small
    std::string last_variant = "none";
    std::string last_lvariant = "none";     // the learner unroll's kernels (mz_learner_variant)
    int force_T = 0;                        // MZ_SMALL_T=1|2|4 (tests)
    float* d_hid = nullptr;
    float* d_obs = nullptr; uint8_t* d_legal = nullptr; int32_t* d_tp = nullptr;
    float* d_cv = nullptr; float* d_rv = nullptr; int32_t* d_act = nullptr;
    // ---- device fault word, debug switches and timing events (mz_engine.hip)
    unsigned* d_fault = nullptr;            // device fault word (MZ_FAULT_*), checked at host synchronisation
    int dbg_skip = -1;                      // debug: the hand-off producer that skips its publish
    unsigned long long poll_ticks = MZ_POLL_TICKS;
    int time_nets = 0;                      // mz_debug_enable flag 2: events around each ResNet nets launch
    int time_unroll = 0;                    // flag 4: events around each ResNet learner unroll launch
                                            // (and each mz_learn_multi* launch)
    std::vector<hipEvent_t> tev; size_t tev_used = 0;
    unsigned long long* d_stamps = nullptr;
    int32_t* d_sel_stats = nullptr;         // mz_debug_enable flag 1: [max_games][2] select counters of the small kernel
    // ---- ResNet engine: downsampler, plans, search buffers (mz_engine_resnet.hip)
    // ResNet config of the networks after the downsampler (= conf without
    // one): observation_shape = the representation tail's input board and
    // channels, stacked_observations = 0 (ResNetHP.downsample, configs[4])
    mz_config rconf{};
    int ds = 0;                             // downsampler (mz_downsample.hip) on
    DsPlan dsplan{};
    DsPlan* d_dsplan = nullptr;
    size_t ds_lds = 0, ds_n = 0;            // its LDS bytes, its parameter count (first in the repr net)
    int rin_feat = 0;                       // representation tail input features (obs_feat without downsampler)
    float* d_dsout = nullptr;               // [max_games][rin_feat] search roots' downsampled observations
    float* d_dsb = nullptr; int dsb_cap = 0;   // [cap][rin_feat] scratch: learner batches, net_forward
    // ResNet networks (mz_resnet.hip): host plans, device copies, tile width
    std::vector<RPlan> rplan;               // [3]
    RPlan* d_rplan = nullptr;               // [3]
    int rn_ng = 0;
    // the learner unroll's chain (mz_runroll_chain1 / _chain_r): the same nets on narrow (one-sample) tiles
    std::vector<RPlan> rplan_l;
    RPlan* d_rplan_l = nullptr;
    size_t rn_lds_l = 0;
    size_t rn_lds[3] = {0, 0, 0};
    float bn_s = 1.0f;
    int* d_rpath = nullptr; int* d_rgst = nullptr;          // ResNet search: [G][2(S+2)], [G][RG_INTS]
    uint2* d_rcache = nullptr; int* d_rnN = nullptr;        // [G][S+1]: the LDS tree step's cached select
    int* d_rhk = nullptr; float* d_rov = nullptr; float* d_rologit = nullptr; float* d_ror = nullptr;
    int rn_dyn_split = 0;                   // first reward-head layer of the dynamics plan
    bool rd_chain = false;                  // the chain runs as mz_runroll_chain_r (rd_chain_ok)
    bool rp_pred = false;                   // one-item predictions run as mz_runroll_pred_r (rp_pred_ok)
    float* d_rtrunk = nullptr;              // [max_games][H] dynamics trunk outputs (mz_rsearch_nets)
    unsigned long long* d_tprog = nullptr;  // [tiles] their publish words
    unsigned long long tprog_epoch = 0;     // mz_rsearch_nets launches
    std::vector<int> rtab;                  // offset tables of the narrow (chain) plans
    int* d_rtab = nullptr;
    size_t rtree_lds = 0;                                    // LDS of the LDS-cached ResNet tree step (0 = HBM kernel)
    // ---- learner: ADAM state, batches, unroll scratch, RCCL, prefetch, multi-step banks (mz_learner_host.hip)
    float* d_m = nullptr; float* d_v = nullptr; float* d_grad = nullptr;
    double bp1 = 0.9, bp2 = 0.999;
    int bcap = 0;
    float *d_bobs = nullptr, *d_bact = nullptr, *d_btv = nullptr, *d_btr = nullptr, *d_btp = nullptr,
          *d_bgs = nullptr, *d_pv = nullptr, *d_pp = nullptr, *d_pr = nullptr, *d_loss = nullptr;
    double* d_sq = nullptr;                 // [3][MZ_L2_BLOCKS] partial Σθ²
    size_t* d_netoff = nullptr;             // [3] flat offset, [3] count per net
    unsigned* d_counter = nullptr;          // last-block counter of mz_learner_grad_kernel
    float* d_lterm = nullptr;               // [2][B(K+1)] loss terms
    float* d_bw = nullptr;                                   // host batch PER weights (mz_learner_step)
    float* d_rhs = nullptr;                 // [bcap][K][H] learner unroll scratch (h between the nets)
    float* d_rts = nullptr;                 // [bcap][K][H] dynamics trunk outputs (the reward heads' input)
    unsigned long long* d_prog = nullptr;   // [bcap] mz_runroll_fused_r progress words
    unsigned long long prog_epoch = 0;      // launches of mz_runroll_fused_r (prog_base = epoch · 64)
    void* dp_comm = nullptr; int dp_world = 0, dp_rank = 0;  // mz_dp_init: RCCL communicator
    float* d_dp_cnt = nullptr;              // mz_train_run at world > 1: the finished-game count exchange
    // get_batch one step ahead (the one-launch FC learner, PER off): the launch
    // for step t also samples step t+1's batch into the other batch set and
    // stamps that set's header {epoch, games played, step, B}; the next launch
    // uses a set only if its header still matches (the same shard state — a
    // stored game bumps `played` — step and B), else it samples in place.
    // Anything else that fills set 0 or re-creates the shard bumps the epoch.
    float *d_rs2_obs = nullptr, *d_rs2_act = nullptr, *d_rs2_tv = nullptr, *d_rs2_tr = nullptr,
          *d_rs2_tp = nullptr, *d_rs2_gs = nullptr;
    int32_t* d_rs2_index = nullptr;
    int pf_cap = 0, pf_cur = 0;
    long long* d_pf_hdr = nullptr;          // [2][4]
    long long pf_epoch = 1;
    // L learner steps per launch pair (mz_learner_train_multi_dev, ChainParams): the bank of
    // MZ_MULTI_MAX small-kernel images (θ_t .. θ_{t+L-1}), per-step batches, read-outs,
    // loss terms, Σθ² partials, fold counters and losses, for batches up to ml_cap
    float* d_bank_w = nullptr; float* d_bank_b = nullptr;
    // ResNet nets: the MFMA image bank (W, B), the flat-parameter bank, per-step unroll scratch (h, trunk
    // outputs), progress words and downsampled batches
    float* d_tbank_w = nullptr; float* d_tbank_b = nullptr; float* d_fbank = nullptr;
    float* d_ml_hs = nullptr; float* d_ml_ts = nullptr; float* d_ml_dsb = nullptr;
    unsigned long long* d_ml_prog = nullptr;
    unsigned long long ml_prog_epoch = 0;   // multi-step fused launches (d_ml_prog's prog_base = epoch · 64)
    int ml_cap = 0, ml_cap_L = 0, ml_last_B = 0, ml_last_L = 0, ml_last_R = 0;   // (ring: ensure_multi)
    float *d_ml_obs = nullptr, *d_ml_act = nullptr, *d_ml_tv = nullptr, *d_ml_tr = nullptr, *d_ml_tp = nullptr,
          *d_ml_gs = nullptr, *d_ml_pv = nullptr, *d_ml_pp = nullptr, *d_ml_pr = nullptr, *d_ml_terms = nullptr,
          *d_ml_out = nullptr;
    int32_t* d_ml_index = nullptr;
    double* d_ml_part = nullptr;
    unsigned* d_ml_cnt = nullptr;
    float* d_chx = nullptr;                 // [MZ_MULTI_MAX][hx_n] mz_learn_chain helpers' θ (ChainParams::hx)
    unsigned long long* d_chcnt = nullptr;  // [3·MZ_L2_BLOCKS] their slots' arrival counters
    // ---- corrected-gradient learner: the unrolled graph and its arenas (mz_backprop_host.hip)
    int learn_mode = MZ_LEARN_REF_SEMANTICS;
    bool bp_built = false;
    // the corrected learner for the ResNet nets (mz_rbp_sample / mz_rbp_dw)
    bool rbp_built = false;
    int rbp_n_app = 0, rbp_n_head = 0, rbp_arena = 0, rbp_obs_t = 0, rbp_dt = 0, rbp_xs = 0, rbp_n_job = 0, rbp_cap = 0;
    int rbp_ring = 0;                      // forward / backward LDS ring slots of mz_rbp_sample
    int2* d_rbp_gzero = nullptr; int rbp_n_gzero = 0;
    int rbp_threads = 256;
    int rbp_job0[4] = {0, 0, 0, 0};
    RbpApp* d_rbp_apps = nullptr; BpHead* d_rbp_heads = nullptr;
    RbpLayer* d_rbp_layers = nullptr; RbpUse* d_rbp_uses = nullptr; RbpJob* d_rbp_jobs = nullptr;
    float* d_rbp_act = nullptr; float* d_rbp_grad = nullptr;
    float* d_rbp_terms = nullptr; double* d_rbp_sq = nullptr;
    // ... through the downsampler (mz_dsbp_*): per-sample arenas, one dW job per conv output channel
    int dsbp_arena = 0, dsbp_dt = 0, dsbp_n_job = 0, dsbp_cap = 0;
    DsBpLayer* d_dsbp_lay = nullptr; DsDwJob* d_dsbp_jobs = nullptr;
    float* d_dsbp_act = nullptr; float* d_dsbp_grad = nullptr;
    int bp_n_app = 0, bp_n_head = 0, bp_n_job = 0, bp_tile_floats = 0, bp_obs_t = 0, bp_tiles_cap = 0;
    BpApp* d_bp_apps = nullptr; BpHead* d_bp_heads = nullptr; BpLayer* d_bp_layers = nullptr;
    BpUse* d_bp_uses = nullptr; BpJob* d_bp_jobs = nullptr;
    int2* d_bp_funits = nullptr; int* d_bp_flev = nullptr; int2* d_bp_bunits = nullptr; int* d_bp_blev = nullptr;
    int bp_n_flev = 0, bp_n_blev = 0, bp_n_funit = 0, bp_n_bunit = 0;
    int* d_bp_fsync = nullptr; int* d_bp_bsync = nullptr; int bp_cache_floats = 0, bp_obs_s = -1;
    // mz_debug_bp_plan: the cache's slots, the kernel's dynamic LDS, and what the plan leaves to the arena
    int bp_slot_floats = 0, bp_nslot = 0, bp_lds_bytes = 0, bp_plan[5] = {0, 0, 0, 0, 0};
    double* d_bp_sq = nullptr; int bp_job0[4] = {0, 0, 0, 0};
    float* d_bp_act = nullptr; float* d_bp_grad = nullptr; float* d_bp_terms = nullptr;
    // ---- self-play slots, opponents, the test worker (mz_selfplay_host.hip)
    // device self-play + replay shard (mz_selfplay.hip); own allocation list (re-init frees it)
    int sp_env = -1, sp_G = 0, sp_T = 0, sp_osz = 0, sp_cap = 0;
    uint8_t* d_sp_board = nullptr; int32_t* d_sp_player = nullptr; uint8_t* d_sp_over = nullptr;
    uint32_t* d_sp_ekey = nullptr; int sp_frames = 0;
    SpHist sp_hist{}, sp_ring{};
    long long* d_sp_counters = nullptr;
    int32_t* d_sp_done = nullptr; int32_t* d_sp_rpos = nullptr;
    float* d_sp_temp = nullptr;             // [G] per-slot temperatures (temperature_threshold)
    float* d_sp_tgame = nullptr;            // [G] each game's own temperature (mz_train_run)
    bool sp_latch = false;                  // mz_selfplay_move latches temperatures per game
    bool sp_has_games = false;              // the FIFO never empties once a game is in
    bool sp_reset_pending = false;          // Atari-like env: the initial games start at the first move
    float* d_sp_dpow = nullptr;
    int sp_eval = 0, sp_opp = MZ_OPP_SELF, sp_mzp = 1;    // mz_selfplay_mode
    int sp_expert_depth = 0;                              // mz_expert_depth (0: the env's default)
    int sp_mcts_sims = 0, sp_mcts_rollouts = 0;           // mz_mcts_opponent (0: the defaults)
    double* d_mcts_sqrt = nullptr;                        // [MZM_MAX_SIMS + 1] sqrt(k) (the first MZ_OPP_MCTS use)
    // the network-only player (mz_eval_players): the kinds of MuZero's and the other side's rows,
    // and on ResNet engines the two forward launches' outputs [max_games][H | 1 | A] (mz_engine_create_resnet)
    int ev_kind[2] = {MZ_PLAYER_SEARCH, MZ_PLAYER_SEARCH};
    float* d_pr_h = nullptr; float* d_pr_v = nullptr; float* d_pr_p = nullptr;
    // the solved TicTacToe table (mz_expert_table): the handle's, built by the first on = 1
    bool xtable_on = false;
    int8_t* d_xtable = nullptr;                           // [MZX_TTT_CODES][MZX_TTT_ENTRY]
    long long* d_eval = nullptr;                          // [4] evaluation tally
    // the test worker (mz_test_*).  Handle settings: mz_test_config, mz_train_set_test.
    // The record ring stays with the handle (allocated by the first mz_test_play); the test slots
    // are self-play state (in sp_allocs, allocated by the first mz_test_play after a re-init).
    int test_E = 0, test_opp = MZ_OPP_SELF, test_mzp = 1;
    int64_t test_interval = 0; uint32_t test_goff = 0; float test_temp = 0.0f;
    long long* d_test_counts = nullptr;                   // [MZ_TEST_RECORDS][8]
    double* d_test_sums = nullptr;                        // [MZ_TEST_RECORDS][3]
    int64_t test_total = 0;                               // evaluations since create / mz_test_clear
    // judging (mz_test_audit): the audit ring beside the records, allocated by the first
    // evaluation that judges; which rows hold an audit is host bookkeeping
    bool test_audit = false;
    long long* d_test_audit = nullptr;                    // [MZ_TEST_RECORDS][4]
    std::vector<uint8_t> test_audited = std::vector<uint8_t>(MZ_TEST_RECORDS, 0);
    struct TestSlots {
        int E = 0;                                        // 0: not allocated
        bool played = false;                              // an evaluation's games are in `hist`
        uint8_t* board = nullptr; int32_t* player = nullptr; uint8_t* over = nullptr; uint32_t* ekey = nullptr;
        SpHist hist{};
        int32_t* done = nullptr; int32_t* frozen = nullptr; float* temp = nullptr;
        float* cv2 = nullptr; float* rv2 = nullptr; int32_t* act2 = nullptr;   // MZ_OPP_NETWORK's second outputs
    } ts;
    // ---- replay shard: sampler batches, PER, symmetry, Reanalyse (mz_replay_host.hip)
    float *d_rs_obs = nullptr, *d_rs_act = nullptr, *d_rs_tv = nullptr, *d_rs_tr = nullptr, *d_rs_tp = nullptr,
          *d_rs_gs = nullptr;
    int32_t* d_rs_index = nullptr;
    int rs_cap = 0;
    float* d_rs_w = nullptr; float* d_per_cum = nullptr; float* d_per_p = nullptr;   // PER sampling
    long long* d_per_total = nullptr;
    int rs_last_B = 0;                                       // batch size of the last get_batch
    // board symmetry (mz_replay_set_symmetry): the setting is the handle's; the tables of
    // the env's group are self-play state (built by mz_selfplay_init for a board env, behind the
    // discount powers in d_sp_dpow's buffer): [sym_n][plane] cells, then [sym_n][A] actions
    bool sym_on = false;
    int sym_n = 0;
    int32_t* d_sym = nullptr;
    // mz_replay_reanalyse on ResNet engines: staging of one chunk (in sp_allocs)
    float *d_rn_x = nullptr, *d_rn_h = nullptr, *d_rn_v = nullptr, *d_rn_p = nullptr;
    int rn_cap = 0;
    size_t rean_lds = 0;                    // mz_reanalyse_fc's dynamic-LDS attribute
    // mz_replay_reanalyse_search: the io of one batched search of max_games rows (in sp_allocs,
    // allocated with sp_ring.rcv at the first call that has work)
    float *d_rq_obs = nullptr, *d_rq_cv = nullptr, *d_rq_rv = nullptr;
    uint8_t* d_rq_legal = nullptr;
    int32_t *d_rq_tp = nullptr, *d_rq_act = nullptr, *d_rq_state = nullptr;
    // mz_replay_reanalyse_next: the round's packed (slot, pos) rows (in sp_allocs), and
    // mz_train_set_reanalyse's rounds inside mz_train_run
    int32_t* d_rean_rows = nullptr;
    int rean_rows_cap = 0;
    int tr_rean_mode = 0, tr_rean_rounds = 0, tr_rean_expl = 0;
    // ---- actor-learner loop, the opponent's weight set, the run log (mz_train_host.hip)
    std::string tr_ckpt_path;               // mz_train_set_networks_path: periodic checkpoints
    // actor–learner loop (mz_train_*): the actors' weight set (flat + the
    // search images), the queued nets (remote_NNs, flat), the learner step t
    struct WSet { float* flat = nullptr; float* Wp = nullptr; float* Bp = nullptr; float* smw = nullptr;
                  float* smb = nullptr; };
    WSet tr_actor;
    // MZ_OPP_NETWORK: the opponent's weight set, a handle setting allocated by the
    // first mz_opponent_* call that fills it; opp_have = the nets given so far (bit per net, 7 =
    // complete); the opponent search's outputs (in sp_allocs, allocated when the mode is first used)
    WSet opp;
    unsigned opp_have = 0;
    float* d_cv2 = nullptr; float* d_rv2 = nullptr; int32_t* d_act2 = nullptr;
    float* d_tr_queued = nullptr;
    int tr_B = 0;
    int64_t tr_t = 0, tr_games = 0, tr_refresh = 0;
    long long* h_tr_cnt = nullptr;          // pinned: num_played_games read back once per move
    long long* h_tr_pub = nullptr;          // coherent pinned: mz_tr_publish's {count, fault, sequence}
    long long tr_pub_seq = 0;
    // the run log (mz_train_set_log).  The interval is a handle setting; the accumulators,
    // the chunk's loss rows and the record ring are the handle's, allocated by the first interval > 0
    int64_t log_interval = 0;
    LogAcc* d_log_acc = nullptr;
    float* d_log_rows = nullptr;                          // [MZ_MULTI_LMAX][8]
    long long* d_log_counts = nullptr;                    // [MZ_LOG_RECORDS][16]
    double* d_log_sums = nullptr;                         // [MZ_LOG_RECORDS][16]
    int64_t log_total = 0;                                // records since create / mz_train_log_clear
};

// θ after up to two given steps, copied out by the chain launch that computes them (mz_train_run:
// the actors' and the queued sets at refresh steps inside one learner chunk)
struct MultiCap {
    int64_t t[2];                                   // absolute learner steps (< 0: none)
    float* dst[2];                                  // nflat floats each
    const mz_handle::WSet* img0;                    // NULL or set 0's search images, written by the chain too
    bool* imaged0;                                  // set when a chain launch wrote them
};

// Hidden from here on: the helpers are inline or cross-file, none of them an export of libmz.so.
#pragma GCC visibility push(hidden)

#define MZ_TRY(h, expr)                                                                  \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                \
            return -1;                                                                   \
        }                                                                                \
    } while (0)

inline int fail(mz_handle* h, const std::string& m) { h->err = m; return -2; }
// the stream of a `_dev` call: the caller's, or the handle's own
inline hipStream_t stream_of(const mz_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->stream; }

// Host-synchronous entry points (weights, state, replay read-outs, debug
// copies) wait for ALL of this process's work on the device, not only the
// handle's stream: `_dev` calls may have queued work on a caller stream
// (torch's, created non-blocking like the handle's), which a blocking
// hipMemcpy would not wait for.  A caller that orders its own
// work narrows the wait to one named stream plus the handle's own with
// mz_set_sync_stream, so unrelated device work is not waited for.
inline hipError_t sync_device(mz_handle* h) {
    if (!h->sync_narrow) return hipDeviceSynchronize();
    hipError_t e = hipStreamSynchronize(h->sync_stream);
    return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

// After a synchronisation: a kernel that gave up on a cross-workgroup publish
// (mz_poll_ge) left bits in d_fault; report them once (the word is cleared)
// as this call's error.  The outputs of the launches since the last check
// are then not to be trusted.
inline int check_fault(mz_handle* h) {
    if (!h->d_fault) return 0;
    unsigned v = 0;
    MZ_TRY(h, hipMemcpy(&v, h->d_fault, 4, hipMemcpyDeviceToHost));
    if (!v) return 0;
    MZ_TRY(h, hipMemset(h->d_fault, 0, 4));
    char wait[32];
    std::snprintf(wait, sizeof(wait), "%.3g s", (double)h->poll_ticks / 1e8);   // the 100 MHz constant clock
    std::string m = std::string("device fault: a workgroup waited ") + wait + " for a publish that never came (";
    if (v & MZ_FAULT_RS_TRUNK) m += "mz_rsearch_nets trunk hand-off ";
    if (v & MZ_FAULT_RD_PROGRESS) m += "mz_runroll_fused_r chain progress ";
    h->err = m + "); the results of the launches since the last synchronisation are invalid (search results, "
                 "games self-play stored from them, losses, read-outs; the ref_semantics weights and ADAM state "
                 "do not read them and stay valid)";
    return -1;
}

// every host-synchronous call: wait (sync_device), then report a device fault
#define MZ_SYNC(h)                                    \
    do {                                              \
        MZ_TRY(h, sync_device(h));                    \
        if (check_fault(h)) return -1;                \
    } while (0)

template <typename T>
inline hipError_t dalloc(mz_handle* h, T** p, size_t n) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T) + 16);
    if (e == hipSuccess) h->allocs.push_back(*p);
    return e;
}
// free one dalloc'd buffer before the handle is destroyed (the caller has drained the work using it)
inline hipError_t dfree(mz_handle* h, void* p) {
    auto it = std::find(h->allocs.begin(), h->allocs.end(), p);
    if (it == h->allocs.end()) return hipErrorInvalidValue;
    h->allocs.erase(it);
    return hipFree(p);
}

template <typename T>
inline hipError_t spalloc(mz_handle* h, T** p, size_t n, bool zero = true) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T) + 16);
    if (e == hipSuccess) {
        h->sp_allocs.push_back(*p);
        if (zero) e = hipMemset(*p, 0, n * sizeof(T) + 16);
    }
    return e;
}

// mz_engine_create / mz_engine_create_resnet: the first failing step ends the call (rc, h in scope)
#define CK(x) do { if ((rc = (x)) != 0) { g_create_error = h->err; mz_engine_destroy(h); return rc; } } while (0)

extern thread_local std::string g_create_error;    // mz_create_error's text (mz_engine.hip)

// Helpers that one host file defines and another calls (the rest stay static in their file).
namespace mz {

// mz_engine.hip
int repack(mz_handle* h, hipStream_t st = nullptr);
size_t tree_game_bytes(int S, int A);
int ensure_batch(mz_handle* h, int B);
SpParams sp_params(mz_handle* h, bool test = false);
int learner_multi(mz_handle* h, int32_t B, uint32_t step0, int32_t L, const double* eta, float* losses_dev,
                  float* theta_dev, hipStream_t st, float* out_last = nullptr, const MultiCap* cap = nullptr);
ReanParams rean_params(mz_handle* h);
int rean_search_io(mz_handle* h, ReanParams& Q);
int rean_next_check(mz_handle* h, int mode);
int dp_sum_count(mz_handle* h, int64_t* v, hipStream_t st);
// mz_engine_resnet.hip
std::vector<RSpec> rn_specs(const mz_config& c, const mz_resnet_hp& hp, int net, size_t* nparams);
size_t rd_chain_lds(const mz_handle* h);
size_t rp_pred_lds(const mz_handle* h);
int alloc_learner(mz_handle* h);
size_t rsearch_root_lds(const mz_handle* h);
size_t fbank_stride(const mz_handle* h);
int ds_launch(mz_handle* h, const float* x, float* y, int n, hipStream_t st, const float* flat = nullptr,
              int per_step = 0);
int ensure_dsb(mz_handle* h, int n);
size_t rsearch_nets_lds(const mz_handle* h);
// mz_backprop_host.hip
int bp_grad(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st);
// mz_train_host.hip
int log_rebase(mz_handle* h, long long played);
void wset_swap(mz_handle* h, mz_handle::WSet& w);
}  // namespace mz
#pragma GCC visibility pop
