// mz_train_host.hip — host side of libmz: the actor–learner loop, the run log, the opponent's
// weight set and the engine's side of the snapshots.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <algorithm>
#include <cstring>
#include <string>

#include "mz_handle.h"
#include "mz_internal.h"
#include "mz_selfplay_params.h"
#include "mz_ckpt_iface.h"
#include "mz_snap_iface.h"

using namespace mz;

int mz_train_set_reanalyse(mz_handle* h, int mode, int rounds_per_move, int exploration) {
    if (!h) return -2;
    if (mode != MZ_REAN_OFF && mode != MZ_REAN_BY_VALUE && mode != MZ_REAN_BY_SEARCH)
        return fail(h, "mz_train_set_reanalyse: mode must be MZ_REAN_OFF, MZ_REAN_BY_VALUE or MZ_REAN_BY_SEARCH");
    if (rounds_per_move < 0) return fail(h, "mz_train_set_reanalyse: rounds_per_move must be >= 0");
    if (mode != MZ_REAN_OFF && h->sp_env >= 0 && rean_next_check(h, mode)) return -1;
    h->tr_rean_mode = mode; h->tr_rean_rounds = rounds_per_move; h->tr_rean_expl = exploration != 0;
    return 0;
}

int mz_train_set_test(mz_handle* h, int64_t interval, uint32_t game_offset, float temperature) {
    if (!h) return -2;
    if (interval < 0) return fail(h, "mz_train_set_test: interval must be >= 0");
    if (interval > 0 && h->test_E < 1)
        return fail(h, "mz_train_set_test: no test slots (mz_test_config with games >= 1 first)");
    h->test_interval = interval; h->test_goff = game_offset; h->test_temp = temperature;
    return 0;
}

// the run log starts over on a new shard (mz_selfplay_init, a passing mz_snapshot_load, the log
// switched on): zero accumulators, and the shard's `played` games so far are not this log's.  The
// record ring and log_total stay.  The caller has drained the device.
int mz::log_rebase(mz_handle* h, long long played) {
    if (!h->d_log_acc) return 0;
    LogAcc a;
    std::memset(&a, 0, sizeof(a));
    a.logged_upto = played;
    MZ_TRY(h, hipMemcpy(h->d_log_acc, &a, sizeof(a), hipMemcpyHostToDevice));
    return 0;
}

// ---- actor–learner loop (self_play! ‖ learning!, Q16)
// The actors search with their own weight set; the learner trains the
// engine's weights.  The set is swapped in around each self-play move (the
// search kernels read the images the handle points at).
void mz::wset_swap(mz_handle* h, mz_handle::WSet& w) {
    std::swap(h->d_flat, w.flat); std::swap(h->d_Wp, w.Wp); std::swap(h->d_Bp, w.Bp);
    std::swap(h->d_sm_w, w.smw); std::swap(h->d_sm_bias, w.smb);
}
// flat -> the set's search images (the repack of the handle's current images)
static int wset_repack(mz_handle* h, mz_handle::WSet& w, hipStream_t st) {
    const int T = 256;
    hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_w_n + T - 1) / T)), dim3(T), 0, st,
                       w.flat, h->d_srcW, w.Wp, h->packed_w_n);
    if (h->packed_b_n)
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_b_n + T - 1) / T)), dim3(T), 0, st,
                           w.flat, h->d_srcB, w.Bp, h->packed_b_n);
    if (h->small_ok) {
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_w_n + T - 1) / T)), dim3(T), 0, st,
                           w.flat, h->d_sm_srcw, w.smw, h->sm_w_n);
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_b_n + T - 1) / T)), dim3(T), 0, st,
                           w.flat, h->d_sm_srcb, w.smb, h->sm_b_n);
    }
    MZ_TRY(h, hipGetLastError());
    return 0;
}
// ParameterSchedulers 0.2.3 Cos(λ0 = 1e-4, λ1 = 1e-1, period = 10) under
// Stateful, step t >= 1 (Learning.jl:319, 382)
static double cos_schedule(int64_t t) {
    const double l0 = 1e-4, l1 = 1e-1, range = std::fabs(l0 - l1), off = std::min(l0, l1);
    const double a = 6.283185307179586 * (double)(t - 1) / 10.0;
    return range * (1.0 + std::cos(a)) / 2.0 + off;
}

static float temp_fn(int64_t t) { return t < 500000 ? 1.0f : t < 750000 ? 0.5f : 0.25f; }   // SelfPlay.jl:48-56

int mz_train_init(mz_handle* h, int32_t B) { return mz_train_init_at(h, B, 0); }

int mz_train_set_networks_path(mz_handle* h, const char* networks_path) {
    if (!h) return -2;
    h->tr_ckpt_path = networks_path ? networks_path : "";
    return 0;
}

// the actors' weight set, the queued nets and the move's pinned hand-back words (once per handle)
static int train_alloc(mz_handle* h) {
    mz_handle::WSet& w = h->tr_actor;
    if (w.flat) return 0;
    MZ_TRY(h, dalloc(h, &w.flat, h->nflat));
    MZ_TRY(h, dalloc(h, &w.Wp, h->packed_w_n));
    if (h->packed_b_n) MZ_TRY(h, dalloc(h, &w.Bp, h->packed_b_n));
    if (h->small_ok) { MZ_TRY(h, dalloc(h, &w.smw, h->sm_w_n)); MZ_TRY(h, dalloc(h, &w.smb, h->sm_b_n)); }
    MZ_TRY(h, dalloc(h, &h->d_tr_queued, h->nflat));
    MZ_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_tr_cnt), 4 * sizeof(long long)));
    MZ_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->h_tr_pub), 4 * sizeof(long long), hipHostMallocCoherent));
    std::memset(h->h_tr_pub, 0, 4 * sizeof(long long));
    h->tr_pub_seq = 0;
    return 0;
}

int mz_train_init_at(mz_handle* h, int32_t B, int64_t t0) {
    if (!h) return -2;
    if (t0 < 0) return fail(h, "the starting training step must be >= 0");
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (B < 1) return fail(h, "batch_size must be >= 1");
    if (h->conf.checkpoint_interval < 1) return fail(h, "checkpoint_interval must be >= 1");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (train_alloc(h)) return -1;
    mz_handle::WSet& w = h->tr_actor;
    // actors and the queue start from the learner's current (initial) nets (main.jl:23)
    MZ_TRY(h, hipMemcpyAsync(w.flat, h->d_flat, h->nflat * 4, hipMemcpyDeviceToDevice, h->stream));
    MZ_TRY(h, hipMemcpyAsync(h->d_tr_queued, h->d_flat, h->nflat * 4, hipMemcpyDeviceToDevice, h->stream));
    if (wset_repack(h, w, h->stream)) return -1;
    MZ_TRY(h, hipMemcpyAsync(h->h_tr_cnt, h->d_sp_counters, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    MZ_TRY(h, hipStreamSynchronize(h->stream));
    // games already in progress keep visit_softmax_temperature_fn(t0) to their end
    std::vector<float> tg((size_t)h->sp_G, temp_fn(t0));
    MZ_TRY(h, hipMemcpy(h->d_sp_tgame, tg.data(), tg.size() * 4, hipMemcpyHostToDevice));
    h->tr_B = B; h->tr_t = t0; h->tr_refresh = 0;
    h->tr_games = h->h_tr_cnt[0];
    return 0;
}

// the move's hand-back to the host: the finished-game count and the fault word, then a sequence
// number, stored into coherent pinned host memory at system scope; the host spins on the sequence
// number instead of two copy launches and a stream synchronisation (measured in the trace: 30-60 us
// from the copies' end to the next launch)
extern "C" __global__ void mz_tr_publish(const long long* counters, const unsigned* fault, long long* host,
                                         long long seq) {
    if (threadIdx.x == 0) {
        __hip_atomic_store(host + 0, counters[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host + 1, fault ? (long long)*fault : 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host + 2, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// wait for publish `seq` (bounded: after 60 s the stream is synchronised, which reports a launch error)
static int tr_wait_publish(mz_handle* h, long long seq, hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned n = 0; __atomic_load_n(h->h_tr_pub + 2, __ATOMIC_ACQUIRE) != seq; ++n) {
        if ((n & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
            MZ_TRY(h, hipStreamSynchronize(st));
            if (__atomic_load_n(h->h_tr_pub + 2, __ATOMIC_ACQUIRE) == seq) break;
            return fail(h, "mz_train: the move's publish never arrived");
        }
        __builtin_ia32_pause();
    }
    return 0;
}

// the move's reanalyse rounds (mz_train_set_reanalyse), with the learner's nets: round r has the
// keys (move, game_offset + r * max_games)
static int train_rean_rounds(mz_handle* h, uint32_t move, uint32_t game_offset, hipStream_t st) {
    for (int r = 0; r < h->tr_rean_rounds; ++r)
        if (mz_replay_reanalyse_next(h, h->tr_rean_mode, h->tr_rean_expl, move,
                                     game_offset + (uint32_t)r * (uint32_t)h->max_games, st))
            return -1;
    return 0;
}

// ---- the run log: three tiny launches in stream order, nothing read back
// behind a training move's mz_sp_store: the shard's new games
static int log_games(mz_handle* h, hipStream_t st) {
    hipLaunchKernelGGL(mz_log_games, dim3(1), dim3(1024), 0, st, sp_params(h), h->d_log_acc);
    MZ_TRY(h, hipGetLastError());
    return 0;
}
// behind a learner chunk: its n loss rows in d_log_rows
static int log_steps(mz_handle* h, int n, hipStream_t st) {
    LogArgs L;
    std::memset(&L, 0, sizeof(L));
    L.acc = h->d_log_acc; L.rows = h->d_log_rows; L.n = n;
    hipLaunchKernelGGL(mz_log_steps, dim3(1), dim3(64), 0, st, L);
    MZ_TRY(h, hipGetLastError());
    return 0;
}
// record log_total from whatever is accumulated, with the learner at step tr_t
static int log_commit(mz_handle* h, hipStream_t st) {
    const size_t slot = (size_t)(h->log_total % MZ_LOG_RECORDS);
    LogArgs L;
    std::memset(&L, 0, sizeof(L));
    L.acc = h->d_log_acc; L.counts = h->d_log_counts + slot * 16; L.sums = h->d_log_sums + slot * 16;
    L.counters = h->d_sp_counters; L.cap = h->sp_cap;
    L.t1 = h->tr_t; L.refreshes = h->tr_refresh; L.eta = cos_schedule(h->tr_t);
    hipLaunchKernelGGL(mz_log_commit, dim3(1), dim3(64), 0, st, L);
    MZ_TRY(h, hipGetLastError());
    ++h->log_total;
    return 0;
}
// the commit rule (the test worker's): the call's learner steps crossed a multiple of the interval
static int log_crossed(mz_handle* h, int64_t t0, hipStream_t st) {
    const int64_t iv = h->log_interval;
    return iv > 0 && h->tr_t / iv > t0 / iv ? log_commit(h, st) : 0;
}

// ---- the run log's host side (the launches: log_games / log_steps / log_commit above)
int mz_train_set_log(mz_handle* h, int64_t interval) {
    if (!h) return -2;
    if (interval < 0) return fail(h, "mz_train_set_log: interval must be >= 0");
    if (interval > 0 && h->log_interval == 0) {     // switched on: the shard's games so far are not this log's
        MZ_TRY(h, hipSetDevice(h->device));
        MZ_SYNC(h);
        if (!h->d_log_acc) {
            MZ_TRY(h, dalloc(h, &h->d_log_acc, 1));
            MZ_TRY(h, dalloc(h, &h->d_log_rows, (size_t)MZ_MULTI_LMAX * 8));
            MZ_TRY(h, dalloc(h, &h->d_log_counts, (size_t)MZ_LOG_RECORDS * 16));
            MZ_TRY(h, dalloc(h, &h->d_log_sums, (size_t)MZ_LOG_RECORDS * 16));
        }
        long long played = 0;
        if (h->sp_env >= 0) MZ_TRY(h, hipMemcpy(&played, h->d_sp_counters, sizeof(played), hipMemcpyDeviceToHost));
        if (log_rebase(h, played)) return -1;
    }
    h->log_interval = interval;
    return 0;
}

int mz_train_log_flush(mz_handle* h, void* stream) {
    if (!h) return -2;
    if (!h->tr_B) return fail(h, "mz_train_init first");
    if (h->log_interval <= 0) return fail(h, "mz_train_log_flush: the run log is off (mz_train_set_log first)");
    MZ_TRY(h, hipSetDevice(h->device));
    return log_commit(h, stream_of(h, stream));
}

int mz_train_log_results(mz_handle* h, int64_t* total, int64_t* counts, double* sums, int32_t max_records) {
    if (!h) return -2;
    if (max_records < 0) return fail(h, "mz_train_log_results: max_records must be >= 0");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (total) *total = h->log_total;
    const int64_t held = std::min<int64_t>(h->log_total, MZ_LOG_RECORDS);
    const int64_t n = std::min<int64_t>(max_records, held);
    for (int64_t i = 0; i < n; ++i) {
        const size_t slot = (size_t)((h->log_total - n + i) % MZ_LOG_RECORDS);
        long long c[16];
        if (counts) {
            MZ_TRY(h, hipMemcpy(c, h->d_log_counts + slot * 16, sizeof(c), hipMemcpyDeviceToHost));
            for (int k = 0; k < 16; ++k) counts[i * 16 + k] = c[k];
        }
        if (sums) MZ_TRY(h, hipMemcpy(sums + i * 16, h->d_log_sums + slot * 16, 16 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mz_train_log_clear(mz_handle* h) {
    if (!h) return -2;
    h->log_total = 0;
    if (!h->d_log_acc) return 0;
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long upto = 0;                             // the games folded so far stay folded
    MZ_TRY(h, hipMemcpy(&upto, &h->d_log_acc->logged_upto, sizeof(upto), hipMemcpyDeviceToHost));
    return log_rebase(h, upto);
}

// 1. one self-play move with the actors' nets (SelfPlay.jl:343-380); temperature
//    visit_softmax_temperature_fn(t) (:48-56, 396-397) for the games that start on
//    this move (a game in progress keeps its own).  *nfin = the games save_game
//    stored (slot order, inside the move).  The fault word rides along with the
//    counter copy: one stream wait per move, no second blocking copy.
//    `rean` (mz_train_run): the move's reanalyse rounds go on the stream behind the
//    hand-back and before the host waits for it, so the wait overlaps them.
static int train_move(mz_handle* h, uint32_t move, uint32_t game_offset, int64_t* nfin, hipStream_t st,
                      bool rean = false) {
    rean = rean && h->tr_rean_mode != MZ_REAN_OFF;
    const float temp = temp_fn(h->tr_t);
    wset_swap(h, h->tr_actor);
    h->sp_latch = true;
    const int rc = mz_selfplay_move(h, move, game_offset, temp, st);
    h->sp_latch = false;
    wset_swap(h, h->tr_actor);
    if (rc) return rc;
    const long long seq = ++h->tr_pub_seq;
    hipLaunchKernelGGL(mz_tr_publish, dim3(1), dim3(64), 0, st, (const long long*)h->d_sp_counters,
                       (const unsigned*)h->d_fault, h->h_tr_pub, seq);
    MZ_TRY(h, hipGetLastError());
    // the run log folds the shard's new games (the move's saves, and any a host put in since the last
    // move) behind the hand-back, so the host's wait overlaps it
    if (h->log_interval > 0 && !h->sp_eval && log_games(h, st)) return -1;
    if (rean && train_rean_rounds(h, move, game_offset, st)) return -1;
    if (tr_wait_publish(h, seq, st)) return -1;
    h->h_tr_cnt[0] = h->h_tr_pub[0];
    h->h_tr_cnt[1] = h->h_tr_pub[1];
    if (h->h_tr_cnt[1] && check_fault(h)) return -1;
    *nfin = h->h_tr_cnt[0] - h->tr_games;
    h->tr_games = h->h_tr_cnt[0];
    return 0;
}

// the actors take the queued nets, the learner's nets are queued (SelfPlay.jl:399-401 /
// Learning.jl:416-418: one checkpoint behind); past round(0.9 training_steps) the nets
// go to disk (Learning.jl:427-432, round half to even as Julia's round)
static int train_refresh(mz_handle* h, int64_t t, hipStream_t st) {
    MZ_TRY(h, hipMemcpyAsync(h->tr_actor.flat, h->d_tr_queued, h->nflat * 4, hipMemcpyDeviceToDevice, st));
    if (wset_repack(h, h->tr_actor, st)) return -1;
    MZ_TRY(h, hipMemcpyAsync(h->d_tr_queued, h->d_flat, h->nflat * 4, hipMemcpyDeviceToDevice, st));
    ++h->tr_refresh;
    if (!h->tr_ckpt_path.empty() && (double)t > std::nearbyint(0.9 * (double)h->conf.training_steps)) {
        MZ_TRY(h, hipStreamSynchronize(st));
        const std::string path = h->tr_ckpt_path + "/" + std::to_string(t) + ".safetensors";
        if (mz_checkpoint_save(h, path.c_str(), t)) return -1;
    }
    return 0;
}

// 2. `nreq` learner steps while t <= training_steps (Learning.jl:327), get_batch keyed by
//    the step number, eta = Cos(step); every checkpoint_interval steps (t % ci == 0, t > 1)
//    an actor refresh.  Round 6: the steps of one call run as ONE mz_learner_train_multi_dev
//    chunk across the refresh points (up to 256 steps per call): nothing
//    reads the actors' or the queued nets between two learner steps of one move, so only
//    the sets after the last refresh matter — θ of the last refresh step is queued, θ of the
//    one before it (or, with one refresh, the previously queued nets) goes to the actors, and
//    the chain launch that computes those θ copies them out (MultiCap).  With periodic
//    checkpoint files (networks_path) the chunks end at every
//    refresh step as in round 5 (the checkpoint writes the learner's nets of that step).
static int train_learn(mz_handle* h, int64_t nreq, float* losses_dev, hipStream_t st, int64_t* done) {
    const bool per_refresh = !h->tr_ckpt_path.empty();
    const int64_t ci = h->conf.checkpoint_interval;
    auto is_refresh = [&](int64_t t) { return t % ci == 0 && t > 1; };
    const int64_t n_all = std::max<int64_t>(0, std::min<int64_t>(nreq, (int64_t)h->conf.training_steps + 1 - h->tr_t));
    *done = 0;
    if (n_all == 0) return 0;
    // the actors' set: θ of the next-to-last refresh step, its search images written by the chain launch
    // that computes it (else repacked after the call)
    bool imaged = false;
    MultiCap cap{{-1, -1}, {h->tr_actor.flat, h->d_tr_queued}, &h->tr_actor, &imaged};
    int64_t nref = 0;
    if (!per_refresh) {
        // the refresh steps in (t, t + n]: the last two
        const int64_t t_lo = h->tr_t, t_hi = h->tr_t + n_all;
        for (int64_t r = t_hi / ci * ci; r > t_lo && nref < 2; r -= ci)
            if (is_refresh(r)) { cap.t[1 - nref] = r; ++nref; }
        const int64_t first = (t_lo / ci + 1) * ci;   // the total count
        nref = 0;
        for (int64_t r = first; r <= t_hi; r += ci) nref += is_refresh(r) ? 1 : 0;
        if (nref == 1) {               // the actors take the nets queued before this call
            MZ_TRY(h, hipMemcpyAsync(h->tr_actor.flat, h->d_tr_queued, h->nflat * 4, hipMemcpyDeviceToDevice, st));
            cap.t[0] = -1;
        }
    }
    double eta[MZ_MULTI_LMAX];
    for (int64_t k = 0; k < n_all;) {
        const int64_t t0 = h->tr_t + 1;
        int64_t n = std::min<int64_t>(n_all - k, MZ_MULTI_LMAX);
        if (per_refresh) {                                 // the chunk ends at the next refresh step
            int64_t tb = (t0 + ci - 1) / ci * ci;
            if (tb <= 1) tb += ci;
            n = std::min<int64_t>(n, tb - t0 + 1);
        }
        const int64_t t = t0 + n - 1;
        // the run log: every step's losses go to the handle's rows, mz_log_steps folds them behind the
        // chunk, and the caller's losses_dev gets a copy of the last row.  Off: the pointers below are
        // the caller's as ever and nothing more is issued.
        float* rows = h->log_interval > 0 ? h->d_log_rows : nullptr;
        if (n == 1) {
            if (mz_learner_train_dev(h, h->tr_B, (uint32_t)t, cos_schedule(t), rows ? rows : losses_dev, st)) return -1;
            for (int j = 0; j < 2; ++j)
                if (cap.t[j] == t)
                    MZ_TRY(h, hipMemcpyAsync(cap.dst[j], h->d_flat, h->nflat * 4, hipMemcpyDeviceToDevice, st));
        } else {
            for (int64_t i = 0; i < n; ++i) eta[i] = cos_schedule(t0 + i);
            if (learner_multi(h, h->tr_B, (uint32_t)t0, (int32_t)n, eta, rows, nullptr, st, rows ? nullptr : losses_dev,
                              per_refresh ? nullptr : &cap))
                return -1;
        }
        if (rows) {
            if (losses_dev)
                MZ_TRY(h, hipMemcpyAsync(losses_dev, rows + 8 * (n - 1), 6 * 4, hipMemcpyDeviceToDevice, st));
            if (log_steps(h, (int)n, st)) return -1;
        }
        h->tr_t = t;
        *done += n;
        k += n;
        if (per_refresh && is_refresh(t) && train_refresh(h, t, st)) return -1;
    }
    if (!per_refresh && nref > 0) {
        if (!(nref >= 2 && imaged) && wset_repack(h, h->tr_actor, st)) return -1;
        h->tr_refresh += nref;
    }
    return 0;
}

int mz_train_move(mz_handle* h, uint32_t move, uint32_t game_offset, int64_t* nfin, void* stream) {
    if (!h) return -2;
    if (!h->tr_B) return fail(h, "mz_train_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    int64_t n = 0;
    if (train_move(h, move, game_offset, &n, stream_of(h, stream))) return -1;
    if (nfin) *nfin = n;
    return 0;
}

int mz_train_learn(mz_handle* h, int64_t steps, float* losses_dev, int64_t* state_out, void* stream) {
    if (!h) return -2;
    if (!h->tr_B) return fail(h, "mz_train_init first");
    if (steps < 0) return fail(h, "steps must be >= 0");
    MZ_TRY(h, hipSetDevice(h->device));
    int64_t done = 0;
    const int64_t t0 = h->tr_t;
    if (train_learn(h, steps, losses_dev, stream_of(h, stream), &done)) return -1;
    if (log_crossed(h, t0, stream_of(h, stream))) return -1;       // the run log's commit rule, per call
    if (state_out) {
        state_out[0] = h->tr_t; state_out[1] = h->tr_games; state_out[2] = h->tr_refresh; state_out[3] = done;
    }
    return 0;
}

int mz_train_run(mz_handle* h, int32_t moves, uint32_t move0, uint32_t game_offset, int64_t* state_out,
                 float* losses_dev, void* stream) {
    if (!h) return -2;
    if (!h->tr_B) return fail(h, "mz_train_init first");
    if (moves < 0) return fail(h, "moves must be >= 0");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    int64_t steps = 0;
    for (int32_t mv = 0; mv < moves; ++mv) {
        int64_t nfin = 0, done = 0;
        if (train_move(h, move0 + (uint32_t)mv, game_offset, &nfin, st, true)) return -1;
        // data parallel (mz_dp_init): every rank takes the learner steps of the games all
        // ranks finished, so the replicas stay identical
        if (h->dp_comm && h->dp_world > 1 && dp_sum_count(h, &nfin, st)) return -1;
        const int64_t t0 = h->tr_t;
        if (train_learn(h, nfin, losses_dev, st, &done)) return -1;
        steps += done;
        if (log_crossed(h, t0, st)) return -1;      // the run log's commit rule, per move (mz_train_set_log)
        // the test worker (mz_train_set_test): the move's learner steps crossed a multiple of the
        // interval -> one evaluation with the learner's nets after the move's last step (the chunk is
        // not cut), where the next move's Reanalyse rounds search with them too
        const int64_t iv = h->test_interval, t1 = h->tr_t;
        if (iv > 0 && t1 / iv > t0 / iv &&
            mz_test_play(h, t1, (uint32_t)t1 * (uint32_t)h->sp_T, h->test_goff, h->test_temp, st))
            return -1;
    }
    if (state_out) {
        state_out[0] = h->tr_t; state_out[1] = h->tr_games; state_out[2] = h->tr_refresh; state_out[3] = steps;
    }
    return 0;
}

int mz_train_weights_get(mz_handle* h, int which, int net, float* flat, size_t n) {
    if (!h) return -2;
    if (which == MZ_TRAIN_LEARNER) return mz_weights_get(h, net, flat, n);
    if (!h->tr_B) return fail(h, "mz_train_init first");
    if (which != MZ_TRAIN_ACTOR && which != MZ_TRAIN_QUEUED) return fail(h, "which: learner, actor or queued");
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (n != h->nparams[net]) return fail(h, "wrong parameter count");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const float* src = which == MZ_TRAIN_ACTOR ? h->tr_actor.flat : h->d_tr_queued;
    MZ_TRY(h, hipMemcpy(flat, src + h->flat_off[net], n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the opponent's weight set (MZ_OPP_NETWORK): a handle setting like
// mz_expert_depth; mz_selfplay_init, mz_snapshot_load and mz_weights_set leave it alone
static int opp_alloc(mz_handle* h) {
    if (h->opp.flat) return 0;
    mz_handle::WSet w;
    MZ_TRY(h, dalloc(h, &w.flat, h->nflat));
    MZ_TRY(h, dalloc(h, &w.Wp, h->packed_w_n));
    if (h->packed_b_n) MZ_TRY(h, dalloc(h, &w.Bp, h->packed_b_n));
    if (h->small_ok) { MZ_TRY(h, dalloc(h, &w.smw, h->sm_w_n)); MZ_TRY(h, dalloc(h, &w.smb, h->sm_b_n)); }
    h->opp = w;
    return 0;
}

int mz_opponent_weights_set(mz_handle* h, int net, const float* flat, size_t n) {
    if (!h) return -2;
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (!flat) return fail(h, "opponent_weights_set: null weights");
    if (n != h->nparams[net]) return fail(h, "opponent_weights_set: wrong parameter count");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // no search still reads the old set
    if (opp_alloc(h)) return -1;
    MZ_TRY(h, hipMemcpyAsync(h->opp.flat + h->flat_off[net], flat, n * 4, hipMemcpyHostToDevice, h->stream));
    h->opp_have |= 1u << net;
    if (h->opp_have == 7u && wset_repack(h, h->opp, h->stream)) return -1;   // the images need all three nets
    MZ_SYNC(h);
    return 0;
}

int mz_opponent_weights_get(mz_handle* h, int net, float* flat, size_t n) {
    if (!h) return -2;
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (!flat) return fail(h, "opponent_weights_get: null buffer");
    if (n != h->nparams[net]) return fail(h, "opponent_weights_get: wrong parameter count");
    if (!(h->opp_have >> net & 1u)) return fail(h, "opponent_weights_get: this net of the set was never given");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // a stream-ordered mz_opponent_from has landed
    MZ_TRY(h, hipMemcpy(flat, h->opp.flat + h->flat_off[net], n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mz_opponent_from(mz_handle* h, int which, void* stream) {
    if (!h) return -2;
    if (which != MZ_TRAIN_LEARNER && which != MZ_TRAIN_ACTOR && which != MZ_TRAIN_QUEUED)
        return fail(h, "opponent_from: which must be MZ_TRAIN_LEARNER, MZ_TRAIN_ACTOR or MZ_TRAIN_QUEUED");
    if (which != MZ_TRAIN_LEARNER && !h->tr_B) return fail(h, "opponent_from: mz_train_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    if (opp_alloc(h)) return -1;
    hipStream_t st = stream_of(h, stream);
    const float* src = which == MZ_TRAIN_LEARNER ? h->d_flat
                       : which == MZ_TRAIN_ACTOR ? h->tr_actor.flat : h->d_tr_queued;
    MZ_TRY(h, hipMemcpyAsync(h->opp.flat, src, h->nflat * 4, hipMemcpyDeviceToDevice, st));
    if (wset_repack(h, h->opp, st)) return -1;
    h->opp_have = 7u;
    return 0;
}

// mz_opponent_load's engine side (mz_ckpt_iface.h): a validated file's three nets become the set
int mz_opponent_put(mz_handle* h, const float* flat) {
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (opp_alloc(h)) return -1;
    MZ_TRY(h, hipMemcpyAsync(h->opp.flat, flat, h->nflat * 4, hipMemcpyHostToDevice, h->stream));
    if (wset_repack(h, h->opp, h->stream)) return -1;
    h->opp_have = 7u;
    MZ_SYNC(h);
    return 0;
}

// ---- snapshots (mz_snapshot.hip; mz_snap_iface.h): the engine's side
// `train`: the weight sets of mz_train_init exist and belong to the view
static void snap_fill_view(mz_handle* h, MzSnapView* v, bool train) {
    v->device = h->device; v->stream = h->stream;
    v->env = h->sp_env; v->G = h->sp_G; v->cap = h->sp_cap; v->T = h->sp_T; v->osz = h->sp_osz; v->A = h->A;
    v->per = h->conf.PER != 0; v->seed = h->seed;
    v->ring = h->sp_ring; v->hist = h->sp_hist; v->counters = h->d_sp_counters;
    v->hist.prio = nullptr; v->hist.gprio = nullptr;      // allocated, never used: not state
    if (!v->per) { v->ring.prio = nullptr; v->ring.gprio = nullptr; }
    v->board = h->d_sp_board; v->player = h->d_sp_player; v->over = h->d_sp_over; v->ekey = h->d_sp_ekey;
    v->tgame = h->d_sp_tgame; v->eval = h->d_eval;
    v->reset_pending = h->sp_reset_pending;
    v->train = train;
    v->tr[0] = h->tr_B; v->tr[1] = h->tr_t; v->tr[2] = h->tr_refresh;
    v->actor = h->tr_actor.flat; v->queued = h->d_tr_queued; v->nflat = h->nflat;
    v->settings = "{\"reanalyse\":[" + std::to_string(h->tr_rean_mode) + "," + std::to_string(h->tr_rean_rounds) + "," +
                  std::to_string(h->tr_rean_expl) + "],\"selfplay_mode\":[" + std::to_string(h->sp_eval) + "," +
                  std::to_string(h->sp_opp) + "," + std::to_string(h->sp_mzp) + "],\"learner_mode\":" +
                  std::to_string(h->learn_mode) + ",\"debug\":" +
                  std::to_string(h->dump_tree | h->time_nets << 1 | h->time_unroll << 2) + ",\"networks_path\":" +
                  (h->tr_ckpt_path.empty() ? "0" : "1") + "}";
}

int mz_snap_view(mz_handle* h, MzSnapView* v) {
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    snap_fill_view(h, v, h->tr_B > 0);
    return 0;
}

void mz_snap_engine_geometry(const mz_handle* h, mzsnap::EngineGeometry* e) {
    const mz_config& c = h->conf;
    const int W = c.observation_shape[0], H = c.observation_shape[1], C = c.observation_shape[2];
    e->network = mz_net_kind(h); e->config = mz_describe(h);
    // the envs mz_selfplay_init accepts for this config, with their record bytes per move
    e->env_osz[MZ_ENV_TICTACTOE] = W == 3 && H == 3 && C == 3 && h->A == 9 ? 27 : 0;
    e->env_osz[MZ_ENV_CONNECT4] = W == 6 && H == 7 && C == 3 && h->A == 7 ? 126 : 0;
    e->env_osz[MZ_ENV_ATARI] = W == 84 && H == 84 && C == 4 && h->A == 18 && c.stacked_observations == 0 ? 84 * 84 : 0;
    e->max_games = h->max_games; e->T = (long long)c.max_moves + 1; e->A = h->A; e->per = c.PER != 0;
    e->seed = h->seed;
}

int mz_snap_restore_begin(mz_handle* h, int env, int G, int cap, bool rcv, bool train, MzSnapView* v) {
    const bool had = h->sp_env >= 0;
    const int ev = h->sp_eval, opp = h->sp_opp, mzp = h->sp_mzp;
    if (int rc = mz_selfplay_init(h, env, G, cap)) return rc;
    if (had) { h->sp_eval = ev; h->sp_opp = opp; h->sp_mzp = mzp; }   // a setting of the loading host
    if (rcv) {
        ReanParams Q = rean_params(h);
        if (rean_search_io(h, Q)) return -1;
        MZ_TRY(h, hipMemset(h->sp_ring.rcv, 0, (size_t)h->sp_cap * h->sp_T * h->A * 4));
    }
    if (train) {
        if (h->conf.checkpoint_interval < 1) return fail(h, "checkpoint_interval must be >= 1");
        if (train_alloc(h)) return -1;       // tr_B stays 0 until mz_snap_restore_end sets the snapshot's
    }
    MZ_SYNC(h);
    snap_fill_view(h, v, train);
    return 0;
}

int mz_snap_restore_end(mz_handle* h, const long long* counters, int reset_pending, const long long* tr) {
    MZ_TRY(h, hipSetDevice(h->device));
    h->sp_reset_pending = reset_pending != 0;
    h->sp_has_games = counters[0] > 0;
    if (tr) {
        if (wset_repack(h, h->tr_actor, h->stream)) return -1;
        h->tr_B = (int)tr[0]; h->tr_t = tr[1]; h->tr_refresh = tr[2];
        h->tr_games = counters[0];
        h->h_tr_cnt[0] = counters[0];
    }
    ++h->pf_epoch;                           // no batch drawn ahead survives: the next step samples in place
    MZ_SYNC(h);
    return log_rebase(h, counters[0]);       // the run log: the file's games are not this log's
}
