// mz_reanalyse.hip — MuZero Reanalyze on the device replay shard
// (ReplayBuffer.jl:8, 56-67; the reference's unbuilt worker, muzero.jl:15-19):
// reanalysed_predicted_root_values[pos] = value head of prediction(
// representation(stacked observation at pos)) for the selected games, written
// to ring.rrv next to ring.rv, ring.rean[slot] set once per game and
// counters[3] (num_reanalysed_games) bumped once per game.  No workgroup
// waits for another: the samplers that read rrv run in later launches.
//
// The selected games' positions are flattened as p = game · T + pos
// (T = max_moves + 1, the ring's row length); pos >= len is dead.
//
// The second half (mz_replay_reanalyse_search, at the end of this file)
// searches the same rows again: mz_reanalyse_sgather builds the inputs of one
// batched search per max_games rows, the engine's search launches run, and
// mz_reanalyse_sscatter writes child_visits to ring.rcv and the search's root
// values to ring.rrv.  ring.rean is a bit mask: MZ_REAN_VALUES (rrv valid),
// MZ_REAN_POLICIES (rcv valid).
//
// The worker (mz_replay_reanalyse_next) runs either half on one round of rows
// that mz_reanalyse_pack chose on the device: whole games from a cursor that
// lives behind the counters, only their live positions, as a list of (slot,
// pos) pairs the five kernels read in place of the flattened grid.
#include "mz_mlp_device.h"
#include "mz_replay_device.h"
#include "mz_env_device.h"

// The held range and the selection, from the device counter (no host sync):
// returns the number of rows of the flattened grid that can be live (T per
// selected game that is held), *oldest = game number of shard game 0.  With a
// row list (mz_replay_reanalyse_next) the rows are the round's packed ones and
// their number is the header's n_rows.
__device__ __forceinline__ int rean_rows(const ReanParams& Q, long long* oldest) {
    if (Q.rows) {
        *oldest = 0;
        const long long n = Q.counters[MZ_REAN_HDR + 2];
        return (int)(n < 0 ? 0 : n > Q.R ? Q.R : n);
    }
    const long long played = Q.counters[0];
    const int n = (int)(played < Q.cap ? played : Q.cap);
    *oldest = played - n + 1;
    const int left = n - Q.first;
    return (Q.count < 0 || Q.count > left ? left : Q.count) * Q.T;    // <= 0: nothing selected is held
}

// flattened position p -> ring slot and 0-based pos; false if dead
__device__ __forceinline__ bool rean_pos(const ReanParams& Q, long long oldest, int nrows, int p, int* slot, int* pos) {
    if (p < 0 || p >= nrows) return false;
    if (Q.rows) {                         // a packed row: live by construction
        const int2 r = reinterpret_cast<const int2*>(Q.rows)[p];
        *slot = r.x; *pos = r.y;
        return true;
    }
    const int gi = p / Q.T;
    *pos = p - gi * Q.T;
    *slot = (int)((oldest + Q.first + gi - 1) % Q.cap);
    return *pos < Q.ring.len[*slot];
}

// pos 0 of a live game marks it (every stored game has len >= 1): ORs `bits`
// (MZ_REAN_VALUES / MZ_REAN_POLICIES) into the slot's mask, so a value-only
// pass keeps the policies an earlier search pass left
__device__ __forceinline__ void rean_mark(const ReanParams& Q, int slot, int bits) {
    atomicOr(Q.ring.rean + slot, bits);
    atomicAdd(reinterpret_cast<unsigned long long*>(Q.counters + 3), 1ull);
}

// One round of the worker, one wave.  With played = counters[0], n = min(played,
// cap) and oldest = played - n + 1: a cursor outside [oldest, played] goes to
// oldest (a wrap, or the games evicted since), then games cursor, cursor + 1, ...
// are taken while they are <= played and the running sum of len stays <= R; no
// wrap inside a round.  Lane l of chunk c looks at game cursor + 64 c + l: the
// lanes form an inclusive prefix sum of len, the total so far rides in a
// register every lane holds, and a ballot finds the first lane that is past
// `played` or over R.  Every stored game has 1 <= len <= T <= R, so a round on a
// non-empty shard takes a game, at most R games are looked at and the loop ends
// within R/64 + 1 chunks whatever the ring holds.  A taken game's rows go to
// rows[start .. start + len): start + len <= R.  The cursor moves to the first
// game not taken; the header {first game number, games, n_rows} is what the
// kernels above (n_rows) and mz_replay_reanalyse_cursor read.
extern "C" __global__ __launch_bounds__(64) void mz_reanalyse_pack(ReanParams Q, int32_t* rows) {
    const int lane = threadIdx.x;
    const long long played = Q.counters[0];
    long long first = Q.counters[MZ_REAN_CURSOR];
    int total = 0, games = 0;
    if (played > 0) {
        const long long n = played < Q.cap ? played : Q.cap;
        const long long oldest = played - n + 1;
        if (first < oldest || first > played) first = oldest;
        const int chunks = Q.R / 64 + 1;
        for (int c = 0; c < chunks; ++c) {
            const long long g = first + (long long)c * 64 + lane;
            const bool held = g <= played;
            const int slot = held ? (int)((g - 1) % Q.cap) : 0;
            int len = held ? Q.ring.len[slot] : 0;
            len = len < 0 ? 0 : len > Q.T ? Q.T : len;
            int inc = len;
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(inc, d);
                if (lane >= d) inc += t;
            }
            const int tot = total + inc;
            const unsigned long long stop = __ballot(!held || tot > Q.R);
            const int take = stop ? __ffsll((long long)stop) - 1 : 64;     // the lanes below are taken
            if (lane < take)
                for (int pos = 0; pos < len; ++pos) {
                    rows[2 * (tot - len + pos)] = slot;
                    rows[2 * (tot - len + pos) + 1] = pos;
                }
            if (take > 0) total = __shfl(tot, take - 1);
            games += take;
            if (take < 64) break;
        }
    }
    if (lane == 0) {
        Q.counters[MZ_REAN_CURSOR] = first + games;
        Q.counters[MZ_REAN_HDR] = first;
        Q.counters[MZ_REAN_HDR + 1] = games;
        Q.counters[MZ_REAN_HDR + 2] = total;
    }
}

// stream-ordered mz_replay_reanalyse_seek
extern "C" __global__ void mz_reanalyse_seek(long long* counters, long long game_number) {
    if (threadIdx.x == 0 && blockIdx.x == 0) counters[MZ_REAN_CURSOR] = game_number;
}

// FC engines.  Workgroups walk 16-position tiles in a grid-stride loop; per
// tile the four waves build the stacked observations from the ring bytes
// (stacked_obs, one wave per position) into an LDS staging block [16][F],
// the block is transposed into the plan's x_rep columns, the root plan
// (representation, then prediction from h_out) runs with run_plan, and lanes
// 0..15 write the value row.  LDS: lds_total floats of the activation layout
// + 16·F of staging.
//
// The weights are read per tile (run_plan), not kept in registers: the
// register-resident executor (res_load / res_run on a resident image of this
// plan, 256 weight VGPRs, one workgroup per CU) was built and measured 6-8 %
// slower at the configs[1] shard than four of these workgroups per CU reading
// the 300 KB image from L2, and it only fits layers of K <= 64.
extern "C" __global__ __launch_bounds__(MZ_THREADS) void mz_reanalyse_fc(ReanParams Q) {
    extern __shared__ __attribute__((aligned(16))) float act[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    long long oldest;
    const int nrows = rean_rows(Q, &oldest);
    if (nrows <= 0) return;
    const int ntiles = (nrows + MZ_TILE - 1) / MZ_TILE;
    float* xs = act + Q.lds_total;
    for (int i = tid; i < Q.lds_total; i += MZ_THREADS) act[i] = 0.0f;     // padded input rows stay 0
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int slot = 0, pos = 0;
        const bool live = lane < MZ_TILE && rean_pos(Q, oldest, nrows, tile * MZ_TILE + lane, &slot, &pos);
        const unsigned mask = (unsigned)__ballot(live) & 0xffffu;          // the same in every wave
        if (!mask) continue;                                               // a dead tile: no networks
        __syncthreads();                  // the zero fill / the previous tile is done with the LDS
        for (int j = wave; j < MZ_TILE; j += MZ_THREADS / 64) {
            float* out = xs + j * Q.F;
            if ((mask >> j) & 1u) {
                const int sj = __shfl(slot, j), pj = __shfl(pos, j);
                const size_t base = (size_t)sj * Q.T;
                stacked_obs(out, Q.ring.obs + (base + pj) * Q.osz, Q.ring.obs + base * Q.osz, Q.ring.act + base,
                            pj + 1, Q.osz, Q.P, Q.stacked, lane);
            } else {
                for (int k = lane; k < Q.F; k += 64) out[k] = 0.0f;
            }
        }
        __syncthreads();
        for (int i = tid; i < MZ_TILE * Q.F; i += MZ_THREADS) {
            const int j = i / Q.F, k = i - j * Q.F;
            act[Q.x_rep + k * 16 + j] = xs[i];
        }
        __syncthreads();
        run_plan(Q.plan_root, Q.Wp, Q.Bp, act);
        if (live && wave == 0) {          // run_plan ended in a barrier
            Q.ring.rrv[(size_t)slot * Q.T + pos] = mz_post_act(Q.v_act, act[Q.v_out + lane]);
            if (pos == 0) rean_mark(Q, slot, MZ_REAN_VALUES);
        }
    }
}

// ResNet engines, positions [p0, p0 + pn): one wave per position writes its
// stacked observation (f32, zeros if dead) to stage_x[i][F] ...
extern "C" __global__ __launch_bounds__(256) void mz_reanalyse_gather(ReanParams Q) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Q.pn) return;
    long long oldest;
    const int nrows = rean_rows(Q, &oldest);
    float* out = Q.stage_x + (size_t)i * Q.F;
    int slot = 0, pos = 0;
    if (rean_pos(Q, oldest, nrows, Q.p0 + i, &slot, &pos)) {
        const size_t base = (size_t)slot * Q.T;
        stacked_obs(out, Q.ring.obs + (base + pos) * Q.osz, Q.ring.obs + base * Q.osz, Q.ring.act + base, pos + 1,
                    Q.osz, Q.P, Q.stacked, lane);
    } else {
        for (int k = lane; k < Q.F; k += 64) out[k] = 0.0f;
    }
}

// ... and after mz_rnet_forward_kernel (REPR, then PRED) the live positions'
// values go from stage_v[i] to the ring.
extern "C" __global__ __launch_bounds__(256) void mz_reanalyse_scatter(ReanParams Q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q.pn) return;
    long long oldest;
    const int nrows = rean_rows(Q, &oldest);
    int slot = 0, pos = 0;
    if (!rean_pos(Q, oldest, nrows, Q.p0 + i, &slot, &pos)) return;
    Q.ring.rrv[(size_t)slot * Q.T + pos] = Q.stage_v[i];
    if (pos == 0) rean_mark(Q, slot, MZ_REAN_VALUES);
}

// every held or stale slot back to `nothing`
extern "C" __global__ void mz_reanalyse_clear(int32_t* rean, int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) rean[i] = 0;
}

// ---- Reanalyse by search (mz_replay_reanalyse_search): rows [p0, p0 + pn) of
// the flattened grid become the games of one batched search, gather -> the
// engine's search launches -> scatter.
//
// One wave per row: the inputs mz_sp_prepare gave the search when the move was
// played — the stacked observation, to_play = tp[pos], the legal mask of the
// stored board for that player (env_legal_board, over = 0: a stored position
// was played from) — or the dummy (zero observation, every action legal,
// to_play 1) for a dead row and for a row the search must not see: an empty
// mask, or a to_play outside 1..players (both only from mz_replay_save_game
// with arbitrary bytes).
extern "C" __global__ __launch_bounds__(256) void mz_reanalyse_sgather(ReanParams Q) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Q.pn) return;
    long long oldest;
    const int nrows = rean_rows(Q, &oldest);
    float* out = Q.stage_x + (size_t)i * Q.F;
    int slot = 0, pos = 0, state = MZ_REAN_DEAD, tp = 1;
    uint32_t m = Q.A >= 32 ? 0xFFFFFFFFu : (1u << Q.A) - 1u;
    if (rean_pos(Q, oldest, nrows, Q.p0 + i, &slot, &pos)) {
        const size_t base = (size_t)slot * Q.T;
        const int t = Q.ring.tp[base + pos];
        uint32_t lm = 0;
        if (t >= 1 && t <= Q.players)
            lm = env_legal_board(Q.env, Q.ring.obs + (base + pos) * Q.osz, t, 0, Q.W, Q.H, Q.A) & m;
        state = lm ? MZ_REAN_LIVE : MZ_REAN_EMPTY;
        if (lm) { m = lm; tp = t; }
    }
    if (state == MZ_REAN_LIVE) {
        const size_t base = (size_t)slot * Q.T;
        stacked_obs(out, Q.ring.obs + (base + pos) * Q.osz, Q.ring.obs + base * Q.osz, Q.ring.act + base, pos + 1,
                    Q.osz, Q.P, Q.stacked, lane);
    } else {
        for (int k = lane; k < Q.F; k += 64) out[k] = 0.0f;
    }
    for (int a = lane; a < Q.A; a += 64) Q.stage_legal[(size_t)i * Q.A + a] = (m >> a) & 1u;
    if (lane == 0) { Q.stage_tp[i] = tp; Q.stage_state[i] = state; }
}

// One thread per (row, action): a searched row's child_visits and root value
// go to rcv / rrv, an unsearched stored position keeps copies of its originals,
// a dead row writes nothing; pos 0 sets both flag bits and counts the game.
extern "C" __global__ __launch_bounds__(256) void mz_reanalyse_sscatter(ReanParams Q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Q.pn * Q.A) return;
    const int i = e / Q.A, a = e - i * Q.A;
    const int state = Q.stage_state[i];
    if (state == MZ_REAN_DEAD) return;
    long long oldest;
    const int nrows = rean_rows(Q, &oldest);
    int slot = 0, pos = 0;
    if (!rean_pos(Q, oldest, nrows, Q.p0 + i, &slot, &pos)) return;
    const size_t r = (size_t)slot * Q.T + pos;
    const bool live = state == MZ_REAN_LIVE;
    Q.ring.rcv[r * Q.A + a] = live ? Q.stage_cv[(size_t)i * Q.A + a] : Q.ring.cv[r * Q.A + a];
    if (a == 0) {
        Q.ring.rrv[r] = live ? Q.stage_rv[i] : Q.ring.rv[r];
        if (pos == 0) rean_mark(Q, slot, MZ_REAN_VALUES | MZ_REAN_POLICIES);
    }
}
