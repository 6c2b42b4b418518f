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
#include "mz_mlp_device.h"
#include "mz_replay_device.h"

// The held range and the selection, from the device counter (no host sync):
// returns the number of selected games that are held, *oldest = game number
// of shard game 0.
__device__ __forceinline__ int rean_games(const ReanParams& Q, long long* oldest) {
    const long long played = Q.counters[0];
    const int n = (int)(played < Q.cap ? played : Q.cap);
    *oldest = played - n + 1;
    const int left = n - Q.first;
    return Q.count < 0 || Q.count > left ? left : Q.count;        // <= 0: nothing selected is held
}

// flattened position p -> ring slot and 0-based pos; false if dead
__device__ __forceinline__ bool rean_pos(const ReanParams& Q, long long oldest, int cnt, int p, int* slot, int* pos) {
    const int gi = p / Q.T;
    if (p < 0 || gi >= cnt) return false;
    *pos = p - gi * Q.T;
    *slot = (int)((oldest + Q.first + gi - 1) % Q.cap);
    return *pos < Q.ring.len[*slot];
}

// pos 0 of a live game marks it (every stored game has len >= 1)
__device__ __forceinline__ void rean_mark(const ReanParams& Q, int slot) {
    Q.ring.rean[slot] = 1;
    atomicAdd(reinterpret_cast<unsigned long long*>(Q.counters + 3), 1ull);
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
    const int cnt = rean_games(Q, &oldest);
    if (cnt <= 0) return;
    const int ntiles = (cnt * Q.T + MZ_TILE - 1) / MZ_TILE;
    float* xs = act + Q.lds_total;
    for (int i = tid; i < Q.lds_total; i += MZ_THREADS) act[i] = 0.0f;     // padded input rows stay 0
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int slot = 0, pos = 0;
        const bool live = lane < MZ_TILE && rean_pos(Q, oldest, cnt, tile * MZ_TILE + lane, &slot, &pos);
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
            if (pos == 0) rean_mark(Q, slot);
        }
    }
}

// ResNet engines, positions [p0, p0 + pn): one wave per position writes its
// stacked observation (f32, zeros if dead) to stage_x[i][F] ...
extern "C" __global__ __launch_bounds__(256) void mz_reanalyse_gather(ReanParams Q) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= Q.pn) return;
    long long oldest;
    const int cnt = rean_games(Q, &oldest);
    float* out = Q.stage_x + (size_t)i * Q.F;
    int slot = 0, pos = 0;
    if (cnt > 0 && rean_pos(Q, oldest, cnt, Q.p0 + i, &slot, &pos)) {
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
    const int cnt = rean_games(Q, &oldest);
    int slot = 0, pos = 0;
    if (cnt <= 0 || !rean_pos(Q, oldest, cnt, Q.p0 + i, &slot, &pos)) return;
    Q.ring.rrv[(size_t)slot * Q.T + pos] = Q.stage_v[i];
    if (pos == 0) rean_mark(Q, slot);
}

// every held or stale slot back to `nothing`
extern "C" __global__ void mz_reanalyse_clear(int32_t* rean, int cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) rean[i] = 0;
}
