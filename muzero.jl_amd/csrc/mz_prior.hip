// mz_prior.hip — the network-only player (AlphaZero.jl's
// NetworkOnly): a row's move is drawn from the prediction's policy at the
// root, with no tree.  (v, p) = prediction(representation(obs)) exactly as
// mz_net_forward returns them; the policy over the legal actions and the
// action are mz_prior_rules.h's, lane a of a row's group = action a.  The
// row's (π, v, action) go where a search row has its visit fractions, root
// value and action, so mz_sp_pick / mz_sp_commit and everything behind them
// read them unchanged.  The draw is the ACTION stream's, the one
// select_action takes for the same row: no new stream.
#include "mz_mlp_device.h"
#include "mz_tree_device.h"
#include "mz_selfplay_params.h"
#include "mz_prior_rules.h"

// Steps 2 and 3 of the definition for one GW-lane group, called by every lane
// of the group with its own action's p (lanes >= A: anything).  Returns π of
// this lane's action; *action = the 0-based action, in every lane.  `legal`
// is not empty; st = the group's GW floats of LDS staging.
template <int GW>
__device__ __forceinline__ float prior_group(float p, uint32_t legal, int A, float T, uint32_t r, float* st, int a,
                                             int* action) {
    legal &= A >= 32 ? 0xffffffffu : (1u << A) - 1u;
    const bool lg = (legal >> a) & 1u;
    const int n = __builtin_popcount(legal);
    const int last = 31 - __builtin_clz(legal);
    const float s = gseqsum<GW>(lg ? p : 0.0f, A, st, a);    // illegal lanes add +0
    const float pi = lg ? mzp_pi(p, s, n) : 0.0f;
    if (isinf(T)) {
        *action = mzp_kth_bit(legal, mz_rng_below(r, (uint32_t)n));
        return pi;
    }
    if (T == 0.0f) {                                  // the first maximum of π over the legal actions
        int best = -1;
        float bp = 0.0f;
#pragma unroll
        for (int b = 0; b < GW; ++b) {
            const float pb = __shfl(pi, b, GW);
            if (((legal >> b) & 1u) && (best < 0 || pb > bp)) { best = b; bp = pb; }
        }
        *action = best;
        return pi;
    }
    const float w = lg ? mzp_weight(pi, T) : 0.0f;
    float S = 0.0f;                                   // the ordered scans read the lanes by shuffle
#pragma unroll
    for (int b = 0; b < GW; ++b) {
        const float wb = __shfl(w, b, GW);
        if ((legal >> b) & 1u) S = S + wb;
    }
    const float u = mzp_u(r, S);
    float cum = 0.0f;
    int pick = -1;
#pragma unroll
    for (int b = 0; b < GW; ++b) {
        const float wb = __shfl(w, b, GW);
        if (((legal >> b) & 1u) && pick < 0) { cum = cum + wb; if (cum > u) pick = b; }
    }
    *action = pick >= 0 ? pick : last;
    return pi;
}

// a row's legal mask from its A bytes
__device__ __forceinline__ uint32_t prior_legal(const uint8_t* legal, int A) {
    uint32_t m = 0;
    for (int b = 0; b < A; ++b) if (legal[b]) m |= 1u << b;
    return m;
}

// FC engines (A <= 16).  One workgroup per tile of MZ_TILE rows: the stacked
// observations go to the plan's x_rep columns, the root plan (representation,
// then prediction from h_out) runs with run_plan as in the search's root and
// mz_reanalyse_fc, and the tile's sixteen 16-lane groups finish their rows:
// the policy head's softmax over all A logits (max, det_expf, ascending f32
// sum, divide: mz_forward_kernel's), then prior_group.  No tree, no scratch,
// no atomics.  LDS: lds_total floats of the activation layout, [16][16]
// floats of seqsum staging, 16 legal masks.
extern "C" __global__ __launch_bounds__(MZ_THREADS) void mz_prior_fc(PriorParams Q) {
    extern __shared__ __attribute__((aligned(16))) float act[];
    float* stage = act + Q.lds_total;
    uint32_t* sg_legal = reinterpret_cast<uint32_t*>(stage + MZ_TILE * 16);
    const int tid = threadIdx.x;
    const int g = tid >> 4, a = tid & 15;
    const int A = Q.A;
    const int tile0 = blockIdx.x * MZ_TILE;
    const int gg = tile0 + g;
    const bool active = gg < Q.G;
    for (int i = tid; i < Q.lds_total; i += MZ_THREADS) act[i] = 0.0f;     // padded input rows stay 0
    __syncthreads();
    for (int i = tid; i < MZ_TILE * Q.obs_feat; i += MZ_THREADS) {
        const int gl = i / Q.obs_feat, k = i - gl * Q.obs_feat;
        const int ggl = tile0 + gl;
        act[Q.x_rep + k * 16 + gl] = ggl < Q.G ? Q.obs[(size_t)ggl * Q.obs_feat + k] : 0.0f;
    }
    if (a == 0) {                                     // a row past G, or one with no legal action: every action
        const uint32_t m = active ? prior_legal(Q.legal + (size_t)gg * A, A) : 0u;
        sg_legal[g] = m ? m : (1u << A) - 1u;         // (A <= 16) — its result is not written
    }
    __syncthreads();
    run_plan(Q.plan_root, Q.Wp, Q.Bp, act);          // ends in a barrier
    const uint32_t legal = sg_legal[g];
    float* st = stage + 16 * g;
    const bool in = a < A;
    const float x = in ? act[Q.p_out + a * 16 + g] : -INFINITY;
    const float m = gmax<16>(x);
    const float ex = in ? det_expf(x - m) : 0.0f;
    const float s = gseqsum<16>(ex, A, st, a);
    const float p = in ? ex / s : 0.0f;
    const uint32_t r = mz_rng_u32(Q.seed, MZ_RNG_ACTION, Q.game_offset + (uint32_t)gg, Q.rng_step, 0);
    const float T = Q.temp_g ? Q.temp_g[active ? gg : 0] : Q.temperature;
    int action;
    const float pi = prior_group<16>(p, legal, A, T, r, st, a, &action);
    if (active) {
        if (in) Q.policy[(size_t)gg * A + a] = pi;
        if (a == 0) {
            Q.value[gg] = mz_post_act(Q.v_act, act[Q.v_out + g]);
            Q.action[gg] = action + 1;
        }
    }
}

// ResNet engines: after the downsampler (where the engine has one) and the two
// mz_rnet_forward_kernel launches (REPR, then PRED with its softmax) wrote
// p [G][A] and v [G], one GW-lane group per row finishes it.  GW = 32 where
// A > 16.  The staging is the workgroup's own 256 floats.
template <int GW>
__device__ __forceinline__ void prior_pick_body(const PriorParams& Q) {
    __shared__ __attribute__((aligned(16))) float stage[256];
    const int tid = threadIdx.x;
    const int g = tid / GW, a = tid % GW;
    const int A = Q.A;
    const int gg = blockIdx.x * (256 / GW) + g;
    const bool active = gg < Q.G;
    const size_t row = (size_t)(active ? gg : 0);
    uint32_t legal = 0;
    if (a < A && Q.legal[row * A + a]) legal = 1u << a;
    legal = gor<GW>(legal);
    if (!legal) legal = A >= 32 ? 0xffffffffu : (1u << A) - 1u;            // not written: see mz_prior_fc
    const float p = a < A ? Q.p[row * A + a] : 0.0f;
    const uint32_t r = mz_rng_u32(Q.seed, MZ_RNG_ACTION, Q.game_offset + (uint32_t)gg, Q.rng_step, 0);
    const float T = Q.temp_g ? Q.temp_g[row] : Q.temperature;
    int action;
    const float pi = prior_group<GW>(p, legal, A, T, r, stage + GW * g, a, &action);
    if (active) {
        if (a < A) Q.policy[row * A + a] = pi;
        if (a == 0) { Q.value[gg] = Q.v[gg]; Q.action[gg] = action + 1; }
    }
}
extern "C" __global__ __launch_bounds__(256) void mz_prior_pick(PriorParams Q) { prior_pick_body<16>(Q); }
extern "C" __global__ __launch_bounds__(256) void mz_prior_pick32(PriorParams Q) { prior_pick_body<32>(Q); }
