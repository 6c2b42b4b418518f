// mz_prior_rules.h — the network-only player: the policy over
// the legal actions and the action it plays, from the prediction's policy p
// (the policy head's softmax over all A actions, what mz_net_forward returns).
// Plain C++17 and HIP: the scalar pieces run in the lanes of mz_prior_fc /
// mz_prior_pick (mz_prior.hip), and the serial mzp_row below is the same rule
// on one thread, for the CPU sanitizer harness (tests/sanitize/
// prior_rules_main.cpp).  Python mirror: selfplay.prior_policy / prior_pick.
//
// Definition (one row: p[0..A), a non-empty legal set, temperature T >= 0 or
// +inf, the row's ACTION draw r — the one select_action takes in a search):
//   policy  s = the ascending f32 sum of p[a] over the legal a (an illegal a adds +0);
//           π[a] = p[a] / s for a legal a, 0 for an illegal one; s == 0 (every
//           legal p underflowed): π[a] = 1.0f / (float)n_legal for a legal a.
//   action  T == 0: the first maximum of π over the legal actions.
//           T == +inf: the mz_rng_below(r, n_legal)-th legal action.
//           else w[a] = π[a] at T == 1, and at any other T
//             w[a] = (float)det_exp(det_log((double)π[a]) · (double)(1.0f / T))
//           where π[a] > 0, else 0; S = the ascending f32 sum of w over the
//           legal a; u = (float)(r >> 8) · 2^-24 · S; the first legal b whose
//           running f32 sum exceeds u, else the last legal action (a defensive
//           end: the running sum ends at S, and S > u unless S is 0 or so small
//           a subnormal that u rounds up to it; π of the policy step sums to
//           about 1, so neither arises from it).
// Actions are 0-based here; the engine's outputs add 1.
#pragma once
#include <stdint.h>

#include "../../include/mz_detmath.h"

// π[a] of a legal action from its p, the legal sum s and the legal count n
MZ_HD float mzp_pi(float p, float s, int n) { return s == 0.0f ? 1.0f / (float)n : p / s; }

// w[a] of a legal action at a finite T > 0
MZ_HD float mzp_weight(float pi, float T) {
    if (T == 1.0f) return pi;
    return pi > 0.0f ? (float)det_exp(det_log((double)pi) * (double)(1.0f / T)) : 0.0f;
}

// u of the categorical draw from the weights' sum S
MZ_HD float mzp_u(uint32_t r, float S) { return (float)(r >> 8) * 5.9604644775390625e-08f * S; }

// the k-th (0-based, ascending) set bit of m; k < popcount(m).  (nth_set_bit of mz_tree_device.h, restated:
// this header also compiles on the host without the device headers, for the CPU harness.)
MZ_HD int mzp_kth_bit(uint32_t m, uint32_t k) {
    for (; k > 0; --k) m &= m - 1;
    return __builtin_ctz(m);
}

// One row on one thread: writes π to pi_out[0..A) and returns the 0-based
// action, -1 for an empty legal set, A outside 1..32, or a T that is negative or NaN.
static inline int mzp_row(const float* p, const uint8_t* legal, int A, float T, uint32_t r, float* pi_out) {
    if (A < 1 || A > 32 || !(T >= 0.0f)) return -1;
    uint32_t m = 0;
    for (int a = 0; a < A; ++a) m |= (uint32_t)(legal[a] != 0) << a;
    if (!m) return -1;
    const int n = __builtin_popcount(m), last = 31 - __builtin_clz(m);
    float s = 0.0f;
    for (int a = 0; a < A; ++a) s = s + (((m >> a) & 1u) ? p[a] : 0.0f);
    for (int a = 0; a < A; ++a) pi_out[a] = ((m >> a) & 1u) ? mzp_pi(p[a], s, n) : 0.0f;
    if (T == 0.0f) {
        int best = -1;
        for (int a = 0; a < A; ++a)
            if (((m >> a) & 1u) && (best < 0 || pi_out[a] > pi_out[best])) best = a;
        return best;
    }
    if (isinf(T)) return mzp_kth_bit(m, mz_rng_below(r, (uint32_t)n));
    float S = 0.0f;
    for (int a = 0; a < A; ++a)
        if ((m >> a) & 1u) S = S + mzp_weight(pi_out[a], T);
    const float u = mzp_u(r, S);
    float cum = 0.0f;
    for (int a = 0; a < A; ++a)
        if ((m >> a) & 1u) {
            cum = cum + mzp_weight(pi_out[a], T);
            if (cum > u) return a;
        }
    return last;
}
