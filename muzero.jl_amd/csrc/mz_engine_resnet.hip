// mz_engine_resnet.hip — host side of libmz: the ResNet engine's plans and mz_engine_create_resnet.
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mz_handle.h"
#include "mz_internal.h"
#include "mz_tree_device.h"   // pbterm_count, pbterm_index (the search tables)
#include "mz_resnet_params.h"

using namespace mz;

// ------------------------------------------------------------- ResNet nets
// Row a14: the intended architecture of Learning.jl:148-255,
// op for op as oracle/mz_oracle.c onet_build_resnet, in Flux.params order:
// Conv weight (kw,kh,cin,cout) col-major, bias, BatchNorm β, γ; Dense W
// (out,in) col-major, b.
std::vector<RSpec> mz::rn_specs(const mz_config& c, const mz_resnet_hp& hp, int net, size_t* nparams) {
    const int W = c.observation_shape[0], H = c.observation_shape[1], C = c.observation_shape[2];
    const int nf = hp.num_filters, nb = hp.num_blocks, hs = hp.width_hidden, A = c.action_space_size;
    const int P = W * H, nvf = hp.num_first_head_filters, npf = hp.num_second_head_filters;
    std::vector<RSpec> v;
    size_t n = 0;
    auto conv = [&](int ch, int cin, int cout, int kw, int kh) {
        RSpec r{ch, 1, cin, cout, kw, kh, MZ_ACT_RELU, 1, 0, 0, 0, 0, 0};
        r.woff = n; n += (size_t)kw * kh * cin * cout;
        r.boff = n; n += (size_t)cout;
        r.bnoff = n; n += (size_t)2 * cout;
        v.push_back(r);
    };
    auto block = [&](int ch, int f, int kw, int kh) { conv(ch, f, f, kw, kh); v.back().res_save = 1;
                                                      conv(ch, f, f, kw, kh); v.back().res_add = 1; };
    auto dense = [&](int ch, int in, int out, int act) {
        RSpec r{ch, 0, in, out, 1, 1, act, 0, 0, 0, 0, 0, 0};
        r.woff = n; n += (size_t)in * out;
        r.boff = n; n += (size_t)out;
        v.push_back(r);
    };
    if (net == MZ_NET_REPR) {
        const int kw = hp.conv_kernel_size[0], kh = hp.conv_kernel_size[1];
        conv(0, C * (c.stacked_observations + 1) + c.stacked_observations, nf, kw, kh);
        for (int i = 0; i < nb; ++i) block(0, nf, kw, kh);
    } else if (net == MZ_NET_PRED) {
        conv(0, nf, nf, 1, 1);
        for (int i = 0; i < nb; ++i) block(0, nf, 1, 1);
        conv(1, nf, nvf, 1, 1);
        dense(1, P * nvf, hs, MZ_ACT_RELU);
        for (int i = 0; i < hp.depth_value; ++i) dense(1, hs, hs, MZ_ACT_RELU);
        dense(1, hs, 1, MZ_ACT_TANH);
        conv(2, nf, npf, 1, 1);
        dense(2, P * npf, hs, MZ_ACT_IDENTITY);
        for (int i = 0; i < hp.depth_value; ++i) dense(2, hs, hs, MZ_ACT_RELU);    // :222 depth_value
        dense(2, hs, A, MZ_ACT_IDENTITY);
    } else {
        conv(0, nf + 1, nf, 1, 1);
        for (int i = 0; i < nb; ++i) block(0, nf, 1, 1);
        conv(1, nf, nf, 1, 1);
        for (int i = 0; i < nb; ++i) block(1, nf, 1, 1);
        conv(2, nf, nvf, 1, 1);
        dense(2, P * nvf, hs, MZ_ACT_RELU);
        for (int i = 0; i < hp.depth_value; ++i) dense(2, hs, hs, MZ_ACT_RELU);
        dense(2, hs, 1, hp.reward_activation);
    }
    *nparams = n;
    return v;
}

// LDS plan of one net for a tile of NG games (floats).  Trunk: X -> B0, each
// block B0 -> B1 -> B0 (residual in place); head 1 reads B0 (the dynamics
// state head runs its tower in B2 / B1, B2 aliasing the dead input X); head 2
// reads B0 through the small buffers S0..S2; outputs O0 / O1.
// Offset table of a narrow plan's layer L with a kernel > 1x1 (MODE 4 of
// rn_layer_t): for quarter q, chunk c, column n < ncols_t and bank slot
// sl = ((n >> 2) & 3) ^ σ(kl), the byte addresses of B(k, n), k = (q·nq + 4c +
// jj)·4 + kl, jj = 0..3 — the same operand MODE 2 gathers through the k table —
// or of the zero float for taps off the board, padded steps and columns past
// the tile.  One 16-byte read gives a lane a chunk's four addresses.
static void rn_otab_fill(std::vector<int>& t, const RLayer& L, int NG, int W, int P, int ncols_t, int zero_off) {
    static const int sinv[4] = {0, 2, 3, 1};                      // σ^-1, σ = (0, 3, 1, 2)
    const int nch = ((L.nq + 3) & ~3) / 4;
    for (int q = 0; q < 4; ++q)
        for (int c = 0; c < nch; ++c)
            for (int n = 0; n < ncols_t; ++n)
                for (int sl = 0; sl < 4; ++sl)
                    for (int jj = 0; jj < 4; ++jj) {
                        const int kl = sinv[sl ^ ((n >> 2) & 3)], j = 4 * c + jj, k = (q * L.nq + j) * 4 + kl;
                        int a = zero_off;
                        if (j < L.nq && k < L.K && n < P * NG) {
                            const int ci = k / L.kk, r = k - ci * L.kk, jy = r / L.kw, ix = r - jy * L.kw;
                            const int dx = (L.kw - 1 - ix) - L.pw, dy = (L.kh - 1 - jy) - L.ph;
                            const int p = n / NG, g = n - p * NG, px = p % W + dx, py = p / W + dy;
                            if (px >= 0 && px < W && py >= 0 && py < P / W)
                                a = L.in_off + ci * P * NG + (px + W * py) * NG + g;
                        }
                        t.push_back(a * 4);
                    }
}

// mz_runroll_chain_r applies when the plane is one column block (the narrow
// tiles are one sample wide) and the dynamics chain ([0, dyn_split)) is RD_NL
// 1x1 conv layers of 64 channels with BatchNorm + relu: layer 0 on the plain
// input with 4 < nq <= 8 (nf + 1 channels: two A chunks), the others K = 64 on
// k-blocked inputs.  (A three-block variant for 4-block towers, 18 layers, kept
// 304 VGPRs resident and spilled: 1.27k vs 1.53k learner steps/s on Connect4
// ResNet-8; it was removed.)
size_t mz::rd_chain_lds(const mz_handle* h) { return h->rn_lds_l + (size_t)h->rn_dyn_split * 64 * 16; }
static bool rd_chain_ok(const mz_handle* h) {
    const RPlan& R = h->rplan_l[MZ_NET_DYN];
    if ((h->plane + 15) / 16 != 1 || h->rn_dyn_split != RD_NL) return false;
    for (int i = 0; i < h->rn_dyn_split; ++i) {
        const RLayer& L = R.L[i];
        if (L.kk != 1 || L.cout != 64 || L.n_ob != 4 || !L.spatial || !L.bn || L.act != MZ_ACT_RELU) return false;
        if (i == 0 ? (L.in_kb || L.nq <= 4 || L.nq > 8) : (!L.in_kb || L.K != 64 || L.nq != 4)) return false;
    }
    return rd_chain_lds(h) <= kLdsMax;
}
// mz_runroll_pred_r applies when the prediction trunk ([0, RP_NL), the
// first head layer next) is RP_NL such layers, all on k-blocked inputs
size_t mz::rp_pred_lds(const mz_handle* h) { return h->rn_lds_l + (size_t)RP_NL * 64 * 16; }
static bool rp_pred_ok(const mz_handle* h) {
    const RPlan& R = h->rplan_l[MZ_NET_PRED];
    if ((h->plane + 15) / 16 != 1 || R.n <= RP_NL || R.L[RP_NL].cout == 64) return false;
    if (2 * h->rhp.num_blocks + 1 != RP_NL) return false;
    for (int i = 0; i < RP_NL; ++i) {
        const RLayer& L = R.L[i];
        if (L.kk != 1 || L.cout != 64 || L.n_ob != 4 || !L.spatial || !L.bn || L.act != MZ_ACT_RELU ||
            !L.in_kb || L.K != 64 || L.nq != 4)
            return false;
    }
    // the heads in rn_specs order: value [RP_NL, RP_NL + nv), policy after (the fused
    // launch runs them in separate blocks)
    const int nv = 3 + h->rhp.depth_value;
    if (R.n != RP_NL + 2 * nv || R.L[RP_NL].cout != h->rhp.num_first_head_filters ||
        R.L[RP_NL + nv].cout != h->rhp.num_second_head_filters || R.L[RP_NL + nv - 1].cout != 1)
        return false;
    return rp_pred_lds(h) <= kLdsMax;
}

static RPlan rn_plan(const mz_handle* h, const std::vector<RSpec>& sp, int net, int NG, size_t flat_off,
                     int& w_img, std::vector<int>* srcw, bool sep_b2 = false, std::vector<int>* otab = nullptr) {
    const mz_config& c = h->rconf;
    const int W = c.observation_shape[0], Hh = c.observation_shape[1], P = W * Hh;
    const int nf = h->rhp.num_filters, hs = h->rhp.width_hidden;
    const int in_feat = net == MZ_NET_REPR ? h->rin_feat : net == MZ_NET_PRED ? h->H : h->H + h->plane;
    const int big = nf * P * NG;
    int off = 0;
    auto region = [&](int n) { int o = off; off += (n + 3) / 4 * 4; return o; };
    RPlan R;
    std::memset(&R, 0, sizeof(R));
    // the dynamics state head's B2 aliases the dead input X, or (sep_b2, when the
    // LDS allows) has its own region, so that its layout can be k-blocked
    const int X = region(std::max(in_feat * NG, net == MZ_NET_DYN && !sep_b2 ? big : 0));
    const int B0 = region(big), B1 = region(big);
    // (aliased, B2 sits at the END of X's region, at a different offset from X:
    // a region's layout follows the readers of its offset, so B2 can be
    // k-blocked for the state head's 1x1 convs while X stays plain for the
    // K = nf + 1 first layer; X is dead once that layer has run)
    const int xsz = (std::max(in_feat * NG, net == MZ_NET_DYN && !sep_b2 ? big : 0) + 3) / 4 * 4;
    const int B2 = net == MZ_NET_DYN && sep_b2 ? region(big) : X + (xsz - big) / 4 * 4;
    // the head convs write S0 (every conv off the trunk but the dynamics state head's tower, which
    // runs in B2 / B1); their width is a hyperparameter of its own and may equal num_filters
    int headc = 0;
    for (const RSpec& r : sp)
        if (r.chain && r.conv && !(net == MZ_NET_DYN && r.chain == 1)) headc = std::max(headc, r.cout * P * NG);
    const int S0 = region(std::max(headc, hs * NG)), S1 = region(hs * NG), S2 = region(hs * NG);
    const int O0 = net == MZ_NET_PRED ? region(NG) : B0;             // REPR / DYN out0 = h (B0 / B2)
    const int O1 = net == MZ_NET_REPR ? 0 : region((net == MZ_NET_PRED ? h->A : 1) * NG);
    R.in_off = X; R.in_feat = in_feat;
    int cur[3] = {X, B0, B0};                                        // current input of each chain
    int ping[3] = {0, S1, S1};
    for (size_t i = 0; i < sp.size(); ++i) {
        const RSpec& r = sp[i];
        RLayer& L = R.L[R.n++];
        L.kk = r.kw * r.kh; L.kw = r.kw; L.kh = r.kh; L.pw = r.kw / 2; L.ph = r.kh / 2;
        L.K = r.conv ? r.kw * r.kh * r.cin : r.cin;
        L.cout = r.cout; L.nq = (L.K + 15) / 16; L.n_ob = (r.cout + 15) / 16;
        L.spatial = r.conv; L.act = r.act; L.bn = r.bn; L.res_add = r.res_add;
        L.boff = (int)(flat_off + r.boff); L.bnoff = (int)(flat_off + r.bnoff);
        L.ktab = -1;
        L.in_off = cur[r.chain];
        const bool last_in_chain = i + 1 == sp.size() || sp[i + 1].chain != r.chain;
        if (r.chain == 0) {
            if (r.res_add) { L.out_off = B0; L.res_off = B0; L.in_off = B1; }
            else if (r.res_save) L.out_off = B1;
            else L.out_off = B0;
            cur[0] = r.res_save ? B1 : B0;
            if (r.res_add) cur[0] = B0;
            if (last_in_chain) { cur[1] = cur[2] = B0; }
        } else if (r.chain == 1 && net == MZ_NET_DYN) {            // state head tower in B2 / B1
            if (r.res_add) { L.in_off = B1; L.out_off = B2; L.res_off = B2; }
            else if (r.res_save) { L.out_off = B1; }
            else L.out_off = B2;
            cur[1] = r.res_save ? B1 : B2;
        } else {                                                    // conv head -> Dense chain
            if (last_in_chain) L.out_off = r.chain == 1 ? O0 : O1;
            else if (r.conv) L.out_off = S0;
            else { L.out_off = ping[r.chain]; ping[r.chain] = ping[r.chain] == S1 ? S2 : S1; }
            cur[r.chain] = L.out_off;
        }
        // A fragments [ob][q][j/4][lane][j%4] (NQ padded to NQ4 = 4⌈NQ/4⌉ with
        // zeros): one 16-byte load gives a lane four k-steps of a quarter chain
        L.w_img = w_img;
        const int nq4 = (L.nq + 3) & ~3;
        for (int ob = 0; ob < L.n_ob; ++ob)
            for (int q = 0; q < 4; ++q)
                for (int jc = 0; jc < nq4 / 4; ++jc)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int jj = 0; jj < 4; ++jj) {
                            const int j = 4 * jc + jj;
                            const int o = ob * 16 + (lane & 15), k = (q * L.nq + j) * 4 + (lane >> 4);
                            int src = -1;
                            if (j < L.nq && o < r.cout && k < L.K)
                                src = (int)(flat_off + r.woff + (r.conv ? (size_t)k + (size_t)L.K * o
                                                                        : (size_t)o + (size_t)r.cout * k));
                            if (srcw) srcw->push_back(src);
                        }
        w_img += L.n_ob * 4 * nq4 * 64;
        // epilogue image: per output row o, {bias, γ, β, 0} (a lane's four rows
        // are four 16-byte loads; ADAM scatters into it through the same inverse map)
        L.ep_img = w_img;
        for (int o = 0; o < L.n_ob * 16; ++o) {
            const bool in = o < r.cout;
            const int e[4] = {in ? (int)(flat_off + r.boff + o) : -1,
                              in && r.bn ? (int)(flat_off + r.bnoff + r.cout + o) : -1,
                              in && r.bn ? (int)(flat_off + r.bnoff + o) : -1, -1};
            if (srcw) for (int x = 0; x < 4; ++x) srcw->push_back(e[x]);
        }
        w_img += L.n_ob * 16 * 4;
        if (L.kk > 1 && !otab) L.ktab = region(L.K);
    }
    // layouts, per LDS region: k-blocked when every layer that reads the region
    // as its B operand is a 1x1 conv / Dense with K % 64 == 0 (a region's
    // layout never changes, so in-place residual blocks and aliased regions
    // stay consistent); the final outputs are checked plain below
    auto capable = [&](const RLayer& L) { return L.kk == 1 && L.K % 64 == 0; };
    // (the k-blocked position of an element depends on the column count, so a region a conv
    // writes, P·NG columns, and a Dense layer reads as its flattened features, NG columns,
    // stays plain, where the two agree: a head conv whose P·cout is a multiple of 64)
    auto kb = [&](int off) {
        bool any = false, all = true, dense_in = false, conv_out = false;
        for (int j = 0; j < R.n; ++j) {
            if (R.L[j].in_off == off) { any = true; all &= capable(R.L[j]); dense_in |= !R.L[j].spatial; }
            if (R.L[j].out_off == off) conv_out |= R.L[j].spatial != 0;
        }
        return (int)(any && all && !(dense_in && conv_out));
    };
    R.in_kb = kb(X);
    for (int j = 0; j < R.n; ++j) {
        R.L[j].in_kb = kb(R.L[j].in_off);
        R.L[j].out_kb = kb(R.L[j].out_off);
        R.L[j].res_kb = R.L[j].res_add ? kb(R.L[j].res_off) : 0;
    }
    if (net == MZ_NET_REPR) { R.out0_off = B0; R.out0_n = h->H; R.out1_n = 0; }
    else if (net == MZ_NET_PRED) { R.out0_off = O0; R.out0_n = 1; R.out1_off = O1; R.out1_n = h->A; }
    else { R.out0_off = B2; R.out0_n = h->H; R.out1_off = O1; R.out1_n = 1; }
    R.out0_act = R.out1_act = MZ_ACT_IDENTITY;
    for (int j = 0; j < R.n; ++j) {
        if (R.L[j].out_off == R.out0_off) R.out0_act = R.L[j].act;
        if (R.out1_n && R.L[j].out_off == R.out1_off) R.out1_act = R.L[j].act;
    }
    if (otab) {   // narrow plans: offset tables for the kernels > 1x1 (shared by layers of the same input / shape)
        const int n_nb = (P * NG + 15) >> 4, nbw = n_nb == 1 ? 1 : n_nb == 2 ? 2 : 3;
        const int ncols_t = (n_nb + nbw - 1) / nbw * nbw * 16;
        const int zero = region(4);
        std::vector<int> t;
        std::vector<std::pair<std::vector<int>, int>> seen;      // (in_off, K, kw, kh) -> table offset in t
        for (int i = 0; i < R.n; ++i) {
            RLayer& L = R.L[i];
            if (L.kk == 1) continue;
            const std::vector<int> key = {L.in_off, L.K, L.kw, L.kh};
            int at = -1;
            for (auto& e : seen) if (e.first == key) at = e.second;
            if (at < 0) { at = (int)t.size(); seen.push_back({key, at}); rn_otab_fill(t, L, NG, W, P, ncols_t, zero); }
            L.ktab = at;                                           // relative until the region is placed
            L.otab = 1;
        }
        if (!t.empty() && (size_t)(off + t.size() + 16 * 16 * 4) * 4 <= kLdsMax) {
            R.tab_lds = region((int)t.size());
            R.tab_n = (int)t.size();
            R.tab_src = (int)otab->size();
            R.zero_off = zero;
            otab->insert(otab->end(), t.begin(), t.end());
            for (int i = 0; i < R.n; ++i) if (R.L[i].otab) R.L[i].ktab += R.tab_lds;
        } else {                                                   // does not fit: the k-table gather (MODE 2)
            for (int i = 0; i < R.n; ++i) if (R.L[i].otab) { R.L[i].otab = 0; R.L[i].ktab = -1; }
        }
        for (int i = 0; i < R.n; ++i)                              // k tables for the layers that still need one
            if (R.L[i].kk > 1 && !R.L[i].otab && R.L[i].ktab < 0) R.L[i].ktab = region(R.L[i].K);
    }
    region(16 * 16 * 4);           // slack: past-the-tile lanes of k-blocked reads (MODE 3) read up to 15 columns on
    R.n_ktab = 0;
    for (int j = 0; j < R.n; ++j) R.n_ktab += R.L[j].kk > 1 && !R.L[j].otab;
    R.lds_floats = off;
    R.out0_kb = kb(R.out0_off);
    for (int j = 0; j < R.n; ++j) R.k[j] = rn_rk_pack(R.L[j]);
    if ((R.out0_kb && net == MZ_NET_PRED) || (R.out1_n && kb(R.out1_off))) R.n = -1;   // (never: read as plain)
    return R;
}

// The packed layer entry (rn_rk_pack) carries a layer's k table / offset table LDS offset in
// 16 signed bits: a plan whose table lies past 32767 does not run (a narrower tile may)
static bool rn_ktab_ok(const RPlan& R) {
    for (int j = 0; j < R.n; ++j)
        if (R.L[j].kk > 1 && R.L[j].ktab > 32767) return false;
    return true;
}

// pUCT tables (libm log2/sqrt on the host: the values the oracle computes
// inline), the action-plane values a/|A|, and the pb_term triangle
static int alloc_search_tables(mz_handle* h) {
    const mz_config& c = h->conf;
    const int S = h->S, A = h->A;
    std::vector<double> pbc(S + 2), sq(S + 2);
    for (int n = 0; n < S + 2; ++n) {
        pbc[n] = std::log2((double)(n + c.pb_c_base + 1) / (double)c.pb_c_base) + (double)c.pb_c_init;
        sq[n] = std::sqrt((double)n);
    }
    std::vector<float> av(A);
    for (int a = 0; a < A; ++a) av[a] = (float)((double)(a + 1) / (double)A);
    std::vector<double> pbt(pbterm_count(S), 0.0);
    for (int np = 0; np <= S + 1; ++np)
        for (int nc = 0; nc <= np; ++nc) pbt[pbterm_index(np, nc)] = pbc[np] * (sq[np] / (double)(nc + 1));
    MZ_TRY(h, dalloc(h, &h->d_pbc, pbc.size()));
    MZ_TRY(h, dalloc(h, &h->d_sqrt, sq.size()));
    MZ_TRY(h, dalloc(h, &h->d_aval, av.size()));
    MZ_TRY(h, dalloc(h, &h->d_pbterm, pbt.size()));
    MZ_TRY(h, hipMemcpy(h->d_pbc, pbc.data(), pbc.size() * 8, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_sqrt, sq.data(), sq.size() * 8, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_aval, av.data(), av.size() * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_pbterm, pbt.data(), pbt.size() * 8, hipMemcpyHostToDevice));
    return 0;
}

// loss / Σθ² scratch, per-net offsets and the last-block counter of
// mz_learner_grad_kernel
int mz::alloc_learner(mz_handle* h) {
    MZ_TRY(h, dalloc(h, &h->d_loss, 8));
    MZ_TRY(h, dalloc(h, &h->d_sq, 3 * MZ_L2_BLOCKS));
    size_t oc[6] = {h->flat_off[0], h->flat_off[1], h->flat_off[2], h->nparams[0], h->nparams[1], h->nparams[2]};
    MZ_TRY(h, dalloc(h, &h->d_netoff, 6));
    MZ_TRY(h, dalloc(h, &h->d_counter, 1));
    MZ_TRY(h, hipMemset(h->d_counter, 0, 4));
    MZ_TRY(h, dalloc(h, &h->d_fault, 1));
    MZ_TRY(h, hipMemset(h->d_fault, 0, 4));
    // debug (tests/test_fault_gpu.py): MZ_DEBUG_SKIP_PUBLISH=1 at create makes
    // tile / sample 0 of the cross-workgroup hand-offs skip its publish, with a
    // 10 ms poll bound, so the reported fault can be tested
    if (std::getenv("MZ_DEBUG_SKIP_PUBLISH")) { h->dbg_skip = 0; h->poll_ticks = 1000000ull; }
    MZ_TRY(h, hipMemcpy(h->d_netoff, oc, sizeof(oc), hipMemcpyHostToDevice));
    return 0;
}

size_t mz::rsearch_root_lds(const mz_handle* h) {
    const int gw = h->A > 16 ? 32 : 16;     // softmax / noise staging [16][gw] x 2
    return (size_t)std::max(h->rplan[0].lds_floats, h->rplan[1].lds_floats) * 4 + (size_t)2 * 16 * gw * 4;
}

// The downsampler of Learning.jl:175-187 (op for op as oracle/mz_oracle.c
// onet_build_resnet with downsample, `size` read as conv_kernel_size):
// Conv(k, C => C, stride 2), 2 blocks, Conv(k, C => 2C, stride 2), 3 blocks,
// MeanPool((3,3), stride 2, pad 1), 3 blocks, MeanPool — then the tail
// Conv(k, 2C => nf) + BatchNorm + blocks is the RPlan of rconf.  Parameters
// (Flux.params order, first in the representation's flat vector): strided
// conv W, b; block conv W, b, β, γ.  Returns the parameter count.
static size_t ds_build(mz_handle* h, DsPlan& D) {
    const mz_config& c = h->conf;
    const int kw = h->rhp.conv_kernel_size[0], kh = h->rhp.conv_kernel_size[1];
    int C = c.observation_shape[2] * (c.stacked_observations + 1) + c.stacked_observations;
    int w = c.observation_shape[0], hh = c.observation_shape[1];
    std::memset(&D, 0, sizeof(D));
    D.in_feat = w * hh * C;
    size_t n = 0;
    int cur = -1;
    auto s2 = [](int x, int k) { return (x + 2 * (k / 2) - k) / 2 + 1; };
    auto conv = [&](int cin, int cout, int stride, int bn, int act) -> DsLayer& {
        DsLayer& L = D.L[D.n++];
        L.kind = DS_CONV; L.cin = cin; L.cout = cout; L.kw = kw; L.kh = kh; L.pw = kw / 2; L.ph = kh / 2;
        L.stride = stride; L.Wi = w; L.Hi = hh;
        L.Wo = stride == 2 ? s2(w, kw) : w; L.Ho = stride == 2 ? s2(hh, kh) : hh;
        L.act = act; L.bn = bn;
        L.woff = (int)n; n += (size_t)kw * kh * cin * cout;
        L.boff = (int)n; n += (size_t)cout;
        if (bn) { L.bnoff = (int)n; n += (size_t)2 * cout; }
        L.pn = (int)(n - (size_t)L.woff);
        D.w_floats = std::max(D.w_floats, kw * kh * cin * cout);
        w = L.Wo; hh = L.Ho;
        return L;
    };
    auto strided = [&](int cin, int cout) {
        DsLayer& L = conv(cin, cout, 2, 0, MZ_ACT_IDENTITY);
        L.in_buf = cur; L.out_buf = cur == 0 ? 1 : 0; cur = L.out_buf;
    };
    auto block = [&](int f) {
        DsLayer& a = conv(f, f, 1, 1, MZ_ACT_RELU);
        a.in_buf = cur; a.out_buf = 1 - cur;
        DsLayer& b = conv(f, f, 1, 1, MZ_ACT_RELU);
        b.in_buf = 1 - cur; b.out_buf = cur; b.res_add = 1; b.res_buf = cur;
    };
    auto pool = [&](int f) {
        DsLayer& L = D.L[D.n++];
        L.kind = DS_POOL; L.cin = f; L.cout = f; L.kw = 3; L.kh = 3; L.pw = 1; L.ph = 1; L.stride = 2;
        L.Wi = w; L.Hi = hh; L.Wo = s2(w, 3); L.Ho = s2(hh, 3); L.act = MZ_ACT_IDENTITY;
        L.in_buf = cur; L.out_buf = 1 - cur; cur = L.out_buf;
        w = L.Wo; hh = L.Ho;
    };
    strided(C, C);
    for (int i = 0; i < 2; ++i) block(C);
    strided(C, 2 * C);
    for (int i = 0; i < 3; ++i) block(2 * C);
    pool(2 * C);
    for (int i = 0; i < 3; ++i) block(2 * C);
    pool(2 * C);
    D.L[D.n - 1].out_buf = -1;                       // the last layer writes the output to HBM
    D.out_feat = w * hh * 2 * C;
    for (int i = 0; i < D.n; ++i) {
        const DsLayer& L = D.L[i];
        if (i > 0) D.buf_floats = std::max(D.buf_floats, L.cin * L.Wi * L.Hi);
        D.buf_floats = std::max(D.buf_floats, L.cout * L.Wo * L.Ho);
    }
    D.buf_floats = (D.buf_floats + 3) & ~3;
    D.w_floats = (D.w_floats + 3) & ~3;
    h->rconf = c;
    h->rconf.observation_shape[0] = w; h->rconf.observation_shape[1] = hh; h->rconf.observation_shape[2] = 2 * C;
    h->rconf.stacked_observations = 0;
    // LDS: buffer 0 | buffer 1 (from buf_floats; the staged observation for layer 0 when it fits, layer 0
    // writing buffer 0) | one conv's packed parameters | the generic conv's weights and tap tables
    for (int i = 0; i < D.n; ++i) D.pn_max = std::max(D.pn_max, D.L[i].pn);
    D.pn_max = (D.pn_max + 3) & ~3;
    const size_t gen = (size_t)D.pn_max + D.w_floats + 512;
    const size_t in4 = ((size_t)D.in_feat + 3) & ~(size_t)3;
    D.ptot = (int)(n - (size_t)D.L[0].woff);
    D.stage_in = D.L[0].kind == DS_CONV && D.L[0].in_buf < 0 && D.L[0].out_buf == 0 && D.in_feat % 4 == 0 &&
                 D.L[0].woff % 4 == 0 && (size_t)2 * D.buf_floats + D.ptot <= in4 &&
                 ((size_t)D.buf_floats + std::max<size_t>(D.buf_floats, in4) + gen) * 4 <= kLdsMax;
    D.lds_floats = (int)((size_t)D.buf_floats + (D.stage_in ? std::max<size_t>(D.buf_floats, in4) : D.buf_floats));
    h->ds_lds = ((size_t)D.lds_floats + gen) * 4;
    return n;
}

// run the downsampler over n items: x (in_feat, n) -> y (rin_feat, n); with
// per_step > 0 item i uses the parameters flat + (i / per_step)·nflat (the
// multi-step learner's per-step bank), else the engine's
// the flat bank's per-step stride (rlearner_multi): nflat rounded up to 4 floats, so the downsampler's
// float4 parameter staging (DsParams.per_step) reads 16-byte aligned rows
size_t mz::fbank_stride(const mz_handle* h) { return (h->nflat + 3) / 4 * 4; }
int mz::ds_launch(mz_handle* h, const float* x, float* y, int n, hipStream_t st, const float* flat,
                  int per_step) {
    DsParams Q;
    Q.n_items = n; Q.bn_s = h->bn_s; Q.plan = h->d_dsplan; Q.flat = h->d_flat; Q.x = x; Q.y = y;
    Q.stamps = nullptr;
    Q.per_step = per_step; Q.flat_stride = fbank_stride(h);
    if (flat) Q.flat = flat;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, 128)));
    Q.stamps = h->d_stamps;
#endif
    void* args[] = {&Q};
    MZ_TRY(h, hipLaunchKernel((const void*)mz_downsample_kernel, dim3(n), dim3(DS_THREADS), args, h->ds_lds, st));
    return 0;
}
int mz::ensure_dsb(mz_handle* h, int n) {
    if (n <= h->dsb_cap) return 0;
    if (h->d_dsb) { (void)hipFree(h->d_dsb); h->d_dsb = nullptr; }
    MZ_TRY(h, hipMalloc(&h->d_dsb, (size_t)n * h->rin_feat * 4));
    h->dsb_cap = n;
    return 0;
}
size_t mz::rsearch_nets_lds(const mz_handle* h) {
    return (size_t)std::max(h->rplan[1].lds_floats, h->rplan[2].lds_floats) * 4;
}

int mz_engine_create_resnet(const mz_config* conf, const mz_resnet_hp* hyper, int device, int max_games,
                            uint64_t rng_seed, mz_handle** out) {
    g_create_error.clear();
    if (!conf || !hyper || !out) { g_create_error = "null argument"; return -2; }
    *out = nullptr;
    mz_handle* h = new mz_handle();
    h->kind = 1; h->conf = *conf; h->rhp = *hyper; h->device = device; h->max_games = max_games;
    h->seed = rng_seed;
    auto bad = [&](const std::string& m) { g_create_error = m; delete h; return -2; };
    const mz_config& c = *conf;
    if (c.action_space_size < 1 || c.action_space_size > 32)
        return bad("action_space_size must be in 1..32 (16- or 32-lane select groups)");
    if (c.players < 1 || c.players > 2) return bad("players must be 1 or 2");
    if (c.num_iters < 1 || c.num_iters > 65000) return bad("num_iters out of range");
    if (hyper->conv_kernel_size[0] % 2 == 0 || hyper->conv_kernel_size[1] % 2 == 0 ||
        hyper->conv_kernel_size[0] > 15 || hyper->conv_kernel_size[1] > 15)
        return bad("conv_kernel_size must be odd and <= 15 (Learning.jl:164 asserts odd)");
    if (hyper->num_filters < 1 || hyper->num_blocks < 0 || hyper->width_hidden < 1) return bad("bad ResNetHP");
    if (max_games < 1) return bad("max_games must be >= 1");
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed (no GPU?)");
    const int W = c.observation_shape[0], Hh = c.observation_shape[1], C = c.observation_shape[2];
    h->obs_feat = W * Hh * (C * (c.stacked_observations + 1) + c.stacked_observations);
    h->rconf = c;
    h->A = c.action_space_size; h->S = c.num_iters;
    if (hyper->downsample) {
        h->ds = 1;
        h->ds_n = ds_build(h, h->dsplan);
        if (h->dsplan.L[0].kw * h->dsplan.L[0].kh * 2 * h->dsplan.L[0].cin > 256)
            return bad("downsampler: conv_kernel_size x 2C input channels exceeds 256 taps");
        if (h->ds_lds > kLdsMax) return bad("downsampler activations exceed the LDS");
    }
    const int rW = h->rconf.observation_shape[0], rH = h->rconf.observation_shape[1];
    h->rin_feat = h->ds ? h->dsplan.out_feat : h->obs_feat;
    h->plane = rW * rH;
    h->H = rW * rH * hyper->num_filters;
    std::vector<RSpec> sp[3];
    size_t off = 0;
    for (int n = 0; n < 3; ++n) {
        sp[n] = rn_specs(h->rconf, *hyper, n, &h->nparams[n]);
        h->flat_off[n] = off;
        if (n == MZ_NET_REPR) h->nparams[n] += h->ds_n;     // downsampler params first
        off += h->nparams[n];
    }
    h->nflat = off;
    // widest tile whose three plans fit the LDS
    for (int ng = 16; ng >= 1 && !h->rn_ng; ng /= 2) {
        int wi = 0;
        bool fits = true;
        for (int n = 0; n < 3; ++n) {
            const RPlan R = rn_plan(h, sp[n], n, ng, h->flat_off[n] + (n == 0 ? h->ds_n : 0), wi, nullptr);
            fits &= (size_t)R.lds_floats * 4 <= kLdsMax && rn_ktab_ok(R);
        }
        if (fits) h->rn_ng = ng;
    }
    if (!h->rn_ng)
        return bad("ResNet activations exceed the LDS even for one game per tile (or a k table lies past LDS "
                   "offset 32767)");
    h->bn_s = sqrtf(1.0f + 1e-5f);
    int rc = 0;
    CK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess ? 0 : fail(h, "hipStreamCreate"));
    std::vector<int> sw;
    int wi = 0;
    h->rplan.resize(3);
    for (int n = 0; n < 3; ++n) {
        {
            int wt = wi;
            const bool sep = (size_t)rn_plan(h, sp[n], n, h->rn_ng, 0, wt, nullptr, true).lds_floats * 4 <= kLdsMax;
            h->rplan[n] = rn_plan(h, sp[n], n, h->rn_ng, h->flat_off[n] + (n == 0 ? h->ds_n : 0), wi, &sw, sep);
        }
        CK(h->rplan[n].n < 0 ? fail(h, "ResNet plan: a k-blocked output buffer") : 0);
        CK(!rn_ktab_ok(h->rplan[n]) ? fail(h, "ResNet plan: a k table past LDS offset 32767") : 0);
        h->rn_lds[n] = (size_t)h->rplan[n].lds_floats * 4;
    }
    for (int n = 1; n < 3; ++n)                          // mz_rsearch_nets has no k-table path (NOKK)
        for (int i = 0; i < h->rplan[n].n; ++i) {
            const RLayer& L = h->rplan[n].L[i];
            CK(L.kk > 1 ? fail(h, "ResNet plan: a prediction / dynamics kernel > 1x1") : 0);
            // and applies a tanh only where the read-out does (RAWTANH): on the outputs
            CK(L.act == MZ_ACT_TANH && L.out_off != h->rplan[n].out0_off &&
                       !(h->rplan[n].out1_n && L.out_off == h->rplan[n].out1_off)
                   ? fail(h, "ResNet plan: a tanh layer that is not an output") : 0);
        }
    h->packed_w_n = sw.size(); h->packed_b_n = 0;
    h->rn_dyn_split = (int)sp[MZ_NET_DYN].size();     // the reward head: the dynamics layers of chain 2
    for (size_t i = 0; i < sp[MZ_NET_DYN].size(); ++i)
        if (sp[MZ_NET_DYN][i].chain == 2) { h->rn_dyn_split = (int)i; break; }
    {   // learner chain tiles: one sample wide
        const int ngl = 1;
        int wl = 0;
        h->rplan_l.resize(3);
        for (int n = 0; n < 3; ++n) {
            int wt = wl;
            const bool sep = (size_t)rn_plan(h, sp[n], n, ngl, 0, wt, nullptr, true).lds_floats * 4 <= kLdsMax;
            h->rplan_l[n] = rn_plan(h, sp[n], n, ngl, h->flat_off[n] + (n == 0 ? h->ds_n : 0), wl, nullptr, sep,
                                    &h->rtab);
            CK(h->rplan_l[n].n < 0 ? fail(h, "ResNet plan: a k-blocked output buffer") : 0);
            CK(!rn_ktab_ok(h->rplan_l[n]) ? fail(h, "ResNet learner plan: a k table past LDS offset 32767") : 0);
            h->rn_lds_l = std::max(h->rn_lds_l, (size_t)h->rplan_l[n].lds_floats * 4);
        }
        h->rd_chain = rd_chain_ok(h);
        h->rp_pred = rp_pred_ok(h);
    }
    h->inv_tile.assign(h->nflat, -1);
    for (size_t i = 0; i < sw.size(); ++i) if (sw[i] >= 0) h->inv_tile[(size_t)sw[i]] = (int)i;
    h->inv_small.assign(h->nflat, -1);
    auto al = [&](auto** p, size_t n) -> int { MZ_TRY(h, dalloc(h, p, n)); return 0; };
    auto al_i = [&](int** p, const std::vector<int>& v) -> int {
        MZ_TRY(h, dalloc(h, p, v.size()));
        MZ_TRY(h, hipMemcpy(*p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return 0;
    };
    CK(al_i(&h->d_srcW, sw));
    CK(al_i(&h->d_inv_tile, h->inv_tile));
    CK(al_i(&h->d_inv_small, h->inv_small));
    CK(al(&h->d_rplan, 3));
    CK(hipMemcpy(h->d_rplan, h->rplan.data(), 3 * sizeof(RPlan), hipMemcpyHostToDevice) == hipSuccess
           ? 0 : fail(h, "copy"));
    if (!h->rtab.empty()) CK(al_i(&h->d_rtab, h->rtab));
    CK(al(&h->d_rplan_l, 3));
    CK(hipMemcpy(h->d_rplan_l, h->rplan_l.data(), 3 * sizeof(RPlan), hipMemcpyHostToDevice) == hipSuccess
           ? 0 : fail(h, "copy"));
    CK(al(&h->d_flat, h->nflat));
    CK(al(&h->d_Wp, h->packed_w_n));
    if (h->rd_chain && h->rp_pred) {                // second image set of mz_runroll_fused_r's ADAM blocks
        CK(al(&h->d_Wp2, h->packed_w_n));
        CK(hipMemset(h->d_Wp2, 0, h->packed_w_n * 4) == hipSuccess ? 0 : fail(h, "memset"));
    }
    CK(hipMemset(h->d_flat, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(repack(h));
    CK(al(&h->d_m, h->nflat)); CK(al(&h->d_v, h->nflat)); CK(al(&h->d_grad, h->nflat));
    CK(hipMemset(h->d_m, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(hipMemset(h->d_v, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(alloc_learner(h));
    const size_t lmax = std::max(h->rn_lds[0], std::max(h->rn_lds[1], h->rn_lds[2]));
    CK(hipFuncSetAttribute((const void*)mz_rnet_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)lmax) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(rnet)"));
    CK(rsearch_root_lds(h) > kLdsMax ? fail(h, "ResNet root tile exceeds the LDS") : 0);
    CK(hipFuncSetAttribute((const void*)mz_rsearch_root, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)rsearch_root_lds(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(root)"));
    CK(hipFuncSetAttribute((const void*)mz_rsearch_root32, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)rsearch_root_lds(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(root32)"));
    if (h->ds) {
        CK(hipFuncSetAttribute((const void*)mz_downsample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)h->ds_lds) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(downsample)"));
        CK(al(&h->d_dsplan, 1));
        CK(hipMemcpy(h->d_dsplan, &h->dsplan, sizeof(DsPlan), hipMemcpyHostToDevice) == hipSuccess
               ? 0 : fail(h, "copy"));
        CK(al(&h->d_dsout, (size_t)max_games * h->rin_feat));
    }
    CK(hipFuncSetAttribute((const void*)mz_runroll_pred, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)lmax) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(runroll_pred)"));
    for (const void* k : {(const void*)mz_runroll_pred_n1, (const void*)mz_runroll_chain1})
        CK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->rn_lds_l) == hipSuccess
               ? 0 : fail(h, "hipFuncSetAttribute(runroll narrow)"));
    if (h->rd_chain)
        CK(hipFuncSetAttribute((const void*)mz_runroll_chain_r, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)rd_chain_lds(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(runroll_chain_r)"));
    if (h->rp_pred)
        CK(hipFuncSetAttribute((const void*)mz_runroll_pred_r, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)rp_pred_lds(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(runroll_pred_r)"));
    if (h->rd_chain && h->rp_pred)
        CK(hipFuncSetAttribute((const void*)mz_runroll_fused_r, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)std::max(rd_chain_lds(h), rp_pred_lds(h))) == hipSuccess
               ? 0 : fail(h, "hipFuncSetAttribute(runroll_fused_r)"));
    CK(hipFuncSetAttribute((const void*)mz_rsearch_nets, hipFuncAttributeMaxDynamicSharedMemorySize,
                           (int)rsearch_nets_lds(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(nets)"));
    // search buffers (trees and hidden states in HBM)
    {
        const size_t G = (size_t)max_games, S = (size_t)h->S, A = (size_t)h->A, H = (size_t)h->H;
        h->tree_game_bytes = tree_game_bytes(h->S, h->A);
        CK(alloc_search_tables(h));
        // +64: the tree step copies the to_play bytes as dwords (up to 3 bytes past them)
        CK(al(&h->d_tree, G * h->tree_game_bytes + 64));
        CK(al(&h->d_hid, G * (S + 1) * H));
        {
            const int gw = h->A > 16 ? 32 : 16;
            const RsTreeLds L = rs_tree_lds(h->S, h->tree_game_bytes, gw);
            h->rtree_lds = (size_t)L.total <= kLdsMax && !std::getenv("MZ_RTREE_HBM") ? (size_t)L.total : 0;
            if (h->rtree_lds)
                CK(hipFuncSetAttribute(gw == 32 ? (const void*)mz_rsearch_tree_lds32 : (const void*)mz_rsearch_tree_lds,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->rtree_lds) == hipSuccess
                       ? 0 : fail(h, "hipFuncSetAttribute(tree_lds)"));
        }
        CK(al(&h->d_rpath, G * 2 * (S + 2))); CK(al(&h->d_rgst, G * RG_INTS));
        CK(al(&h->d_rcache, G * (S + 1))); CK(al(&h->d_rnN, G * (S + 1)));
        CK(al(&h->d_rhk, G * (S + 1))); CK(al(&h->d_rov, G)); CK(al(&h->d_rologit, G * A)); CK(al(&h->d_ror, G));
        CK(al(&h->d_obs, G * h->obs_feat)); CK(al(&h->d_legal, G * A)); CK(al(&h->d_tp, G));
        CK(al(&h->d_cv, G * A)); CK(al(&h->d_rv, G)); CK(al(&h->d_act, G));
        // the network-only player's two forward launches write here (mz_prior_eval_dev)
        CK(al(&h->d_pr_h, G * (size_t)h->rplan[MZ_NET_REPR].out0_n)); CK(al(&h->d_pr_v, G));
        CK(al(&h->d_pr_p, G * A));
    }
    CK(hipStreamSynchronize(h->stream) == hipSuccess ? 0 : fail(h, "sync"));
    *out = h;
    return 0;
}
