// mz_engine.hip — host side of libmz: the C ABI of include/mz.h.
//
// Builds the layer/plan description of the FeedForwardHP networks
// (Learning.jl:87-142), packs Flux-order weights into the MFMA fragment
// image, owns every device buffer of one engine (one handle per GPU), and
// launches the search / forward / learner kernels on the handle's stream.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mz_internal.h"
#include "mz_tree_device.h"   // tree_bytes (tree layout shared with the kernels)

#include "mz_small_params.h"
#include "mz_resnet_params.h"
#include "mz_backprop_params.h"
#include "mz_selfplay_params.h"
#include "mz_expert_rules.h"
#include "mz_mcts_rules.h"
#include "mz_ckpt_iface.h"
#include "mz_snap_iface.h"
#include "mz_handle.h"

using namespace mz;

thread_local std::string g_create_error;

static int timing_events(mz_handle* h, hipEvent_t* e0, hipEvent_t* e1);

// ------------------------------------------------------------ specs & plans
static void add_layer(mz_handle* h, int net, int chain, int in, int out, int act, bool bn = false) {
    LayerSpec L;
    L.net = net; L.chain = chain; L.in = in; L.out = out; L.act = act;
    L.flux_w = h->flat_off[net] + h->nparams[net]; h->nparams[net] += (size_t)in * out;
    L.flux_b = h->flat_off[net] + h->nparams[net]; h->nparams[net] += (size_t)out;
    if (bn) { L.bn = 1; L.flux_be = h->flat_off[net] + h->nparams[net]; h->nparams[net] += (size_t)2 * out; }
    L.nq = (in + 15) / 16;
    L.n_ob = (out + 15) / 16;
    L.packed_w = (int)h->packed_w_n; h->packed_w_n += (size_t)L.n_ob * 4 * L.nq * 64;
    // packed bias image: b, then (BatchNorm) γ and β, each n_ob*16 entries
    L.packed_b = (int)h->packed_b_n; h->packed_b_n += (size_t)L.n_ob * 16 * (bn ? 3 : 1);
    h->chains[net][chain].push_back((int)h->layers.size());
    h->layers.push_back(L);
}

// init_representation / init_prediction / init_dynamics (Learning.jl:87-142)
static void build_specs(mz_handle* h) {
    const mz_config& c = h->conf;
    const mz_ffhp& p = h->hp;
    const int W = c.observation_shape[0], Hh = c.observation_shape[1], C = c.observation_shape[2];
    const int hs = p.width_hidden, hid = p.hidden_state_size, A = c.action_space_size;
    h->obs_feat = W * Hh * (C * (c.stacked_observations + 1) + c.stacked_observations);   // :88
    h->plane = W * Hh;
    h->H = hid; h->A = A; h->S = c.num_iters;
    const bool bn = p.use_batch_norm != 0;                 // make_dense (Learning.jl:70-78)
    // repr
    h->flat_off[MZ_NET_REPR] = 0;
    add_layer(h, MZ_NET_REPR, CH_TRUNK, h->obs_feat, hs, MZ_ACT_RELU, bn);
    for (int i = 0; i < p.depth_representation; ++i) add_layer(h, MZ_NET_REPR, CH_TRUNK, hs, hs, MZ_ACT_RELU, bn);
    add_layer(h, MZ_NET_REPR, CH_TRUNK, hs, hid, MZ_ACT_IDENTITY);
    // pred
    h->flat_off[MZ_NET_PRED] = h->nparams[MZ_NET_REPR];
    add_layer(h, MZ_NET_PRED, CH_TRUNK, hid, hs, MZ_ACT_RELU, bn);
    for (int i = 0; i < p.depth_prediction; ++i) add_layer(h, MZ_NET_PRED, CH_TRUNK, hs, hs, MZ_ACT_RELU, bn);
    for (int i = 0; i < p.depth_value; ++i) add_layer(h, MZ_NET_PRED, CH_HEAD1, hs, hs, MZ_ACT_RELU, bn);
    add_layer(h, MZ_NET_PRED, CH_HEAD1, hs, 1, MZ_ACT_TANH);
    for (int i = 0; i < p.depth_policy; ++i) add_layer(h, MZ_NET_PRED, CH_HEAD2, hs, hs, MZ_ACT_RELU, bn);
    add_layer(h, MZ_NET_PRED, CH_HEAD2, hs, A, MZ_ACT_IDENTITY);
    // dyn
    h->flat_off[MZ_NET_DYN] = h->flat_off[MZ_NET_PRED] + h->nparams[MZ_NET_PRED];
    add_layer(h, MZ_NET_DYN, CH_TRUNK, W * Hh * (C + 1), hs, MZ_ACT_RELU, bn);                 // :120
    for (int i = 0; i < p.depth_dynamics; ++i) add_layer(h, MZ_NET_DYN, CH_TRUNK, hs, hs, MZ_ACT_RELU, bn);
    for (int i = 0; i < p.depth_state_head; ++i) add_layer(h, MZ_NET_DYN, CH_HEAD1, hs, hs, MZ_ACT_RELU, bn);
    add_layer(h, MZ_NET_DYN, CH_HEAD1, hs, hid, MZ_ACT_IDENTITY);
    for (int i = 0; i < p.depth_reward; ++i) add_layer(h, MZ_NET_DYN, CH_HEAD2, hs, hs, MZ_ACT_RELU, bn);
    add_layer(h, MZ_NET_DYN, CH_HEAD2, hs, 1, p.reward_activation);
    h->nflat = h->flat_off[MZ_NET_DYN] + h->nparams[MZ_NET_DYN];

    // LDS activation layout (floats), every region [rows][16]
    int off = 0;
    auto region = [&](int rows) { int o = off; off += rows * 16; return o; };
    auto in_rows = [&](int net) { return 16 * h->layers[h->chains[net][CH_TRUNK][0]].nq; };
    h->lay.rows_rep = in_rows(MZ_NET_REPR);
    h->lay.rows_pred = in_rows(MZ_NET_PRED);
    h->lay.rows_dyn = in_rows(MZ_NET_DYN);
    h->lay.x_pred = region(h->lay.rows_pred);
    h->lay.x_dyn = region(h->lay.rows_dyn);
    h->lay.h_out = region(mz_round16(hid));
    h->lay.v_out = region(16);
    h->lay.p_out = region(mz_round16(A));
    h->lay.r_out = region(16);
    auto chain_bufs = [&](int net) {
        for (int ch = 0; ch < 3; ++ch) {
            int rows = 0;
            for (int li : h->chains[net][ch]) rows = std::max(rows, 16 * h->layers[li].n_ob);
            if (rows == 0) { h->chain_buf[net][ch][0] = h->chain_buf[net][ch][1] = -1; continue; }
            h->chain_buf[net][ch][0] = region(rows);
            h->chain_buf[net][ch][1] = region(rows);
        }
    };
    chain_bufs(MZ_NET_PRED);
    // the representation (input + chain) only runs before / apart from the
    // dynamics net in every plan: they share one LDS union
    const int u0 = off;
    chain_bufs(MZ_NET_DYN);
    const int dyn_end = off;
    off = u0;
    h->lay.x_rep = region(h->lay.rows_rep);
    chain_bufs(MZ_NET_REPR);
    off = std::max(off, dyn_end);
    h->lay.total = off;
}

// Place chain `ch` of `net` in plan `pb` from stage `st0`; returns the end stage.
static int place_chain(mz_handle* h, PlanBuild& pb, int net, int ch, int st0, int in_first, int out_last) {
    const std::vector<int>& ls = h->chains[net][ch];
    const int n = (int)ls.size();
    pb.ensure(st0 + n);
    for (int i = 0; i < n; ++i) {
        const LayerSpec& S = h->layers[ls[i]];
        LayerDesc d;
        d.w_off = S.packed_w; d.b_off = S.packed_b; d.nq = S.nq; d.n_ob = S.n_ob; d.act = S.act; d.bn = S.bn;
        d.in_off = i == 0 ? in_first : h->chain_buf[net][ch][(i - 1) & 1];
        d.out_off = i == n - 1 ? out_last : h->chain_buf[net][ch][i & 1];
        d.out_rows = S.out;
        // value / reward heads' output activation is applied at read-out
        if (i == n - 1 && ch == CH_HEAD1 && net == MZ_NET_PRED) { h->lay.v_act = d.act; d.act = MZ_ACT_IDENTITY; }
        if (i == n - 1 && ch == CH_HEAD2 && net == MZ_NET_DYN) { h->lay.r_act = d.act; d.act = MZ_ACT_IDENTITY; }
        const int di = (int)pb.layers.size();
        pb.layers.push_back(d);
        for (int ob = 0; ob < S.n_ob; ++ob) pb.stages[st0 + i].push_back({di, ob});
    }
    return st0 + n;
}
static int trunk_out(mz_handle* h, int net) {
    const int n = (int)h->chains[net][CH_TRUNK].size();
    return h->chain_buf[net][CH_TRUNK][(n - 1) & 1];
}
// A two-headed net (pred / dyn) from stage st0 with trunk input `in`.
static int place_split_net(mz_handle* h, PlanBuild& pb, int net, int st0, int in) {
    const int t = place_chain(h, pb, net, CH_TRUNK, st0, in, trunk_out(h, net));
    const int to = trunk_out(h, net);
    int e1, e2;
    if (net == MZ_NET_PRED) {
        e1 = place_chain(h, pb, net, CH_HEAD1, t, to, h->lay.v_out);
        e2 = place_chain(h, pb, net, CH_HEAD2, t, to, h->lay.p_out);
    } else {
        e1 = place_chain(h, pb, net, CH_HEAD1, t, to, h->lay.h_out);
        e2 = place_chain(h, pb, net, CH_HEAD2, t, to, h->lay.r_out);
    }
    return std::max(e1, e2);
}

static int upload_plan(mz_handle* h, const PlanBuild& pb, int** dst) {
    std::vector<int> img = pb.image();
    MZ_TRY(h, dalloc(h, dst, img.size()));
    MZ_TRY(h, hipMemcpy(*dst, img.data(), img.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

static int build_plans(mz_handle* h) {
    PlanBuild repr, pred, dyn, root, sim;
    place_chain(h, repr, MZ_NET_REPR, CH_TRUNK, 0, h->lay.x_rep, h->lay.h_out);
    place_split_net(h, pred, MZ_NET_PRED, 0, h->lay.x_pred);
    place_split_net(h, dyn, MZ_NET_DYN, 0, h->lay.x_dyn);
    const int e = place_chain(h, root, MZ_NET_REPR, CH_TRUNK, 0, h->lay.x_rep, h->lay.h_out);
    place_split_net(h, root, MZ_NET_PRED, e, h->lay.h_out);
    place_split_net(h, sim, MZ_NET_PRED, 0, h->lay.x_pred);
    place_split_net(h, sim, MZ_NET_DYN, 0, h->lay.x_dyn);
    const PlanBuild* all[5] = {&repr, &pred, &dyn, &root, &sim};
    for (int i = 0; i < 5; ++i)
        if (all[i]->stages.size() > MZ_MAX_STAGES) return fail(h, "network too deep for the plan executor");
    for (int i = 0; i < 5; ++i) if (upload_plan(h, *all[i], &h->d_plan[i])) return -1;
    // Register-resident image: the tasks of each stage go round-robin to the
    // 4 waves exactly as run_plan deals them; eligible when every wave has
    // <= MZ_RES_TASKS tasks of K <= 64 (nq <= 4).
    const int NW = MZ_THREADS / 64, NT = 16, RT = 9;    // MZ_RES_TASKS, ints per ResTask
    std::vector<std::vector<int>> per(NW);
    bool ok = true;
    for (int st = 0; st < (int)sim.stages.size(); ++st)
        for (int t = 0; t < (int)sim.stages[st].size(); ++t) {
            const LayerDesc& L = sim.layers[sim.stages[st][t].first];
            const int w = t % NW;
            if (L.nq > 4) ok = false;
            const int rt[RT] = {st, L.w_off, L.b_off, L.nq, sim.stages[st][t].second, L.act, L.in_off, L.out_off,
                                L.bn ? L.n_ob : 0};
            per[w].insert(per[w].end(), rt, rt + RT);
        }
    for (auto& v : per) if ((int)v.size() / RT > NT) ok = false;
    if (ok) {
        std::vector<int> img = {(int)sim.stages.size(), NT};
        for (auto& v : per) {
            img.push_back((int)v.size() / RT);
            img.insert(img.end(), v.begin(), v.end());
            img.resize(img.size() + (size_t)(NT * RT - (int)v.size()), 0);
        }
        MZ_TRY(h, dalloc(h, &h->d_plan_sim_res, img.size()));
        MZ_TRY(h, hipMemcpy(h->d_plan_sim_res, img.data(), img.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return 0;
}


// ------------------------------------------------------------- small kernel
// Schedule the layers of one network set onto stages x 2 slots x 16 4-row
// blocks (mz_small.hip): list scheduling by longest remaining path; layers
// sharing a slot must have equal kq.  Returns false if not eligible.
struct SmSched {
    int n_stages = 0;
    std::vector<int> stage;            // per layer-in-set
    std::vector<int> slot, block0;
    std::vector<int> kq[SM_MAX_SIM > SM_MAX_ROOT ? SM_MAX_SIM : SM_MAX_ROOT];
};

static bool sm_schedule(const mz_handle* h, const std::vector<int>& set, const std::vector<std::vector<int>>& deps,
                        int max_stages, std::vector<int>& st, std::vector<int>& sl, std::vector<int>& b0,
                        std::vector<std::array<int, 2>>& stage_kq) {
    const int n = (int)set.size();
    std::vector<int> prio(n, 1);
    for (int it = 0; it < n; ++it)             // longest path to the end (deps point backwards)
        for (int i = 0; i < n; ++i)
            for (int d : deps[i]) prio[d] = std::max(prio[d], prio[i] + 1);
    st.assign(n, -1); sl.assign(n, -1); b0.assign(n, -1);
    stage_kq.clear();
    int done = 0;
    for (int s = 0; done < n; ++s) {
        if (s >= max_stages) return false;
        std::vector<int> ready;
        for (int i = 0; i < n; ++i) {
            if (st[i] >= 0) continue;
            bool ok = true;
            for (int d : deps[i]) ok &= st[d] >= 0 && st[d] < s;
            if (ok) ready.push_back(i);
        }
        std::stable_sort(ready.begin(), ready.end(), [&](int a, int b) { return prio[a] > prio[b]; });
        // 4 groups of 16 rows per slot: the 16 lanes of a DPP row serve the
        // 16 rows of one group and broadcast one shared input vector
        int fr[SM_SLOTS];
        for (int x = 0; x < SM_SLOTS; ++x) fr[x] = 4;
        std::array<int, 2> kq = {0, 0};
        for (int i : ready) {
            const LayerSpec& L = h->layers[set[i]];
            const int nb = (L.out + 15) / 16;
            for (int x = 0; x < SM_SLOTS; ++x)
                if (fr[x] >= nb) {
                    st[i] = s; sl[i] = x; b0[i] = 4 * (4 - fr[x]); fr[x] -= nb; ++done;   // b0 in 4-row units
                    break;
                }
        }
        stage_kq.push_back(kq);
    }
    return true;
}

static int build_small(mz_handle* h) {
    for (const LayerSpec& L : h->layers)
        if (L.in > 64 || L.out > 64) return 0;          // not eligible: tile-16 kernel only
    if (h->A > 16) return 0;
    // network sets: SIM = prediction + dynamics, ROOT = representation
    std::vector<int> sim, root;
    auto add_net = [&](std::vector<int>& set, int net) {
        for (int ch = 0; ch < 3; ++ch) for (int li : h->chains[net][ch]) set.push_back(li);
    };
    add_net(sim, MZ_NET_PRED); add_net(sim, MZ_NET_DYN); add_net(root, MZ_NET_REPR);
    auto deps_of = [&](const std::vector<int>& set) {
        std::vector<std::vector<int>> d(set.size());
        auto pos = [&](int li) { for (size_t i = 0; i < set.size(); ++i) if (set[i] == li) return (int)i; return -1; };
        for (size_t i = 0; i < set.size(); ++i) {
            const LayerSpec& L = h->layers[set[i]];
            const auto& chain = h->chains[L.net][L.chain];
            const int k = (int)(std::find(chain.begin(), chain.end(), set[i]) - chain.begin());
            if (k > 0) d[i].push_back(pos(chain[k - 1]));
            else if (L.chain != CH_TRUNK) d[i].push_back(pos(h->chains[L.net][CH_TRUNK].back()));
        }
        return d;
    };
    std::vector<int> st_s, sl_s, b0_s, st_r, sl_r, b0_r;
    std::vector<std::array<int, 2>> kq_s, kq_r;
    if (!sm_schedule(h, sim, deps_of(sim), SM_MAX_SIM, st_s, sl_s, b0_s, kq_s)) return 0;
    if (!sm_schedule(h, root, deps_of(root), SM_MAX_ROOT, st_r, sl_r, b0_r, kq_r)) return 0;
    h->sm_n_sim = (int)kq_s.size();
    h->sm_n_root = (int)kq_r.size();
    const int nrec = h->sm_n_sim + h->sm_n_root;
    // weight / bias gather images: [rec] stage images (sm_widx) and [rec][slot][row]; with
    // BatchNorm FC layers the bias image has two more sections of the same shape: γ, β
    bool any_bn = false;
    for (const LayerSpec& L : h->layers) any_bn |= L.bn != 0;
    h->sm_bn = any_bn;
    const size_t nri = (size_t)nrec * SM_SLOTS * 64;
    std::vector<int> sw((size_t)nrec * SM_SLOTS * 256 * 16, -1), sb(nri * (any_bn ? 3 : 1), -1);
    auto fill = [&](const std::vector<int>& set, const std::vector<int>& st, const std::vector<int>& sl,
                    const std::vector<int>& b0, int rec0) {
        for (size_t i = 0; i < set.size(); ++i) {
            const LayerSpec& L = h->layers[set[i]];
            const int kq = 4 * ((L.in + 15) / 16), r = rec0 + st[i];
            for (int row = 0; row < L.out; ++row) {
                const int srow = 4 * b0[i] + row;                       // slot row
                sb[((size_t)r * SM_SLOTS + sl[i]) * 64 + srow] = (int)(L.flux_b + row);
                if (L.bn) {
                    sb[nri + ((size_t)r * SM_SLOTS + sl[i]) * 64 + srow] = (int)(L.flux_be + L.out + row);   // γ
                    sb[2 * nri + ((size_t)r * SM_SLOTS + sl[i]) * 64 + srow] = (int)(L.flux_be + row);      // β
                }
                for (int q = 0; q < 4; ++q)
                    for (int j = 0; j < kq; ++j) {
                        const int k = q * kq + j;
                        if (k >= L.in) continue;
                        sw[sm_widx(r, sl[i], q, srow, j)] =
                            (int)(L.flux_w + row + (size_t)L.out * k);
                    }
            }
        }
    };
    fill(sim, st_s, sl_s, b0_s, 0);
    fill(root, st_r, sl_r, b0_r, h->sm_n_sim);
    h->sm_w_n = sw.size(); h->sm_b_n = sb.size();
    // nonzero-chunk masks (mz_small_params.h SM_NZM_N): per stage and wave,
    // bit q*4 + c set when any row of the wave's group gathers a weight into
    // chunk c of DPP row q
    h->sm_nzm.assign(SM_NZM_ALLOC, 0);        // zero padding past SM_NZM_N
    for (int r = 0; r < nrec; ++r)
        for (int sl2 = 0; sl2 < SM_SLOTS; ++sl2)
            for (int srow = 0; srow < 64; ++srow)
                for (int q = 0; q < 4; ++q)
                    for (int j = 0; j < 16; ++j)
                        if (sw[sm_widx(r, sl2, q, srow, j)] >= 0)
                            h->sm_nzm[(size_t)(sl2 * 4 + (srow >> 4)) * SM_NZM_ST + r] |= 1u << (q * 4 + j / 4);
    h->inv_small.assign(h->nflat, -1);
    for (size_t i = 0; i < sw.size(); ++i) if (sw[i] >= 0) h->inv_small[(size_t)sw[i]] = (int)i;
    for (size_t i = 0; i < sb.size(); ++i) if (sb[i] >= 0) h->inv_small[(size_t)sb[i]] = -(int)i - 2;
    MZ_TRY(h, dalloc(h, &h->d_zero16, 16));
    MZ_TRY(h, hipMemset(h->d_zero16, 0, 64));
    MZ_TRY(h, dalloc(h, &h->d_sm_srcw, sw.size()));
    MZ_TRY(h, dalloc(h, &h->d_sm_srcb, sb.size()));
    MZ_TRY(h, dalloc(h, &h->d_sm_w, sw.size()));
    MZ_TRY(h, dalloc(h, &h->d_sm_bias, sb.size()));
    MZ_TRY(h, hipMemcpy(h->d_sm_srcw, sw.data(), sw.size() * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_sm_srcb, sb.data(), sb.size() * 4, hipMemcpyHostToDevice));
    // per-T LDS layouts and records
    const int Ts[3] = {1, 2, 4};
    for (int ti = 0; ti < 3; ++ti) {
        const int T = Ts[ti];
        int off = 0;
        auto region = [&](int rows) { int o = off; off += (rows * T + 3) / 4 * 4; return o; };
        // every input buffer has 64 rows (zero beyond K): the kernel runs 16
        // steps per quarter and reads rows up to 3*kq + 15 < 64
        int* lay = h->sm_lay[ti];
        lay[1] = region(64);
        lay[2] = region(64);
        lay[3] = region(64);
        lay[4] = region(h->H);
        lay[5] = region(1);
        lay[6] = region(h->A);
        lay[7] = region(1);
        int cb[3][3][2];
        for (int net = 0; net < 3; ++net)
            for (int ch = 0; ch < 3; ++ch) { cb[net][ch][0] = region(64); cb[net][ch][1] = region(64); }
        lay[0] = off;
        auto io = [&](int li, int& in_off, int& out_off) {
            const LayerSpec& L = h->layers[li];
            const auto& chain = h->chains[L.net][L.chain];
            const int k = (int)(std::find(chain.begin(), chain.end(), li) - chain.begin());
            const int n = (int)chain.size();
            const auto& trunk = h->chains[L.net][CH_TRUNK];
            const int trunk_out = cb[L.net][CH_TRUNK][((int)trunk.size() - 1) & 1];
            if (k > 0) in_off = cb[L.net][L.chain][(k - 1) & 1];
            else if (L.chain != CH_TRUNK) in_off = trunk_out;
            else in_off = L.net == MZ_NET_REPR ? lay[1] : L.net == MZ_NET_PRED ? lay[2] : lay[3];
            if (k < n - 1) out_off = cb[L.net][L.chain][k & 1];
            else if (L.chain == CH_TRUNK) out_off = L.net == MZ_NET_REPR ? lay[4] : trunk_out;
            else if (L.net == MZ_NET_PRED) out_off = L.chain == CH_HEAD1 ? lay[5] : lay[6];
            else out_off = L.chain == CH_HEAD1 ? lay[4] : lay[7];
        };
        // int4 per [stage][slot][row] (mz_small_params.h): {address of the row's input
        // element, quarter stride | flags, output address (-1 = unused), bias (filled on
        // device)}, in bytes from the activation buffer; unused rows read offset 0 with
        // zero weights
        std::vector<int> rec((size_t)nrec * SM_REC_INTS, 0);
        for (size_t i = 0; i < rec.size(); i += 4) rec[i + 2] = -1;
        auto rec_fill = [&](const std::vector<int>& set, const std::vector<int>& st, const std::vector<int>& sl,
                            const std::vector<int>& b0, int rec0) {
            for (size_t i = 0; i < set.size(); ++i) {
                const LayerSpec& L = h->layers[set[i]];
                int in_off, out_off;
                io(set[i], in_off, out_off);
                int* R = rec.data() + (size_t)(rec0 + st[i]) * SM_REC_INTS;
                const int kq = 4 * ((L.in + 15) / 16);
                // every row of the layer's 16-row groups carries its input element's
                // address and the quarter stride (a layer starts on a 16-row group, so
                // element row & 15 is the lane's within its DPP row); rows beyond L.out
                // have zero weights and no output
                const int rows = (L.out + 15) / 16 * 16;
                const int flags = (L.act == MZ_ACT_RELU ? SM_REC_RELU : 0) | (L.bn ? SM_REC_BN : 0) |
                                  (in_off == lay[2] ? SM_REC_PRED : 0);
                for (int row = 0; row < rows; ++row) {
                    int* e = R + 4 * (sl[i] * 64 + 4 * b0[i] + row);
                    e[0] = (in_off + (row & 15) * T) * 4;
                    e[1] = kq * T * 4 | flags;
                    e[2] = row < L.out ? (out_off + row * T) * 4 : -1;
                }
            }
        };
        rec_fill(sim, st_s, sl_s, b0_s, 0);
        rec_fill(root, st_r, sl_r, b0_r, h->sm_n_sim);
        MZ_TRY(h, dalloc(h, &h->d_sm_rec[ti], rec.size()));
        MZ_TRY(h, hipMemcpy(h->d_sm_rec[ti], rec.data(), rec.size() * 4, hipMemcpyHostToDevice));
        const int S = h->S, NN = S + 1, PS = 2 * (S + 2);
        size_t ints = (size_t)lay[0] + (size_t)(nrec + 1) * SM_REC_INTS +
                      ((size_t)T * NN * h->H + 3) / 4 * 4 + 296 + ((size_t)T * PS + 3) / 4 * 4 +
                      (size_t)4 * (S + 2) + MZ_MAX_ACTIONS;
        // + the pb_term triangle (the small kernel requires it in LDS; when
        // the total exceeds the LDS budget the tile-16 kernel is used)
        h->sm_lds[ti] = ints * 4 + (size_t)T * h->tree_game_bytes + pbterm_count(S) * 8 +
                        // the cached select: entries, path levels, N per slot, tags
                        (size_t)T * (8 * NN + 8 * (S + 2) + 4 * NN) + 16 + 4 * 16 + 4 * 8 + 4 * 4 +
                        (any_bn ? nri * 8 : 0);                          // BatchNorm (γ, β) per record row
    }
    return 1;
}

// MFMA fragment image: packed W [ob][ks][lane] <- W[ob*16 + (lane&15)][ks*4 + (lane>>4)]
// (Flux W is (out,in) column-major: element (o,i) at flux_w + o + out*i).
static int build_pack_index(mz_handle* h) {
    std::vector<int> sw(h->packed_w_n, -1), sb(h->packed_b_n, -1);
    for (const LayerSpec& L : h->layers) {
        const int nks = 4 * L.nq;
        for (int ob = 0; ob < L.n_ob; ++ob)
            for (int ks = 0; ks < nks; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int o = ob * 16 + (lane & 15), k = ks * 4 + (lane >> 4);
                    const size_t dst = (size_t)L.packed_w + ((size_t)ob * nks + ks) * 64 + lane;
                    if (o < L.out && k < L.in) sw[dst] = (int)(L.flux_w + o + (size_t)L.out * k);
                }
        for (int o = 0; o < L.out; ++o) sb[(size_t)L.packed_b + o] = (int)(L.flux_b + o);
        if (L.bn)                                   // γ, β after the bias (LayerDesc.bn)
            for (int o = 0; o < L.out; ++o) {
                sb[(size_t)L.packed_b + L.n_ob * 16 + o] = (int)(L.flux_be + L.out + o);
                sb[(size_t)L.packed_b + 2 * L.n_ob * 16 + o] = (int)(L.flux_be + o);
            }
    }
    h->inv_tile.assign(h->nflat, -1);
    for (size_t i = 0; i < sw.size(); ++i) if (sw[i] >= 0) h->inv_tile[(size_t)sw[i]] = (int)i;
    for (size_t i = 0; i < sb.size(); ++i) if (sb[i] >= 0) h->inv_tile[(size_t)sb[i]] = -(int)i - 2;
    MZ_TRY(h, dalloc(h, &h->d_srcW, sw.size()));
    MZ_TRY(h, dalloc(h, &h->d_srcB, sb.size()));
    MZ_TRY(h, hipMemcpy(h->d_srcW, sw.data(), sw.size() * sizeof(int), hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_srcB, sb.data(), sb.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int mz::repack(mz_handle* h, hipStream_t st) {
    const int T = 256;
    if (!st) st = h->stream;
    hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_w_n + T - 1) / T)), dim3(T), 0, st,
                       h->d_flat, h->d_srcW, h->d_Wp, h->packed_w_n);
    if (h->packed_b_n)
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_b_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_srcB, h->d_Bp, h->packed_b_n);
    if (h->small_ok) {
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_w_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_sm_srcw, h->d_sm_w, h->sm_w_n);
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_b_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_sm_srcb, h->d_sm_bias, h->sm_b_n);
    }
    if (h->d_sm_w2) {                            // the second image set (one-launch learner step)
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_w_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_srcW, h->d_Wp2, h->packed_w_n);
        if (h->packed_b_n)
            hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->packed_b_n + T - 1) / T)), dim3(T), 0, st,
                               h->d_flat, h->d_srcB, h->d_Bp2, h->packed_b_n);
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_w_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_sm_srcw, h->d_sm_w2, h->sm_w_n);
        hipLaunchKernelGGL(mz_repack_kernel, dim3((unsigned)((h->sm_b_n + T - 1) / T)), dim3(T), 0, st,
                           h->d_flat, h->d_sm_srcb, h->d_sm_bias2, h->sm_b_n);
    }
    MZ_TRY(h, hipGetLastError());
    return 0;
}

// LDS of mz_unroll_small{1,2}: activations, records (+1 slack stage), staging
static size_t unroll_small_lds(const mz_handle* h, int ti) {
    const size_t nri = (size_t)(h->sm_n_sim + h->sm_n_root) * SM_SLOTS * 64;
    return ((size_t)h->sm_lay[ti][0] + (size_t)(h->sm_n_sim + h->sm_n_root + 1) * SM_REC_INTS + 64) * 4 +
           (h->sm_bn ? nri * 8 : 0);                                   // BatchNorm (γ, β) per record row
}

size_t mz::tree_game_bytes(int S, int A) {
    return tree_bytes((S + 1) * A, S + 1);
}
static size_t search_lds_base(const mz_handle* h) {
    return (size_t)h->lay.total * 4 + (size_t)(416 + 16 * 2 * (h->S + 2)) * 4;
}
static size_t search_lds_bytes(const mz_handle* h) {
    return search_lds_base(h) + (h->lds_tree ? (size_t)MZ_TILE * h->tree_game_bytes : 0);
}

// mz_prior_fc: the activation layout, [16][16] floats of staging, 16 legal masks
static size_t prior_lds_bytes(const mz_handle* h) { return ((size_t)h->lay.total + MZ_TILE * 16 + MZ_TILE) * 4; }

typedef void (*search_fn)(SearchParams);
static search_fn search_kernel(const mz_handle* h) {
    if (h->use_res) return h->lds_tree ? mz_search_kernel_lds_res : mz_search_kernel_hbm_res;
    return h->lds_tree ? mz_search_kernel_lds : mz_search_kernel_hbm;
}

// ------------------------------------------------------------------- ABI
const char* mz_create_error(void) { return g_create_error.c_str(); }
const char* mz_last_error(const mz_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// ---- RCCL, loaded on first use (dlopen: libmz has no link dependency on it;
// RTLD_NOLOAD first so a process that already holds an RCCL — torch's — shares it)
// ncclUniqueId: a 128-byte struct that ncclCommInitRank takes BY VALUE
struct RcclId { uint8_t b[MZ_DP_ID_BYTES]; };
struct RcclApi {
    bool ok = false;
    int (*get_id)(void*) = nullptr;                                    // ncclGetUniqueId(ncclUniqueId*)
    int (*init_rank)(void**, int, RcclId, int) = nullptr;              // ncclCommInitRank(comm*, n, id, rank)
    int (*allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*destroy)(void*) = nullptr;
    const char* (*err)(int) = nullptr;
};
static RcclApi& rccl() {
    static RcclApi api;
    static bool tried = false;
    if (tried) return api;
    tried = true;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW);
    if (!lib) return api;
    api.get_id = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclGetUniqueId"));
    api.allreduce = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(
        dlsym(lib, "ncclAllReduce"));
    api.destroy = reinterpret_cast<int (*)(void*)>(dlsym(lib, "ncclCommDestroy"));
    api.err = reinterpret_cast<const char* (*)(int)>(dlsym(lib, "ncclGetErrorString"));
    api.init_rank = reinterpret_cast<int (*)(void**, int, RcclId, int)>(dlsym(lib, "ncclCommInitRank"));
    api.ok = api.get_id && api.init_rank && api.allreduce && api.destroy;
    return api;
}
static void dp_destroy(mz_handle* h) {
    if (h->dp_comm && rccl().ok) (void)rccl().destroy(h->dp_comm);
    h->dp_comm = nullptr; h->dp_world = 0;
}

void mz_engine_destroy(mz_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : h->sp_allocs) (void)hipFree(p);
    if (h->d_dsb) (void)hipFree(h->d_dsb);
    if (h->h_tr_cnt) (void)hipHostFree(h->h_tr_cnt);
    if (h->h_tr_pub) (void)hipHostFree(h->h_tr_pub);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    dp_destroy(h);
    delete h;
}

int mz_engine_create(const mz_config* conf, const mz_ffhp* hyper, int device, int max_games, uint64_t rng_seed,
                     mz_handle** out) {
    g_create_error.clear();
    if (!conf || !hyper || !out) { g_create_error = "null argument"; return -2; }
    *out = nullptr;
    mz_handle* h = new mz_handle();
    h->conf = *conf; h->hp = *hyper; h->device = device; h->max_games = max_games; h->seed = rng_seed;
    auto bad = [&](const std::string& m) { g_create_error = m; delete h; return -2; };
    const mz_config& c = *conf;
    if (c.action_space_size < 1 || c.action_space_size > 16)
        return bad("action_space_size must be in 1..16 (16-lane select groups)");
    if (c.players < 1 || c.players > 2) return bad("players must be 1 or 2");
    if (c.num_iters < 1 || c.num_iters >= (1 << 20)) return bad("num_iters out of range");
    if (hyper->hidden_state_size != c.observation_shape[0] * c.observation_shape[1] * c.observation_shape[2])
        return bad("hidden_state_size must equal prod(observation_shape) (the FC path reshapes h to it)");
    if (max_games < 1) return bad("max_games must be >= 1");
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed (no GPU?)");
    build_specs(h);
    if (c.num_iters > 65000) return bad("num_iters must be <= 65000 (16-bit visit counts in the tree)");
    h->tree_game_bytes = tree_game_bytes(c.num_iters, c.action_space_size);
    h->lds_tree = search_lds_base(h) + (size_t)MZ_TILE * h->tree_game_bytes <= kLdsMax;
    if (search_lds_bytes(h) > kLdsMax) return bad("LDS budget exceeded (width/num_iters too large)");
    int rc = 0;
    CK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess ? 0 : fail(h, "hipStreamCreate"));
    CK(build_plans(h));
    CK(build_pack_index(h));
    auto al_i = [&](int** p, const std::vector<int>& v) -> int {
        MZ_TRY(h, dalloc(h, p, v.size()));
        MZ_TRY(h, hipMemcpy(*p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
        return 0;
    };
    {
        int r = build_small(h);
        if (r < 0) { g_create_error = h->err; mz_engine_destroy(h); return r; }
        h->small_ok = r == 1;
        for (int ti = 0; ti < 3 && h->small_ok; ++ti) h->small_ok = h->sm_lds[ti] <= kLdsMax;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->n_cu = prop.multiProcessorCount;
        if (!h->small_ok) h->inv_small.assign(h->nflat, -1);
        CK(al_i(&h->d_inv_tile, h->inv_tile));
        CK(al_i(&h->d_inv_small, h->inv_small));
        const char* fk = std::getenv("MZ_SEARCH_KERNEL");
        if (fk) h->force_kernel = std::strcmp(fk, "tile16") == 0 ? 1 : std::strcmp(fk, "small") == 0 ? 2 : 0;
        const char* ft = std::getenv("MZ_SMALL_T");
        if (ft) { const int t = std::atoi(ft); h->force_T = (t == 1 || t == 2 || t == 4) ? t : 0; }
        if (h->small_ok) {
            const void* ks[6] = {(const void*)mz_search_small1, (const void*)mz_search_small2,
                                 (const void*)mz_search_small4, (const void*)mz_search_small1_bn,
                                 (const void*)mz_search_small2_bn, (const void*)mz_search_small4_bn};
            for (int ti = 0; ti < 6; ++ti)
                CK(hipFuncSetAttribute(ks[ti], hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->sm_lds[ti % 3]) ==
                           hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(small)"));
            const void* ku[4] = {(const void*)mz_unroll_small1, (const void*)mz_unroll_small2,
                                 (const void*)mz_unroll_small1_bn, (const void*)mz_unroll_small2_bn};
            for (int ti = 0; ti < 4; ++ti)
                CK(hipFuncSetAttribute(ku[ti], hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)unroll_small_lds(h, ti & 1)) == hipSuccess
                       ? 0 : fail(h, "hipFuncSetAttribute(unroll_small)"));
        }
    }
    const int S = h->S, A = h->A, H = h->H;
    const size_t G = (size_t)max_games;
    auto al = [&](auto** p, size_t n) -> int { MZ_TRY(h, dalloc(h, p, n)); return 0; };
    CK(al(&h->d_flat, h->nflat));
    CK(al(&h->d_Wp, h->packed_w_n));
    CK(al(&h->d_Bp, h->packed_b_n));
    if (h->small_ok) {
        CK(al(&h->d_Wp2, h->packed_w_n)); CK(al(&h->d_Bp2, h->packed_b_n));
        CK(al(&h->d_sm_w2, h->sm_w_n)); CK(al(&h->d_sm_bias2, h->sm_b_n));
        const void* kl[8] = {(const void*)mz_learn_small1, (const void*)mz_learn_small2,
                             (const void*)mz_learn_multi1, (const void*)mz_learn_multi2,
                             (const void*)mz_learn_small1_bn, (const void*)mz_learn_small2_bn,
                             (const void*)mz_learn_multi1_bn, (const void*)mz_learn_multi2_bn};
        for (int ti = 0; ti < 8; ++ti)
            CK(hipFuncSetAttribute(kl[ti], hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)unroll_small_lds(h, ti & 1)) == hipSuccess
                   ? 0 : fail(h, "hipFuncSetAttribute(learn_small)"));
        const void* k4[2] = {(const void*)mz_learn_multi4, (const void*)mz_learn_multi4_bn};
        for (int j = 0; j < 2; ++j)
            CK(hipFuncSetAttribute(k4[j], hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)unroll_small_lds(h, 2)) == hipSuccess
                   ? 0 : fail(h, "hipFuncSetAttribute(learn_multi4)"));
    }
    CK(hipMemset(h->d_flat, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(repack(h));
    // tables: libm log2/sqrt on the host, the values the oracle computes inline
    std::vector<double> pbc(S + 2), sq(S + 2);
    for (int n = 0; n < S + 2; ++n) {
        pbc[n] = std::log2((double)(n + c.pb_c_base + 1) / (double)c.pb_c_base) + (double)c.pb_c_init;
        sq[n] = std::sqrt((double)n);
    }
    std::vector<float> av(A);
    for (int a = 0; a < A; ++a) av[a] = (float)((double)(a + 1) / (double)A);
    CK(al(&h->d_pbc, pbc.size()));
    CK(al(&h->d_sqrt, sq.size()));
    CK(al(&h->d_aval, av.size()));
    CK(hipMemcpy(h->d_pbc, pbc.data(), pbc.size() * 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : fail(h, "copy"));
    CK(hipMemcpy(h->d_sqrt, sq.data(), sq.size() * 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : fail(h, "copy"));
    CK(hipMemcpy(h->d_aval, av.data(), av.size() * 4, hipMemcpyHostToDevice) == hipSuccess ? 0 : fail(h, "copy"));
    // the same f64 expression select evaluates, tabulated (Nc < Np <= S+1)
    std::vector<double> pbt(pbterm_count(S), 0.0);
    for (int np = 0; np <= S + 1; ++np)
        for (int nc = 0; nc <= np; ++nc) pbt[pbterm_index(np, nc)] = pbc[np] * (sq[np] / (double)(nc + 1));
    CK(al(&h->d_pbterm, pbt.size()));
    CK(hipMemcpy(h->d_pbterm, pbt.data(), pbt.size() * 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : fail(h, "copy"));
    CK(al(&h->d_tree, G * h->tree_game_bytes));
    CK(al(&h->d_hid, G * (S + 1) * H));
    CK(al(&h->d_obs, G * h->obs_feat)); CK(al(&h->d_legal, G * A)); CK(al(&h->d_tp, G));
    CK(al(&h->d_cv, G * A)); CK(al(&h->d_rv, G)); CK(al(&h->d_act, G));
    CK(al(&h->d_m, h->nflat)); CK(al(&h->d_v, h->nflat)); CK(al(&h->d_grad, h->nflat));
    CK(hipMemset(h->d_m, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(hipMemset(h->d_v, 0, h->nflat * 4) == hipSuccess ? 0 : fail(h, "memset"));
    CK(alloc_learner(h));
    h->use_res = h->d_plan_sim_res != nullptr && std::getenv("MZ_NO_RESIDENT") == nullptr;
    {
        const search_fn ks[4] = {mz_search_kernel_lds, mz_search_kernel_hbm, mz_search_kernel_lds_res,
                                 mz_search_kernel_hbm_res};
        for (auto k : ks)
            CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)search_lds_bytes(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute"));
        // the network-only player's tile: less than any search tile's (no per-game state, no tree)
        CK(hipFuncSetAttribute((const void*)mz_prior_fc, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)prior_lds_bytes(h)) == hipSuccess ? 0 : fail(h, "hipFuncSetAttribute(prior)"));
    }
    CK(hipStreamSynchronize(h->stream) == hipSuccess ? 0 : fail(h, "sync"));
    *out = h;
    return 0;
}

int mz_net_param_count(const mz_handle* h, int net, size_t* n) {
    if (!h || !n || net < 0 || net > 2) return -2;
    *n = h->nparams[net];
    return 0;
}

int mz_grad_count(const mz_handle* h, size_t* n) {
    if (!h || !n) return -2;
    *n = h->nflat;
    return 0;
}

int mz_weights_set(mz_handle* h, int net, const float* flat, size_t n) {
    if (!h) return -2;
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (n != h->nparams[net]) return fail(h, "weights_set: wrong parameter count");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // no search / learner launch still reads the old weights
    MZ_TRY(h, hipMemcpyAsync(h->d_flat + h->flat_off[net], flat, n * 4, hipMemcpyHostToDevice, h->stream));
    if (repack(h)) return -1;
    MZ_SYNC(h);
    return 0;
}

int mz_weights_get(mz_handle* h, int net, float* flat, size_t n) {
    if (!h) return -2;
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (n != h->nparams[net]) return fail(h, "weights_get: wrong parameter count");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // learner steps queued on any stream have landed
    MZ_TRY(h, hipMemcpyAsync(flat, h->d_flat + h->flat_off[net], n * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_SYNC(h);
    return 0;
}

static int rnet_forward(mz_handle* h, int net, const float* x, int n, float* out0, float* out1) {
    const RPlan& R = h->rplan[net];
    const bool ds = h->ds && net == MZ_NET_REPR;
    const int xin = ds ? h->obs_feat : R.in_feat;     // the raw observation goes through the downsampler
    float *dx = nullptr, *d0 = nullptr, *d1 = nullptr;
    MZ_TRY(h, hipMalloc(&dx, (size_t)n * xin * 4));
    MZ_TRY(h, hipMalloc(&d0, (size_t)n * R.out0_n * 4));
    MZ_TRY(h, hipMalloc(&d1, (size_t)n * std::max(R.out1_n, 1) * 4));
    (void)hipMemcpyAsync(dx, x, (size_t)n * xin * 4, hipMemcpyHostToDevice, h->stream);
    if (ds) {
        if (ensure_dsb(h, n) || ds_launch(h, dx, h->d_dsb, n, h->stream)) {
            (void)hipFree(dx); (void)hipFree(d0); (void)hipFree(d1);
            return -1;
        }
    }
    RNetParams Q;
    Q.ng = h->rn_ng; Q.W = h->rconf.observation_shape[0]; Q.H = h->rconf.observation_shape[1];
    Q.P = Q.W * Q.H; Q.n_items = n; Q.softmax1 = net == MZ_NET_PRED; Q.bn_s = h->bn_s;
    Q.plan = h->d_rplan + net; Q.Wimg = h->d_Wp; Q.flat = h->d_flat; Q.x = ds ? h->d_dsb : dx; Q.out0 = d0;
    Q.out1 = d1;
    void* args[] = {&Q};
    hipError_t le = hipLaunchKernel((const void*)mz_rnet_forward_kernel, dim3((n + Q.ng - 1) / Q.ng), dim3(RN_THREADS),
                                    args, h->rn_lds[net], h->stream);
    (void)hipMemcpyAsync(out0, d0, (size_t)n * R.out0_n * 4, hipMemcpyDeviceToHost, h->stream);
    if (out1 && R.out1_n) (void)hipMemcpyAsync(out1, d1, (size_t)n * R.out1_n * 4, hipMemcpyDeviceToHost, h->stream);
    hipError_t se = sync_device(h);
    (void)hipFree(dx); (void)hipFree(d0); (void)hipFree(d1);
    MZ_TRY(h, le);
    MZ_TRY(h, se);
    return check_fault(h);
}

int mz_net_forward(mz_handle* h, int net, const float* x, int n, float* out0, float* out1) {
    if (!h) return -2;
    if (net < 0 || net > 2) return fail(h, "bad net id");
    if (n < 0) return fail(h, "negative batch");
    if (n == 0) return 0;
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // weights written by `_dev` calls on other streams
    if (h->kind == 1) return rnet_forward(h, net, x, n, out0, out1);
    const int H = h->H, A = h->A;
    const int in_feat = net == MZ_NET_REPR ? h->obs_feat : net == MZ_NET_PRED ? H : H + h->plane;
    const int in_off = net == MZ_NET_REPR ? h->lay.x_rep : net == MZ_NET_PRED ? h->lay.x_pred : h->lay.x_dyn;
    const int o0 = net == MZ_NET_PRED ? 1 : H;
    const int o0_off = net == MZ_NET_PRED ? h->lay.v_out : h->lay.h_out;
    const int o1 = net == MZ_NET_PRED ? A : 1;
    const int o1_off = net == MZ_NET_PRED ? h->lay.p_out : h->lay.r_out;
    float *dx = nullptr, *d0 = nullptr, *d1 = nullptr;
    MZ_TRY(h, hipMalloc(&dx, (size_t)n * in_feat * 4));
    MZ_TRY(h, hipMalloc(&d0, (size_t)n * o0 * 4));
    MZ_TRY(h, hipMalloc(&d1, (size_t)n * o1 * 4));
    (void)hipMemcpyAsync(dx, x, (size_t)n * in_feat * 4, hipMemcpyHostToDevice, h->stream);
    hipLaunchKernelGGL(mz_forward_kernel, dim3((n + MZ_TILE - 1) / MZ_TILE), dim3(MZ_THREADS),
                       (size_t)h->lay.total * 4, h->stream, h->d_plan[net], h->d_Wp, h->d_Bp, h->lay.total, in_off,
                       in_feat, dx, n, o0_off, o0, d0, o1_off, o1, net == MZ_NET_REPR ? nullptr : d1,
                       net == MZ_NET_PRED ? 1 : 0, net == MZ_NET_PRED ? h->lay.v_act : MZ_ACT_IDENTITY,
                       net == MZ_NET_DYN ? h->lay.r_act : MZ_ACT_IDENTITY);
    hipError_t le = hipGetLastError();
    (void)hipMemcpyAsync(out0, d0, (size_t)n * o0 * 4, hipMemcpyDeviceToHost, h->stream);
    if (out1 && net != MZ_NET_REPR) (void)hipMemcpyAsync(out1, d1, (size_t)n * o1 * 4, hipMemcpyDeviceToHost, h->stream);
    hipError_t se = sync_device(h);
    (void)hipFree(dx); (void)hipFree(d0); (void)hipFree(d1);
    MZ_TRY(h, le);
    MZ_TRY(h, se);
    return check_fault(h);
}

// ResNet search: root launch, S x (tree step, networks), final tree step
static int rsearch(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, const int32_t* to_play,
                   int exploration, uint32_t rng_step, uint32_t game_offset, float temperature, float* child_visits,
                   float* root_value, int32_t* action_out, hipStream_t st, const float* temp_g) {
    RSearchParams P;
    std::memset(&P, 0, sizeof(P));
    P.temp_g = temp_g;
    P.G = G; P.S = h->S; P.A = h->A; P.H = h->H; P.W = h->rconf.observation_shape[0];
    P.P = h->plane; P.players = h->conf.players; P.obs_feat = h->rin_feat; P.exploration = exploration;
    P.rng_step = rng_step; P.game_offset = game_offset; P.seed = h->seed; P.temperature = temperature;
    P.discount = h->conf.discount; P.dirichlet_alpha = h->conf.dirichlet_alpha;
    P.exploration_eps = h->conf.exploration_eps;
    P.obs = obs; P.legal = legal_mask; P.to_play = to_play;
    P.child_visits = child_visits; P.root_value = root_value; P.action_out = action_out;
    P.pbc_tab = h->d_pbc; P.sqrt_tab = h->d_sqrt; P.aval_tab = h->d_aval; P.pbterm = h->d_pbterm;
    P.tree = h->d_tree; P.tree_game_bytes = h->tree_game_bytes; P.hid = h->d_hid;
    P.cache = h->d_rcache; P.nN = h->d_rnN;
    P.path = h->d_rpath; P.gst = h->d_rgst; P.hk = h->d_rhk;
    P.o_v = h->d_rov; P.o_logit = h->d_rologit; P.o_r = h->d_ror;
    P.ng = h->rn_ng; P.bn_s = h->bn_s; P.plans = h->d_rplan; P.Wimg = h->d_Wp; P.flat = h->d_flat;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, 128)));
    P.stamps = h->d_stamps;
#endif
    if (h->ds) {                                    // representation: downsampler, then the tail in the root
        if (ds_launch(h, obs, h->d_dsout, G, st)) return -1;
        P.obs = h->d_dsout;
    }
    void* args[] = {&P};
    const int gw = h->A > 16 ? 32 : 16;             // lanes per game in the tree kernels
    const unsigned tiles = (unsigned)((G + P.ng - 1) / P.ng), groups = (unsigned)((G + 256 / gw - 1) / (256 / gw));
    // the dynamics reward head on the prediction workgroup (mz_rsearch_nets): its trunk hand-off
    if (!h->d_rtrunk) {
        const size_t mt = (size_t)(h->max_games + P.ng - 1) / P.ng;
        MZ_TRY(h, dalloc(h, &h->d_rtrunk, (size_t)h->max_games * h->H));
        MZ_TRY(h, dalloc(h, &h->d_tprog, mt));
        MZ_TRY(h, hipMemset(h->d_tprog, 0, mt * sizeof(unsigned long long)));
    }
    P.trunk_nl = 1 + 2 * h->rhp.num_blocks; P.dyn_split = h->rn_dyn_split;
    P.trunk = h->d_rtrunk; P.tprog = h->d_tprog;
    P.fault = h->d_fault; P.poll_ticks = h->poll_ticks; P.dbg_skip = h->dbg_skip;
    P.no_moved_skip = 0;
    const void* kroot = gw == 32 ? (const void*)mz_rsearch_root32 : (const void*)mz_rsearch_root;
    // tree step: LDS-cached (one wave per 64/gw games) unless the tree exceeds the LDS
    const bool tl = h->rtree_lds != 0;
    const void* ktree = tl ? (gw == 32 ? (const void*)mz_rsearch_tree_lds32 : (const void*)mz_rsearch_tree_lds)
                           : (gw == 32 ? (const void*)mz_rsearch_tree32 : (const void*)mz_rsearch_tree);
    const unsigned tgrid = tl ? (unsigned)((G + 64 / gw - 1) / (64 / gw)) : groups;
    MZ_TRY(h, hipLaunchKernel(kroot, dim3(tiles), dim3(RN_THREADS), args, rsearch_root_lds(h), st));
    for (int s = 0; s <= h->S; ++s) {
        P.s = s;
        MZ_TRY(h, hipLaunchKernel(ktree, dim3(tgrid), dim3(tl ? 64 * RT_WAVES : 256), args, tl ? h->rtree_lds : 0, st));
        if (s == h->S) break;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (h->time_nets) {
            if (h->tev_used + 2 > h->tev.size())
                for (int i = 0; i < 2; ++i) {
                    hipEvent_t e;
                    MZ_TRY(h, hipEventCreate(&e));
                    h->tev.push_back(e);
                }
            e0 = h->tev[h->tev_used++]; e1 = h->tev[h->tev_used++];
            MZ_TRY(h, hipEventRecord(e0, st));
        }
        P.tepoch = ++h->tprog_epoch;
        MZ_TRY(h, hipLaunchKernel((const void*)mz_rsearch_nets, dim3(tiles, 2), dim3(RN_THREADS_NETS), args,
                                  rsearch_nets_lds(h), st));
        if (e1) MZ_TRY(h, hipEventRecord(e1, st));
    }
    h->last_variant = "mz_rsearch";
    return 0;
}

// the batched search; temp_g: per-game temperatures (device, G) or NULL =
// `temperature` for every game
static int search_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, const int32_t* to_play,
                      int exploration, uint32_t rng_step, uint32_t game_offset, float temperature,
                      float* child_visits, float* root_value, int32_t* action_out, void* stream,
                      const float* temp_g) {
    if (!h) return -2;
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (G == 0) return 0;
    if (h->kind == 1)
        return rsearch(h, G, obs, legal_mask, to_play, exploration, rng_step, game_offset, temperature,
                       child_visits, root_value, action_out, stream_of(h, stream), temp_g);
    SearchParams P;
    std::memset(&P, 0, sizeof(P));
    P.temp_g = temp_g;
    P.G = G; P.S = h->S; P.A = h->A; P.H = h->H; P.players = h->conf.players; P.obs_feat = h->obs_feat;
    P.plane = h->plane; P.exploration = exploration; P.rng_step = rng_step; P.game_offset = game_offset;
    P.seed = h->seed; P.temperature = temperature; P.discount = h->conf.discount;
    P.dirichlet_alpha = h->conf.dirichlet_alpha; P.exploration_eps = h->conf.exploration_eps;
    P.obs = obs; P.legal = legal_mask; P.to_play = to_play;
    P.child_visits = child_visits; P.root_value = root_value; P.action_out = action_out;
    P.Wp = h->d_Wp; P.Bp = h->d_Bp; P.plan_root = h->d_plan[3]; P.plan_sim = h->d_plan[4];
    P.plan_sim_res = h->use_res ? h->d_plan_sim_res : nullptr;
    P.lay = h->lay; P.pbc_tab = h->d_pbc; P.sqrt_tab = h->d_sqrt; P.aval_tab = h->d_aval;
    P.tree = h->d_tree; P.tree_game_bytes = h->tree_game_bytes; P.dump_tree = h->dump_tree;
    P.hid = h->d_hid;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * h->max_games));
    P.stamps = h->d_stamps;
#endif
    hipStream_t st = stream_of(h, stream);
    const bool small = h->small_ok && h->force_kernel != 1 && (h->force_kernel == 2 || G <= 4 * h->n_cu);
    if (small) {
        const int T = h->force_T ? h->force_T : G <= h->n_cu ? 1 : G <= 2 * h->n_cu ? 2 : 4;
        const int ti = T == 1 ? 0 : T == 2 ? 1 : 2;
        SmallParams Q;
        std::memset(&Q, 0, sizeof(Q));
        Q.temp_g = temp_g;
        Q.G = G; Q.S = h->S; Q.A = h->A; Q.H = h->H; Q.players = h->conf.players; Q.obs_feat = h->obs_feat;
        Q.plane = h->plane; Q.exploration = exploration; Q.rng_step = rng_step; Q.game_offset = game_offset;
        Q.seed = h->seed; Q.temperature = temperature; Q.discount = h->conf.discount;
        Q.dirichlet_alpha = h->conf.dirichlet_alpha; Q.exploration_eps = h->conf.exploration_eps;
        Q.obs = obs; Q.legal = legal_mask; Q.to_play = to_play;
        Q.child_visits = child_visits; Q.root_value = root_value; Q.action_out = action_out;
        Q.n_sim = h->sm_n_sim; Q.n_root = h->sm_n_root;
        Q.w_sim = h->d_sm_w;
        std::memcpy(Q.nzm, h->sm_nzm.data(), sizeof(Q.nzm));
        Q.bn = h->sm_bn;
        Q.zero16 = reinterpret_cast<const float4*>(h->d_zero16);
        Q.w_root = h->d_sm_w + (size_t)h->sm_n_sim * SM_SLOTS * 256 * 16;
        Q.rec = h->d_sm_rec[ti]; Q.bias = h->d_sm_bias;
        const int* lay = h->sm_lay[ti];
        Q.act_total = lay[0]; Q.x_rep = lay[1]; Q.x_pred = lay[2]; Q.x_dyn = lay[3]; Q.h_out = lay[4];
        Q.v_out = lay[5]; Q.p_out = lay[6]; Q.r_out = lay[7];
        Q.v_act = h->lay.v_act; Q.r_act = h->lay.r_act;
        Q.pbc_tab = h->d_pbc; Q.sqrt_tab = h->d_sqrt; Q.aval_tab = h->d_aval;
        Q.pbterm = h->d_pbterm;
        Q.tree = h->d_tree; Q.tree_game_bytes = h->tree_game_bytes; Q.dump_tree = h->dump_tree;
        if (h->dump_tree) {
            if (!h->d_sel_stats) MZ_TRY(h, dalloc(h, &h->d_sel_stats, (size_t)2 * h->max_games));
            Q.sel_stats = h->d_sel_stats;
        }
#ifdef MZ_STAMPS
        Q.stamps = h->d_stamps;
#endif
        const void* k = h->sm_bn ? (T == 1 ? (const void*)mz_search_small1_bn : T == 2 ? (const void*)mz_search_small2_bn
                                                                                   : (const void*)mz_search_small4_bn)
                                 : (T == 1 ? (const void*)mz_search_small1 : T == 2 ? (const void*)mz_search_small2
                                                                                   : (const void*)mz_search_small4);
        void* args[] = {&Q};
        MZ_TRY(h, hipLaunchKernel(k, dim3((G + T - 1) / T), dim3(SM_THREADS), args, h->sm_lds[ti], st));
        h->last_variant = std::string(T == 1 ? "mz_search_small1" : T == 2 ? "mz_search_small2" : "mz_search_small4") +
                          (h->sm_bn ? "_bn" : "");
    } else {
        hipLaunchKernelGGL(search_kernel(h), dim3((G + MZ_TILE - 1) / MZ_TILE), dim3(MZ_THREADS),
                           search_lds_bytes(h), st, P);
        h->last_variant = h->use_res ? (h->lds_tree ? "mz_search_kernel_lds_res" : "mz_search_kernel_hbm_res")
                                     : (h->lds_tree ? "mz_search_kernel_lds" : "mz_search_kernel_hbm");
    }
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_mcts_search_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, const int32_t* to_play,
                       int exploration, uint32_t rng_step, uint32_t game_offset, float temperature,
                       float* child_visits, float* root_value, int32_t* action_out, void* stream) {
    return search_dev(h, G, obs, legal_mask, to_play, exploration, rng_step, game_offset, temperature, child_visits,
                      root_value, action_out, stream, nullptr);
}

int mz_mcts_search(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, const int32_t* to_play,
                   int exploration, uint32_t rng_step, uint32_t game_offset, float temperature, float* child_visits,
                   float* root_value, int32_t* action_out) {
    if (!h) return -2;
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (G == 0) return 0;
    const int A = h->A;
    for (int g = 0; g < G; ++g) {       // @assert !isempty(legal_actions) (SelfPlay.jl:243)
        int any = 0;
        for (int a = 0; a < A; ++a) any |= legal_mask[(size_t)g * A + a] != 0;
        if (!any) return fail(h, "Legal actions should not be an empty array (game " + std::to_string(g) + ")");
        if (to_play[g] < 1 || to_play[g] > h->conf.players) return fail(h, "to_play out of range");
    }
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // `_dev` work on other streams first
    MZ_TRY(h, hipMemcpyAsync(h->d_obs, obs, (size_t)G * h->obs_feat * 4, hipMemcpyHostToDevice, h->stream));
    MZ_TRY(h, hipMemcpyAsync(h->d_legal, legal_mask, (size_t)G * A, hipMemcpyHostToDevice, h->stream));
    MZ_TRY(h, hipMemcpyAsync(h->d_tp, to_play, (size_t)G * 4, hipMemcpyHostToDevice, h->stream));
    int rc = mz_mcts_search_dev(h, G, h->d_obs, h->d_legal, h->d_tp, exploration, rng_step, game_offset, temperature,
                                h->d_cv, h->d_rv, h->d_act, h->stream);
    if (rc) return rc;
    MZ_TRY(h, hipMemcpyAsync(child_visits, h->d_cv, (size_t)G * A * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_TRY(h, hipMemcpyAsync(root_value, h->d_rv, (size_t)G * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_TRY(h, hipMemcpyAsync(action_out, h->d_act, (size_t)G * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_SYNC(h);
    return 0;
}

int mz_set_sync_stream(mz_handle* h, void* stream, int narrow) {
    if (!h) return -1;
    h->sync_stream = (hipStream_t)stream;
    h->sync_narrow = narrow != 0;
    return 0;
}

int mz_debug_enable(mz_handle* h, int flags) {
    if (!h) return -2;
    h->dump_tree = flags & 1;
    h->time_nets = (flags >> 1) & 1;
    h->time_unroll = (flags >> 2) & 1;
    return 0;
}

int mz_debug_tree(mz_handle* h, int G, int32_t* eN, float* eW, float* eP, float* eR, int32_t* eC, int32_t* ntp) {
    if (!h) return -2;
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (h->lds_tree && !h->dump_tree) return fail(h, "mz_debug_tree needs mz_debug_enable(h, 1) before the search");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const int S = h->S, A = h->A, NN = S + 1, E = NN * A;
    const size_t gb = h->tree_game_bytes;
    std::vector<char> buf((size_t)G * gb);
    MZ_TRY(h, hipMemcpy(buf.data(), h->d_tree, buf.size(), hipMemcpyDeviceToHost));
    for (int g = 0; g < G; ++g) {
        const char* b = buf.data() + (size_t)g * gb;
        // edge records {nc, w, p, ev} (mz_tree_device.h)
        const uint32_t* rec = reinterpret_cast<const uint32_t*>(b);
        auto nc = [&](size_t i) { return rec[4 * i]; };
        auto w = [&](size_t i) { float v; std::memcpy(&v, rec + 4 * i + 1, 4); return v; };
        auto p = [&](size_t i) { float v; std::memcpy(&v, rec + 4 * i + 2, 4); return v; };
        const float* nr = reinterpret_cast<const float*>(b + 16 * (size_t)E);
        const int8_t* tp = reinterpret_cast<const int8_t*>(b + 16 * (size_t)E + 4 * (size_t)NN);
        // only expanded slots hold data: slot e is expanded iff e == 0 or some edge points at it
        std::vector<char> expd(NN, 0);
        expd[0] = 1;
        for (int i = 0; i < E; ++i) if ((nc(i) >> 16) != 0 && expd[i / A]) expd[(nc(i) >> 16) - 1] = 1;
        for (int e = 0; e < NN; ++e) {
            if (ntp) ntp[(size_t)g * NN + e] = expd[e] ? tp[e] : 0;
            for (int a = 0; a < A; ++a) {
                const size_t k = ((size_t)g * NN + e) * A + a, i = (size_t)e * A + a;
                const bool x = expd[e] != 0;
                const int c = x ? (int)(nc(i) >> 16) - 1 : -1;
                if (eN) eN[k] = x ? (int32_t)(nc(i) & 0xffffu) : 0;
                if (eW) eW[k] = x ? w(i) : 0.0f;
                if (eP) eP[k] = x ? p(i) : 0.0f;
                if (eR) eR[k] = c >= 0 ? nr[c] : 0.0f;
                if (eC) eC[k] = c;
            }
        }
    }
    return 0;
}

int mz_debug_select_stats(mz_handle* h, int G, int32_t* fast, int32_t* walked) {
    if (!h) return -2;
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (!h->dump_tree) return fail(h, "mz_debug_select_stats needs mz_debug_enable(h, 1) before the search");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    // only the small kernels count: any other search leaves both at 0
    const bool small = h->d_sel_stats && h->last_variant.rfind("mz_search_small", 0) == 0;
    std::vector<int32_t> buf((size_t)2 * G, 0);
    if (small && G > 0) MZ_TRY(h, hipMemcpy(buf.data(), h->d_sel_stats, buf.size() * 4, hipMemcpyDeviceToHost));
    for (int g = 0; g < G; ++g) {
        if (fast) fast[g] = buf[2 * (size_t)g];
        if (walked) walked[g] = buf[2 * (size_t)g + 1];
    }
    return 0;
}

// ------------------------------------------------------------- learner
int mz::ensure_batch(mz_handle* h, int B) {
    if (B <= h->bcap) return 0;
    const int K = h->conf.num_unroll_steps, A = h->A;
    float** bufs[] = {&h->d_bobs, &h->d_bact, &h->d_btv, &h->d_btr, &h->d_btp, &h->d_bgs, &h->d_pv, &h->d_pp, &h->d_pr};
    size_t sizes[] = {(size_t)B * h->obs_feat, (size_t)B * (K + 1), (size_t)B * (K + 1), (size_t)B * (K + 1),
                      (size_t)B * (K + 1) * A, (size_t)B, (size_t)B * (K + 1), (size_t)B * (K + 1) * A,
                      (size_t)B * (K + 1)};
    for (int i = 0; i < 9; ++i) MZ_TRY(h, dalloc(h, bufs[i], sizes[i]));
    MZ_TRY(h, dalloc(h, &h->d_lterm, (size_t)2 * B * (K + 1)));
    MZ_TRY(h, dalloc(h, &h->d_bw, (size_t)B));
    if (h->kind == 1) {
        MZ_TRY(h, dalloc(h, &h->d_rhs, (size_t)B * std::max(K, 1) * h->H));
        MZ_TRY(h, dalloc(h, &h->d_rts, (size_t)B * std::max(K, 1) * h->H));
        MZ_TRY(h, dalloc(h, &h->d_prog, (size_t)B));
        MZ_TRY(h, hipMemset(h->d_prog, 0, (size_t)B * sizeof(unsigned long long)));
        h->prog_epoch = 0;
    }
    h->bcap = B;
    return 0;
}

static int learner_losses(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st,
                          int v_act, int r_act, bool fuse_adam = false, double eta = 0.0, bool l2_done = false);
static void adam_advance(mz_handle* h);

// the instance of a small-kernel family for T = {1, 2, 4}[ti] samples per workgroup (mz_small.hip)
enum { SMK_UNROLL = 0, SMK_LEARN = 1, SMK_MULTI = 2 };
static const void* small_kernel(const mz_handle* h, int family, int ti) {
    static const void* const k[3][2][3] = {
        {{(const void*)mz_unroll_small1, (const void*)mz_unroll_small2, nullptr},
         {(const void*)mz_unroll_small1_bn, (const void*)mz_unroll_small2_bn, nullptr}},
        {{(const void*)mz_learn_small1, (const void*)mz_learn_small2, nullptr},
         {(const void*)mz_learn_small1_bn, (const void*)mz_learn_small2_bn, nullptr}},
        {{(const void*)mz_learn_multi1, (const void*)mz_learn_multi2, (const void*)mz_learn_multi4},
         {(const void*)mz_learn_multi1_bn, (const void*)mz_learn_multi2_bn, (const void*)mz_learn_multi4_bn}}};
    return k[family][h->sm_bn ? 1 : 0][ti];
}

// ---- the ResNet learner unroll (mz_runroll_*), one step or the steps of a multi-step sub-chunk
static size_t runroll_lds(const mz_handle* h) {
    return std::max(h->rn_lds[0], std::max(h->rn_lds[1], h->rn_lds[2]));
}
// the parameters every unroll launch of the engine shares; the caller adds its batch, read-outs,
// scratch and parameter images (and the ms_* strides of a multi-step launch)
static void runroll_params(const mz_handle* h, int B, RUnrollParams& U) {   // (filled in place: no copy)
    std::memset(&U, 0, sizeof(U));                 // (ms = 0: one step; the fused-ADAM fields unused unless set)
    U.B = B; U.K = h->conf.num_unroll_steps; U.A = h->A; U.H = h->H;
    U.W = h->rconf.observation_shape[0]; U.P = h->plane; U.obs_feat = h->rin_feat; U.ng = h->rn_ng; U.bn_s = h->bn_s;
    U.plans = h->d_rplan; U.plans_l = h->d_rplan_l; U.ng_l = 1;
    U.dyn_split = h->rn_dyn_split; U.otab = h->d_rtab;
}
// Launch the unroll of U: one step (steps = 0: U.ms = 0, grid z = 1) or `steps` steps on gridDim.z.
// prog / epoch: the fused launch's progress words and its launch counter (the one-step launch:
// d_prog, which must exist; the multi-step launch: the steps' slice of d_ml_prog).  One step only:
// rq (the get_batch launch, folded into the fused launch when it applies) and fuse_adam (the Σθ² /
// ADAM slices beside the fused unroll into the second image set; *l2_fused tells the caller to swap
// the sets).  Leaves the launched kernels' names in last_lvariant.
static int runroll_launch(mz_handle* h, RUnrollParams& U, int steps, hipStream_t st, unsigned long long* prog,
                          unsigned long long* epoch, const RpSampleParams* rq = nullptr, bool fuse_adam = false,
                          double eta = 0.0, bool* l2_fused = nullptr) {
    const int B = U.B, KH = std::max(U.K, 1);
    const unsigned nz = steps ? steps : 1;
    void* args[] = {&U};
    U.ms = steps;
    // the B·K predictions on wide tiles (ng items) once they fill the chip
    // (B = 2048: 640 workgroups; one-item tiles there measured 2.4x slower),
    // else one-item tiles (B = 32: 160 workgroups instead of 10)
    const bool wide_p = (B * KH + U.ng - 1) / U.ng >= h->n_cu;
    // one launch (mz_runroll_fused_r): the chain blocks, then the items, each
    // item waiting for its sample's chain instead of the whole launch; with
    // rq, each chain block also draws its sample (the get_batch launch folded in)
    const bool fused = h->rd_chain && h->rp_pred && !wide_p && U.K + 1 < 64 && !h->ds && prog;
    if (rq && !fused) {
        hipLaunchKernelGGL(mz_rp_sample, dim3((B + 3) / 4), dim3(256), 0, st, *rq);
        MZ_TRY(h, hipGetLastError());
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;          // mz_debug_enable flag 4: the unroll launches' duration
    if (h->time_unroll) {
        if (timing_events(h, &e0, &e1)) return -1;
        MZ_TRY(h, hipEventRecord(e0, st));
    }
    if (fused || steps) {                           // (a multi-step launch carries these in every form)
        U.rp_nv = 3 + h->rhp.depth_value;           // value head: conv, Dense, depth_value × Dense, Dense
        U.fault = h->d_fault; U.poll_ticks = h->poll_ticks; U.dbg_skip = h->dbg_skip;
    }
    std::string& variant = h->last_lvariant;        // (assigned in place: no allocation per launch)
    // chain on narrow (one-sample) tiles, then the B·K predictions.  The chain's units are one
    // column block (the 1-block instances, a fifth of the code), also on planes of several
    // blocks: a Connect4 1x1 conv of 4 row blocks x 3 column blocks then has 12 units for the
    // 8 waves instead of 4 three-block ones (the same tiles, bit for bit; configs[3] learner
    // 1.62 k -> 1.75 k steps/s, tools/gpu_r04d.sh)
    U.rd_ep_off = (int)(h->rn_lds_l / 4);
    U.rd_trunk_nl = 1 + 2 * h->rhp.num_blocks;
    const unsigned ny = U.K > 0 ? 2 : 1;
    if (fused) {
        U.prog = prog;
        U.prog_base = (++*epoch) * 64ull;
        U.n_chain = B;
        U.fuse_sample = rq != nullptr;
        if (rq) U.rq = *rq;
        // ADAM beside the unroll: the launch reads the current image (d_Wp) and
        // writes the updated one into d_Wp2, swapped after the launch
        U.n_l2 = fuse_adam && h->d_Wp2 ? 96 : 0;
        if (!steps) {
            U.ad = LgAdam{1, h->d_m, h->d_v, h->bp1, h->bp2, eta, h->d_Wp2, h->d_Bp, h->d_inv_tile, nullptr,
                          nullptr, h->d_inv_small};
            U.flat_w = h->d_flat; U.netoff = h->d_netoff; U.part = h->d_sq;
        }
        if (l2_fused) *l2_fused = U.n_l2 > 0;
        variant = "mz_runroll_fused_r";
        const int nitems = B * KH * (U.K > 0 ? 3 : 2);
        MZ_TRY(h, hipLaunchKernel((const void*)mz_runroll_fused_r, dim3(nz * (B + U.n_l2 + nitems)),
                                  dim3(RD_THREADS), args, std::max(rd_chain_lds(h), rp_pred_lds(h)), st));
    } else {
        variant = h->rd_chain ? "mz_runroll_chain_r" : "mz_runroll_chain1";
        MZ_TRY(h, hipLaunchKernel(h->rd_chain ? (const void*)mz_runroll_chain_r : (const void*)mz_runroll_chain1,
                                  dim3(B, 1, nz), dim3(h->rd_chain ? RD_THREADS : RN_THREADS), args,
                                  h->rd_chain ? rd_chain_lds(h) : h->rn_lds_l, st));
        // the B·K predictions and reward heads (wide_p above)
        if (wide_p) {
            variant += "+mz_runroll_pred";
            MZ_TRY(h, hipLaunchKernel((const void*)mz_runroll_pred, dim3((B * KH + U.ng - 1) / U.ng, ny, nz),
                                      dim3(RN_THREADS), args, runroll_lds(h), st));
        } else if (h->rp_pred) {
            variant += "+mz_runroll_pred_r";
            MZ_TRY(h, hipLaunchKernel((const void*)mz_runroll_pred_r, dim3(B * KH, ny, nz), dim3(RD_THREADS), args,
                                      rp_pred_lds(h), st));
        } else {
            variant += "+mz_runroll_pred_n1";
            MZ_TRY(h, hipLaunchKernel((const void*)mz_runroll_pred_n1, dim3(B * KH, ny, nz), dim3(RN_THREADS), args,
                                      h->rn_lds_l, st));
        }
    }
    if (e1) MZ_TRY(h, hipEventRecord(e1, st));
    return 0;
}

// ResNet learner: the unroll on the network kernels, then the shared loss /
// ∇ = 2θ kernel (the plans' outputs are already activated)
static int rlearner_grad(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st,
                         bool fuse_adam = false, double eta = 0.0, const RpSampleParams* rq = nullptr) {
    const int B = b->batch_size;
    if (B < 1) return fail(h, "batch_size must be >= 1");
    if (ensure_batch(h, B)) return -1;
    RUnrollParams U;
    runroll_params(h, B, U);
    U.obs = b->observation; U.actions = b->actions;
    if (h->ds) {                                    // representation (:347): downsampler, then the tail
        if (ensure_dsb(h, B) || ds_launch(h, b->observation, h->d_dsb, B, st)) return -1;
        U.obs = h->d_dsb;
    }
    U.pv = h->d_pv; U.pp = h->d_pp; U.pr = h->d_pr;
    U.hs = h->d_rhs; U.ts = h->d_rts; U.Wimg = h->d_Wp; U.flat = h->d_flat;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, 128)));
    U.stamps = h->d_stamps;
#endif
    bool l2_fused = false;
    if (runroll_launch(h, U, 0, st, h->d_prog, &h->prog_epoch, rq, fuse_adam, eta, &l2_fused)) return -1;
    if (learner_losses(h, b, grad_dev, losses_dev, st, MZ_ACT_IDENTITY, MZ_ACT_IDENTITY, fuse_adam, eta, l2_fused))
        return -1;
    if (l2_fused) {
        std::swap(h->d_Wp, h->d_Wp2);
        adam_advance(h);
    }
    return 0;
}

static int fc_unroll(mz_handle* h, const mz_batch* b, hipStream_t st, const RpSampleParams* rp);
static int small_unroll_ti(const mz_handle* h, int B);
static int small_unroll_params(mz_handle* h, const mz_batch* b, int ti, const RpSampleParams* rp,
                               SmallUnrollParams* Uo);

// forward unroll + losses + ∇ = 2θ into grad_dev (device batch pointers)
int mz_learner_grad_dev(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, void* stream) {
    if (!h || !b) return -2;
    if (b->batch_size < 1) return fail(h, "batch_size must be >= 1");
    if (h->learn_mode == MZ_LEARN_CORRECTED)
        return bp_grad(h, b, grad_dev, losses_dev, stream_of(h, stream));
    if (h->kind == 1) return rlearner_grad(h, b, grad_dev, losses_dev, stream_of(h, stream));
    if (ensure_batch(h, b->batch_size)) return -1;
    hipStream_t st = stream_of(h, stream);
    if (fc_unroll(h, b, st, nullptr)) return -1;
    return learner_losses(h, b, grad_dev, losses_dev, st, h->lay.v_act, h->lay.r_act);
}

// FC learner unroll of batch b (Learning.jl:327-343); rp != nullptr: the
// batch is drawn from the replay shard by get_batch (mz_rp_sample's body),
// inside the small unroll kernel when it applies, else by its own launch
static int fc_unroll(mz_handle* h, const mz_batch* b, hipStream_t st, const RpSampleParams* rp) {
    const int B = b->batch_size, K = h->conf.num_unroll_steps, A = h->A;
    const int ti_u = small_unroll_ti(h, B);
    if (ti_u >= 0) {
        // the search's stage schedule and register images, T samples per
        // workgroup (ADAM keeps the images current)
        const int ti = ti_u, T = ti + 1;
        SmallUnrollParams U;
        if (small_unroll_params(h, b, ti, rp, &U)) return -1;
        void* args[] = {&U};
        MZ_TRY(h, hipLaunchKernel(small_kernel(h, SMK_UNROLL, ti), dim3((B + T - 1) / T), dim3(SM_THREADS), args,
                                  unroll_small_lds(h, ti), st));
        h->last_lvariant = ti == 0 ? "mz_unroll_small1" : "mz_unroll_small2";
    } else {
        if (rp) {
            hipLaunchKernelGGL(mz_rp_sample, dim3((B + 3) / 4), dim3(256), 0, st, *rp);
            MZ_TRY(h, hipGetLastError());
        }
        UnrollParams U;
        U.B = B; U.K = K; U.A = A; U.H = h->H; U.plane = h->plane; U.obs_feat = h->obs_feat;
        U.obs = b->observation; U.actions = b->actions; U.pv = h->d_pv; U.pp = h->d_pp; U.pr = h->d_pr;
        U.Wp = h->d_Wp; U.Bp = h->d_Bp; U.plan_repr = h->d_plan[0]; U.plan_sim = h->d_plan[4]; U.lay = h->lay;
        hipLaunchKernelGGL(mz_unroll_kernel, dim3((B + MZ_TILE - 1) / MZ_TILE), dim3(MZ_THREADS),
                           (size_t)h->lay.total * 4, st, U);
        h->last_lvariant = "mz_unroll_kernel";
    }
    MZ_TRY(h, hipGetLastError());
    return 0;
}

// the small unroll holds the nets with T = ti + 1 samples per workgroup
static bool small_unroll_fits(const mz_handle* h, int ti) {
    const int K = h->conf.num_unroll_steps, A = h->A;
    // one item per thread in the unroll's per-step loops; a/|A| staging of 64 floats
    return h->small_ok && (ti + 1) * h->H <= 256 && (ti + 1) * h->plane <= 256 &&
           (ti + 1) * (A + 2) <= SM_THREADS && (ti + 1) * (K + 1) <= 64 &&
           (ti + 1) * h->obs_feat <= SM_THREADS;                // one observation item per thread (setup)
}
// T = 2 when B exceeds 4 samples per CU; -1 if the small unroll cannot hold the nets
static int small_unroll_ti(const mz_handle* h, int B) {
    const int ti_u = B <= 4 * h->n_cu ? 0 : 1;         // (two per workgroup at B = 32: 29.5 k vs 34.0 k steps/s)
    return small_unroll_fits(h, ti_u) ? ti_u : -1;
}

// parameters of mz_unroll_small* / mz_learn_small* for batch b (T = ti + 1
// samples per workgroup, the search's stage schedule and register images)
static int small_unroll_params(mz_handle* h, const mz_batch* b, int ti, const RpSampleParams* rp,
                               SmallUnrollParams* Uo) {
    const int B = b->batch_size, K = h->conf.num_unroll_steps, A = h->A;
    {
        const int* lay = h->sm_lay[ti];
        SmallUnrollParams U;
        U.B = B; U.K = K; U.A = A; U.H = h->H; U.plane = h->plane; U.obs_feat = h->obs_feat;
        U.obs = b->observation; U.actions = b->actions; U.pv = h->d_pv; U.pp = h->d_pp; U.pr = h->d_pr;
        U.n_sim = h->sm_n_sim; U.n_root = h->sm_n_root; U.w_sim = h->d_sm_w;
        U.w_root = h->d_sm_w + (size_t)h->sm_n_sim * SM_SLOTS * 256 * 16;
        std::memcpy(U.nzm, h->sm_nzm.data(), sizeof(U.nzm));
        U.bn = h->sm_bn;
        U.zero16 = reinterpret_cast<const float4*>(h->d_zero16);
        U.bias = h->d_sm_bias; U.rec = h->d_sm_rec[ti]; U.act_total = lay[0];
        U.x_rep = lay[1]; U.x_pred = lay[2]; U.x_dyn = lay[3]; U.h_out = lay[4]; U.v_out = lay[5];
        U.p_out = lay[6]; U.r_out = lay[7]; U.v_act = h->lay.v_act; U.r_act = h->lay.r_act;
        U.stamps = nullptr;
#ifdef MZ_STAMPS
        if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, B)));
        U.stamps = h->d_stamps;
#endif
        U.sample = rp != nullptr;
        U.pf_hdr = nullptr; U.pf_epoch = 0;
        if (rp) U.rp = *rp; else std::memset(&U.rp, 0, sizeof(U.rp));
        *Uo = U;
    }
    return 0;
}

static LgAdam adam_args(mz_handle* h, int on, double eta) {
    return LgAdam{on, h->d_m, h->d_v, h->bp1, h->bp2, eta, h->d_Wp, h->d_Bp, h->d_inv_tile, h->d_sm_w,
                  h->d_sm_bias, h->d_inv_small};
}
// after an ADAM update: βp .= βp .* β
static void adam_advance(mz_handle* h) {
    h->bp1 = h->bp1 * 0.9;
    h->bp2 = h->bp2 * 0.999;
}

// losses + ∇ = 2θ from the unroll outputs in d_pv / d_pp / d_pr; with
// fuse_adam (world = 1) the ∇ is not stored: each parameter slice's block
// applies the ADAM update (learning rate eta) right after reading θ for Σθ²
static int learner_losses(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st,
                          int v_act, int r_act, bool fuse_adam, double eta, bool l2_done) {
    const int B = b->batch_size, K = h->conf.num_unroll_steps, A = h->A;
    float* lo = losses_dev ? losses_dev : h->d_loss;
    float* g = grad_dev ? grad_dev : h->d_grad;
    const int gw = A > 16 ? 32 : 16;            // lanes per (sample, step) group
    const int nlb = (B * (K + 1) + MZ_THREADS / gw - 1) / (MZ_THREADS / gw);
    const LgAdam ad = adam_args(h, fuse_adam ? 1 : 0, eta);
    // l2_done: the Σθ² slices (and the ADAM step) ran in the unroll launch; only the loss blocks and the fold
    hipLaunchKernelGGL(gw == 32 ? mz_learner_grad_kernel32 : mz_learner_grad_kernel,
                       dim3(nlb + (l2_done ? 0 : 3 * MZ_L2_BLOCKS)), dim3(MZ_THREADS), 0, st, B, K, A,
                       v_act, r_act, h->d_pv, h->d_pp, h->d_pr, b->target_values, b->target_policies,
                       b->gradient_scale, h->d_lterm, h->d_flat, h->d_netoff, g, h->d_sq, h->d_counter, lo, b->weights, ad);
    MZ_TRY(h, hipGetLastError());
    if (fuse_adam && !l2_done) adam_advance(h);
    return 0;
}

int mz_learner_set_mode(mz_handle* h, int mode) {
    if (!h) return -2;
    if (mode != MZ_LEARN_REF_SEMANTICS && mode != MZ_LEARN_CORRECTED) return fail(h, "unknown learner mode");
    h->learn_mode = mode;
    return 0;
}

int mz_learner_apply_dev(mz_handle* h, const float* grad_dev, float grad_scale, double eta, void* stream) {
    if (!h) return -2;
    hipStream_t st = stream_of(h, stream);
    const float* g = grad_dev ? grad_dev : h->d_grad;
    hipLaunchKernelGGL(mz_adam_kernel, dim3(128), dim3(MZ_THREADS), 0, st, h->d_flat, h->d_m, h->d_v, g,
                       grad_scale, h->nflat, h->bp1, h->bp2, eta, h->d_Wp, h->d_Bp, h->d_inv_tile, h->d_sm_w,
                       h->d_sm_bias, h->d_inv_small);
    adam_advance(h);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_learner_step(mz_handle* h, const mz_batch* b, double eta, float* losses_out) {
    if (!h || !b) return -2;
    const int B = b->batch_size, K = h->conf.num_unroll_steps, A = h->A;
    MZ_TRY(h, hipSetDevice(h->device));
    if (B < 1) return fail(h, "batch_size must be >= 1");
    if (ensure_batch(h, B)) return -1;
    MZ_SYNC(h);                  // `_dev` work on other streams first
    hipStream_t st = h->stream;
    MZ_TRY(h, hipMemcpyAsync(h->d_bobs, b->observation, (size_t)B * h->obs_feat * 4, hipMemcpyHostToDevice, st));
    MZ_TRY(h, hipMemcpyAsync(h->d_bact, b->actions, (size_t)B * (K + 1) * 4, hipMemcpyHostToDevice, st));
    MZ_TRY(h, hipMemcpyAsync(h->d_btv, b->target_values, (size_t)B * (K + 1) * 4, hipMemcpyHostToDevice, st));
    MZ_TRY(h, hipMemcpyAsync(h->d_btr, b->target_rewards, (size_t)B * (K + 1) * 4, hipMemcpyHostToDevice, st));
    MZ_TRY(h, hipMemcpyAsync(h->d_btp, b->target_policies, (size_t)B * (K + 1) * A * 4, hipMemcpyHostToDevice, st));
    MZ_TRY(h, hipMemcpyAsync(h->d_bgs, b->gradient_scale, (size_t)B * 4, hipMemcpyHostToDevice, st));
    if (b->weights) MZ_TRY(h, hipMemcpyAsync(h->d_bw, b->weights, (size_t)B * 4, hipMemcpyHostToDevice, st));
    mz_batch db = *b;
    db.observation = h->d_bobs; db.actions = h->d_bact; db.target_values = h->d_btv;
    db.target_rewards = h->d_btr; db.target_policies = h->d_btp; db.gradient_scale = h->d_bgs;
    db.weights = b->weights ? h->d_bw : nullptr;
    int rc = mz_learner_grad_dev(h, &db, h->d_grad, h->d_loss, st);
    if (rc) return rc;
    rc = mz_learner_apply_dev(h, h->d_grad, 1.0f, eta, st);
    if (rc) return rc;
    if (losses_out) MZ_TRY(h, hipMemcpyAsync(losses_out, h->d_loss, 6 * 4, hipMemcpyDeviceToHost, st));
    MZ_TRY(h, hipStreamSynchronize(st));
    return check_fault(h);
}

// the next (start, stop) event pair of the measurement list (mz_debug_kernel_time)
static int timing_events(mz_handle* h, hipEvent_t* e0, hipEvent_t* e1) {
    if (h->tev_used + 2 > h->tev.size())
        for (int i = 0; i < 2; ++i) {
            hipEvent_t e;
            MZ_TRY(h, hipEventCreate(&e));
            h->tev.push_back(e);
        }
    *e0 = h->tev[h->tev_used++]; *e1 = h->tev[h->tev_used++];
    return 0;
}

int mz_debug_kernel_time(mz_handle* h, double* total_ms, int* launches) {
    if (!h) return -2;
    MZ_TRY(h, hipSetDevice(h->device));
    double t = 0.0;
    for (size_t i = 0; i + 1 < h->tev_used; i += 2) {
        MZ_TRY(h, hipEventSynchronize(h->tev[i + 1]));
        float ms = 0.0f;
        MZ_TRY(h, hipEventElapsedTime(&ms, h->tev[i], h->tev[i + 1]));
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = (int)(h->tev_used / 2);
    h->tev_used = 0;
    return 0;
}

int mz_debug_unroll(mz_handle* h, int B, float* values, float* policies, float* rewards) {
    if (!h) return -2;
    if (B < 0 || B > h->bcap) return fail(h, "B exceeds the last learner batch");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const size_t n = (size_t)B * (h->conf.num_unroll_steps + 1);
    if (values) MZ_TRY(h, hipMemcpy(values, h->d_pv, n * 4, hipMemcpyDeviceToHost));
    if (policies) MZ_TRY(h, hipMemcpy(policies, h->d_pp, n * h->A * 4, hipMemcpyDeviceToHost));
    if (rewards) MZ_TRY(h, hipMemcpy(rewards, h->d_pr, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Diagnostic: per-workgroup phase cycles of the last search (stamp build only).
extern "C" int mz_debug_stamps(mz_handle* h, unsigned long long* out, int n_blocks) {
    if (!h) return -2;
#ifdef MZ_STAMPS
    if (!h->d_stamps) return fail(h, "no stamps recorded");
    MZ_SYNC(h);
    MZ_TRY(h, hipMemcpy(out, h->d_stamps, (size_t)n_blocks * 8 * 8, hipMemcpyDeviceToHost));
    return 0;
#else
    (void)out; (void)n_blocks;
    return fail(h, "libmz built without -DMZ_STAMPS");
#endif
}

const char* mz_search_variant(const mz_handle* h) {
    if (!h) return "";
    return h->last_variant.c_str();
}

const char* mz_learner_variant(const mz_handle* h) {
    if (!h) return "";
    return h->last_lvariant.c_str();
}

int mz_resnet_tile_games(const mz_handle* h) { return h && h->kind == 1 ? h->rn_ng : 0; }
int mz_downsample_staged(const mz_handle* h) { return h && h->kind == 1 && h->ds ? h->dsplan.stage_in : -1; }

// ------------------------------------------------ checkpoint interface (mz_ckpt_iface.h)
static const char* kNetNames[3] = {"representation", "prediction", "dynamics"};

std::vector<MzParamDesc> mz_param_table(const mz_handle* h) {
    std::vector<MzParamDesc> t;
    for (int net = 0; net < 3; ++net) {
        int i = 0;
        auto add = [&](std::vector<int64_t> shp, size_t off) {
            size_t cnt = 1;
            for (int64_t d : shp) cnt *= (size_t)d;
            t.push_back(MzParamDesc{std::string(kNetNames[net]) + "." + std::to_string(i++), shp, off, cnt});
        };
        if (h->kind == 0) {                                   // Dense: W (out, in), b (out)
            for (const LayerSpec& L : h->layers) {
                if (L.net != net) continue;
                add({L.out, L.in}, L.flux_w);
                add({L.out}, L.flux_b);
                if (L.bn) { add({L.out}, L.flux_be); add({L.out}, L.flux_be + L.out); }   // BatchNorm β, γ
            }
        } else {                                              // Conv: W (kw,kh,cin,cout), b, BatchNorm β, γ
            size_t np = 0;
            if (net == MZ_NET_REPR && h->ds)                  // the downsampler's convs first (MeanPool: none)
                for (int i = 0; i < h->dsplan.n; ++i) {
                    const DsLayer& L = h->dsplan.L[i];
                    if (L.kind != DS_CONV) continue;
                    add({L.kw, L.kh, L.cin, L.cout}, h->flat_off[net] + L.woff);
                    add({L.cout}, h->flat_off[net] + L.boff);
                    if (L.bn) { add({L.cout}, h->flat_off[net] + L.bnoff); add({L.cout}, h->flat_off[net] + L.bnoff + L.cout); }
                }
            for (const RSpec& r : rn_specs(h->rconf, h->rhp, net, &np)) {
                const size_t base = h->flat_off[net] + (net == MZ_NET_REPR ? h->ds_n : 0);
                if (r.conv) {
                    add({r.kw, r.kh, r.cin, r.cout}, base + r.woff);
                    add({r.cout}, base + r.boff);
                    add({r.cout}, base + r.bnoff);
                    add({r.cout}, base + r.bnoff + r.cout);
                } else {
                    add({r.cout, r.cin}, base + r.woff);
                    add({r.cout}, base + r.boff);
                }
            }
        }
    }
    return t;
}

size_t mz_flat_count(const mz_handle* h) { return h->nflat; }

int mz_state_get(mz_handle* h, float* flat, float* m, float* v, double* beta_pow) {
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (flat) MZ_TRY(h, hipMemcpy(flat, h->d_flat, h->nflat * 4, hipMemcpyDeviceToHost));
    if (m) MZ_TRY(h, hipMemcpy(m, h->d_m, h->nflat * 4, hipMemcpyDeviceToHost));
    if (v) MZ_TRY(h, hipMemcpy(v, h->d_v, h->nflat * 4, hipMemcpyDeviceToHost));
    if (beta_pow) { beta_pow[0] = h->bp1; beta_pow[1] = h->bp2; }
    return 0;
}

int mz_state_set(mz_handle* h, const float* flat, const float* m, const float* v, const double* beta_pow) {
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    MZ_TRY(h, hipMemcpy(h->d_flat, flat, h->nflat * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_m, m, h->nflat * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_v, v, h->nflat * 4, hipMemcpyHostToDevice));
    h->bp1 = beta_pow[0]; h->bp2 = beta_pow[1];
    if (repack(h)) return -1;
    MZ_SYNC(h);
    return 0;
}

std::string mz_net_kind(const mz_handle* h) { return h->kind == 0 ? "fc" : "resnet"; }

std::string mz_describe(const mz_handle* h) {
    const mz_config& c = h->conf;
    std::string s = "{\"observation_shape\":[" + std::to_string(c.observation_shape[0]) + "," +
                    std::to_string(c.observation_shape[1]) + "," + std::to_string(c.observation_shape[2]) + "]" +
                    ",\"action_space_size\":" + std::to_string(c.action_space_size) +
                    ",\"stacked_observations\":" + std::to_string(c.stacked_observations) +
                    ",\"num_unroll_steps\":" + std::to_string(c.num_unroll_steps);
    if (h->kind == 0) {
        const mz_ffhp& p = h->hp;
        s += ",\"width_hidden\":" + std::to_string(p.width_hidden) +
             ",\"depth_representation\":" + std::to_string(p.depth_representation) +
             ",\"depth_prediction\":" + std::to_string(p.depth_prediction) +
             ",\"depth_dynamics\":" + std::to_string(p.depth_dynamics) +
             ",\"depth_policy\":" + std::to_string(p.depth_policy) + ",\"depth_value\":" + std::to_string(p.depth_value) +
             ",\"depth_reward\":" + std::to_string(p.depth_reward) +
             ",\"depth_state_head\":" + std::to_string(p.depth_state_head) +
             ",\"hidden_state_size\":" + std::to_string(p.hidden_state_size) +
             ",\"reward_activation\":" + std::to_string(p.reward_activation);
    } else {
        const mz_resnet_hp& p = h->rhp;
        s += ",\"num_blocks\":" + std::to_string(p.num_blocks) + ",\"num_filters\":" + std::to_string(p.num_filters) +
             ",\"conv_kernel_size\":[" + std::to_string(p.conv_kernel_size[0]) + "," +
             std::to_string(p.conv_kernel_size[1]) + "]" +
             ",\"num_first_head_filters\":" + std::to_string(p.num_first_head_filters) +
             ",\"num_second_head_filters\":" + std::to_string(p.num_second_head_filters) +
             ",\"depth_value\":" + std::to_string(p.depth_value) + ",\"width_hidden\":" + std::to_string(p.width_hidden) +
             ",\"downsample\":" + std::to_string(p.downsample) +
             ",\"reward_activation\":" + std::to_string(p.reward_activation);
    }
    return s + "}";
}

int mz_set_error(mz_handle* h, const std::string& msg) { return fail(h, msg); }

static int sp_alloc_hist(mz_handle* h, SpHist& r, size_t n) {
    const size_t T = (size_t)h->sp_T, A = (size_t)h->A;
    MZ_TRY(h, spalloc(h, &r.obs, n * T * h->sp_osz));
    MZ_TRY(h, spalloc(h, &r.act, n * T));
    MZ_TRY(h, spalloc(h, &r.rew, n * T));
    MZ_TRY(h, spalloc(h, &r.tp, n * T));
    MZ_TRY(h, spalloc(h, &r.cv, n * T * A));
    MZ_TRY(h, spalloc(h, &r.rv, n * T));
    MZ_TRY(h, spalloc(h, &r.len, n));
    MZ_TRY(h, spalloc(h, &r.prio, n * T));
    MZ_TRY(h, spalloc(h, &r.gprio, n));
    return 0;
}

// `test`: the rows are the test worker's slots (h->ts) in evaluation mode with mz_test_config's
// opponent; the shard, the counters and the tally are not theirs (null: no launch of theirs reads them)
SpParams mz::sp_params(mz_handle* h, bool test) {
    SpParams S;
    std::memset(&S, 0, sizeof(S));
    const mz_config& c = h->conf;
    S.G = h->sp_G; S.env = h->sp_env; S.W = c.observation_shape[0]; S.H = c.observation_shape[1];
    S.osz = h->sp_osz; S.P = h->plane; S.A = h->A; S.F = h->obs_feat; S.stacked = c.stacked_observations;
    S.T = h->sp_T; S.max_moves = c.max_moves;
    S.board = h->d_sp_board; S.player = h->d_sp_player; S.over = h->d_sp_over;
    S.frames = h->sp_frames; S.ekey = h->d_sp_ekey;
    S.hist = h->sp_hist; S.ring = h->sp_ring; S.cap = h->sp_cap; S.counters = h->d_sp_counters;
    S.obs = h->d_obs; S.legal = h->d_legal; S.tp = h->d_tp; S.cv = h->d_cv; S.rv = h->d_rv; S.act = h->d_act;
    S.done = h->d_sp_done; S.ring_pos = h->d_sp_rpos;
    S.eval = h->sp_eval; S.opponent = h->sp_opp; S.muzero_player = h->sp_mzp;
    S.seed = h->seed; S.eval_counts = h->d_eval;
    S.per = c.PER != 0; S.per_alpha = c.PER_alpha; S.td = c.td_steps; S.disc_pow = h->d_sp_dpow;
    if (test) {
        const mz_handle::TestSlots& t = h->ts;
        S.G = t.E;
        S.board = t.board; S.player = t.player; S.over = t.over; S.ekey = t.ekey;
        S.hist = t.hist; S.done = t.done; S.frozen = t.frozen;
        S.ring = SpHist{}; S.cap = 0; S.counters = nullptr; S.ring_pos = nullptr; S.eval_counts = nullptr;
        S.eval = 1; S.opponent = h->test_opp; S.muzero_player = h->test_mzp;
    }
    return S;
}

// the conf must match the env (mz_selfplay_init, mz_expert_eval)
static int sp_env_check(mz_handle* h, int env_kind) {
    const mz_config& c = h->conf;
    const int W = c.observation_shape[0], H = c.observation_shape[1], C = c.observation_shape[2];
    if (env_kind == MZ_ENV_TICTACTOE) {
        if (W != 3 || H != 3 || C != 3 || h->A != 9) return fail(h, "TicTacToe needs observation_shape (3,3,3), 9 actions");
    } else if (env_kind == MZ_ENV_CONNECT4) {
        if (W != 6 || H != 7 || C != 3 || h->A != 7) return fail(h, "Connect4 needs observation_shape (6,7,3), 7 actions");
    } else if (env_kind == MZ_ENV_ATARI) {
        if (W != 84 || H != 84 || C != 4 || h->A != 18 || c.stacked_observations != 0)
            return fail(h, "the Atari-like env needs observation_shape (84,84,4), 18 actions, stacked_observations 0");
    } else {
        return fail(h, "unknown env_kind");
    }
    return 0;
}

// The symmetry group of the handle's board env from its board shape: cell (i, j) is
// i + W·j.  TicTacToe (a square board, one action per cell): the dihedral group, id s = transpose if
// s >= 4, then s & 3 quarter turns (a, b) -> (b, W - 1 - a); the action table is the cell table.
// Connect4 (H columns of W rows, one action per column): the mirror (w, h) -> (w, H - 1 - h).
// cell [n][W·H], act [n][A]; returns n (0: the env has no group).
static int sym_tables(const mz_handle* h, std::vector<int32_t>& cell, std::vector<int32_t>& act) {
    const int W = h->conf.observation_shape[0], H = h->conf.observation_shape[1], P = W * H, A = h->A;
    int n = 0;
    if (h->sp_env == MZ_ENV_TICTACTOE && W == H && A == P) n = 8;
    else if (h->sp_env == MZ_ENV_CONNECT4 && A == H) n = 2;
    cell.assign((size_t)n * P, 0); act.assign((size_t)n * A, 0);
    for (int s = 0; s < n; ++s)
        for (int j = 0; j < H; ++j)
            for (int i = 0; i < W; ++i) {
                int a = i, b = j;
                if (n == 8) {
                    if (s >= 4) { a = j; b = i; }
                    for (int q = 0; q < (s & 3); ++q) { const int t = a; a = b; b = W - 1 - t; }
                    act[(size_t)s * A + i + W * j] = a + W * b;
                } else {
                    if (s == 1) b = H - 1 - j;
                    act[(size_t)s * A + j] = b;
                }
                cell[(size_t)s * P + i + W * j] = a + W * b;
            }
    return n;
}

// The sampler's small constants in one device buffer (mz_selfplay_init: it lives and dies with the
// shard's allocations): f32(discount^n) as Julia's Float32^Int (≈ f32(pow(f64))), n = 0..td+1, then
// the env's symmetry tables (RpSampleParams names them by their offset from disc_pow)
static int sp_constants(mz_handle* h) {
    const mz_config& c = h->conf;
    std::vector<float> dp(c.td_steps + 2);
    for (int n = 0; n < (int)dp.size(); ++n) dp[n] = (float)std::pow((double)c.discount, (double)n);
    std::vector<int32_t> cell, act;
    h->sym_n = sym_tables(h, cell, act);
    MZ_TRY(h, spalloc(h, &h->d_sp_dpow, dp.size() + cell.size() + act.size()));
    MZ_TRY(h, hipMemcpy(h->d_sp_dpow, dp.data(), dp.size() * 4, hipMemcpyHostToDevice));
    h->d_sym = nullptr;
    if (!h->sym_n) return 0;
    h->d_sym = reinterpret_cast<int32_t*>(h->d_sp_dpow + dp.size());
    MZ_TRY(h, hipMemcpy(h->d_sym, cell.data(), cell.size() * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_sym + cell.size(), act.data(), act.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// D of the expert opponent: the handle's mz_expert_depth, 0 = the env's default
static int expert_depth_of(const mz_handle* h, int env_kind) {
    return h->sp_expert_depth ? h->sp_expert_depth : env_kind == MZ_ENV_TICTACTOE ? 9 : 4;
}

// the lookup (mz_expert_table_move) stands in for the search exactly when the switch is on, the env is
// TicTacToe and the effective depth is the table's 9
static bool expert_table_in_use(const mz_handle* h) {
    return h->xtable_on && h->d_xtable && h->sp_env == MZ_ENV_TICTACTOE && expert_depth_of(h, h->sp_env) == 9;
}

// ---- the rules-MCTS opponent
// rows per workgroup: what fits the LDS with (S + 1)·A edge records a row, at most mz_expert_move's 4
static int mcts_games_per_block(int sims, int A) {
    const size_t row = (size_t)(sims + 1) * A * sizeof(MctsEdge);
    return (int)std::min<size_t>(4, std::max<size_t>(1, kLdsMax / row));
}

// what the first use needs, outside any launch path: the sqrt table and the kernel's LDS ceiling
static int mcts_prepare(mz_handle* h) {
    if (h->d_mcts_sqrt) return 0;
    static_assert((size_t)(MZM_MAX_SIMS + 1) * 9 * sizeof(MctsEdge) <= kLdsMax, "the largest tree fits one workgroup");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_TRY(h, hipFuncSetAttribute((const void*)mz_mcts_move, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    std::vector<double> sq(MZM_MAX_SIMS + 1);
    for (size_t k = 0; k < sq.size(); ++k) sq[k] = std::sqrt((double)k);
    double* d = nullptr;
    MZ_TRY(h, dalloc(h, &d, sq.size()));
    MZ_TRY(h, hipMemcpy(d, sq.data(), sq.size() * 8, hipMemcpyHostToDevice));
    h->d_mcts_sqrt = d;
    return 0;
}

static void mcts_launch(const SpParams& S, int sims, int rollouts, const double* sqrt_tab, int32_t* act, int32_t* n,
                        int32_t* w, hipStream_t st) {
    MctsArgs X{sims, rollouts, mcts_games_per_block(sims, S.A), sqrt_tab, act, n, w};
    const size_t lds = (size_t)X.games * (sims + 1) * S.A * sizeof(MctsEdge);
    hipLaunchKernelGGL(mz_mcts_move, dim3((S.G + X.games - 1) / X.games), dim3(64 * X.games), lds, st, S, X);
}

// MZ_OPP_NETWORK: the opponent search's outputs, part of the self-play state (a snapshot load
// re-creates that state and keeps the mode, so the move asks again)
static int opp_io(mz_handle* h) {
    if (h->d_act2) return 0;
    const size_t G = (size_t)h->sp_G;
    MZ_TRY(h, spalloc(h, &h->d_cv2, G * h->A, false));
    MZ_TRY(h, spalloc(h, &h->d_rv2, G, false));
    MZ_TRY(h, spalloc(h, &h->d_act2, G, false));
    return 0;
}

// ---- the network-only player
// G rows' (π, v, action) with the nets the handle points at, stream-ordered; temp_g as search_dev's.
// FC engines: one mz_prior_fc launch.  ResNet engines: the downsampler where the engine has one, the two
// forward launches of rean_values' ResNet branch into the handle's buffers, then mz_prior_pick.
static int prior_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, uint32_t rng_step,
                     uint32_t game_offset, float temperature, float* policy, float* value, int32_t* action,
                     hipStream_t st, const float* temp_g) {
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (G == 0) return 0;
    PriorParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.G = G; Q.A = h->A; Q.obs_feat = h->obs_feat; Q.rng_step = rng_step; Q.game_offset = game_offset;
    Q.seed = h->seed; Q.temperature = temperature; Q.temp_g = temp_g;
    Q.obs = obs; Q.legal = legal_mask; Q.policy = policy; Q.value = value; Q.action = action;
    void* args[] = {&Q};
    if (h->kind != 1) {
        Q.plan_root = h->d_plan[3]; Q.Wp = h->d_Wp; Q.Bp = h->d_Bp;
        Q.x_rep = h->lay.x_rep; Q.v_out = h->lay.v_out; Q.p_out = h->lay.p_out; Q.v_act = h->lay.v_act;
        Q.lds_total = h->lay.total;
        MZ_TRY(h, hipLaunchKernel((const void*)mz_prior_fc, dim3((G + MZ_TILE - 1) / MZ_TILE), dim3(MZ_THREADS), args,
                                  prior_lds_bytes(h), st));
        return 0;
    }
    const RPlan& Rr = h->rplan[MZ_NET_REPR];
    const RPlan& Rp = h->rplan[MZ_NET_PRED];
    if (Rp.in_feat != Rr.out0_n || Rp.out0_n != 1 || Rp.out1_n != h->A)
        return fail(h, "prior: unexpected ResNet plan shapes");
    const float* x = obs;
    if (h->ds) {                                    // representation: downsampler, then the tail
        if (ds_launch(h, obs, h->d_dsout, G, st)) return -1;
        x = h->d_dsout;
    }
    for (int net = MZ_NET_REPR; net <= MZ_NET_PRED; ++net) {
        RNetParams N;
        N.ng = h->rn_ng; N.W = h->rconf.observation_shape[0]; N.H = h->rconf.observation_shape[1];
        N.P = N.W * N.H; N.n_items = G; N.softmax1 = net == MZ_NET_PRED; N.bn_s = h->bn_s;
        N.plan = h->d_rplan + net; N.Wimg = h->d_Wp; N.flat = h->d_flat;
        N.x = net == MZ_NET_REPR ? x : h->d_pr_h;
        N.out0 = net == MZ_NET_REPR ? h->d_pr_h : h->d_pr_v;
        N.out1 = h->d_pr_p;
        void* nargs[] = {&N};
        MZ_TRY(h, hipLaunchKernel((const void*)mz_rnet_forward_kernel, dim3((G + N.ng - 1) / N.ng), dim3(RN_THREADS),
                                  nargs, h->rn_lds[net], st));
    }
    Q.p = h->d_pr_p; Q.v = h->d_pr_v;
    const int gw = h->A > 16 ? 32 : 16;
    MZ_TRY(h, hipLaunchKernel(gw == 32 ? (const void*)mz_prior_pick32 : (const void*)mz_prior_pick,
                              dim3((G + 256 / gw - 1) / (256 / gw)), dim3(256), args, 0, st));
    return 0;
}

static const char* const kOppNetsMissing =
    "opponent: MZ_OPP_NETWORK needs the opponent's nets (mz_opponent_weights_set / _from / _load first)";

int mz_prior_eval_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, int opponent_set,
                      uint32_t rng_step, uint32_t game_offset, float temperature, float* policy, float* value,
                      int32_t* action, void* stream) {
    if (!h) return -2;
    if (opponent_set != 0 && opponent_set != 1) return fail(h, "prior: opponent_set must be 0 or 1");
    if (opponent_set && h->opp_have != 7u) return fail(h, kOppNetsMissing);
    if (!(temperature >= 0.0f)) return fail(h, "prior: temperature must be >= 0 (+inf allowed)");
    if (opponent_set) wset_swap(h, h->opp);
    const int rc = prior_dev(h, G, obs, legal_mask, rng_step, game_offset, temperature, policy, value, action,
                             stream_of(h, stream), nullptr);
    if (opponent_set) wset_swap(h, h->opp);
    return rc;
}

int mz_prior_eval(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, int opponent_set, uint32_t rng_step,
                  uint32_t game_offset, float temperature, float* policy, float* value, int32_t* action) {
    if (!h) return -2;
    if (G < 0 || G > h->max_games) return fail(h, "G exceeds max_games");
    if (opponent_set != 0 && opponent_set != 1) return fail(h, "prior: opponent_set must be 0 or 1");
    if (opponent_set && h->opp_have != 7u) return fail(h, kOppNetsMissing);
    if (!(temperature >= 0.0f)) return fail(h, "prior: temperature must be >= 0 (+inf allowed)");
    if (G == 0) return 0;
    const int A = h->A;
    for (int g = 0; g < G; ++g) {
        int any = 0;
        for (int a = 0; a < A; ++a) any |= legal_mask[(size_t)g * A + a] != 0;
        if (!any) return fail(h, "Legal actions should not be an empty array (game " + std::to_string(g) + ")");
    }
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);                  // `_dev` work on other streams first
    MZ_TRY(h, hipMemcpyAsync(h->d_obs, obs, (size_t)G * h->obs_feat * 4, hipMemcpyHostToDevice, h->stream));
    MZ_TRY(h, hipMemcpyAsync(h->d_legal, legal_mask, (size_t)G * A, hipMemcpyHostToDevice, h->stream));
    int rc = mz_prior_eval_dev(h, G, h->d_obs, h->d_legal, opponent_set, rng_step, game_offset, temperature, h->d_cv,
                               h->d_rv, h->d_act, h->stream);
    if (rc) return rc;
    MZ_TRY(h, hipMemcpyAsync(policy, h->d_cv, (size_t)G * A * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_TRY(h, hipMemcpyAsync(value, h->d_rv, (size_t)G * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_TRY(h, hipMemcpyAsync(action, h->d_act, (size_t)G * 4, hipMemcpyDeviceToHost, h->stream));
    MZ_SYNC(h);
    return 0;
}

// one side's rows of an evaluation move: its kind on the nets the handle points at
static int player_dev(mz_handle* h, int kind, const SpParams& S, float* cv, float* rv, int32_t* act, hipStream_t st) {
    if (kind == MZ_PLAYER_PRIOR)
        return prior_dev(h, S.G, h->d_obs, h->d_legal, S.step, S.game_offset, S.temperature, cv, rv, act, st, S.temp_g);
    return search_dev(h, S.G, h->d_obs, h->d_legal, h->d_tp, 1, S.step, S.game_offset, S.temperature, cv, rv, act, st,
                      S.temp_g);
}

// Does an evaluation move against `opponent` issue a secondary launch (the other side's kind on its
// weights, into second outputs)?  Only a network player on the other side can differ from the primary:
// in weights (MZ_OPP_NETWORK) or in kind (MZ_OPP_SELF with two different kinds).
static bool eval_secondary(const mz_handle* h, int opponent) {
    return opponent == MZ_OPP_NETWORK || (opponent == MZ_OPP_SELF && h->ev_kind[0] != h->ev_kind[1]);
}

// One move of S's rows up to the commit, shared by mz_selfplay_move (the self-play slots) and
// mz_test_play (the test slots): mz_sp_prepare -> the primary launch on the engine's io with the handle's
// current nets (the search; in evaluation play MuZero's kind, mz_eval_players) -> the secondary launch
// where the other side is a network player that differs in kind or in weights (outputs cv2 / rv2 / act2)
// and mz_sp_pick -> the rules opponents' launches -> mz_sp_commit.  The keys, the temperature and the
// mode are S's.  `judge` (a judging evaluation of mz_test_play; null everywhere else): the audit row,
// which the expert's launch feeds on MuZero's turns from the action the primary left in d_act; with
// another opponent that launch is made for the judge alone.
static int sp_move_body(mz_handle* h, const SpParams& S, float* cv2, float* rv2, int32_t* act2, hipStream_t st,
                        long long* judge = nullptr) {
    const int G = S.G;
    const dim3 waves((G + 3) / 4);
    hipLaunchKernelGGL(mz_sp_prepare, waves, dim3(256), 0, st, S);
    MZ_TRY(h, hipGetLastError());
    int rc = player_dev(h, S.eval ? h->ev_kind[0] : MZ_PLAYER_SEARCH, S, h->d_cv, h->d_rv, h->d_act, st);
    if (rc) return rc;
    if (S.eval && eval_secondary(h, S.opponent)) {   // the other side's own player; its turns take that whole result
        if (!act2) return fail(h, "eval players: the second outputs are not allocated");
        const bool theirs = S.opponent == MZ_OPP_NETWORK;
        if (theirs) wset_swap(h, h->opp);
        rc = player_dev(h, h->ev_kind[1], S, cv2, rv2, act2, st);
        if (theirs) wset_swap(h, h->opp);
        if (rc) return rc;
        PickArgs X{h->d_cv, h->d_rv, h->d_act, cv2, rv2, act2};
        hipLaunchKernelGGL(mz_sp_pick, waves, dim3(256), 0, st, S, X);
    }
    if ((S.eval && S.opponent == MZ_OPP_EXPERT) || judge) {   // the expert's turns: its move replaces the search's action
        ExpertArgs X{expert_depth_of(h, h->sp_env), h->d_act, nullptr, nullptr, judge};
        if (expert_table_in_use(h)) {                // the solved table: a lookup in place of the search
            X.table = h->d_xtable;
            hipLaunchKernelGGL(mz_expert_table_move, waves, dim3(256), 0, st, S, X);
        } else {
            hipLaunchKernelGGL(mz_expert_move, waves, dim3(256), 0, st, S, X);
        }
    }
    if (S.eval && S.opponent == MZ_OPP_MCTS) {       // the rules MCTS's turns: its move replaces the search's action
        if (!h->d_mcts_sqrt) return fail(h, "mcts opponent: not prepared (mz_selfplay_mode / mz_test_config first)");
        mcts_launch(S, h->sp_mcts_sims ? h->sp_mcts_sims : MZM_DEF_SIMS,
                    h->sp_mcts_rollouts ? h->sp_mcts_rollouts : MZM_DEF_ROLLOUTS, h->d_mcts_sqrt, h->d_act, nullptr,
                    nullptr, st);
    }
    hipLaunchKernelGGL(mz_sp_commit, waves, dim3(256), 0, st, S);
    return 0;
}

int mz_selfplay_init(mz_handle* h, int env_kind, int G, int replay_games) {
    if (!h) return -2;
    const mz_config& c = h->conf;
    const int W = c.observation_shape[0], H = c.observation_shape[1], C = c.observation_shape[2];
    if (int rc = sp_env_check(h, env_kind)) return rc;
    if (G < 1 || G > h->max_games) return fail(h, "G must be in 1..max_games");
    if (replay_games < G) return fail(h, "replay_games must be >= G (one move can finish every slot)");
    if (c.max_moves < 1) return fail(h, "max_moves must be >= 1");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    for (void* p : h->sp_allocs) (void)hipFree(p);
    h->sp_allocs.clear();
    h->rs_cap = 0;
    h->pf_cap = 0; h->pf_cur = 0; h->d_pf_hdr = nullptr; ++h->pf_epoch;
    h->sp_has_games = false;
    h->sp_reset_pending = false;
    h->tr_B = 0;                                // a new shard: mz_train_init again
    if (env_kind != h->sp_env) h->sym_on = false;       // mz_replay_set_symmetry is kept for the same env only
    h->sp_env = env_kind; h->sp_G = G; h->sp_cap = replay_games;
    h->sp_T = c.max_moves + 1; h->sp_osz = W * H * C;
    h->sp_frames = 0;
    if (env_kind == MZ_ENV_ATARI) { h->sp_osz = W * H; h->sp_frames = C; }   // one frame per move
    MZ_TRY(h, spalloc(h, &h->d_sp_board, (size_t)G * h->sp_osz));
    MZ_TRY(h, spalloc(h, &h->d_sp_player, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_sp_over, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_sp_ekey, (size_t)G));
    if (sp_alloc_hist(h, h->sp_hist, (size_t)G)) return -1;
    if (sp_alloc_hist(h, h->sp_ring, (size_t)replay_games)) return -1;
    // reanalysed_predicted_root_values of the shard's games (mz_replay_reanalyse); rean zeroed = `nothing`
    MZ_TRY(h, spalloc(h, &h->sp_ring.rrv, (size_t)replay_games * h->sp_T));
    MZ_TRY(h, spalloc(h, &h->sp_ring.rean, (size_t)replay_games));
    h->rn_cap = 0;                              // the ResNet staging buffers were in sp_allocs
    h->sp_ring.rcv = nullptr; h->d_rq_obs = nullptr;    // so were rcv and the reanalyse search's io
    h->d_rean_rows = nullptr; h->rean_rows_cap = 0;     // and the worker's row list
    h->d_cv2 = nullptr; h->d_rv2 = nullptr; h->d_act2 = nullptr;   // and MZ_OPP_NETWORK's second outputs
    h->ts = mz_handle::TestSlots{};                     // and the test worker's slots (its settings and records stay)
    MZ_TRY(h, spalloc(h, &h->d_sp_counters, MZ_SP_COUNTERS));
    const long long cursor0 = 1;                        // the reanalyse cursor: game number 1
    MZ_TRY(h, hipMemcpy(h->d_sp_counters + MZ_REAN_CURSOR, &cursor0, sizeof(cursor0), hipMemcpyHostToDevice));
    MZ_TRY(h, spalloc(h, &h->d_sp_done, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_sp_rpos, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_sp_temp, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_sp_tgame, (size_t)G));
    MZ_TRY(h, spalloc(h, &h->d_eval, 4));
    MZ_TRY(h, spalloc(h, &h->d_per_cum, (size_t)h->sp_cap));
    MZ_TRY(h, spalloc(h, &h->d_per_p, (size_t)h->sp_cap));
    MZ_TRY(h, spalloc(h, &h->d_per_total, 1));
    h->sp_eval = 0; h->sp_opp = MZ_OPP_SELF; h->sp_mzp = 1;
    if (sp_constants(h)) return -1;                     // discount powers, the env's symmetry tables
    if (log_rebase(h, 0)) return -1;                    // the run log: a new shard (its ring and setting stay)
    if (env_kind == MZ_ENV_ATARI) {
        // every slot: new game, its key and first frame drawn on the device at
        // the first mz_selfplay_move, keyed by the global game id game_offset +
        // slot that the move carries (ranks of a data-parallel job hold
        // different games, not copies of slot 0..G-1's)
        h->sp_reset_pending = true;
        return 0;
    }
    // every slot: new game (boards: empty plane set, player 1)
    std::vector<uint8_t> b((size_t)G * h->sp_osz, 0);
    const int cells = W * H;
    for (int g = 0; g < G; ++g)
        for (int k = 2 * cells; k < 3 * cells; ++k) b[(size_t)g * h->sp_osz + k] = 1;
    std::vector<int32_t> pl(G, 1);
    MZ_TRY(h, hipMemcpy(h->d_sp_board, b.data(), b.size(), hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(h->d_sp_player, pl.data(), (size_t)G * 4, hipMemcpyHostToDevice));
    return 0;
}

int mz_selfplay_move(mz_handle* h, uint32_t rng_step, uint32_t game_offset, float temperature, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    SpParams S = sp_params(h);
    S.step = rng_step; S.game_offset = game_offset;
    // temperature_threshold (SelfPlay.jl:344-346): per-slot temperatures
    const bool thr = h->conf.temperature_threshold >= 0;
    S.temperature = temperature; S.temp_threshold = h->conf.temperature_threshold;
    S.temp_g = thr || h->sp_latch ? h->d_sp_temp : nullptr;
    S.tgame = h->sp_latch ? h->d_sp_tgame : nullptr;
    const int G = h->sp_G;
    const dim3 waves((G + 3) / 4);
    // the other side has a player of its own: the opponent's nets (mz_selfplay_mode checked the set and
    // the env; both stay), or another kind on the same nets (mz_eval_players).  A no-op once allocated.
    const bool arena = h->sp_eval && eval_secondary(h, h->sp_opp);
    if (arena && opp_io(h)) return -1;
    if (h->sp_reset_pending) {                      // the initial Atari-like games (mz_selfplay_init)
        SpParams R = S;
        R.reset_step = 0xFFFFFFFFu;
        hipLaunchKernelGGL(mz_sp_reset, waves, dim3(256), 0, st, R);
        MZ_TRY(h, hipGetLastError());
        h->sp_reset_pending = false;
    }
    if (int rc = sp_move_body(h, S, h->d_cv2, h->d_rv2, h->d_act2, st)) return rc;
    hipLaunchKernelGGL(mz_sp_order, dim3(1), dim3(1024), 0, st, S);
    hipLaunchKernelGGL(mz_sp_store, dim3(G), dim3(256), 0, st, S);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_selfplay_mode(mz_handle* h, int mode, int opponent, int muzero_player) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (mode != MZ_SP_TRAIN && mode != MZ_SP_EVAL) return fail(h, "mode must be MZ_SP_TRAIN or MZ_SP_EVAL");
    if (opponent != MZ_OPP_SELF && opponent != MZ_OPP_RANDOM && opponent != MZ_OPP_EXPERT && opponent != MZ_OPP_NETWORK &&
        opponent != MZ_OPP_MCTS)
        return fail(h, "opponent must be MZ_OPP_SELF, MZ_OPP_RANDOM, MZ_OPP_EXPERT, MZ_OPP_NETWORK or MZ_OPP_MCTS");
    if (opponent == MZ_OPP_EXPERT && h->sp_env == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    if (opponent == MZ_OPP_MCTS && h->sp_env == MZ_ENV_ATARI)
        return fail(h, "mcts opponent: needs a two-player board env");
    if (muzero_player != 1 && muzero_player != 2) return fail(h, "muzero_player must be 1 or 2");
    if (opponent == MZ_OPP_MCTS && mcts_prepare(h)) return -1;
    if (opponent == MZ_OPP_NETWORK) {
        if (h->sp_env == MZ_ENV_ATARI) return fail(h, "opponent network: needs a two-player board env");
        if (h->opp_have != 7u)
            return fail(h, "opponent: MZ_OPP_NETWORK needs the opponent's nets (mz_opponent_weights_set / _from / "
                           "_load first)");
    }
    // the second outputs: the opponent's nets, or two kinds on one set of nets (mz_eval_players)
    if (mode == MZ_SP_EVAL && eval_secondary(h, opponent)) {
        MZ_TRY(h, hipSetDevice(h->device));
        if (opp_io(h)) return -1;
    }
    h->sp_eval = mode == MZ_SP_EVAL; h->sp_opp = opponent; h->sp_mzp = muzero_player;
    return 0;
}

int mz_eval_players(mz_handle* h, int muzero_kind, int other_kind) {
    if (!h) return -2;
    for (int k : {muzero_kind, other_kind})
        if (k != MZ_PLAYER_SEARCH && k != MZ_PLAYER_PRIOR)
            return fail(h, "eval players: a kind must be MZ_PLAYER_SEARCH or MZ_PLAYER_PRIOR");
    h->ev_kind[0] = muzero_kind; h->ev_kind[1] = other_kind;
    // the second outputs of the mode in force, where the new kinds make a secondary launch necessary
    // (mz_selfplay_mode and the first mz_test_play after it do the same for theirs)
    if (h->sp_env >= 0 && h->sp_eval && eval_secondary(h, h->sp_opp)) {
        MZ_TRY(h, hipSetDevice(h->device));
        if (opp_io(h)) return -1;
    }
    return 0;
}

int mz_expert_depth(mz_handle* h, int depth) {
    if (!h) return -2;
    if (depth < 0 || depth > MZX_MAX_DEPTH) return fail(h, "expert: depth must be in 0..9 (0 = the env's default)");
    h->sp_expert_depth = depth;
    return 0;
}

int mz_mcts_opponent(mz_handle* h, int sims, int rollouts) {
    if (!h) return -2;
    if (sims < 0 || sims > MZM_MAX_SIMS) return fail(h, "mcts opponent: sims must be in 0..1024 (0 = the default, 64)");
    if (rollouts < 0 || rollouts > MZM_MAX_ROLLOUTS)
        return fail(h, "mcts opponent: rollouts must be in 0..64 (0 = the default, 16)");
    h->sp_mcts_sims = sims; h->sp_mcts_rollouts = rollouts;
    return 0;
}

int mz_mcts_eval(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players, int sims,
                 int rollouts, uint32_t rng_step, uint32_t game_offset, int32_t* n_out, int32_t* w_out) {
    if (!h || !boards || !players || !n_out || !w_out) return -2;
    if (int rc = sp_env_check(h, env_kind)) return rc;
    if (env_kind == MZ_ENV_ATARI) return fail(h, "mcts opponent: needs a two-player board env");
    if (G < 1) return fail(h, "mcts opponent: G must be >= 1");
    if (sims < 1 || sims > MZM_MAX_SIMS) return fail(h, "mcts opponent: sims must be in 1..1024");
    if (rollouts < 1 || rollouts > MZM_MAX_ROLLOUTS) return fail(h, "mcts opponent: rollouts must be in 1..64");
    const int A = h->A, osz = 3 * mzx_cells(env_kind);
    for (int g = 0; g < G; ++g) {
        ExpertPos pos;
        if (players[g] != 1 && players[g] != 2) return fail(h, "mcts opponent: player must be 1 or 2");
        if (!mzx_pos_from_planes(env_kind, boards + (size_t)g * osz, players[g], &pos))
            return fail(h, "mcts opponent: every cell must be set in exactly one plane");
    }
    if (mcts_prepare(h)) return -1;
    uint8_t* d_b = nullptr; int32_t* d_p = nullptr; int32_t* d_n = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_b), (size_t)G * osz);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_p), (size_t)G * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_n), (size_t)G * A * 8);   // n then w
    if (e == hipSuccess) e = hipMemcpy(d_b, boards, (size_t)G * osz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_p, players, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        SpParams S;
        std::memset(&S, 0, sizeof(S));
        S.G = G; S.env = env_kind; S.W = h->conf.observation_shape[0]; S.H = h->conf.observation_shape[1];
        S.osz = osz; S.A = A; S.board = d_b; S.player = d_p;
        S.seed = h->seed; S.step = rng_step; S.game_offset = game_offset;
        mcts_launch(S, sims, rollouts, h->d_mcts_sqrt, nullptr, d_n, d_n + (size_t)G * A, h->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(n_out, d_n, (size_t)G * A * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(w_out, d_n + (size_t)G * A, (size_t)G * A * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_b); (void)hipFree(d_p); (void)hipFree(d_n);
    MZ_TRY(h, e);
    return 0;
}

int mz_expert_eval(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players, int depth,
                   int32_t* scores) {
    if (!h || !boards || !players || !scores) return -2;
    if (int rc = sp_env_check(h, env_kind)) return rc;
    if (env_kind == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    if (G < 1) return fail(h, "expert: G must be >= 1");
    if (depth < 1 || depth > MZX_MAX_DEPTH) return fail(h, "expert: depth must be in 1..9");
    const int A = h->A, osz = 3 * mzx_cells(env_kind);
    for (int g = 0; g < G; ++g) {
        ExpertPos pos;
        if (players[g] != 1 && players[g] != 2) return fail(h, "expert: player must be 1 or 2");
        if (!mzx_pos_from_planes(env_kind, boards + (size_t)g * osz, players[g], &pos))
            return fail(h, "expert: every cell must be set in exactly one plane");
    }
    MZ_TRY(h, hipSetDevice(h->device));
    uint8_t* d_b = nullptr; int32_t* d_p = nullptr; int32_t* d_s = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_b), (size_t)G * osz);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_p), (size_t)G * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_s), (size_t)G * A * 4);
    if (e == hipSuccess) e = hipMemcpy(d_b, boards, (size_t)G * osz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_p, players, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        SpParams S;
        std::memset(&S, 0, sizeof(S));
        S.G = G; S.env = env_kind; S.W = h->conf.observation_shape[0]; S.H = h->conf.observation_shape[1];
        S.osz = osz; S.A = A; S.board = d_b; S.player = d_p;
        ExpertArgs X{depth, nullptr, d_s};
        hipLaunchKernelGGL(mz_expert_move, dim3((G + 3) / 4), dim3(256), 0, h->stream, S, X);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(scores, d_s, (size_t)G * A * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_b); (void)hipFree(d_p); (void)hipFree(d_s);
    MZ_TRY(h, e);
    return 0;
}

// the fill: the search kernel's own depth-9 scores of every code, packed
static int expert_table_build(mz_handle* h) {
    const int n = MZX_TTT_CODES;
    MZ_TRY(h, dalloc(h, &h->d_xtable, (size_t)n * MZX_TTT_ENTRY));
    uint8_t* d_b = nullptr; int32_t* d_p = nullptr; int32_t* d_s = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_b), (size_t)n * 27);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_p), (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_s), (size_t)n * 9 * 4);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mz_expert_table_rows, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_b, d_p, 0, n);
        SpParams S;
        std::memset(&S, 0, sizeof(S));
        S.G = n; S.env = MZ_ENV_TICTACTOE; S.W = 3; S.H = 3; S.osz = 27; S.A = 9; S.board = d_b; S.player = d_p;
        ExpertArgs X{9, nullptr, d_s};
        hipLaunchKernelGGL(mz_expert_move, dim3((n + 3) / 4), dim3(256), 0, h->stream, S, X);
        hipLaunchKernelGGL(mz_expert_table_pack, dim3((n * MZX_TTT_ENTRY + 255) / 256), dim3(256), 0, h->stream,
                           (const int32_t*)d_s, h->d_xtable, 0, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_b); (void)hipFree(d_p); (void)hipFree(d_s);
    if (e != hipSuccess) { (void)dfree(h, h->d_xtable); h->d_xtable = nullptr; }
    MZ_TRY(h, e);
    return 0;
}

int mz_expert_table(mz_handle* h, int on) {
    if (!h) return -2;
    if (on != 0 && on != 1) return fail(h, "expert table: on must be 0 or 1");
    if (on) {
        if (int rc = sp_env_check(h, MZ_ENV_TICTACTOE)) return rc;   // this conf can never play TicTacToe
        if (!h->d_xtable) {
            MZ_TRY(h, hipSetDevice(h->device));
            MZ_SYNC(h);
            if (expert_table_build(h)) return -1;
        }
    }
    h->xtable_on = on != 0;
    return 0;
}

int mz_expert_table_get(mz_handle* h, void* scores, int32_t* built, int32_t* in_use) {
    if (!h) return -2;
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (built) *built = h->d_xtable != nullptr;
    if (in_use) *in_use = expert_table_in_use(h);
    if (scores) {
        if (!h->d_xtable) return fail(h, "expert table: not built (mz_expert_table(h, 1) first)");
        std::vector<int8_t> t((size_t)MZX_TTT_CODES * MZX_TTT_ENTRY);
        MZ_TRY(h, hipMemcpy(t.data(), h->d_xtable, t.size(), hipMemcpyDeviceToHost));
        int8_t* out = static_cast<int8_t*>(scores);
        for (int c = 0; c < MZX_TTT_CODES; ++c)
            for (int a = 0; a < 9; ++a) out[(size_t)c * 9 + a] = t[(size_t)c * MZX_TTT_ENTRY + a];
    }
    return 0;
}

int mz_expert_judge(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players,
                    const int32_t* actions, int depth, int64_t* out4) {
    if (!h || !boards || !players || !actions || !out4) return -2;
    if (int rc = sp_env_check(h, env_kind)) return rc;
    if (env_kind == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    if (G < 1) return fail(h, "expert: G must be >= 1");
    if (depth < 1 || depth > MZX_MAX_DEPTH) return fail(h, "expert: depth must be in 1..9");
    const int A = h->A, osz = 3 * mzx_cells(env_kind);
    for (int g = 0; g < G; ++g) {
        ExpertPos pos;
        if (players[g] != 1 && players[g] != 2) return fail(h, "expert: player must be 1 or 2");
        if (!mzx_pos_from_planes(env_kind, boards + (size_t)g * osz, players[g], &pos))
            return fail(h, "expert: every cell must be set in exactly one plane");
        if (actions[g] < 1 || actions[g] > A || !((mzx_legal(pos) >> (actions[g] - 1)) & 1u))
            return fail(h, "expert: action not legal on its board");
    }
    MZ_TRY(h, hipSetDevice(h->device));
    uint8_t* d_b = nullptr; int32_t* d_p = nullptr; int32_t* d_a = nullptr; long long* d_j = nullptr;
    long long j[4] = {0, 0, 0, 0};
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_b), (size_t)G * osz);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_p), (size_t)G * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_a), (size_t)G * 4);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_j), sizeof(j));
    if (e == hipSuccess) e = hipMemcpy(d_b, boards, (size_t)G * osz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_p, players, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_a, actions, (size_t)G * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_j, j, sizeof(j), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        SpParams S;
        std::memset(&S, 0, sizeof(S));
        S.G = G; S.env = env_kind; S.W = h->conf.observation_shape[0]; S.H = h->conf.observation_shape[1];
        S.osz = osz; S.A = A; S.board = d_b; S.player = d_p;
        S.opponent = MZ_OPP_SELF;                   // every row is judged
        ExpertArgs X{depth, d_a, nullptr, nullptr, d_j};
        hipLaunchKernelGGL(mz_expert_move, dim3((G + 3) / 4), dim3(256), 0, h->stream, S, X);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(j, d_j, sizeof(j), hipMemcpyDeviceToHost);
    (void)hipFree(d_b); (void)hipFree(d_p); (void)hipFree(d_a); (void)hipFree(d_j);
    MZ_TRY(h, e);
    for (int i = 0; i < 4; ++i) out4[i] = j[i];
    return 0;
}

int mz_eval_results(mz_handle* h, int64_t* out4) {
    if (!h || !out4) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c[4];
    MZ_TRY(h, hipMemcpy(c, h->d_eval, sizeof(c), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out4[i] = c[i];
    return 0;
}

// ---- the test worker: evaluation games on their own slots
// mz_selfplay_mode's refusals, for mz_test_config's setting (checked again by every mz_test_play:
// the env and the opponent set may have changed since)
static int test_check(mz_handle* h, int games, int opponent, int muzero_player) {
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (games < 0 || games > h->max_games) return fail(h, "mz_test_config: games must be in 0..max_games");
    if (opponent != MZ_OPP_SELF && opponent != MZ_OPP_RANDOM && opponent != MZ_OPP_EXPERT && opponent != MZ_OPP_NETWORK &&
        opponent != MZ_OPP_MCTS)
        return fail(h, "opponent must be MZ_OPP_SELF, MZ_OPP_RANDOM, MZ_OPP_EXPERT, MZ_OPP_NETWORK or MZ_OPP_MCTS");
    if (opponent == MZ_OPP_EXPERT && h->sp_env == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    if (opponent == MZ_OPP_MCTS && h->sp_env == MZ_ENV_ATARI)
        return fail(h, "mcts opponent: needs a two-player board env");
    if (muzero_player != 1 && muzero_player != 2) return fail(h, "muzero_player must be 1 or 2");
    if (opponent == MZ_OPP_MCTS && mcts_prepare(h)) return -1;
    if (opponent == MZ_OPP_NETWORK) {
        if (h->sp_env == MZ_ENV_ATARI) return fail(h, "opponent network: needs a two-player board env");
        if (h->opp_have != 7u)
            return fail(h, "opponent: MZ_OPP_NETWORK needs the opponent's nets (mz_opponent_weights_set / _from / "
                           "_load first)");
    }
    return 0;
}

// the test slots: self-play state (sp_allocs).  Nothing is zeroed: mz_test_begin starts every slot,
// and every other word is written before it is read.
static int test_alloc(mz_handle* h) {
    mz_handle::TestSlots& t = h->ts;
    const size_t E = (size_t)h->test_E, T = (size_t)h->sp_T, A = (size_t)h->A;
    if (t.E != h->test_E) {                  // the first evaluation after a re-init, or another E since
        t = mz_handle::TestSlots{};
        MZ_TRY(h, spalloc(h, &t.board, E * h->sp_osz, false));
        MZ_TRY(h, spalloc(h, &t.player, E, false));
        MZ_TRY(h, spalloc(h, &t.over, E, false));
        MZ_TRY(h, spalloc(h, &t.ekey, E, false));
        MZ_TRY(h, spalloc(h, &t.hist.obs, E * T * h->sp_osz, false));
        MZ_TRY(h, spalloc(h, &t.hist.act, E * T, false));
        MZ_TRY(h, spalloc(h, &t.hist.rew, E * T, false));
        MZ_TRY(h, spalloc(h, &t.hist.tp, E * T, false));
        MZ_TRY(h, spalloc(h, &t.hist.cv, E * T * A, false));
        MZ_TRY(h, spalloc(h, &t.hist.rv, E * T, false));
        MZ_TRY(h, spalloc(h, &t.hist.len, E, false));
        MZ_TRY(h, spalloc(h, &t.done, E, false));
        MZ_TRY(h, spalloc(h, &t.frozen, E, false));
        MZ_TRY(h, spalloc(h, &t.temp, E, false));
        t.E = h->test_E;
    }
    if (eval_secondary(h, h->test_opp) && !t.act2) {
        MZ_TRY(h, spalloc(h, &t.cv2, E * A, false));
        MZ_TRY(h, spalloc(h, &t.rv2, E, false));
        MZ_TRY(h, spalloc(h, &t.act2, E, false));
    }
    if (!h->d_test_counts) {                 // the record ring: the handle's
        MZ_TRY(h, dalloc(h, &h->d_test_counts, (size_t)MZ_TEST_RECORDS * 8));
        MZ_TRY(h, dalloc(h, &h->d_test_sums, (size_t)MZ_TEST_RECORDS * 3));
    }
    return 0;
}

int mz_test_config(mz_handle* h, int32_t games, int opponent, int muzero_player) {
    if (!h) return -2;
    if (int rc = test_check(h, games, opponent, muzero_player)) return rc;
    h->test_E = games; h->test_opp = opponent; h->test_mzp = muzero_player;
    return 0;
}

int mz_test_play(mz_handle* h, int64_t training_step, uint32_t rng_step0, uint32_t game_offset, float temperature,
                 void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->test_E < 1) return fail(h, "mz_test_play: no test slots (mz_test_config with games >= 1 first)");
    if (int rc = test_check(h, h->test_E, h->test_opp, h->test_mzp)) return rc;
    if (h->test_audit && h->sp_env == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    if (test_alloc(h)) return -1;
    if (h->test_audit && !h->d_test_audit) MZ_TRY(h, dalloc(h, &h->d_test_audit, (size_t)MZ_TEST_RECORDS * 4));
    const mz_handle::TestSlots& t = h->ts;
    SpParams S = sp_params(h, true);
    S.game_offset = game_offset; S.reset_step = 0xFFFFFFFFu;
    S.temperature = temperature; S.temp_threshold = h->conf.temperature_threshold;
    S.temp_g = h->conf.temperature_threshold >= 0 ? t.temp : nullptr;
    const size_t slot = (size_t)(h->test_total % MZ_TEST_RECORDS);
    TestRec R{h->d_test_counts + slot * 8, h->d_test_sums + slot * 3, (long long)training_step, rng_step0, t.frozen,
              h->conf.players};
    hipLaunchKernelGGL(mz_test_begin, dim3((t.E + 3) / 4), dim3(256), 0, st, S, R);
    MZ_TRY(h, hipGetLastError());
    // judging (mz_test_audit): the evaluation's audit row, zeroed on the stream; off: nothing is issued
    long long* judge = h->test_audit ? h->d_test_audit + slot * 4 : nullptr;
    if (judge) MZ_TRY(h, hipMemsetAsync(judge, 0, 4 * sizeof(long long), st));
    h->test_audited[slot] = judge != nullptr;
    // the host never learns when every slot is done: always T moves, the frozen slots as dummy rows
    for (int m = 0; m < h->sp_T; ++m) {
        S.step = rng_step0 + (uint32_t)m;
        if (int rc = sp_move_body(h, S, t.cv2, t.rv2, t.act2, st, judge)) return rc;
        hipLaunchKernelGGL(mz_test_tally, dim3(1), dim3(1024), 0, st, S, R);
        MZ_TRY(h, hipGetLastError());
    }
    h->ts.played = true;
    ++h->test_total;
    return 0;
}

int mz_test_results(mz_handle* h, int64_t* total, int64_t* counts, double* sums, int32_t max_records) {
    if (!h) return -2;
    if (max_records < 0) return fail(h, "mz_test_results: max_records must be >= 0");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (total) *total = h->test_total;
    const int64_t held = std::min<int64_t>(h->test_total, MZ_TEST_RECORDS);
    const int64_t n = std::min<int64_t>(max_records, held);
    for (int64_t i = 0; i < n; ++i) {
        const size_t slot = (size_t)((h->test_total - n + i) % MZ_TEST_RECORDS);
        long long c[8];
        MZ_TRY(h, hipMemcpy(c, h->d_test_counts + slot * 8, sizeof(c), hipMemcpyDeviceToHost));
        if (counts) for (int k = 0; k < 8; ++k) counts[i * 8 + k] = c[k];
        if (sums) MZ_TRY(h, hipMemcpy(sums + i * 3, h->d_test_sums + slot * 3, 3 * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

int mz_test_clear(mz_handle* h) {
    if (!h) return -2;
    h->test_total = 0;
    std::fill(h->test_audited.begin(), h->test_audited.end(), (uint8_t)0);
    return 0;
}

int mz_test_audit(mz_handle* h, int on) {
    if (!h) return -2;
    if (on != 0 && on != 1) return fail(h, "mz_test_audit: on must be 0 or 1");
    if (on && h->sp_env == MZ_ENV_ATARI) return fail(h, "expert: needs a two-player board env");
    h->test_audit = on != 0;
    return 0;
}

int mz_test_audit_results(mz_handle* h, int64_t* total, int64_t* audit, int32_t max_records) {
    if (!h) return -2;
    if (max_records < 0) return fail(h, "mz_test_audit_results: max_records must be >= 0");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    if (total) *total = h->test_total;
    const int64_t held = std::min<int64_t>(h->test_total, MZ_TEST_RECORDS);
    const int64_t n = std::min<int64_t>(max_records, held);
    for (int64_t i = 0; audit && i < n; ++i) {      // mz_test_results' rows, in its order
        const size_t slot = (size_t)((h->test_total - n + i) % MZ_TEST_RECORDS);
        long long a[4] = {-1, 0, 0, 0};             // an evaluation run with judging off
        if (h->test_audited[slot])
            MZ_TRY(h, hipMemcpy(a, h->d_test_audit + slot * 4, sizeof(a), hipMemcpyDeviceToHost));
        for (int k = 0; k < 4; ++k) audit[i * 4 + k] = a[k];
    }
    return 0;
}

int mz_test_get_game(mz_handle* h, int32_t slot, int32_t* T, uint8_t* obs, int32_t* actions, float* rewards,
                     int32_t* to_play, float* child_visits, float* root_values) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (!h->ts.played) return fail(h, "mz_test_get_game: no evaluation since mz_selfplay_init (mz_test_play first)");
    if (slot < 0 || slot >= h->ts.E) return fail(h, "mz_test_get_game: slot out of range");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const size_t base = (size_t)slot * h->sp_T, A = (size_t)h->A;
    const SpHist& r = h->ts.hist;
    int32_t len = 0;
    MZ_TRY(h, hipMemcpy(&len, r.len + slot, 4, hipMemcpyDeviceToHost));
    if (T) *T = len;
    if (obs) MZ_TRY(h, hipMemcpy(obs, r.obs + base * h->sp_osz, (size_t)len * h->sp_osz, hipMemcpyDeviceToHost));
    if (actions) MZ_TRY(h, hipMemcpy(actions, r.act + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (rewards) MZ_TRY(h, hipMemcpy(rewards, r.rew + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (to_play) MZ_TRY(h, hipMemcpy(to_play, r.tp + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (child_visits) MZ_TRY(h, hipMemcpy(child_visits, r.cv + base * A, (size_t)len * A * 4, hipMemcpyDeviceToHost));
    if (root_values) MZ_TRY(h, hipMemcpy(root_values, r.rv + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mz_replay_counts(mz_handle* h, int64_t* counts, int32_t* games_in_buffer) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c[3];
    MZ_TRY(h, hipMemcpy(c, h->d_sp_counters, sizeof(c), hipMemcpyDeviceToHost));
    if (counts) for (int i = 0; i < 3; ++i) counts[i] = c[i];
    if (games_in_buffer) *games_in_buffer = (int32_t)std::min<long long>(c[0], h->sp_cap);
    return 0;
}

int mz_replay_save_game(mz_handle* h, int32_t T, const uint8_t* obs, const int32_t* actions, const float* rewards,
                        const int32_t* to_play, const float* child_visits, const float* root_values) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (T < 1 || T > h->sp_T) return fail(h, "game length must be in 1..max_moves+1");
    if (!obs || !actions || !rewards || !to_play || !child_visits || !root_values) return fail(h, "null array");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c[3];
    MZ_TRY(h, hipMemcpy(c, h->d_sp_counters, sizeof(c), hipMemcpyDeviceToHost));
    const long long num = c[0] + 1;
    const int slot = (int)((num - 1) % h->sp_cap);
    if (num > h->sp_cap) {                          // the FIFO evicts game num - cap (:156-160)
        int32_t old = 0;
        MZ_TRY(h, hipMemcpy(&old, h->sp_ring.len + slot, 4, hipMemcpyDeviceToHost));
        c[2] -= old;
    }
    c[0] = num; c[1] += T; c[2] += T;
    const size_t base = (size_t)slot * h->sp_T, A = (size_t)h->A;
    const SpHist& r = h->sp_ring;
    MZ_TRY(h, hipMemcpy(r.obs + base * h->sp_osz, obs, (size_t)T * h->sp_osz, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.act + base, actions, (size_t)T * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.rew + base, rewards, (size_t)T * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.tp + base, to_play, (size_t)T * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.cv + base * A, child_visits, (size_t)T * A * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.rv + base, root_values, (size_t)T * 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemcpy(r.len + slot, &T, 4, hipMemcpyHostToDevice));
    MZ_TRY(h, hipMemset(r.rean + slot, 0, 4));      // a new game: reanalysed values = `nothing`
    MZ_TRY(h, hipMemcpy(h->d_sp_counters, c, sizeof(c), hipMemcpyHostToDevice));
    if (h->conf.PER) {                              // initial priorities (:136-143)
        hipLaunchKernelGGL(mz_rp_per_init, dim3(1), dim3(64), 0, h->stream, h->sp_ring, slot, (int)T, h->sp_T,
                           h->conf.td_steps, (const float*)h->d_sp_dpow, h->conf.PER_alpha);
        MZ_TRY(h, hipGetLastError());
        MZ_SYNC(h);
    }
    return 0;
}

// get_batch parameters for B samples at learner step `step` into the
// engine's batch arrays (allocated on first use); batch = those arrays
static int rs_params(mz_handle* h, int32_t B, uint32_t step, hipStream_t st, RpSampleParams* Qo, mz_batch* batch,
                     bool prefetching = false) {
    if (!prefetching) ++h->pf_epoch;              // set 0 is about to be refilled: its header is stale
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (B < 1) return fail(h, "batch_size must be >= 1");
    if (!h->sp_has_games) {                       // sample_n_games needs a non-empty buffer
        long long played = 0;
        MZ_TRY(h, hipStreamSynchronize(st));
        MZ_TRY(h, hipMemcpy(&played, h->d_sp_counters, sizeof(played), hipMemcpyDeviceToHost));
        if (played == 0) return fail(h, "replay buffer is empty");
        h->sp_has_games = true;
    }
    const int K1 = h->conf.num_unroll_steps + 1, A = h->A;
    if (B > h->rs_cap) {
        MZ_TRY(h, spalloc(h, &h->d_rs_obs, (size_t)B * h->obs_feat, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_act, (size_t)B * K1, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_tv, (size_t)B * K1, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_tr, (size_t)B * K1, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_tp, (size_t)B * K1 * A, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_gs, (size_t)B, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_index, (size_t)B * 2, false));
        MZ_TRY(h, spalloc(h, &h->d_rs_w, (size_t)B, false));
        h->rs_cap = B;
        ++h->pf_epoch;
    }
    RpSampleParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.B = B; Q.K = K1 - 1; Q.A = A; Q.osz = h->sp_osz; Q.P = h->plane; Q.F = h->obs_feat;
    Q.stacked = h->conf.stacked_observations; Q.T = h->sp_T; Q.td = h->conf.td_steps; Q.cap = h->sp_cap;
    Q.frames = h->sp_frames;
    Q.seed = h->seed; Q.step = step; Q.ring = h->sp_ring; Q.counters = h->d_sp_counters; Q.disc_pow = h->d_sp_dpow;
    Q.obs = h->d_rs_obs; Q.actions = h->d_rs_act; Q.tv = h->d_rs_tv; Q.tr = h->d_rs_tr; Q.tpol = h->d_rs_tp;
    Q.gscale = h->d_rs_gs; Q.index = h->d_rs_index;
    Q.per = h->conf.PER != 0;
    if (Q.per) {                                  // game probabilities of the held games (:91-99)
        Q.per_cum = h->d_per_cum; Q.per_p = h->d_per_p; Q.per_total = h->d_per_total; Q.weights = h->d_rs_w;
        hipLaunchKernelGGL(mz_rp_per_prep, dim3(1), dim3(64), 0, st, h->sp_ring, (const long long*)h->d_sp_counters,
                           h->sp_cap, h->d_per_cum, h->d_per_p, h->d_per_total);
        MZ_TRY(h, hipGetLastError());
    }
    if (h->sym_on && h->d_sym) {                  // mz_replay_set_symmetry: every path draws under the env's group
        Q.sym_n = h->sym_n;                       // (the tables follow disc_pow in its buffer)
        Q.sym_cell = (int)(h->d_sym - reinterpret_cast<int32_t*>(h->d_sp_dpow));
        Q.sym_act = Q.sym_cell + h->sym_n * h->plane;
    }
    *Qo = Q;
    batch->batch_size = B;
    batch->observation = h->d_rs_obs; batch->actions = h->d_rs_act; batch->target_values = h->d_rs_tv;
    batch->target_rewards = h->d_rs_tr; batch->target_policies = h->d_rs_tp; batch->gradient_scale = h->d_rs_gs;
    batch->weights = Q.per ? h->d_rs_w : nullptr;
    return 0;
}

// PER: weight_batch ./= maximum(weight_batch) after the sampling launch
static int per_norm(mz_handle* h, int B, hipStream_t st) {
    if (!h->conf.PER) return 0;
    hipLaunchKernelGGL(mz_rp_per_norm, dim3(1), dim3(256), 0, st, h->d_rs_w, B);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

// PER: update_priorities! of the last sampled batch from the last unroll's values
static int per_update(mz_handle* h, int B, hipStream_t st) {
    if (!h->conf.PER) return 0;
    hipLaunchKernelGGL(mz_rp_per_update, dim3(1), dim3(64), 0, st, h->sp_ring, (const long long*)h->d_sp_counters,
                       h->sp_cap, h->sp_T, B, h->conf.num_unroll_steps, h->conf.PER_alpha, h->d_rs_index, h->d_pv,
                       h->d_rs_tv);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_replay_sample(mz_handle* h, int32_t B, uint32_t step, mz_batch* batch, int32_t* index_batch, void* stream) {
    if (!h || !batch) return -2;
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    RpSampleParams Q;
    if (rs_params(h, B, step, st, &Q, batch)) return -1;
    hipLaunchKernelGGL(mz_rp_sample, dim3((B + 3) / 4), dim3(256), 0, st, Q);
    MZ_TRY(h, hipGetLastError());
    if (per_norm(h, B, st)) return -1;
    h->rs_last_B = B;
    if (index_batch) {
        MZ_TRY(h, hipMemcpyAsync(index_batch, h->d_rs_index, (size_t)B * 8, hipMemcpyDeviceToHost, st));
        MZ_TRY(h, hipStreamSynchronize(st));
    }
    return 0;
}

// the board env's group for the symmetry calls: refusals that name the env
static int sym_env_check(mz_handle* h) {
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->sp_env == MZ_ENV_ATARI) return fail(h, "symmetry: the Atari-like env has no symmetry group");
    if (!h->sym_n || !h->d_sym) return fail(h, "symmetry: the env has no symmetry group");
    return 0;
}

int mz_replay_set_symmetry(mz_handle* h, int on) {
    if (!h) return -2;
    if (int rc = sym_env_check(h)) return rc;
    if (on != 0 && on != 1) return fail(h, "symmetry: on must be 0 (off) or 1 (the env's full group)");
    if (h->sym_on != (on != 0)) ++h->pf_epoch;      // a batch drawn ahead was drawn under the other setting
    h->sym_on = on != 0;
    return 0;
}

int mz_replay_symmetry_get(mz_handle* h, int32_t* n, int32_t* cell_perm, int32_t* action_perm, int32_t* on) {
    if (!h) return -2;
    if (int rc = sym_env_check(h)) return rc;
    MZ_TRY(h, hipSetDevice(h->device));
    const size_t nc = (size_t)h->sym_n * h->plane, na = (size_t)h->sym_n * h->A;
    if (n) *n = h->sym_n;
    if (cell_perm) MZ_TRY(h, hipMemcpy(cell_perm, h->d_sym, nc * 4, hipMemcpyDeviceToHost));
    if (action_perm) MZ_TRY(h, hipMemcpy(action_perm, h->d_sym + nc, na * 4, hipMemcpyDeviceToHost));
    if (on) *on = h->sym_on ? 1 : 0;
    return 0;
}

int mz_batch_symmetry(mz_handle* h, const mz_batch* in_dev, const int32_t* sym_dev, mz_batch* out_dev, void* stream) {
    if (!h || !in_dev || !out_dev || !sym_dev) return -2;
    if (int rc = sym_env_check(h)) return rc;
    const int B = in_dev->batch_size, K1 = h->conf.num_unroll_steps + 1, A = h->A;
    if (B < 1) return fail(h, "batch_size must be >= 1");
    if (out_dev->batch_size != B) return fail(h, "symmetry: the two batches must have the same batch_size");
    const size_t sz[7] = {(size_t)B * h->obs_feat, (size_t)B * K1, (size_t)B * K1, (size_t)B * K1, (size_t)B * K1 * A,
                          (size_t)B, (size_t)B};
    const float* in[7] = {in_dev->observation, in_dev->actions, in_dev->target_values, in_dev->target_rewards,
                          in_dev->target_policies, in_dev->gradient_scale, in_dev->weights};
    const float* out[7] = {out_dev->observation, out_dev->actions, out_dev->target_values, out_dev->target_rewards,
                           out_dev->target_policies, out_dev->gradient_scale, out_dev->weights};
    for (int i = 0; i < 6; ++i)
        if (!in[i] || !out[i]) return fail(h, "symmetry: a batch array is NULL");
    for (int i = 0; i < 7; ++i)                     // the transform scatters: an output may overlap no input
        for (int j = 0; j < 7; ++j)
            if (in[i] && out[j] && in[i] < out[j] + sz[j] && out[j] < in[i] + sz[i])
                return fail(h, "symmetry: the output arrays must not overlap the input arrays (in == out is refused)");
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (out[i] && out[j] && out[i] < out[j] + sz[j] && out[j] < out[i] + sz[i])
                return fail(h, "symmetry: the output arrays overlap each other");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    RpSymParams Y;
    std::memset(&Y, 0, sizeof(Y));
    Y.B = B; Y.K = K1 - 1; Y.A = A; Y.P = h->plane; Y.C = h->sp_osz / h->plane; Y.F = h->obs_feat;
    Y.n = h->sym_n; Y.cell = h->d_sym; Y.act = h->d_sym + (size_t)h->sym_n * h->plane;
    Y.sym = sym_dev;
    Y.obs = in[0]; Y.actions = in[1]; Y.tv = in[2]; Y.tr = in[3]; Y.tpol = in[4]; Y.gscale = in[5];
    Y.o_obs = const_cast<float*>(out[0]); Y.o_actions = const_cast<float*>(out[1]);
    Y.o_tv = const_cast<float*>(out[2]); Y.o_tr = const_cast<float*>(out[3]);
    Y.o_tpol = const_cast<float*>(out[4]); Y.o_gscale = const_cast<float*>(out[5]);
    if (in[6] && out[6]) { Y.weights = in[6]; Y.o_weights = const_cast<float*>(out[6]); }
    hipLaunchKernelGGL(mz_rp_symmetry, dim3((B + 3) / 4), dim3(256), 0, st, Y);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

// the second batch set and the two headers of the get_batch prefetch
static int ensure_pf(mz_handle* h, int B) {
    if (B <= h->pf_cap && h->d_pf_hdr) return 0;
    const int K1 = h->conf.num_unroll_steps + 1, A = h->A;
    MZ_TRY(h, spalloc(h, &h->d_rs2_obs, (size_t)B * h->obs_feat, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_act, (size_t)B * K1, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_tv, (size_t)B * K1, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_tr, (size_t)B * K1, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_tp, (size_t)B * K1 * A, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_gs, (size_t)B, false));
    MZ_TRY(h, spalloc(h, &h->d_rs2_index, (size_t)B * 2, false));
    if (!h->d_pf_hdr) MZ_TRY(h, spalloc(h, &h->d_pf_hdr, 8));   // zeroed: matches no epoch
    h->pf_cap = B;
    ++h->pf_epoch;
    return 0;
}

// point the sampler's outputs and the batch at batch set s (0: d_rs_*, 1: d_rs2_*)
static void pf_set(mz_handle* h, int s, RpSampleParams* Q, mz_batch* b) {
    Q->obs = s ? h->d_rs2_obs : h->d_rs_obs; Q->actions = s ? h->d_rs2_act : h->d_rs_act;
    Q->tv = s ? h->d_rs2_tv : h->d_rs_tv; Q->tr = s ? h->d_rs2_tr : h->d_rs_tr;
    Q->tpol = s ? h->d_rs2_tp : h->d_rs_tp; Q->gscale = s ? h->d_rs2_gs : h->d_rs_gs;
    Q->index = s ? h->d_rs2_index : h->d_rs_index;
    if (b) {
        b->observation = Q->obs; b->actions = Q->actions; b->target_values = Q->tv;
        b->target_rewards = Q->tr; b->target_policies = Q->tpol; b->gradient_scale = Q->gscale;
    }
}

// Learner iteration on a batch drawn from this GPU's replay shard
// (get_batch + learning!, ReplayBuffer.jl:188-217, Learning.jl:327-404) with
// the sampling fused into the FC unroll kernel: results are those of
// mz_replay_sample(step) + mz_learner_grad_dev (+ mz_learner_apply_dev with
// grad_scale 1 for mz_learner_train_dev, whose ADAM update is fused into the
// loss kernel: one GPU, no gradient exchange).
static int learner_sampled(mz_handle* h, int32_t B, uint32_t step, float* grad_dev, float* losses_dev,
                           hipStream_t st, bool train, double eta) {
    MZ_TRY(h, hipSetDevice(h->device));
    RpSampleParams Q;
    mz_batch b;
    const int ti = small_unroll_ti(h, B);
    const bool fused = train && ti >= 0 && !h->conf.PER && h->A <= 16 && h->d_sm_w2 && h->kind != 1 &&
                       h->learn_mode != MZ_LEARN_CORRECTED;
    const bool pf = fused && !std::getenv("MZ_NO_BATCH_PREFETCH");
    if (rs_params(h, B, step, st, &Q, &b, pf)) return -1;
    if (ensure_batch(h, B)) return -1;
    if (pf && ensure_pf(h, B)) return -1;
    h->rs_last_B = B;
    if (h->learn_mode == MZ_LEARN_CORRECTED) {     // sample, backprop, (ADAM)
        hipLaunchKernelGGL(mz_rp_sample, dim3((B + 3) / 4), dim3(256), 0, st, Q);
        MZ_TRY(h, hipGetLastError());
        if (per_norm(h, B, st)) return -1;
        if (bp_grad(h, &b, train ? nullptr : grad_dev, losses_dev, st)) return -1;
        if (per_update(h, B, st)) return -1;                       // Learning.jl:400-404
        return train ? mz_learner_apply_dev(h, nullptr, 1.0f, eta, st) : 0;
    }
    if (h->kind == 1) {                             // ResNet: sample, then the network unroll
        if (h->conf.PER || h->ds) {                 // (else the sample is drawn inside the unroll launch)
            hipLaunchKernelGGL(mz_rp_sample, dim3((B + 3) / 4), dim3(256), 0, st, Q);
            MZ_TRY(h, hipGetLastError());
            if (per_norm(h, B, st)) return -1;
        }
        // one GPU: ADAM fused into the loss / Σθ² kernel (as the FC path)
        if (rlearner_grad(h, &b, train ? nullptr : grad_dev, losses_dev, st, train, eta,
                          h->conf.PER || h->ds ? nullptr : &Q)) return -1;
        return per_update(h, B, st);                               // Learning.jl:400-404
    }
    if (fused) {
        // one launch: unroll + losses ‖ Σθ² + ADAM into the second image set, then swap the sets;
        // with the prefetch, plus step + 1's get_batch into the other batch set
        const int cur = pf ? h->pf_cur : 0;
        RpSampleParams Qn = Q;
        if (pf) {
            pf_set(h, cur, &Q, &b);
            pf_set(h, 1 - cur, &Qn, nullptr);
            Qn.step = step + 1;
        }
        SmallUnrollParams U;
        if (small_unroll_params(h, &b, ti, &Q, &U)) return -1;
        U.pf_hdr = pf ? h->d_pf_hdr + 4 * cur : nullptr;
        U.pf_epoch = h->pf_epoch;
        LearnParams L;
        L.pf_nb = pf ? (B + SM_THREADS / 64 - 1) / (SM_THREADS / 64) : 0;
        L.pfq = Qn;
        L.pf_hdr_next = pf ? h->d_pf_hdr + 4 * (1 - cur) : nullptr;
        L.pf_epoch = h->pf_epoch;
        L.nU = (B + ti) / (ti + 1);
        L.tv = b.target_values; L.tp = b.target_policies; L.gscale = b.gradient_scale;
        L.terms = h->d_lterm; L.flat = h->d_flat; L.netoff = h->d_netoff; L.part = h->d_sq; L.counter = h->d_counter;
        L.out = losses_dev ? losses_dev : h->d_loss;
        L.ad = LgAdam{1, h->d_m, h->d_v, h->bp1, h->bp2, eta, h->d_Wp2, h->d_Bp2, h->d_inv_tile, h->d_sm_w2,
                      h->d_sm_bias2, h->d_inv_small};
        // (the unroll workgroups on one XCD, their weight image fetched into one L2, measured PMC
        // 3.79 MB per launch instead of 6.41 MB, but 31.4 k instead of 33.9 k steps/s: not kept)
        void* args[] = {&U, &L};
        MZ_TRY(h, hipLaunchKernel(small_kernel(h, SMK_LEARN, ti), dim3(L.nU + LEARN_L2_GROUPS + L.pf_nb),
                                  dim3(SM_THREADS), args, unroll_small_lds(h, ti), st));
        if (pf) h->pf_cur = 1 - cur;
        h->last_lvariant = ti == 0 ? "mz_learn_small1" : "mz_learn_small2";
        std::swap(h->d_Wp, h->d_Wp2); std::swap(h->d_Bp, h->d_Bp2);
        std::swap(h->d_sm_w, h->d_sm_w2); std::swap(h->d_sm_bias, h->d_sm_bias2);
        adam_advance(h);
        return 0;
    }
    if (fc_unroll(h, &b, st, &Q)) return -1;
    if (per_norm(h, B, st)) return -1;
    if (learner_losses(h, &b, grad_dev, losses_dev, st, h->lay.v_act, h->lay.r_act, train, eta)) return -1;
    return per_update(h, B, st);                                   // Learning.jl:400-404
}

int mz_replay_update_priorities(mz_handle* h, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (!h->conf.PER) return fail(h, "PER is off in the config");
    if (h->rs_last_B <= 0) return fail(h, "no batch sampled yet");
    MZ_TRY(h, hipSetDevice(h->device));
    return per_update(h, h->rs_last_B, stream_of(h, stream));
}

int mz_replay_get_priorities(mz_handle* h, int32_t i, float* priorities, float* game_priority) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long played = 0;
    MZ_TRY(h, hipMemcpy(&played, h->d_sp_counters, sizeof(played), hipMemcpyDeviceToHost));
    const long long n = std::min<long long>(played, h->sp_cap);
    if (i < 0 || i >= n) return fail(h, "game index out of range");
    const int slot = (int)((played - n + i) % h->sp_cap);
    int32_t T = 0;
    MZ_TRY(h, hipMemcpy(&T, h->sp_ring.len + slot, 4, hipMemcpyDeviceToHost));
    if (priorities)
        MZ_TRY(h, hipMemcpy(priorities, h->sp_ring.prio + (size_t)slot * h->sp_T, (size_t)T * 4, hipMemcpyDeviceToHost));
    if (game_priority) MZ_TRY(h, hipMemcpy(game_priority, h->sp_ring.gprio + slot, 4, hipMemcpyDeviceToHost));
    return 0;
}

int mz_learner_grad_sampled_dev(mz_handle* h, int32_t B, uint32_t step, float* grad_dev, float* losses_dev,
                                void* stream) {
    if (!h) return -2;
    return learner_sampled(h, B, step, grad_dev, losses_dev, stream_of(h, stream), false, 0.0);
}

// ---- data-parallel learner over RCCL through the C ABI
#define MZ_DP_ID_BYTES 128   // sizeof(ncclUniqueId)
int mz_dp_unique_id(uint8_t* id) {
    if (!id) return -2;
    if (!rccl().ok) return -1;
    return rccl().get_id(id) == 0 ? 0 : -1;
}

int mz_dp_init(mz_handle* h, int rank, int world, const uint8_t* id) {
    if (!h || !id) return -2;
    if (world < 1 || rank < 0 || rank >= world) return fail(h, "rank / world out of range");
    if (!rccl().ok) return fail(h, "librccl.so.1 not found");
    MZ_TRY(h, hipSetDevice(h->device));
    dp_destroy(h);
    RcclId v;
    std::memcpy(v.b, id, MZ_DP_ID_BYTES);
    void* comm = nullptr;
    const int rc = rccl().init_rank(&comm, world, v, rank);
    if (rc != 0) return fail(h, std::string("ncclCommInitRank: ") + (rccl().err ? rccl().err(rc) : "error"));
    h->dp_comm = comm; h->dp_world = world; h->dp_rank = rank;
    return 0;
}

int mz_dp_allreduce(mz_handle* h, float* grad_dev, void* stream) {
    if (!h) return -2;
    if (!h->dp_comm) return fail(h, "mz_dp_init first");
    hipStream_t st = stream_of(h, stream);
    float* g = grad_dev ? grad_dev : h->d_grad;
    // ncclFloat32 = 7, ncclSum = 0
    const int rc = rccl().allreduce(g, g, h->nflat, 7, 0, h->dp_comm, st);
    if (rc != 0) return fail(h, std::string("ncclAllReduce: ") + (rccl().err ? rccl().err(rc) : "error"));
    return 0;
}

int mz_learner_train_dp(mz_handle* h, int32_t B, uint32_t step, double eta, float* losses_dev, void* stream) {
    if (!h) return -2;
    if (!h->dp_comm) return fail(h, "mz_dp_init first");
    hipStream_t st = stream_of(h, stream);
    if (learner_sampled(h, B, step, nullptr, losses_dev, st, false, 0.0)) return -1;
    if (mz_dp_allreduce(h, nullptr, st)) return -1;
    return mz_learner_apply_dev(h, nullptr, 1.0f / (float)h->dp_world, eta, st);
}

int mz_learner_train_dev(mz_handle* h, int32_t B, uint32_t step, double eta, float* losses_dev, void* stream) {
    if (!h) return -2;
    return learner_sampled(h, B, step, nullptr, losses_dev, stream_of(h, stream), true, eta);
}

// ---- L consecutive ref_semantics learner steps (ChainParams, mz_small_params.h;
// Learning.jl:327-404 with get_batch keyed by the step, Q11).  The L steps run
// as chunks of up to MZ_MULTI_MAX steps, each one chain launch (the ADAM
// iterations) and unroll launches of up to MZ_MULTI_UNROLL steps, in stream
// order (32-step chains: the chain's fixed costs over twice the steps).  (Measured: the next
// sub-chunk's chain on a second stream, ordered by events, beside the unroll
// launch — 228.8 k vs 279.5 k steps/s at L = 64, 114.6 k vs ~170 k at L = 8:
// the cross-stream event waits cost more than the chain they hide.)
static bool multi_ok(const mz_handle* h) {
    return h->kind == 0 && h->learn_mode == MZ_LEARN_REF_SEMANTICS && !h->conf.PER && h->small_ok && h->A <= 16 &&
           h->d_sm_w2;
}
// Sub-chunk length Ls and T per workgroup for L steps of B samples: one sample
// per workgroup while the L·B workgroups fit one per CU; else two, with as
// many steps per sub-chunk as keep one workgroup per CU (16 at B = 32)
static int multi_plan(const mz_handle* h, int B, int L, int* Ls) {
    int ti;
    // T = 4 (round 6) when the call has the steps to fill the chip with 4 samples per workgroup
    // (twice the steps per unroll launch as T = 2 for about 1.1x a stage's cost); T = 2 when L·B
    // exceeds the CUs; T = 1 below
    const int nU4 = (B + 3) / 4;
    if ((size_t)L * B <= (size_t)h->n_cu && small_unroll_fits(h, 0)) ti = 0;
    else if (L >= std::min(MZ_MULTI_MAX, h->n_cu / nU4) && (size_t)L * nU4 >= (size_t)h->n_cu &&
             small_unroll_fits(h, 2)) ti = 2;
    else if (small_unroll_fits(h, 1)) ti = 1;
    else if (small_unroll_fits(h, 0)) ti = 0;
    else return -1;
    const int T = ti == 2 ? 4 : ti + 1, nU = (B + T - 1) / T;
    const int ls = std::max(1, std::min(ti == 2 ? MZ_MULTI_MAX : MZ_MULTI_UNROLL, h->n_cu / nU));
    *Ls = std::min(ls, L);
    return ti;
}
static int ensure_multi(mz_handle* h, int B, int L) {
    if (h->kind == 1 && !h->d_tbank_w) {
        // the ResNet image bank: 2 halves of MZ_MULTI_MAX copies of the MFMA image (positions no parameter
        // maps to as in the engine's image), the flat bank (θ of each step)
        const size_t nw = h->packed_w_n, nb = std::max<size_t>(h->packed_b_n, 1);
        MZ_TRY(h, dalloc(h, &h->d_tbank_w, (size_t)2 * MZ_MULTI_MAX * nw));
        MZ_TRY(h, dalloc(h, &h->d_tbank_b, (size_t)2 * MZ_MULTI_MAX * nb));
        MZ_TRY(h, dalloc(h, &h->d_fbank, (size_t)2 * MZ_MULTI_MAX * fbank_stride(h)));
        for (int i = 0; i < 2 * MZ_MULTI_MAX; ++i) {
            MZ_TRY(h, hipMemcpy(h->d_tbank_w + (size_t)i * nw, h->d_Wp, nw * 4, hipMemcpyDeviceToDevice));
            if (h->packed_b_n)
                MZ_TRY(h, hipMemcpy(h->d_tbank_b + (size_t)i * nb, h->d_Bp, nb * 4, hipMemcpyDeviceToDevice));
        }
    }
    if (h->kind != 1 && !h->d_bank_w) {
        // two halves of MZ_MULTI_MAX images: sub-chunk k writes half k mod 2 (a chain launch
        // never writes the images an unroll launch still in flight reads)
        MZ_TRY(h, dalloc(h, &h->d_bank_w, (size_t)2 * MZ_MULTI_MAX * h->sm_w_n));
        MZ_TRY(h, dalloc(h, &h->d_bank_b, (size_t)2 * MZ_MULTI_MAX * h->sm_b_n));
        // the positions no parameter maps to (zero chunks, unused rows) as in the
        // engine's images; every mapped position is rewritten by each chain launch
        for (int i = 0; i < 2 * MZ_MULTI_MAX; ++i) {
            MZ_TRY(h, hipMemcpy(h->d_bank_w + (size_t)i * h->sm_w_n, h->d_sm_w, h->sm_w_n * 4, hipMemcpyDeviceToDevice));
            MZ_TRY(h, hipMemcpy(h->d_bank_b + (size_t)i * h->sm_b_n, h->d_sm_bias, h->sm_b_n * 4,
                                hipMemcpyDeviceToDevice));
        }
    }
    // per-step scratch (batches, read-outs, loss terms, partials) is a ring of at most 2·MZ_MULTI_MAX
    // steps (slot = step mod R, R = the largest multiple of the chain length Lc <= 2·MZ_MULTI_MAX, so a
    // chain launch's steps and an unroll launch's steps are contiguous, and a chain launch that reuses
    // an earlier launch's slots runs after its unrolls in stream order); on growth the old arrays are
    // freed after the device drains
    L = std::min(L, 2 * MZ_MULTI_MAX);
    if (B <= h->ml_cap && L <= h->ml_cap_L) return 0;
    const int cb = std::max(B, h->ml_cap), cl = std::max(L, h->ml_cap_L);
    if (h->ml_cap) {
        MZ_TRY(h, hipDeviceSynchronize());
        void* olds[] = {h->d_ml_obs, h->d_ml_act, h->d_ml_tv, h->d_ml_tr, h->d_ml_tp, h->d_ml_gs, h->d_ml_index,
                        h->d_ml_pv, h->d_ml_pp, h->d_ml_pr, h->d_ml_terms, h->d_ml_part, h->d_ml_cnt, h->d_ml_out,
                        h->d_ml_hs, h->d_ml_ts, h->d_ml_prog, h->d_ml_dsb};
        for (void* o : olds) if (o && dfree(h, o)) return -1;
        h->d_ml_hs = h->d_ml_ts = h->d_ml_dsb = nullptr;
        h->d_ml_prog = nullptr;
    }
    const size_t K1 = (size_t)h->conf.num_unroll_steps + 1, A = (size_t)h->A, n = (size_t)cl * cb;
    MZ_TRY(h, dalloc(h, &h->d_ml_obs, n * h->obs_feat));
    MZ_TRY(h, dalloc(h, &h->d_ml_act, n * K1)); MZ_TRY(h, dalloc(h, &h->d_ml_tv, n * K1));
    MZ_TRY(h, dalloc(h, &h->d_ml_tr, n * K1)); MZ_TRY(h, dalloc(h, &h->d_ml_tp, n * K1 * A));
    MZ_TRY(h, dalloc(h, &h->d_ml_gs, n)); MZ_TRY(h, dalloc(h, &h->d_ml_index, 2 * n));
    MZ_TRY(h, dalloc(h, &h->d_ml_pv, n * K1)); MZ_TRY(h, dalloc(h, &h->d_ml_pp, n * K1 * A));
    MZ_TRY(h, dalloc(h, &h->d_ml_pr, n * K1)); MZ_TRY(h, dalloc(h, &h->d_ml_terms, 2 * n * K1));
    MZ_TRY(h, dalloc(h, &h->d_ml_part, (size_t)cl * 3 * MZ_L2_BLOCKS));
    MZ_TRY(h, dalloc(h, &h->d_ml_cnt, (size_t)cl * MZ_MULTI_CNT_STRIDE));
    MZ_TRY(h, hipMemset(h->d_ml_cnt, 0, (size_t)cl * MZ_MULTI_CNT_STRIDE * 4));
    MZ_TRY(h, dalloc(h, &h->d_ml_out, (size_t)cl * 8));
    if (h->kind == 1) {
        const size_t KH = (size_t)std::max(h->conf.num_unroll_steps, 1);
        MZ_TRY(h, dalloc(h, &h->d_ml_hs, n * KH * h->H)); MZ_TRY(h, dalloc(h, &h->d_ml_ts, n * KH * h->H));
        MZ_TRY(h, dalloc(h, &h->d_ml_prog, n));
        MZ_TRY(h, hipMemset(h->d_ml_prog, 0, n * sizeof(unsigned long long)));
        h->ml_prog_epoch = 0;
        if (h->ds) MZ_TRY(h, dalloc(h, &h->d_ml_dsb, n * h->rin_feat));
    }
    h->ml_cap = cb; h->ml_cap_L = cl;
    return 0;
}

// ResNet nets (ref_semantics, no PER): per sub-chunk of Ls steps, the chain launch (ADAM
// iterations into the MFMA image bank and the flat bank, Σθ² per step, the Ls batches), the
// downsampler over the Ls·B observations (Atari), the unroll launch(es) of rlearner_grad's
// form with the steps on gridDim.z (the fused form: step-major chain blocks, then the items;
// RUnrollParams.ms) and one loss launch of Ls·nlb blocks
static bool rmulti_ok(const mz_handle* h) {
    return h->kind == 1 && h->learn_mode == MZ_LEARN_REF_SEMANTICS && !h->conf.PER;
}
// mz_learn_chain's helper workgroups (ChainParams::nh) for the nets with more parameters than one pass
// of the slices.  Measured against none (tools/gpu_r06t.sh): FC 32.1 -> 24.8 us per
// 32-step chain, ResNet configs[2] 63.3 -> 44.2 us.  Returns the helper count.
static int chain_helpers(mz_handle* h, ChainParams& C) {
    const size_t stride = (size_t)MZ_L2_BLOCKS * MZ_THREADS;
    int nht = 0;
    size_t hx_n = 0;
    for (int n = 0; n < 3; ++n) {
        const size_t c = h->nparams[n];
        C.nh[n] = c > stride ? (int)((c - stride + MZ_THREADS - 1) / MZ_THREADS) : 0;
        C.hoff[n] = hx_n;
        hx_n += c > stride ? c : 0;
        nht += C.nh[n];
    }
    if (!nht) return 0;
    if (!h->d_chcnt) {
        MZ_TRY(h, dalloc(h, &h->d_chx, (size_t)MZ_MULTI_MAX * hx_n));
        MZ_TRY(h, dalloc(h, &h->d_chcnt, (size_t)3 * MZ_L2_BLOCKS));
        MZ_TRY(h, hipMemset(h->d_chcnt, 0, (size_t)3 * MZ_L2_BLOCKS * sizeof(unsigned long long)));
    }
    C.hx = h->d_chx; C.hx_n = hx_n; C.hcnt = h->d_chcnt;
    return nht;
}
static void set_caps(ChainParams& C, const MultiCap* cap, int64_t first, int nc) {
    for (int j = 0; j < 2; ++j) {
        const bool in = cap && cap->t[j] >= first && cap->t[j] < first + nc;
        C.cap_i[j] = in ? (int)(cap->t[j] - first) : -1;
        C.cap_dst[j] = in ? cap->dst[j] : nullptr;
    }
    if (C.cap_i[0] >= 0 && cap->img0) {
        C.cap_img[0] = cap->img0->Wp; C.cap_img[1] = cap->img0->Bp;
        C.cap_img[2] = cap->img0->smw; C.cap_img[3] = cap->img0->smb;
        if (cap->imaged0) *cap->imaged0 = true;
    }
}
// the per-step strides of the ring arrays (ensure_multi): observations, (K+1)-rows, policies
struct MultiStrides { int B; size_t s_obs, s_k1, s_tp; };
// q = get_batch of learner step `step` into ring slot `slot` (Q: slot 0), written in place
static void rs_at(RpSampleParams& q, const RpSampleParams& Q, uint32_t step, int slot, const MultiStrides& S) {
    q = Q;
    q.step = step;
    q.obs += slot * S.s_obs; q.actions += slot * S.s_k1; q.tv += slot * S.s_k1; q.tr += slot * S.s_k1;
    q.tpol += slot * S.s_tp; q.gscale += (size_t)slot * S.B; q.index += (size_t)slot * 2 * S.B;
}

// The multi-step driver: chain launches of up to MZ_MULTI_MAX steps (the ADAM iterations into bank
// half k mod 2, the steps' batches with chain_sample), each followed by its steps' sub-chunks of up to
// Ls steps, body(c0, j0, n, ir, Qk, C): the unrolls and losses of the n steps from c0 + j0 on (ring
// slots ir .., batches Qk, parameters at + j0 in C's banks).  Q: get_batch into ring slot 0.
template <class Body>
static int multi_drive(mz_handle* h, uint32_t step0, int L, int Ls, const double* eta, float* theta_dev,
                       hipStream_t st, const MultiCap* cap, const RpSampleParams& Q, const MultiStrides& S,
                       bool chain_sample, Body body) {
    const int B = S.B;
    const size_t nw = h->packed_w_n, nb = std::max<size_t>(h->packed_b_n, 1);
    double p1 = h->bp1, p2 = h->bp2;
    const int Lc = std::min(L, std::max(Ls, MZ_MULTI_MAX / Ls * Ls));
    const int R = 2 * MZ_MULTI_MAX / Lc * Lc;       // the per-step scratch ring (ensure_multi)
    for (int k = 0, c0 = 0; c0 < L; ++k, c0 += Lc) {
        const int nc = std::min(Lc, L - c0), half = k & 1, cr = c0 % R;
        // 1. the ADAM chain θ_{t+c0} .. θ_{t+c0+nc} into bank half k mod 2
        ChainParams C;
        std::memset(&C, 0, sizeof(C));
        C.L = nc; C.flat = h->d_flat; C.M = h->d_m; C.V = h->d_v; C.netoff = h->d_netoff;
        C.inv_tile = h->d_inv_tile; C.inv_small = h->d_inv_small;
        C.Wp = h->d_Wp; C.Bp = h->d_Bp; C.smw = h->d_sm_w; C.smb = h->d_sm_bias;
        if (h->kind == 1) {                         // the MFMA image bank and the flat bank
            C.tbank_w = h->d_tbank_w + (size_t)half * MZ_MULTI_MAX * nw;
            C.tbank_b = h->d_tbank_b + (size_t)half * MZ_MULTI_MAX * nb;
            C.tws = nw; C.tbs = nb;
            C.fbank = h->d_fbank + (size_t)half * MZ_MULTI_MAX * fbank_stride(h);
            C.fstride = fbank_stride(h);
        } else {                                    // the small-kernel image bank
            C.bank_w = h->d_bank_w + (size_t)half * MZ_MULTI_MAX * h->sm_w_n;
            C.bank_b = h->d_bank_b + (size_t)half * MZ_MULTI_MAX * h->sm_b_n;
            C.bws = h->sm_w_n; C.bbs = h->sm_b_n;
        }
        C.theta = theta_dev ? theta_dev + (size_t)c0 * h->nflat : nullptr;
        C.nflat = h->nflat; C.part = h->d_ml_part + (size_t)cr * 3 * MZ_L2_BLOCKS;
        set_caps(C, cap, (int64_t)step0 + c0, nc);
        for (int i = 0; i < nc; ++i) {              // adam_advance's products, step by step
            C.bp1[i] = p1; C.bp2[i] = p2; C.eta[i] = eta[c0 + i];
            p1 = p1 * 0.9; p2 = p2 * 0.999;
        }
        C.B = B; rs_at(C.q, Q, step0 + (uint32_t)c0, cr, S);    // this chunk's batches: steps step0 + c0 ..
        C.s_obs = S.s_obs; C.s_k1 = S.s_k1; C.s_tp = S.s_tp;
        const int nsb = chain_sample ? (nc * B + MZ_THREADS / 64 - 1) / (MZ_THREADS / 64) : 0;
        const int nht = chain_helpers(h, C);
        if (nht < 0) return -1;
        hipLaunchKernelGGL(mz_learn_chain, dim3(nht + 3 * MZ_L2_BLOCKS + nsb), dim3(MZ_THREADS), 0, st, C);
        MZ_TRY(h, hipGetLastError());
        // 2. the sub-chunks: steps step0 + c0 + j0 ..
        for (int j0 = 0; j0 < nc; j0 += Ls) {
            const int n = std::min(Ls, nc - j0), ir = (c0 + j0) % R;
            RpSampleParams Qk;
            rs_at(Qk, Q, step0 + (uint32_t)(c0 + j0), ir, S);
            if (body(c0, j0, n, ir, Qk, C)) return -1;
        }
    }
    for (int i = 0; i < L; ++i) adam_advance(h);
    h->ml_last_B = B; h->ml_last_L = L; h->ml_last_R = R;
    return 0;
}

// ResNet nets (ref_semantics, no PER): per sub-chunk of Ls steps, the downsampler over the Ls·B
// observations (Atari), the unroll launch(es) with the steps on gridDim.z (the fused form: step-major
// chain blocks, then the items; RUnrollParams.ms) and one loss launch of Ls·nlb blocks (Σθ² per step
// from the chain launch)
static int rlearner_multi(mz_handle* h, int32_t B, uint32_t step0, int32_t L, const double* eta, float* losses_dev,
                          float* theta_dev, hipStream_t st, float* out_last, const MultiCap* cap) {
    RpSampleParams Q;
    mz_batch b;
    if (rs_params(h, B, step0, st, &Q, &b, true)) return -1;
    if (ensure_batch(h, B) || ensure_multi(h, B, L)) return -1;
    const int Ls = std::min(L, MZ_MULTI_UNROLL);
    const int K = h->conf.num_unroll_steps, KH = std::max(K, 1), A = h->A;
    const size_t K1 = (size_t)K + 1;
    const MultiStrides S = {B, (size_t)B * h->obs_feat, (size_t)B * K1, (size_t)B * K1 * A};
    const size_t nw = h->packed_w_n;
    Q.obs = h->d_ml_obs; Q.actions = h->d_ml_act; Q.tv = h->d_ml_tv; Q.tr = h->d_ml_tr; Q.tpol = h->d_ml_tp;
    Q.gscale = h->d_ml_gs; Q.index = h->d_ml_index;
    RUnrollParams U;
    runroll_params(h, B, U);
    U.ms_wimg = nw; U.ms_flat = fbank_stride(h); U.ms_obs = (size_t)B * (h->ds ? h->rin_feat : h->obs_feat);
    U.ms_k1 = S.s_k1; U.ms_tp = S.s_tp; U.ms_hs = (size_t)B * KH * h->H;
    const int gw = A > 16 ? 32 : 16;
    const int nlb = (B * (int)K1 + MZ_THREADS / gw - 1) / (MZ_THREADS / gw);
    auto body = [&](int c0, int j0, int n, int ir, const RpSampleParams& Qk, const ChainParams& C) -> int {
        const int i0 = c0 + j0;
        // representation input (Atari: the downsampler with step z's parameters), the unrolls
        U.Wimg = C.tbank_w + (size_t)j0 * nw; U.flat = C.fbank + (size_t)j0 * fbank_stride(h);
        U.obs = Qk.obs; U.actions = Qk.actions;
        if (h->ds) {
            float* y = h->d_ml_dsb + (size_t)ir * B * h->rin_feat;
            if (ds_launch(h, Qk.obs, y, n * B, st, C.fbank + (size_t)j0 * fbank_stride(h), B)) return -1;
            U.obs = y;
        }
        U.pv = h->d_ml_pv + ir * S.s_k1; U.pp = h->d_ml_pp + ir * S.s_tp; U.pr = h->d_ml_pr + ir * S.s_k1;
        U.hs = h->d_ml_hs + (size_t)ir * U.ms_hs; U.ts = h->d_ml_ts + (size_t)ir * U.ms_hs;
        if (runroll_launch(h, U, n, st, h->d_ml_prog + (size_t)ir * B, &h->ml_prog_epoch)) return -1;
        // the loss terms and per-step folds (Σθ² from the chain launch)
        LossMultiParams M;
        std::memset(&M, 0, sizeof(M));
        M.B = B; M.K = K; M.A = A; M.v_act = MZ_ACT_IDENTITY; M.r_act = MZ_ACT_IDENTITY; M.nlb = nlb; M.L = n;
        M.s_k1 = S.s_k1; M.s_tp = S.s_tp; M.pv = U.pv; M.pp = U.pp; M.pr = U.pr;
        M.tv = Qk.tv; M.tp = Qk.tpol; M.gs = Qk.gscale;
        M.terms = h->d_ml_terms + 2 * ir * S.s_k1; M.part = h->d_ml_part + (size_t)ir * 3 * MZ_L2_BLOCKS;
        M.counter = h->d_ml_cnt + (size_t)ir * MZ_MULTI_CNT_STRIDE;
        M.out = losses_dev ? losses_dev + 8 * i0 : h->d_ml_out + 8 * ir;
        M.out_last = i0 + n == L ? out_last : nullptr;
        hipLaunchKernelGGL(gw == 32 ? mz_learner_loss_multi32 : mz_learner_loss_multi, dim3(nlb, n), dim3(MZ_THREADS),
                           0, st, M);
        MZ_TRY(h, hipGetLastError());
        return 0;
    };
    if (multi_drive(h, step0, L, Ls, eta, theta_dev, st, cap, Q, S, true, body)) return -1;
    h->last_lvariant = std::string("mz_learn_chain+") + (h->ds ? "mz_downsample_kernel+" : "") + h->last_lvariant +
                       "+mz_learner_loss_multi";
    return 0;
}

// out_last: also (instead of losses[L-1]) the last step's losses there (mz_train_run)
int mz::learner_multi(mz_handle* h, int32_t B, uint32_t step0, int32_t L, const double* eta, float* losses_dev,
                      float* theta_dev, hipStream_t st, float* out_last, const MultiCap* cap) {
    MZ_TRY(h, hipSetDevice(h->device));
    if (rmulti_ok(h)) return rlearner_multi(h, B, step0, L, eta, losses_dev, theta_dev, st, out_last, cap);
    int Ls = 0;
    const int ti = multi_ok(h) ? multi_plan(h, B, L, &Ls) : -1;
    if (ti < 0) {
        // the same L steps one launch each (ResNet, the corrected mode, PER, wide nets)
        for (int i = 0; i < L; ++i) {
            float* lo = losses_dev ? losses_dev + 8 * i : (i == L - 1 ? out_last : nullptr);
            if (learner_sampled(h, B, step0 + (uint32_t)i, nullptr, lo, st, true, eta[i])) return -1;
            if (i == L - 1 && out_last && losses_dev)
                MZ_TRY(h, hipMemcpyAsync(out_last, lo, 8 * 4, hipMemcpyDeviceToDevice, st));
            if (theta_dev)
                MZ_TRY(h, hipMemcpyAsync(theta_dev + (size_t)i * h->nflat, h->d_flat, h->nflat * 4,
                                         hipMemcpyDeviceToDevice, st));
            for (int j = 0; j < 2; ++j)
                if (cap && cap->t[j] == (int64_t)step0 + i)
                    MZ_TRY(h, hipMemcpyAsync(cap->dst[j], h->d_flat, h->nflat * 4, hipMemcpyDeviceToDevice, st));
        }
        h->ml_last_L = 0;                           // (no multi-step read-outs: mz_debug_unroll_step refuses)
        return 0;
    }
    // FC nets on the small kernel: per sub-chunk, one launch of the n unrolls (with their get_batch),
    // loss terms and per-step folds, Ls steps keeping one workgroup per CU
    RpSampleParams Q;
    mz_batch b;
    if (rs_params(h, B, step0, st, &Q, &b, true)) return -1;   // (the shard; set 0 is not touched)
    if (ensure_batch(h, B) || ensure_multi(h, B, L)) return -1;
    const size_t K1 = (size_t)h->conf.num_unroll_steps + 1, A = (size_t)h->A;
    const MultiStrides S = {B, (size_t)B * h->obs_feat, (size_t)B * K1, (size_t)B * K1 * A};
    Q.obs = h->d_ml_obs; Q.actions = h->d_ml_act; Q.tv = h->d_ml_tv; Q.tr = h->d_ml_tr; Q.tpol = h->d_ml_tp;
    Q.gscale = h->d_ml_gs; Q.index = h->d_ml_index;
    SmallUnrollParams U;
    if (small_unroll_params(h, &b, ti, nullptr, &U)) return -1;
    const int T = ti == 2 ? 4 : ti + 1, nU = (B + T - 1) / T;
    auto body = [&](int c0, int j0, int n, int ir, const RpSampleParams& Qk, const ChainParams& C) -> int {
        const int i0 = c0 + j0;
        LearnMultiParams M;
        std::memset(&M, 0, sizeof(M));
        M.L = n; M.nU = nU;
        M.xcd = n > 1;
        M.bank_w = C.bank_w + (size_t)j0 * h->sm_w_n; M.bank_b = C.bank_b + (size_t)j0 * h->sm_b_n;
        M.bws = h->sm_w_n; M.bbs = h->sm_b_n;
        M.s_obs = S.s_obs; M.s_k1 = S.s_k1; M.s_tp = S.s_tp;
        M.obs = Qk.obs; M.act = Qk.actions; M.tv = Qk.tv; M.tp = Qk.tpol; M.gs = Qk.gscale;
        M.pv = h->d_ml_pv + ir * S.s_k1; M.pp = h->d_ml_pp + ir * S.s_tp; M.pr = h->d_ml_pr + ir * S.s_k1;
        M.terms = h->d_ml_terms + 2 * ir * S.s_k1;
        M.part = h->d_ml_part + (size_t)ir * 3 * MZ_L2_BLOCKS;
        M.counter = h->d_ml_cnt + (size_t)ir * MZ_MULTI_CNT_STRIDE;
        M.out = losses_dev ? losses_dev + 8 * i0 : h->d_ml_out + 8 * ir;
        M.out_last = i0 + n == L ? out_last : nullptr;
        M.sample = Q.sym_n == 0;                    // (each step's get_batch in its unroll workgroups; with the
                                                    // board symmetry on, in the chain launch: DESIGN §23)
        M.q = Qk;
        const int grid = M.xcd ? 8 * ((n + 7) / 8) * nU : n * nU;
        void* args[] = {&U, &M};
        hipEvent_t e0 = nullptr, e1 = nullptr; // mz_debug_enable flag 4: the unroll launch's duration
        if (h->time_unroll) {
            if (timing_events(h, &e0, &e1)) return -1;
            MZ_TRY(h, hipEventRecord(e0, st));
        }
        MZ_TRY(h, hipLaunchKernel(small_kernel(h, SMK_MULTI, ti), dim3(grid), dim3(SM_THREADS), args,
                                  unroll_small_lds(h, ti), st));
        if (e1) MZ_TRY(h, hipEventRecord(e1, st));
        return 0;
    };
    if (multi_drive(h, step0, L, Ls, eta, theta_dev, st, cap, Q, S, Q.sym_n != 0, body)) return -1;
    h->last_lvariant = ti == 0 ? "mz_learn_chain+mz_learn_multi1"
                     : ti == 1 ? "mz_learn_chain+mz_learn_multi2" : "mz_learn_chain+mz_learn_multi4";
    return 0;
}

int mz_learner_train_multi_dev(mz_handle* h, int32_t B, uint32_t step0, int32_t L, const double* eta,
                               float* losses_dev, float* theta_dev, void* stream) {
    if (!h) return -2;
    if (L < 1 || L > MZ_MULTI_LMAX) return fail(h, "L must be in 1 .. 256");
    if (!eta) return fail(h, "eta: one learning rate per step");
    if (B < 1) return fail(h, "batch_size must be >= 1");
    return learner_multi(h, B, step0, L, eta, losses_dev, theta_dev, stream_of(h, stream));
}

int mz_debug_unroll_step(mz_handle* h, int i, int B, float* values, float* policies, float* rewards) {
    if (!h) return -2;
    if (i < 0 || i >= h->ml_last_L || i < h->ml_last_L - h->ml_last_R || B < 0 || B > h->ml_last_B)
        return fail(h, "no such step / batch in the last mz_learner_train_multi_dev");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const size_t K1 = (size_t)h->conf.num_unroll_steps + 1, A = (size_t)h->A, s = (size_t)h->ml_last_B * K1;
    const size_t n = (size_t)B * K1;
    const size_t ir = (size_t)(i % h->ml_last_R);   // the ring slot of step i (ensure_multi)
    if (values) MZ_TRY(h, hipMemcpy(values, h->d_ml_pv + ir * s, n * 4, hipMemcpyDeviceToHost));
    if (policies) MZ_TRY(h, hipMemcpy(policies, h->d_ml_pp + ir * s * A, n * A * 4, hipMemcpyDeviceToHost));
    if (rewards) MZ_TRY(h, hipMemcpy(rewards, h->d_ml_pr + ir * s, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mz_replay_get_game(mz_handle* h, int32_t i, int32_t* T, uint8_t* obs, int32_t* actions, float* rewards,
                       int32_t* to_play, float* child_visits, float* root_values) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c[3];
    MZ_TRY(h, hipMemcpy(c, h->d_sp_counters, sizeof(c), hipMemcpyDeviceToHost));
    const long long held = std::min<long long>(c[0], h->sp_cap);
    if (i < 0 || i >= held) return fail(h, "game index out of range");
    const long long num = c[0] - held + 1 + i;
    const int slot = (int)((num - 1) % h->sp_cap);
    const size_t base = (size_t)slot * h->sp_T, A = (size_t)h->A;
    const SpHist& r = h->sp_ring;
    int32_t len = 0;
    MZ_TRY(h, hipMemcpy(&len, r.len + slot, 4, hipMemcpyDeviceToHost));
    if (T) *T = len;
    if (obs) MZ_TRY(h, hipMemcpy(obs, r.obs + base * h->sp_osz, (size_t)len * h->sp_osz, hipMemcpyDeviceToHost));
    if (actions) MZ_TRY(h, hipMemcpy(actions, r.act + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (rewards) MZ_TRY(h, hipMemcpy(rewards, r.rew + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (to_play) MZ_TRY(h, hipMemcpy(to_play, r.tp + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    if (child_visits) MZ_TRY(h, hipMemcpy(child_visits, r.cv + base * A, (size_t)len * A * 4, hipMemcpyDeviceToHost));
    if (root_values) MZ_TRY(h, hipMemcpy(root_values, r.rv + base, (size_t)len * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- Reanalyse (mz_reanalyse.hip): reanalysed_predicted_root_values on the shard
static const int kReanChunk = 4096;     // ResNet engines: positions per gather / nets / scatter round

// what every reanalyse launch reads: the shard, its geometry and the counters
ReanParams mz::rean_params(mz_handle* h) {
    ReanParams Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.T = h->sp_T; Q.osz = h->sp_osz; Q.P = h->plane; Q.F = h->obs_feat; Q.stacked = h->conf.stacked_observations;
    Q.cap = h->sp_cap; Q.ring = h->sp_ring; Q.counters = h->d_sp_counters;
    return Q;
}

static int rean_values(mz_handle* h, ReanParams& Q, int npos, hipStream_t st);

int mz_replay_reanalyse(mz_handle* h, int32_t first, int32_t count, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->sp_frames > 0 || h->ds) return fail(h, "reanalyse: frame-stack env not built");
    if (first < 0) return fail(h, "reanalyse: first must be >= 0");
    if ((long long)h->sp_cap * h->sp_T > 0x7fffffffLL) return fail(h, "reanalyse: shard too large");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    // how many games are held is only known on the device: the grid covers the
    // selection clipped to the capacity, the kernels clip it to the held range
    const int gmax = count < 0 ? h->sp_cap - first : std::min<int>(count, h->sp_cap - first);
    ++h->pf_epoch;                                  // a batch drawn ahead has the old targets
    if (gmax <= 0) return 0;
    ReanParams Q = rean_params(h);
    Q.first = first; Q.count = count;
    return rean_values(h, Q, gmax * h->sp_T, st);
}

// the value pass over rows [0, npos) of Q's flattened grid or row list
static int rean_values(mz_handle* h, ReanParams& Q, int npos, hipStream_t st) {
    if (h->kind != 1) {
        Q.plan_root = h->d_plan[3]; Q.Wp = h->d_Wp; Q.Bp = h->d_Bp;
        Q.x_rep = h->lay.x_rep; Q.v_out = h->lay.v_out; Q.v_act = h->lay.v_act; Q.lds_total = h->lay.total;
        const size_t lds = ((size_t)h->lay.total + (size_t)MZ_TILE * h->obs_feat) * 4;
        if (lds > kLdsMax) return fail(h, "reanalyse: the tile's activations and observations exceed the LDS");
        if (lds > h->rean_lds) {
            MZ_TRY(h, hipFuncSetAttribute((const void*)mz_reanalyse_fc, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
            h->rean_lds = lds;
        }
        const int ntiles = (npos + MZ_TILE - 1) / MZ_TILE;
        void* args[] = {&Q};
        MZ_TRY(h, hipLaunchKernel((const void*)mz_reanalyse_fc, dim3(std::min(ntiles, 4 * h->n_cu)), dim3(MZ_THREADS),
                                  args, lds, st));
        return 0;
    }
    const RPlan& Rr = h->rplan[MZ_NET_REPR];
    const RPlan& Rp = h->rplan[MZ_NET_PRED];
    if (Rr.in_feat != h->obs_feat || Rp.in_feat != Rr.out0_n || Rp.out0_n != 1)
        return fail(h, "reanalyse: unexpected ResNet plan shapes");
    const int chunk = std::min(npos, kReanChunk);
    if (chunk > h->rn_cap) {
        MZ_TRY(h, spalloc(h, &h->d_rn_x, (size_t)chunk * h->obs_feat, false));
        MZ_TRY(h, spalloc(h, &h->d_rn_h, (size_t)chunk * Rr.out0_n, false));
        MZ_TRY(h, spalloc(h, &h->d_rn_v, (size_t)chunk * Rp.out0_n, false));
        MZ_TRY(h, spalloc(h, &h->d_rn_p, (size_t)chunk * std::max(Rp.out1_n, 1), false));
        h->rn_cap = chunk;
    }
    for (int p0 = 0; p0 < npos; p0 += chunk) {
        const int pn = std::min(chunk, npos - p0);
        Q.p0 = p0; Q.pn = pn; Q.stage_x = h->d_rn_x; Q.stage_v = h->d_rn_v;
        hipLaunchKernelGGL(mz_reanalyse_gather, dim3((pn + 3) / 4), dim3(256), 0, st, Q);
        MZ_TRY(h, hipGetLastError());
        for (int net = MZ_NET_REPR; net <= MZ_NET_PRED; ++net) {
            RNetParams N;
            N.ng = h->rn_ng; N.W = h->rconf.observation_shape[0]; N.H = h->rconf.observation_shape[1];
            N.P = N.W * N.H; N.n_items = pn; N.softmax1 = net == MZ_NET_PRED; N.bn_s = h->bn_s;
            N.plan = h->d_rplan + net; N.Wimg = h->d_Wp; N.flat = h->d_flat;
            N.x = net == MZ_NET_REPR ? h->d_rn_x : h->d_rn_h;
            N.out0 = net == MZ_NET_REPR ? h->d_rn_h : h->d_rn_v;
            N.out1 = h->d_rn_p;
            void* args[] = {&N};
            MZ_TRY(h, hipLaunchKernel((const void*)mz_rnet_forward_kernel, dim3((pn + N.ng - 1) / N.ng),
                                      dim3(RN_THREADS), args, h->rn_lds[net], st));
        }
        hipLaunchKernelGGL(mz_reanalyse_scatter, dim3((pn + 255) / 256), dim3(256), 0, st, Q);
        MZ_TRY(h, hipGetLastError());
    }
    return 0;
}

int mz_replay_clear_reanalysed(mz_handle* h, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    ++h->pf_epoch;
    hipLaunchKernelGGL(mz_reanalyse_clear, dim3((h->sp_cap + 255) / 256), dim3(256), 0, st, h->sp_ring.rean, h->sp_cap);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_replay_reanalysed_count(mz_handle* h, int64_t* n) {
    if (!h || !n) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c = 0;
    MZ_TRY(h, hipMemcpy(&c, h->d_sp_counters + 3, sizeof(c), hipMemcpyDeviceToHost));
    *n = c;
    return 0;
}

int mz_replay_get_reanalysed(mz_handle* h, int32_t i, int32_t* is_set, float* values) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long played = 0;
    MZ_TRY(h, hipMemcpy(&played, h->d_sp_counters, sizeof(played), hipMemcpyDeviceToHost));
    const long long held = std::min<long long>(played, h->sp_cap);
    if (i < 0 || i >= held) return fail(h, "game index out of range");
    const int slot = (int)((played - held + i) % h->sp_cap);
    int32_t set = 0, len = 0;
    MZ_TRY(h, hipMemcpy(&set, h->sp_ring.rean + slot, 4, hipMemcpyDeviceToHost));
    MZ_TRY(h, hipMemcpy(&len, h->sp_ring.len + slot, 4, hipMemcpyDeviceToHost));
    set &= MZ_REAN_VALUES;
    if (is_set) *is_set = set != 0;
    if (values && set)
        MZ_TRY(h, hipMemcpy(values, h->sp_ring.rrv + (size_t)slot * h->sp_T, (size_t)len * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- Reanalyse by search: gather -> the batched search -> scatter per max_games rows
// the search's io and the shard's reanalysed child_visits, allocated by the first call that has work,
// and the search half of the parameters
int mz::rean_search_io(mz_handle* h, ReanParams& Q) {
    const size_t Gc = (size_t)h->max_games, A = (size_t)h->A;
    if (!h->d_rq_obs) {
        MZ_TRY(h, spalloc(h, &h->sp_ring.rcv, (size_t)h->sp_cap * h->sp_T * A, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_legal, Gc * A, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_tp, Gc, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_cv, Gc * A, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_rv, Gc, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_act, Gc, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_state, Gc, false));
        MZ_TRY(h, spalloc(h, &h->d_rq_obs, Gc * h->obs_feat, false));
    }
    Q.ring = h->sp_ring;
    Q.env = h->sp_env; Q.W = h->conf.observation_shape[0]; Q.H = h->conf.observation_shape[1]; Q.A = h->A;
    Q.players = h->conf.players;
    Q.stage_x = h->d_rq_obs; Q.stage_legal = h->d_rq_legal; Q.stage_tp = h->d_rq_tp; Q.stage_state = h->d_rq_state;
    Q.stage_cv = h->d_rq_cv; Q.stage_rv = h->d_rq_rv;
    return 0;
}

int mz_replay_reanalyse_search(mz_handle* h, int32_t first, int32_t count, int exploration, uint32_t rng_step,
                               uint32_t game_offset, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->sp_frames > 0 || h->ds) return fail(h, "reanalyse: frame-stack env not built");
    if (first < 0) return fail(h, "reanalyse: first must be >= 0");
    if ((long long)h->sp_cap * h->sp_T > 0x7fffffffLL) return fail(h, "reanalyse: shard too large");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    // as mz_replay_reanalyse: the rows cover the selection clipped to the capacity, the kernels
    // clip it to the held range
    const int gmax = count < 0 ? h->sp_cap - first : std::min<int>(count, h->sp_cap - first);
    ++h->pf_epoch;                                  // a batch drawn ahead has the old targets
    if (gmax <= 0) return 0;
    const size_t Gc = (size_t)h->max_games, A = (size_t)h->A;
    ReanParams Q = rean_params(h);
    Q.first = first; Q.count = count;
    if (rean_search_io(h, Q)) return -1;
    const int npos = gmax * h->sp_T;
    for (int p0 = 0; p0 < npos; p0 += (int)Gc) {
        const int pn = std::min<int>((int)Gc, npos - p0);
        Q.p0 = p0; Q.pn = pn;
        hipLaunchKernelGGL(mz_reanalyse_sgather, dim3((pn + 3) / 4), dim3(256), 0, st, Q);
        MZ_TRY(h, hipGetLastError());
        // row i is game i of this batch: its Philox id game_offset + p0 + i depends on (selection, position) only
        int rc = search_dev(h, pn, h->d_rq_obs, h->d_rq_legal, h->d_rq_tp, exploration, rng_step,
                            game_offset + (uint32_t)p0, 0.0f, h->d_rq_cv, h->d_rq_rv, h->d_rq_act, st, nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(mz_reanalyse_sscatter, dim3((pn * (int)A + 255) / 256), dim3(256), 0, st, Q);
        MZ_TRY(h, hipGetLastError());
    }
    return 0;
}

int mz_replay_get_reanalysed_policies(mz_handle* h, int32_t i, int32_t* is_set, float* child_visits) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long played = 0;
    MZ_TRY(h, hipMemcpy(&played, h->d_sp_counters, sizeof(played), hipMemcpyDeviceToHost));
    const long long held = std::min<long long>(played, h->sp_cap);
    if (i < 0 || i >= held) return fail(h, "game index out of range");
    const int slot = (int)((played - held + i) % h->sp_cap);
    int32_t set = 0, len = 0;
    MZ_TRY(h, hipMemcpy(&set, h->sp_ring.rean + slot, 4, hipMemcpyDeviceToHost));
    MZ_TRY(h, hipMemcpy(&len, h->sp_ring.len + slot, 4, hipMemcpyDeviceToHost));
    set = (set & MZ_REAN_POLICIES) && h->sp_ring.rcv;
    if (is_set) *is_set = set;
    if (child_visits && set)
        MZ_TRY(h, hipMemcpy(child_visits, h->sp_ring.rcv + (size_t)slot * h->sp_T * h->A, (size_t)len * h->A * 4,
                            hipMemcpyDeviceToHost));
    return 0;
}

// ---- The Reanalyse worker: one round of whole games from the device cursor, live rows only
// (mz_reanalyse_pack), through either pass above.  The host knows neither how many games are held
// nor which the round takes: every launch covers the round's capacity R and reads n_rows on the device.
int mz::rean_next_check(mz_handle* h, int mode) {
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->sp_frames > 0 || h->ds) return fail(h, "reanalyse: frame-stack env not built");
    if (mode != MZ_REAN_BY_VALUE && mode != MZ_REAN_BY_SEARCH)
        return fail(h, "reanalyse: mode must be MZ_REAN_BY_VALUE or MZ_REAN_BY_SEARCH");
    if ((long long)h->sp_cap * h->sp_T > 0x7fffffffLL) return fail(h, "reanalyse: shard too large");
    if (mode == MZ_REAN_BY_SEARCH && h->max_games < h->sp_T)
        return fail(h, "reanalyse: a search round of max_games rows cannot hold one game of max_moves + 1 positions");
    if (mode == MZ_REAN_BY_VALUE && kReanChunk < h->sp_T)
        return fail(h, "reanalyse: a value round cannot hold one game of max_moves + 1 positions");
    return 0;
}

int mz_replay_reanalyse_next(mz_handle* h, int mode, int exploration, uint32_t rng_step, uint32_t game_offset,
                             void* stream) {
    if (!h) return -2;
    if (rean_next_check(h, mode)) return -1;
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    const bool search = mode == MZ_REAN_BY_SEARCH;
    const int R = search ? h->max_games : kReanChunk;
    ++h->pf_epoch;                                  // a batch drawn ahead has the old targets
    if (R > h->rean_rows_cap) {
        MZ_TRY(h, spalloc(h, &h->d_rean_rows, (size_t)R * 2, false));
        h->rean_rows_cap = R;
    }
    ReanParams Q = rean_params(h);
    Q.R = R;
    if (search && rean_search_io(h, Q)) return -1;
    hipLaunchKernelGGL(mz_reanalyse_pack, dim3(1), dim3(64), 0, st, Q, h->d_rean_rows);
    MZ_TRY(h, hipGetLastError());
    Q.rows = h->d_rean_rows;
    // the shard cannot hold more live rows than cap * T: the launches need not cover more
    const int npos = (int)std::min<long long>(R, (long long)h->sp_cap * h->sp_T);
    if (!search) return rean_values(h, Q, npos, st);
    // one search of G = max_games games: row i has Philox id game_offset + i, rows >= n_rows are the dummy
    const int G = h->max_games;
    Q.p0 = 0; Q.pn = G;
    hipLaunchKernelGGL(mz_reanalyse_sgather, dim3((G + 3) / 4), dim3(256), 0, st, Q);
    MZ_TRY(h, hipGetLastError());
    int rc = search_dev(h, G, h->d_rq_obs, h->d_rq_legal, h->d_rq_tp, exploration, rng_step, game_offset, 0.0f,
                        h->d_rq_cv, h->d_rq_rv, h->d_rq_act, st, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(mz_reanalyse_sscatter, dim3((G * h->A + 255) / 256), dim3(256), 0, st, Q);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_replay_reanalyse_cursor(mz_handle* h, int64_t* next_game, int64_t* last_round3) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    long long c[4];
    MZ_TRY(h, hipMemcpy(c, h->d_sp_counters + MZ_REAN_CURSOR, sizeof(c), hipMemcpyDeviceToHost));
    if (next_game) *next_game = c[0];
    if (last_round3) for (int i = 0; i < 3; ++i) last_round3[i] = c[1 + i];
    return 0;
}

int mz_replay_reanalyse_seek(mz_handle* h, int64_t game_number, void* stream) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    MZ_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream_of(h, stream);
    hipLaunchKernelGGL(mz_reanalyse_seek, dim3(1), dim3(64), 0, st, h->d_sp_counters, (long long)game_number);
    MZ_TRY(h, hipGetLastError());
    return 0;
}

int mz_selfplay_slots(mz_handle* h, int32_t* history_len, uint8_t* board, int32_t* player) {
    if (!h) return -2;
    if (h->sp_env < 0) return fail(h, "mz_selfplay_init first");
    if (h->sp_reset_pending)       // the initial games are keyed by the first move's game_offset
        return fail(h, "the Atari-like env draws its initial games at the first mz_selfplay_move");
    MZ_TRY(h, hipSetDevice(h->device));
    MZ_SYNC(h);
    const size_t G = (size_t)h->sp_G;
    if (history_len) MZ_TRY(h, hipMemcpy(history_len, h->sp_hist.len, G * 4, hipMemcpyDeviceToHost));
    if (board) MZ_TRY(h, hipMemcpy(board, h->d_sp_board, G * h->sp_osz, hipMemcpyDeviceToHost));
    if (player) MZ_TRY(h, hipMemcpy(player, h->d_sp_player, G * 4, hipMemcpyDeviceToHost));
    return 0;
}

// a count summed over the ranks of the handle's RCCL communicator (exact below 2^24)
int mz::dp_sum_count(mz_handle* h, int64_t* v, hipStream_t st) {
    if (!h->d_dp_cnt) MZ_TRY(h, dalloc(h, &h->d_dp_cnt, 1));
    float f = (float)*v;
    MZ_TRY(h, hipMemcpyAsync(h->d_dp_cnt, &f, 4, hipMemcpyHostToDevice, st));
    const int rc = rccl().allreduce(h->d_dp_cnt, h->d_dp_cnt, 1, 7, 0, h->dp_comm, st);   // ncclFloat32, ncclSum
    if (rc != 0) return fail(h, std::string("ncclAllReduce: ") + (rccl().err ? rccl().err(rc) : "error"));
    MZ_TRY(h, hipMemcpyAsync(&f, h->d_dp_cnt, 4, hipMemcpyDeviceToHost, st));
    MZ_TRY(h, hipStreamSynchronize(st));
    *v = (int64_t)f;
    return 0;
}

int mz_sync(mz_handle* h) {
    if (!h) return -2;
    MZ_TRY(h, hipSetDevice(h->device));
    // every stream `_dev` work may have gone to (the device, or the narrowed pair of
    // mz_set_sync_stream), so a fault of work queued on a caller stream is reported here
    MZ_SYNC(h);
    return 0;
}
