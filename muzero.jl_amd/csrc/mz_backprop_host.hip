// mz_backprop_host.hip — host side of libmz: the corrected-gradient learner's plans and launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "mz_handle.h"
#include "mz_backprop_params.h"

using namespace mz;

// ---- corrected-gradient learner (MZ_LEARN_CORRECTED, FC nets; mz_backprop.hip)
// The unrolled graph of Learning.jl:347-370: representation(obs); K dynamics
// steps on sa_k = [2h_{k-1} ; a_{k-1}/|A|] (the state head skipped at k = K,
// whose h_K no prediction reads; the reward heads only with
// intermediate_rewards); K+1 predictions on h_0, h_0, h_1 .. h_{K-1} (Q10).
static int build_bp(mz_handle* h) {
    const int K = h->conf.num_unroll_steps, H = h->H;
    std::vector<BpApp> apps;
    std::vector<BpHead> heads;
    int off = 0;
    auto tensor = [&](int rows) { int o = off; off += ((rows + 3) & ~3) * 16; return o; };
    const int obs_t = tensor(h->obs_feat);
    auto dense = [&](int li, int x) {
        const LayerSpec& L = h->layers[li];
        BpApp a{};
        a.op = BP_DENSE; a.w_off = (int)L.flux_w; a.b_off = (int)L.flux_b; a.in = L.in; a.out = L.out;
        a.act = L.act; a.x = x; a.y = tensor(L.out); a.step = li;
        a.bn_off = L.bn ? (int)L.flux_be : -1;                // make_dense's BatchNorm: t kept at z
        a.z = L.bn ? tensor(L.out) : -1;
        apps.push_back(a);
        return a.y;
    };
    auto chain = [&](int net, int ch, int x) {
        for (int li : h->chains[net][ch]) x = dense(li, x);
        return x;
    };
    std::vector<int> hs(K + 1, -1);
    hs[0] = chain(MZ_NET_REPR, CH_TRUNK, obs_t);                                // :347
    for (int k = 1; k <= K; ++k) {                                              // :355-362
        BpApp c{};
        c.op = BP_CONCAT; c.in = H; c.out = H + h->plane; c.x = hs[k - 1]; c.y = tensor(c.out); c.step = k - 1;
        c.bn_off = c.z = -1;
        apps.push_back(c);
        const int t = chain(MZ_NET_DYN, CH_TRUNK, c.y);
        if (k < K) hs[k] = chain(MZ_NET_DYN, CH_HEAD1, t);
        if (h->conf.intermediate_rewards) heads.push_back(BpHead{BP_HEAD_R, chain(MZ_NET_DYN, CH_HEAD2, t), k});
    }
    for (int k = 0; k <= K; ++k) {                                              // :351, :356 (Q10)
        const int t = chain(MZ_NET_PRED, CH_TRUNK, hs[k <= 1 ? 0 : k - 1]);
        heads.push_back(BpHead{BP_HEAD_V, chain(MZ_NET_PRED, CH_HEAD1, t), k});
        heads.push_back(BpHead{BP_HEAD_P, chain(MZ_NET_PRED, CH_HEAD2, t), k});
    }
    // level schedule of the tile kernel (mz_bp_tile_lv).  Forward: an
    // application's level is one past its input's producer (the observation:
    // level 0).  Backward, in reverse application order: one past the latest
    // consumer of its output (the applications reading it, which accumulate
    // G[y]), and past every later application accumulating into the same G[x]
    // (so no two units of a level add into one tensor, and the sequential
    // kernel's accumulation order holds)
    const int na = (int)apps.size();
    std::vector<int> flv(na, 0), blv(na, 0);
    int nfl = 0, nbl = 0;
    for (int a = 0; a < na; ++a) {
        int l = 0;
        for (int p = 0; p < a; ++p) if (apps[p].y == apps[a].x) l = std::max(l, flv[p] + 1);
        flv[a] = l; nfl = std::max(nfl, l + 1);
    }
    for (int a = na - 1; a >= 0; --a) {
        int l = 0;
        for (int c = a + 1; c < na; ++c) {
            if (apps[c].x == apps[a].y) l = std::max(l, blv[c] + 1);           // consumers of y
            if (apps[c].x == apps[a].x) l = std::max(l, blv[c] + 1);           // same G[x], earlier in backward
        }
        blv[a] = l; nbl = std::max(nbl, l + 1);
    }
    // ... then each backward application as late as those constraints allow
    // (the same level count): ASAP piles every prediction head of the unroll
    // into the first levels (~70 units on 16 waves, serialised), ahead of the
    // dynamics chain they do not gate; ALAP spreads them along the chain.
    // Application c must precede a (a < c) when a produces c's input or adds
    // into the same G[x] after it.
    for (int c = 0; c < na; ++c) {
        int l = nbl - 1;
        for (int a = 0; a < c; ++a)
            if (apps[c].x == apps[a].y || apps[c].x == apps[a].x) l = std::min(l, blv[a] - 1);
        blv[c] = l;
    }
    std::vector<int2> fun, bun;
    std::vector<int> flev, blev;
    for (int l = 0; l < nfl; ++l) {
        flev.push_back((int)fun.size());
        for (int a = 0; a < na; ++a)
            if (flv[a] == l) {
                const int nb = apps[a].op == BP_DENSE ? (apps[a].out + 15) / 16 : 1;
                for (int b = 0; b < nb; ++b) fun.push_back(make_int2(a, b));
            }
    }
    flev.push_back((int)fun.size());
    for (int l = 0; l < nbl; ++l) {
        blev.push_back((int)bun.size());
        for (int a = na - 1; a >= 0; --a)
            if (blv[a] == l) {
                const int nb = apps[a].op == BP_DENSE ? (apps[a].in + 15) / 16 : 1;
                for (int b = 0; b < nb; ++b) bun.push_back(make_int2(a, b));
            }
    }
    blev.push_back((int)bun.size());
    // mz_bp_tile_lv's LDS tensor cache: slots of the largest tensor.  Forward,
    // level by level: a tensor read at later levels takes a free slot when it
    // is produced (its readers read the copy) and frees it after its last
    // reading level.  Backward: a ∂L/∂x takes a slot at its first contribution
    // and frees it after its producer's level read it (and wrote it out for
    // mz_bp_dw).  Everything else stays in the arena: the level that writes it
    // ends with a barrier that drains the stores (fsync / bsync), as do the
    // last forward level (the heads and the backward read the arena).
    std::vector<int> fsync(nfl, 0), bsync(nbl, 0);
    int cache_floats = 0, obs_s = -1, slot = 0;
    for (BpApp& a : apps) { a.xs = a.ys = a.gys = a.gxs = -1; a.gxf = 0; }
#if BP_LV_SIMPLE && !BP_LV_PREFETCH
    {
        auto rows16 = [](int r) { return ((r + 3) & ~3) * 16; };
        slot = rows16(h->obs_feat);
        for (const BpApp& a : apps) slot = std::max(slot, rows16(a.out));
        const size_t sched = (size_t)na * sizeof(BpApp) + (fun.size() + bun.size()) * sizeof(int2) +
                             (size_t)(2 * (nfl + nbl) + 8) * sizeof(int);
        // (a schedule that leaves no room for the cache runs without it, not with a wrapped count)
        const int nslot = sched + 64 < kLdsMax
                              ? (int)std::min<size_t>(64, (kLdsMax - sched - 64) / ((size_t)slot * 4)) : 0;
        cache_floats = nslot * slot;
        std::vector<int> free_s;
        for (int i = nslot - 1; i >= 0; --i) free_s.push_back(i * slot);
        // forward
        std::map<int, int> last_read, fslot;                 // tensor -> last reading level, -> slot
        for (int a = 0; a < na; ++a) last_read[apps[a].x] = std::max(last_read.count(apps[a].x) ? last_read[apps[a].x] : -1, flv[a]);
        auto take = [&](int t) {
            if (!last_read.count(t) || free_s.empty()) return -1;
            const int o = free_s.back(); free_s.pop_back();
            fslot[t] = o;
            return o;
        };
        obs_s = take(obs_t);
        for (int l = 0; l < nfl; ++l) {
            for (auto it = fslot.begin(); it != fslot.end();) {
                if (last_read[it->first] < l) { free_s.push_back(it->second); it = fslot.erase(it); }
                else ++it;
            }
            for (int a = 0; a < na; ++a)
                if (flv[a] == l) { auto f = fslot.find(apps[a].x); apps[a].xs = f != fslot.end() ? f->second : -1; }
            for (int a = 0; a < na; ++a)
                if (flv[a] == l) {
                    apps[a].ys = take(apps[a].y);
                    if (apps[a].ys < 0 && last_read.count(apps[a].y)) fsync[l] = 1;
                }
        }
        fsync[nfl - 1] = 1;
        // backward
        free_s.clear();
        for (int i = nslot - 1; i >= 0; --i) free_s.push_back(i * slot);
        std::map<int, int> producer, where, gslot;            // tensor -> app, -> slot or -1 (decided), live slots
        for (int a = 0; a < na; ++a) producer[apps[a].y] = a;
        for (const BpHead& hd : heads) where[hd.y] = -1;      // bp_heads writes these to the arena
        for (int l = 0; l < nbl; ++l) {
            for (auto it = gslot.begin(); it != gslot.end();) {
                if (blv[producer[it->first]] < l) { free_s.push_back(it->second); it = gslot.erase(it); }
                else ++it;
            }
            for (int a = 0; a < na; ++a) {
                if (blv[a] != l) continue;
                auto g = gslot.find(apps[a].y);
                apps[a].gys = g != gslot.end() ? g->second : -1;
            }
            for (int a = 0; a < na; ++a) {
                if (blv[a] != l) continue;
                const int t = apps[a].x;
                auto w = where.find(t);
                if (w == where.end()) {
                    int o = -1;
                    if (producer.count(t) && !free_s.empty()) {
                        o = free_s.back(); free_s.pop_back();
                        gslot[t] = o;
                        apps[a].gxf = 1;
                    }
                    where[t] = o;
                    apps[a].gxs = o;
                } else {
                    apps[a].gxs = w->second;
                }
                if (apps[a].gxs < 0) bsync[l] = 1;
            }
        }
    }
#endif
    // what the plan leaves to the arena (mz_debug_bp_plan): hand-offs between
    // applications that go through HBM and the flagged barriers that order them
    {
        std::map<int, int> producer, readers;
        for (int a = 0; a < na; ++a) { producer[apps[a].y] = a; ++readers[apps[a].x]; }
        int* c = h->bp_plan;
        c[0] = c[1] = c[2] = c[3] = c[4] = 0;
        for (const BpApp& a : apps) {
            if (a.xs < 0 && producer.count(a.x)) ++c[0];      // a produced input read from the arena
            if (a.ys < 0 && readers.count(a.y)) ++c[1];       // an output read later, without a forward slot
            if (a.gxs < 0 && producer.count(a.x)) ++c[2];     // ∂L/∂x added in the arena, its producer reads it there
        }
        for (int f : fsync) c[3] += f;
        for (int f : bsync) c[4] += f;
        h->bp_slot_floats = slot;
        h->bp_nslot = slot ? cache_floats / slot : 0;
    }
    // dW: every layer's applications, one wave per 16x16 block (+ one per bias block)
    std::vector<BpLayer> layers(h->layers.size());
    std::vector<BpUse> uses;
    std::vector<BpJob> jobs;
    for (int n = 0; n < 4; ++n) h->bp_job0[n] = -1;
    for (size_t li = 0; li < h->layers.size(); ++li) {
        const LayerSpec& L = h->layers[li];
        if (h->bp_job0[L.net] < 0) h->bp_job0[L.net] = (int)jobs.size();   // layers are in net order
        BpLayer& bl = layers[li];
        bl.w_off = (int)L.flux_w; bl.b_off = (int)L.flux_b; bl.in = L.in; bl.out = L.out; bl.act = L.act;
        bl.bn_off = L.bn ? (int)L.flux_be : -1;
        bl.use0 = (int)uses.size();
        for (const BpApp& a : apps) if (a.op == BP_DENSE && a.step == (int)li) uses.push_back(BpUse{a.x, a.y, a.z});
        bl.n_use = (int)uses.size() - bl.use0;
        for (int ob = 0; ob < (L.out + 15) / 16; ++ob) {
            for (int ib = 0; ib < (L.in + 15) / 16; ++ib) jobs.push_back(BpJob{(int)li, ob, ib});
            jobs.push_back(BpJob{(int)li, ob, -1});
        }
    }
    auto up = [&](auto** d, const auto& v) -> int {
        MZ_TRY(h, dalloc(h, d, v.size()));
        MZ_TRY(h, hipMemcpy(*d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
        return 0;
    };
    if (up(&h->d_bp_apps, apps) || up(&h->d_bp_heads, heads) || up(&h->d_bp_layers, layers) ||
        up(&h->d_bp_uses, uses) || up(&h->d_bp_jobs, jobs) || up(&h->d_bp_funits, fun) ||
        up(&h->d_bp_flev, flev) || up(&h->d_bp_bunits, bun) || up(&h->d_bp_blev, blev) ||
        up(&h->d_bp_fsync, fsync) || up(&h->d_bp_bsync, bsync))
        return -1;
    h->bp_cache_floats = cache_floats; h->bp_obs_s = obs_s;
    {
        const size_t lv = (size_t)na * sizeof(BpApp) + (fun.size() + bun.size()) * sizeof(int2) +
                          (size_t)(2 * (nfl + nbl) + 8) * sizeof(int) + 16 + (size_t)cache_floats * 4;
        if (lv > kLdsMax) return fail(h, "corrected learner: the level schedule exceeds the LDS");
        h->bp_lds_bytes = (int)lv;
        MZ_TRY(h, hipFuncSetAttribute((const void*)mz_bp_tile_lv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lv));
        MZ_TRY(h, hipFuncSetAttribute((const void*)mz_bp_tile_lv_nobn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lv));
    }
    h->bp_n_flev = nfl; h->bp_n_blev = nbl; h->bp_n_funit = (int)fun.size(); h->bp_n_bunit = (int)bun.size();
    h->bp_n_app = (int)apps.size(); h->bp_n_head = (int)heads.size(); h->bp_n_job = (int)jobs.size();
    h->bp_job0[3] = (int)jobs.size();
    for (int n = 2; n >= 0; --n) if (h->bp_job0[n] < 0) h->bp_job0[n] = h->bp_job0[n + 1];
    MZ_TRY(h, dalloc(h, &h->d_bp_sq, jobs.size()));
    h->bp_tile_floats = off; h->bp_obs_t = obs_t;
    h->bp_built = true;
    return 0;
}

// ---- the corrected learner for the ResNet nets (mz_backprop.hip mz_rbp_*):
// the same unrolled graph as build_bp, on the layers of rn_specs (convs with
// BatchNorm and residual blocks, the heads' 1x1 convs, Dense layers), one
// arena per sample: conv tensors [channel][position], dense vectors.
static int build_rbp(mz_handle* h) {
    const int K = h->conf.num_unroll_steps, P = h->plane, H = h->H;
    std::vector<RbpApp> apps;
    std::vector<BpHead> heads;
    int off = 0, dtf = 0, xsf = 0, max_units = 1;
    auto tensor = [&](int n) { int o = off; off += (n + 3) & ~3; return o; };
    const int obs_t = tensor(h->rin_feat);
    std::vector<RSpec> sp[3];
    size_t np[3];
    for (int n = 0; n < 3; ++n) sp[n] = rn_specs(h->rconf, h->rhp, n, &np[n]);
    // one RbpLayer per spec (nets in order) and its applications
    int lbase[3], nl = 0;
    for (int n = 0; n < 3; ++n) { lbase[n] = nl; nl += (int)sp[n].size(); }
    std::vector<std::vector<RbpUse>> luse(nl);
    const int npb = (P + 15) / 16;
    // the representation's tail follows the downsampler's parameters in net 0
    auto fo = [&](int net) { return h->flat_off[net] + (net == MZ_NET_REPR && h->ds ? h->ds_n : 0); };
    auto chain = [&](int net, int ch, int x, bool first_obs) {
        int saved = -1;
        for (size_t si = 0; si < sp[net].size(); ++si) {
            const RSpec& r = sp[net][si];
            if (r.chain != ch) continue;
            RbpApp a{};
            a.op = r.conv ? RBP_CONV : RBP_DENSE;
            a.w_off = (int)(fo(net) + r.woff); a.b_off = (int)(fo(net) + r.boff);
            a.bn_off = r.conv && r.bn ? (int)(fo(net) + r.bnoff) : -1;
            a.cin = r.cin; a.cout = r.cout; a.kw = r.kw; a.kh = r.kh; a.act = r.act;
            a.x = x; a.y = tensor(r.conv ? r.cout * P : r.cout);
            a.z = a.bn_off >= 0 ? tensor(r.cout * P) : -1;
            a.res = r.res_add ? saved : -1;
            if (r.res_save) saved = x;
            a.step = first_obs ? 1 : 0;
            first_obs = false;
            dtf = std::max(dtf, r.conv ? r.cout * P : r.cout);
            xsf = std::max(xsf, r.conv ? r.cin * P : r.cin);             // the staged input
            if (r.conv && r.kw * r.kh > 1) {                                // padded (mz_backprop.hip rbp_taps)
                const int Wb = h->rconf.observation_shape[0], Pp = (P / Wb + r.kh - 1) * (Wb + r.kw - 1);
                xsf = std::max(xsf, r.cin * Pp);
                dtf = std::max(dtf, r.cout * Pp);
            }
            if (r.conv) {
                max_units = std::max(max_units, std::max((r.cout + 15) / 16, (r.cin + 15) / 16) * npb);
            }
            apps.push_back(a);
            luse[lbase[net] + (int)si].push_back(RbpUse{a.x, a.y, a.z});
            x = a.y;
        }
        return x;
    };
    std::vector<int> hs(K + 1, -1);
    // :347; with the downsampler the first conv also produces ∂L/∂(its input) for mz_dsbp_bwd
    hs[0] = chain(MZ_NET_REPR, 0, obs_t, !h->ds);
    for (int k = 1; k <= K; ++k) {                                              // :355-362
        RbpApp c{};
        c.op = RBP_CONCAT; c.cin = H; c.cout = H + P; c.x = hs[k - 1]; c.y = tensor(c.cout); c.step = k - 1;
        c.bn_off = -1; c.z = -1; c.res = -1;
        dtf = std::max(dtf, c.cout);                                            // a ring slot holds it too
        apps.push_back(c);
        const int t = chain(MZ_NET_DYN, 0, c.y, false);
        if (k < K) hs[k] = chain(MZ_NET_DYN, 1, t, false);
        if (h->conf.intermediate_rewards) heads.push_back(BpHead{BP_HEAD_R, chain(MZ_NET_DYN, 2, t, false), k});
    }
    for (int k = 0; k <= K; ++k) {                                              // :351, :356 (Q10)
        const int t = chain(MZ_NET_PRED, 0, hs[k <= 1 ? 0 : k - 1], false);
        heads.push_back(BpHead{BP_HEAD_V, chain(MZ_NET_PRED, 1, t, false), k});
        heads.push_back(BpHead{BP_HEAD_P, chain(MZ_NET_PRED, 2, t, false), k});
    }
    // mz_rbp_sample's forward LDS ring: application a's output also goes to slot
    // a mod ns; an input or residual produced fewer than ns applications earlier
    // is read there, anything else from the arena, after a barrier that drained
    // the arena stores (fsync on the application before; the backward and the
    // heads read the arena too)
    const int ysz = (dtf + 3) & ~3, xsz = (xsf + 3) & ~3;
    int ns = 4;
    while (ns > 0 && (size_t)(ysz + xsz + ns * ysz) * 4 > kLdsMax) --ns;
    {
        std::map<int, int> producer;
        for (int a = 0; a < (int)apps.size(); ++a) {
            RbpApp& A_ = apps[a];
            auto slot = [&](int t) {
                auto it = producer.find(t);
                return it != producer.end() && a - it->second < ns ? it->second % ns : -1;
            };
            A_.xb = slot(A_.x);
            A_.rb = A_.res >= 0 ? slot(A_.res) : -1;
            A_.yb = ns > 0 ? a % ns : -1;
            A_.fsync = 0;
            if ((A_.xb < 0 || (A_.res >= 0 && A_.rb < 0)) && a > 0) apps[a - 1].fsync = 1;
            producer[A_.y] = a;
        }
        apps.back().fsync = 1;
    }
    // the backward ring (the same slots): in backward order, a tensor's ∂L/∂·
    // takes a free slot at its first contribution when its producer follows
    // within kGLife applications, and frees it when the producer has read it;
    // otherwise it accumulates in the arena (zeroed first, bsync after each
    // contribution).  The accumulation order is the arena's.
    std::vector<int2> gz;
    {
        const int kGLife = 6;
        std::map<int, int> producer, size_of;
        for (int a = 0; a < (int)apps.size(); ++a) {
            producer[apps[a].y] = a;
            size_of[apps[a].y] = apps[a].op == RBP_CONV ? apps[a].cout * P : apps[a].cout;
        }
        std::map<int, int> slot_of;          // tensor -> slot (ring-resident, live)
        std::map<int, int> where;            // tensor -> slot or -1 (decided at the first contribution)
        std::vector<int> free_slots;
        for (int i = ns - 1; i >= 0; --i) free_slots.push_back(i);
        for (int a = (int)apps.size() - 1; a >= 0; --a) {
            RbpApp& A_ = apps[a];
            A_.gyb = A_.gxb = A_.grb = -1; A_.gxf = A_.grf = 0; A_.bsync = 0;
            auto it = slot_of.find(A_.y);
            if (it != slot_of.end()) A_.gyb = it->second;
            auto contribute = [&](int t, int& sb, int& first) {
                auto w = where.find(t);
                if (w == where.end()) {
                    auto pr = producer.find(t);
                    int sl = -1;
                    if (pr != producer.end() && a - pr->second <= kGLife && !free_slots.empty()) {
                        sl = free_slots.back(); free_slots.pop_back();
                        slot_of[t] = sl;
                        first = 1;
                    }
                    where[t] = sl;
                    sb = sl;
                } else {
                    sb = w->second;
                }
                if (sb < 0) A_.bsync = 1;
            };
            const bool dx = A_.op == RBP_CONCAT || !A_.step;
            if (dx) contribute(A_.x, A_.gxb, A_.gxf);
            if (A_.op == RBP_CONV && A_.res >= 0) contribute(A_.res, A_.grb, A_.grf);
            if (A_.gyb >= 0) { free_slots.push_back(A_.gyb); slot_of.erase(A_.y); }
        }
        for (const auto& t : size_of)
            if (where.find(t.first) == where.end() || where[t.first] < 0) gz.push_back(make_int2(t.first, t.second));
        if (h->ds) gz.push_back(make_int2(obs_t, h->rin_feat));
    }
    h->rbp_ring = ns;
    // mz_rbp_dw's jobs, net by net (mz_bp_fold sums each net's Σθ² over its job range):
    // per layer its W blocks, then its bias (BatchNorm) blocks; every parameter once
    std::vector<RbpLayer> layers(nl);
    std::vector<RbpUse> uses;
    std::vector<RbpJob> jobs;
    std::vector<char> covered(h->nflat, 0);
    for (int n = 0; n < 3; ++n) {
        h->rbp_job0[n] = (int)jobs.size();
        for (size_t si = 0; si < sp[n].size(); ++si) {
            const RSpec& r = sp[n][si];
            const int li = lbase[n] + (int)si;
            RbpLayer& L = layers[li];
            L.conv = r.conv; L.w_off = (int)(fo(n) + r.woff); L.b_off = (int)(fo(n) + r.boff);
            L.bn_off = r.conv && r.bn ? (int)(fo(n) + r.bnoff) : -1;
            L.cin = r.cin; L.cout = r.cout; L.kw = r.kw; L.kh = r.kh; L.act = r.act;
            L.use0 = (int)uses.size(); L.n_use = (int)luse[li].size();
            for (const RbpUse& u : luse[li]) uses.push_back(u);
            const int Kw = r.conv ? r.kw * r.kh * r.cin : r.cin;
            for (int ob = 0; ob < (r.cout + 15) / 16; ++ob)
                for (int kb = 0; kb < (Kw + 15) / 16; ++kb) jobs.push_back(RbpJob{li, ob, kb});
            for (int ob = 0; ob < (r.cout + 15) / 16; ++ob) jobs.push_back(RbpJob{li, ob, -1});
            const size_t nw = (size_t)Kw * r.cout, nb = (size_t)r.cout * (L.bn_off >= 0 ? 3 : 1);
            for (size_t i = 0; i < nw; ++i) covered[(size_t)L.w_off + i] = 1;
            for (int o = 0; o < r.cout; ++o) covered[(size_t)L.b_off + o] = 1;
            if (L.bn_off >= 0) for (size_t i = 0; i < (size_t)2 * r.cout; ++i) covered[(size_t)L.bn_off + i] = 1;
            (void)nb;
        }
    }
    h->rbp_job0[3] = (int)jobs.size();
    // the downsampler (mz_dsbp_*): arena tensors per layer, one dW job per conv output channel
    std::vector<DsBpLayer> dlay;
    std::vector<DsDwJob> djobs;
    if (h->ds) {
        const DsPlan& D = h->dsplan;
        int o = 0, maxdt = 0;
        auto t = [&](int n) { const int r = o; o += (n + 3) & ~3; return r; };
        dlay.resize(D.n);
        for (int i = 0; i < D.n; ++i) {
            const DsLayer& L = D.L[i];
            const int n = L.cout * L.Wo * L.Ho;
            dlay[i].x = i == 0 ? -1 : dlay[i - 1].y;
            dlay[i].y = t(n);
            dlay[i].z = L.kind == DS_CONV && L.bn ? t(n) : -1;
            dlay[i].res = L.res_add ? dlay[i - 1].x : -1;
            if (L.kind != DS_CONV) continue;
            maxdt = std::max(maxdt, n);
            const int K = L.kw * L.kh * L.cin;
            if (L.kw * L.kh + 3 > DS_DW_THREADS) return fail(h, "corrected learner: a downsampler conv has too many taps");
            for (int co = 0; co < L.cout; ++co)
                for (int ci = 0; ci < L.cin; ++ci) djobs.push_back(DsDwJob{i, co, ci});
            for (int e = 0; e < K * L.cout; ++e) covered[(size_t)L.woff + e] = 1;
            for (int co = 0; co < L.cout; ++co) covered[(size_t)L.boff + co] = 1;
            if (L.bn) for (int e = 0; e < 2 * L.cout; ++e) covered[(size_t)L.bnoff + e] = 1;
        }
        h->dsbp_dt = o;
        h->dsbp_arena = o + ((maxdt + 3) & ~3);
        h->dsbp_n_job = (int)djobs.size();
    }
    for (size_t i = 0; i < h->nflat; ++i)
        if (!covered[i]) return fail(h, "corrected learner: a parameter no gradient job covers");
    auto up = [&](auto** d, const auto& v) -> int {
        MZ_TRY(h, dalloc(h, d, v.size()));
        MZ_TRY(h, hipMemcpy(*d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
        return 0;
    };
    if (up(&h->d_rbp_apps, apps) || up(&h->d_rbp_heads, heads) || up(&h->d_rbp_layers, layers) ||
        up(&h->d_rbp_uses, uses) || up(&h->d_rbp_jobs, jobs) || up(&h->d_rbp_gzero, gz))
        return -1;
    if (h->ds && (up(&h->d_dsbp_lay, dlay) || up(&h->d_dsbp_jobs, djobs))) return -1;
    h->rbp_n_gzero = (int)gz.size();
    // Σθ² per job: the downsampler's jobs first (net 0), then mz_rbp_dw's
    MZ_TRY(h, dalloc(h, &h->d_rbp_sq, jobs.size() + djobs.size()));
    h->rbp_n_app = (int)apps.size(); h->rbp_n_head = (int)heads.size(); h->rbp_n_job = (int)jobs.size();
    h->rbp_arena = off; h->rbp_obs_t = obs_t; h->rbp_dt = (dtf + 3) & ~3; h->rbp_xs = (xsf + 3) & ~3;
    // a wave per 16x16 conv block of a pass (mz_rbp_sample), 4 to 12 waves
    h->rbp_threads = 64 * std::min(12, std::max(4, max_units));
    const size_t lds = (size_t)(h->rbp_dt * (1 + h->rbp_ring) + h->rbp_xs) * 4;
    if (lds > kLdsMax) return fail(h, "corrected learner: a conv's tensors exceed the LDS");
    // above the 64 KB default (e.g. 256 filters on the 6x7 board: ~86 KB)
    MZ_TRY(h, hipFuncSetAttribute((const void*)mz_rbp_sample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->rbp_built = true;
    return 0;
}

static int rbp_grad(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st) {
    const int B = b->batch_size, K = h->conf.num_unroll_steps;
    if (!h->rbp_built && build_rbp(h)) return -1;
    if (ensure_batch(h, B)) return -1;
    if (B > h->rbp_cap) {
        MZ_TRY(h, dalloc(h, &h->d_rbp_act, (size_t)B * h->rbp_arena));
        MZ_TRY(h, dalloc(h, &h->d_rbp_grad, (size_t)B * h->rbp_arena));
        MZ_TRY(h, dalloc(h, &h->d_rbp_terms, (size_t)B * (K + 1) * 3));
        h->rbp_cap = B;
    }
    if (h->ds && B > h->dsbp_cap) {
        MZ_TRY(h, dalloc(h, &h->d_dsbp_act, (size_t)B * h->dsbp_arena));
        MZ_TRY(h, dalloc(h, &h->d_dsbp_grad, (size_t)B * h->dsbp_arena));
        h->dsbp_cap = B;
    }
    DsBpParams DP;
    if (h->ds) {                                  // the downsampler's forward, its output the tail's input
        if (ensure_dsb(h, B)) return -1;
        DP.B = B; DP.arena = h->dsbp_arena; DP.bn_s = h->bn_s; DP.plan = h->d_dsplan; DP.lay = h->d_dsbp_lay;
        DP.flat = h->d_flat; DP.obs = b->observation; DP.act = h->d_dsbp_act; DP.grad = h->d_dsbp_grad;
        DP.out = h->d_dsb; DP.gout = h->d_rbp_grad; DP.gstride = h->rbp_arena; DP.goff = h->rbp_obs_t;
        DP.dt_off = h->dsbp_dt;
        hipLaunchKernelGGL(mz_dsbp_fwd, dim3(B), dim3(DS_THREADS), 0, st, DP);
    }
    if ((size_t)B * (size_t)std::max(1, K + 1) * (size_t)h->plane >= (1u << 20))
        return fail(h, "corrected learner: batch x unroll x board too large for the dW index");
    RbpParams Q;
    Q.B = B; Q.K = K; Q.A = h->A; Q.H = h->H; Q.P = h->plane; Q.Wb = h->rconf.observation_shape[0];
    Q.obs_feat = h->rin_feat; Q.arena = h->rbp_arena; Q.n_app = h->rbp_n_app; Q.n_head = h->rbp_n_head;
    Q.obs_t = h->rbp_obs_t; Q.intermediate_rewards = h->conf.intermediate_rewards; Q.nflat = (int)h->nflat;
    Q.dt_floats = h->rbp_dt; Q.xs_floats = h->rbp_xs; Q.gzero = h->d_rbp_gzero; Q.n_gzero = h->rbp_n_gzero;
    Q.apps = h->d_rbp_apps; Q.heads = h->d_rbp_heads;
    Q.act = h->d_rbp_act; Q.grad = h->d_rbp_grad; Q.flat = h->d_flat;
    Q.obs = h->ds ? h->d_dsb : b->observation; Q.actions = b->actions; Q.tv = b->target_values;
    Q.tr = b->target_rewards;
    Q.tp = b->target_policies; Q.gscale = b->gradient_scale; Q.weights = b->weights; Q.terms = h->d_rbp_terms;
    Q.pv = h->d_pv; Q.pp = h->d_pp; Q.pr = h->d_pr;
    Q.stamps = nullptr;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, 128)));
    Q.stamps = h->d_stamps;
#endif
    hipLaunchKernelGGL(mz_rbp_sample, dim3(B), dim3(h->rbp_threads),
                       (size_t)(h->rbp_dt * (1 + h->rbp_ring) + h->rbp_xs) * 4, st, Q);
    const int nds = h->ds ? h->dsbp_n_job : 0;
    if (h->ds) {                                  // ∂L/∂(downsampler output) is the arena's obs tensor
        hipLaunchKernelGGL(mz_dsbp_bwd, dim3(B), dim3(DS_THREADS), 0, st, DP);
        DsDwParams DW;
        DW.B = B; DW.arena = h->dsbp_arena; DW.n_job = nds; DW.bn_s = h->bn_s; DW.plan = h->d_dsplan;
        DW.lay = h->d_dsbp_lay; DW.jobs = h->d_dsbp_jobs; DW.obs = b->observation; DW.act = h->d_dsbp_act;
        DW.grad = h->d_dsbp_grad; DW.flat = h->d_flat; DW.out = grad_dev ? grad_dev : h->d_grad; DW.sq = h->d_rbp_sq;
        hipLaunchKernelGGL(mz_dsbp_dw, dim3(nds), dim3(DS_DW_THREADS), 0, st, DW);
    }
    RbpDwParams D;
    D.B = B; D.P = h->plane; D.Wb = h->rconf.observation_shape[0]; D.arena = h->rbp_arena;
    D.jobs = h->d_rbp_jobs; D.layers = h->d_rbp_layers; D.uses = h->d_rbp_uses;
    D.act = h->d_rbp_act; D.grad = h->d_rbp_grad; D.flat = h->d_flat;
    D.out = grad_dev ? grad_dev : h->d_grad; D.sq = h->d_rbp_sq + nds;
    hipLaunchKernelGGL(mz_rbp_dw, dim3(h->rbp_n_job), dim3(64 * RBP_DW_WAVES), 0, st, D);
    BpFoldParams F;
    F.B = B; F.K = K; F.terms = h->d_rbp_terms; F.gscale = b->gradient_scale; F.weights = b->weights;
    F.flat = h->d_flat; F.netoff = h->d_netoff; F.losses = losses_dev ? losses_dev : h->d_loss;
    F.sq = h->d_rbp_sq;
    for (int n = 0; n < 4; ++n) F.job0[n] = n == 0 ? 0 : h->rbp_job0[n] + nds;
    hipLaunchKernelGGL(mz_bp_fold, dim3(4), dim3(256), 0, st, F);
    MZ_TRY(h, hipGetLastError());
    h->last_lvariant = h->ds ? "mz_dsbp+mz_rbp_sample+mz_rbp_dw" : "mz_rbp_sample+mz_rbp_dw";
    return 0;
}

// the FC plan's read-out (include/mz.h): built if needed, nothing launched
int mz_debug_bp_plan(mz_handle* h, int32_t* out, int n) {
    if (!h || !out) return -2;
    if (h->kind == 1) return fail(h, "mz_debug_bp_plan: the ResNet learner has no level schedule");
    if (n < MZ_BP_PLAN_FIELDS) return fail(h, "mz_debug_bp_plan: out holds fewer than MZ_BP_PLAN_FIELDS values");
    MZ_TRY(h, hipSetDevice(h->device));
    if (!h->bp_built && build_bp(h)) return -1;
    const int v[MZ_BP_PLAN_FIELDS] = {h->bp_n_app, h->bp_n_flev, h->bp_n_blev, h->bp_slot_floats, h->bp_nslot,
                                      h->bp_lds_bytes, h->bp_plan[0], h->bp_plan[1], h->bp_plan[2], h->bp_plan[3],
                                      h->bp_plan[4]};
    for (int i = 0; i < MZ_BP_PLAN_FIELDS; ++i) out[i] = v[i];
    return 0;
}

// corrected step: gradient (data term + 2θ) into grad_dev, losses, read-outs
int mz::bp_grad(mz_handle* h, const mz_batch* b, float* grad_dev, float* losses_dev, hipStream_t st) {
    if (h->kind == 1) return rbp_grad(h, b, grad_dev, losses_dev, st);
    const int B = b->batch_size, K = h->conf.num_unroll_steps;
    if (!h->bp_built && build_bp(h)) return -1;
    if (ensure_batch(h, B)) return -1;
    const int tiles = (B + 15) / 16;
    if (tiles > h->bp_tiles_cap) {
        MZ_TRY(h, dalloc(h, &h->d_bp_act, (size_t)tiles * h->bp_tile_floats));
        MZ_TRY(h, dalloc(h, &h->d_bp_grad, (size_t)tiles * h->bp_tile_floats));
        MZ_TRY(h, dalloc(h, &h->d_bp_terms, (size_t)tiles * 16 * (K + 1) * 3));
        h->bp_tiles_cap = tiles;
    }
    BpParams Q;
    Q.B = B; Q.K = K; Q.A = h->A; Q.H = h->H; Q.plane = h->plane; Q.obs_feat = h->obs_feat;
    Q.tile_floats = h->bp_tile_floats; Q.n_app = h->bp_n_app; Q.n_head = h->bp_n_head; Q.obs_t = h->bp_obs_t;
    Q.intermediate_rewards = h->conf.intermediate_rewards;
    Q.apps = h->d_bp_apps; Q.heads = h->d_bp_heads; Q.act = h->d_bp_act; Q.grad = h->d_bp_grad; Q.flat = h->d_flat;
    Q.obs = b->observation; Q.actions = b->actions; Q.tv = b->target_values; Q.tr = b->target_rewards;
    Q.tp = b->target_policies; Q.gscale = b->gradient_scale; Q.weights = b->weights; Q.terms = h->d_bp_terms;
    Q.pv = h->d_pv; Q.pp = h->d_pp; Q.pr = h->d_pr;
    Q.n_flev = h->bp_n_flev; Q.n_blev = h->bp_n_blev; Q.n_funit = h->bp_n_funit; Q.n_bunit = h->bp_n_bunit;
    Q.fsync = h->d_bp_fsync; Q.bsync = h->d_bp_bsync; Q.cache_floats = h->bp_cache_floats; Q.obs_s = h->bp_obs_s;
    Q.nflat = (int)h->nflat;
    const size_t lv_lds = (size_t)Q.n_app * sizeof(BpApp) + (size_t)(Q.n_funit + Q.n_bunit) * sizeof(int2) +
                          (size_t)(2 * (Q.n_flev + Q.n_blev) + 8) * sizeof(int) + 16 + (size_t)Q.cache_floats * 4;
    Q.funits = h->d_bp_funits; Q.flev = h->d_bp_flev; Q.bunits = h->d_bp_bunits; Q.blev = h->d_bp_blev;
    Q.stamps = nullptr;
#ifdef MZ_STAMPS
    if (!h->d_stamps) MZ_TRY(h, dalloc(h, &h->d_stamps, (size_t)8 * std::max(h->max_games, 128)));
    Q.stamps = h->d_stamps;
#endif
    // the level schedule (default) or the one-application-per-barrier kernel
    // (MZ_BP_SEQ=1, the same bits: tests/test_corrected_learner_gpu.py)
    if (std::getenv("MZ_BP_SEQ")) hipLaunchKernelGGL(mz_bp_tile, dim3(tiles), dim3(256), 0, st, Q);
    else if (lv_lds <= kLdsMax)                   // (no BatchNorm layer: the kernel without its per-layer test)
        hipLaunchKernelGGL(h->hp.use_batch_norm ? mz_bp_tile_lv : mz_bp_tile_lv_nobn, dim3(tiles), dim3(BP_LV_THREADS),
                           lv_lds, st, Q);
    else return fail(h, "corrected learner: the level schedule exceeds the LDS");
    BpDwParams D;
    D.tiles = tiles; D.tile_floats = h->bp_tile_floats; D.n_job = h->bp_n_job; D.jobs = h->d_bp_jobs;
    D.layers = h->d_bp_layers; D.uses = h->d_bp_uses; D.act = h->d_bp_act; D.grad = h->d_bp_grad; D.flat = h->d_flat;
    D.out = grad_dev ? grad_dev : h->d_grad;
    D.sq = h->d_bp_sq;
    hipLaunchKernelGGL(mz_bp_dw, dim3(h->bp_n_job), dim3(64), 0, st, D);
    BpFoldParams F;
    F.B = B; F.K = K; F.terms = h->d_bp_terms; F.gscale = b->gradient_scale; F.weights = b->weights;
    F.flat = h->d_flat; F.netoff = h->d_netoff; F.losses = losses_dev ? losses_dev : h->d_loss;
    F.sq = h->d_bp_sq;
    for (int n = 0; n < 4; ++n) F.job0[n] = h->bp_job0[n];
    hipLaunchKernelGGL(mz_bp_fold, dim3(4), dim3(256), 0, st, F);
    MZ_TRY(h, hipGetLastError());
    return 0;
}
