// mz_snap_layout.h — the host-only checks of mz_snapshot_load (mz_snapshot.hip,
// DESIGN §16): the snapshot's metadata, its counter words and its `len` arrays
// are untrusted input, validated here before the engine is touched.  Free of
// HIP and of the engine, like mz_st_header.h next to it, so the same code is
// compiled into libmz and into the CPU AddressSanitizer harness
// (tests/sanitize/snap_layout_asan.cpp).
//
// Every function returns "" or the reason for the refusal.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "mz_st_header.h"

namespace mzsnap {

constexpr const char* kFormat = "libmz-snapshot-1";
constexpr int kCounters = 8;             // = MZ_SP_COUNTERS (mz_selfplay_params.h)

// what the metadata says about the file's geometry
struct Geometry {
    std::string network;                 // "fc" | "resnet"
    std::string config;                  // mz_describe of the saving engine
    long long training_step = 0;
    long long env = 0, G = 0, cap = 0, T = 0, osz = 0, A = 0, per = 0, rcv = 0, train = 0;
    unsigned long long seed = 0;
};

// what the loading engine is
struct EngineGeometry {
    std::string network, config;
    long long env_osz[3] = {0, 0, 0};    // record bytes per move of each env kind this engine can host (0: cannot)
    long long max_games = 0, T = 0, A = 0, per = 0;
    unsigned long long seed = 0;
};

inline bool meta_int(const mzst::JV& md, const char* key, long long lo, long long hi, long long* out) {
    auto it = md.obj.find(key);
    if (it == md.obj.end() || it->second.t != mzst::JV::STR) return false;
    const std::string& s = it->second.str;
    if (s.empty() || s.size() > 19) return false;
    for (size_t i = 0; i < s.size(); ++i)
        if (!(s[i] >= '0' && s[i] <= '9') && !(i == 0 && s[i] == '-' && s.size() > 1)) return false;
    const long long v = std::strtoll(s.c_str(), nullptr, 10);
    if (v < lo || v > hi) return false;
    *out = v;
    return true;
}

inline std::string parse_geometry(const mzst::JV& root, Geometry* g) {
    auto mi = root.obj.find("__metadata__");
    if (mi == root.obj.end() || mi->second.t != mzst::JV::OBJ) return "snapshot: no metadata";
    const mzst::JV& md = mi->second;
    auto str = [&](const char* k, std::string* out) {
        auto it = md.obj.find(k);
        if (it == md.obj.end() || it->second.t != mzst::JV::STR) return false;
        *out = it->second.str;
        return true;
    };
    std::string fmt, seed;
    if (!str("format", &fmt) || fmt != kFormat) return std::string("snapshot: format is not ") + kFormat;
    if (!str("network", &g->network) || !str("config", &g->config)) return "snapshot: metadata lacks network / config";
    const long long i31 = 0x7fffffffLL;
    if (!meta_int(md, "training_step", -(1LL << 62), 1LL << 62, &g->training_step) ||
        !meta_int(md, "env", 0, 2, &g->env) || !meta_int(md, "G", 1, i31, &g->G) ||
        !meta_int(md, "cap", 1, i31, &g->cap) || !meta_int(md, "T", 2, i31, &g->T) ||
        !meta_int(md, "osz", 1, i31, &g->osz) || !meta_int(md, "A", 1, 1 << 20, &g->A) ||
        !meta_int(md, "PER", 0, 1, &g->per) || !meta_int(md, "rcv", 0, 1, &g->rcv) ||
        !meta_int(md, "train", 0, 1, &g->train))
        return "snapshot: bad geometry in the metadata";
    if (!str("rng_seed", &seed) || seed.empty() || seed.size() > 20) return "snapshot: bad rng_seed";
    for (char c : seed)
        if (c < '0' || c > '9') return "snapshot: bad rng_seed";
    g->seed = std::strtoull(seed.c_str(), nullptr, 10);
    if (g->cap < g->G) return "snapshot: cap < G";
    if (g->cap * g->T > i31 || g->G * g->T > i31) return "snapshot: more than 2^31 rows";
    return "";
}

// the file against the engine that loads it
inline std::string check_engine(const Geometry& g, const EngineGeometry& e) {
    if (g.network != e.network) return "snapshot: network kind " + g.network + ", this engine's is " + e.network;
    if (g.config != e.config) return "snapshot: written by an engine with another config / network shapes";
    if (g.env < 0 || g.env > 2 || e.env_osz[g.env] == 0) return "snapshot: its env does not fit this engine's observation_shape";
    if (g.osz != e.env_osz[g.env]) return "snapshot: observation_shape differs";
    if (g.A != e.A) return "snapshot: action_space_size differs";
    if (g.T != e.T) return "snapshot: max_moves differs";
    if (g.per != e.per) return "snapshot: PER flag differs";
    if (g.seed != e.seed) return "snapshot: rng_seed differs (the resume would not be exact)";
    if (g.G > e.max_games) return "snapshot: G exceeds this engine's max_games";
    return "";
}

// the counter words {played, steps, total_samples, reanalysed, cursor, round header[3]}: *n = games held
inline std::string check_counters(const long long* c, long long cap, long long T, long long* n) {
    if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0) return "snapshot: negative counter";
    *n = c[0] < cap ? c[0] : cap;
    if (c[2] > *n * T || c[2] < *n) return "snapshot: total_samples inconsistent with the games held";
    if (c[1] < c[2]) return "snapshot: num_played_steps below total_samples";
    if (c[6] < 0 || c[7] < 0 || c[7] > cap * T) return "snapshot: bad reanalyse round header";
    return "";
}

// `len` of n records, each in [min_len, T]: offs[n + 1] = the exclusive prefix sums (rows of record i
// start at offs[i])
inline std::string check_lens(const int32_t* len, size_t n, long long T, int min_len, std::vector<int32_t>* offs) {
    offs->assign(n + 1, 0);
    long long tot = 0;
    for (size_t i = 0; i < n; ++i) {
        if (len[i] < min_len || len[i] > T) return "snapshot: a game length outside [" + std::to_string(min_len) + ", T]";
        tot += len[i];
        if (tot > 0x7fffffffLL) return "snapshot: more than 2^31 rows";
        (*offs)[i + 1] = (int32_t)tot;
    }
    return "";
}

// the shard's records against the counters; flags: the per-game reanalyse masks
inline std::string check_shard(const long long* c, const std::vector<int32_t>& offs, const int32_t* rean, bool rcv) {
    const size_t n = offs.size() - 1;
    if ((long long)offs[n] != c[2]) return "snapshot: total_samples differs from the sum of the game lengths";
    for (size_t i = 0; i < n; ++i) {
        if (rean[i] < 0 || rean[i] > 3) return "snapshot: bad reanalyse flags";
        if ((rean[i] & 2) && !rcv) return "snapshot: a game flags reanalysed policies the file does not hold";
    }
    return "";
}

}  // namespace mzsnap
