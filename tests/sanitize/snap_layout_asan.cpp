// CPU AddressSanitizer / UBSan harness of the snapshot validator
// (muzero.jl_amd/csrc/mz_snap_layout.h, the checks mz_snapshot_load runs
// before it touches the engine).  A snapshot-shaped header is
// parsed from a heap buffer of exactly its length and walked through
// parse_geometry / check_engine / check_counters / check_lens / check_shard
// and entry_span with the shapes the lengths imply, as the loader does; then
// the same with truncated and mutated headers, and with `len` arrays, flags and
// counters a hostile file can hold.  Arrays live in exact-size heap vectors, so
// a read past the end is an ASan report.  Exit 0 = every case handled.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../muzero.jl_amd/csrc/mz_snap_layout.h"

static int failures = 0;

static void expect(bool cond, const char* what) {
    if (!cond) {
        std::fprintf(stderr, "FAIL: %s\n", what);
        ++failures;
    }
}

static bool parse_exact(const std::string& h, mzst::JV* root) {
    std::vector<char> buf(h.begin(), h.end());
    static char dummy;
    return mzst::parse_header(buf.empty() ? &dummy : buf.data(), buf.size(), root).empty();
}

static std::string entry(const std::string& name, const char* dt, const std::string& shape, long long a, long long b) {
    return "\"" + name + "\":{\"dtype\":\"" + dt + "\",\"shape\":" + shape + ",\"data_offsets\":[" +
           std::to_string(a) + "," + std::to_string(b) + "]}";
}

static std::string meta(const char* fmt, const char* T, const char* seed) {
    return std::string("{\"__metadata__\":{\"format\":\"") + fmt +
           "\",\"network\":\"fc\",\"training_step\":\"7\",\"config\":\"{\\\"observation_shape\\\":[3,3,3]}\","
           "\"env\":\"0\",\"G\":\"4\",\"cap\":\"6\",\"T\":\"" + T + "\",\"osz\":\"27\",\"A\":\"9\",\"PER\":\"0\","
           "\"rcv\":\"0\",\"train\":\"0\",\"rng_seed\":\"" + seed + "\",\"settings\":\"{}\"}";
}

// what the loader does with a parsed header; true if every check passes
static bool walk(const mzst::JV& root, const mzsnap::EngineGeometry& eg, const std::vector<long long>& cnt,
                 const std::vector<int32_t>& len, const std::vector<int32_t>& rean, uint64_t hl, long long fsize) {
    mzsnap::Geometry g;
    if (!mzsnap::parse_geometry(root, &g).empty()) return false;
    if (!mzsnap::check_engine(g, eg).empty()) return false;
    long long n = 0;
    if (!mzsnap::check_counters(cnt.data(), g.cap, g.T, &n).empty()) return false;
    if ((size_t)n != len.size() || len.size() != rean.size()) return false;
    std::vector<int32_t> offs;
    if (!mzsnap::check_lens(len.data(), len.size(), g.T, 1, &offs).empty()) return false;
    if (!mzsnap::check_shard(cnt.data(), offs, rean.data(), g.rcv != 0).empty()) return false;
    long long off = 0;
    const long long R = offs[len.size()];
    return mzst::entry_span(root, "shard.len", "I32", 4, {(int64_t)n}, hl, fsize, &off).empty() &&
           mzst::entry_span(root, "shard.obs", "U8", 1, {R, g.osz}, hl, fsize, &off).empty() &&
           mzst::entry_span(root, "shard.cv", "F32", 4, {R, g.A}, hl, fsize, &off).empty();
}

int main() {
    // 3 held games of 5, 9, 6 rows: R = 20
    const std::vector<int32_t> len = {5, 9, 6}, rean = {0, 1, 0};
    const std::vector<long long> cnt = {3, 20, 20, 1, 2, 1, 1, 9};
    const std::string valid = meta(mzsnap::kFormat, "10", "5") + "," + entry("shard.len", "I32", "[3]", 0, 12) + "," +
                              entry("shard.obs", "U8", "[20,27]", 12, 552) + "," +
                              entry("shard.cv", "F32", "[20,9]", 552, 1272) + "}  ";
    const uint64_t hl = valid.size();
    const long long fsize = 8 + (long long)hl + 1272;
    mzsnap::EngineGeometry eg;
    eg.network = "fc"; eg.config = "{\"observation_shape\":[3,3,3]}";
    eg.env_osz[0] = 27; eg.max_games = 8; eg.T = 10; eg.A = 9; eg.per = 0; eg.seed = 5;
    mzst::JV root;
    expect(parse_exact(valid, &root), "valid header parses");
    expect(walk(root, eg, cnt, len, rean, hl, fsize), "valid snapshot passes");
    expect(!walk(root, eg, cnt, len, rean, hl, fsize - 1), "truncated file");

    // the engine differs
    {
        mzsnap::EngineGeometry e = eg; e.network = "resnet";
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other network kind");
        e = eg; e.config = "{}";
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other config");
        e = eg; e.env_osz[0] = 0; e.env_osz[1] = 126;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other env");
        e = eg; e.T = 9;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other max_moves");
        e = eg; e.per = 1;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other PER");
        e = eg; e.seed = 6;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other seed");
        e = eg; e.max_games = 3;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "G > max_games");
        e = eg; e.A = 7;
        expect(!walk(root, e, cnt, len, rean, hl, fsize), "other action count");
    }
    // the arrays lie
    {
        std::vector<int32_t> l = len;
        l[1] = 11;                                           // T + 1
        expect(!walk(root, eg, cnt, l, rean, hl, fsize), "len T + 1");
        l = len; l[0] = -5;
        expect(!walk(root, eg, cnt, l, rean, hl, fsize), "negative len");
        l = len; l[0] = 0;
        expect(!walk(root, eg, cnt, l, rean, hl, fsize), "empty shard game");
        l = len; l[2] = 5;                                   // sum 19: disagrees with total_samples and the rows
        expect(!walk(root, eg, cnt, l, rean, hl, fsize), "len sum");
        std::vector<long long> c = cnt;
        c[2] = 19; c[1] = 19;                                // ... and with the row tensors alone
        expect(!walk(root, eg, c, l, rean, hl, fsize) , "len sum against the row tensors");
        l = {5, 9, 6, 1};                                    // more games than the counters hold
        expect(!walk(root, eg, cnt, l, {0, 0, 0, 0}, hl, fsize), "n differs from the counters");
        c = cnt; c[0] = -1;
        expect(!walk(root, eg, c, len, rean, hl, fsize), "negative played");
        c = cnt; c[2] = 61;
        expect(!walk(root, eg, c, len, rean, hl, fsize), "total_samples past n T");
        c = cnt; c[1] = 3;
        expect(!walk(root, eg, c, len, rean, hl, fsize), "steps below samples");
        c = cnt; c[7] = 61;
        expect(!walk(root, eg, c, len, rean, hl, fsize), "round rows past cap T");
        expect(!walk(root, eg, cnt, len, {0, 2, 0}, hl, fsize), "policy flag without rcv");
        expect(!walk(root, eg, cnt, len, {0, 4, 0}, hl, fsize), "unknown flag");
        expect(!walk(root, eg, cnt, len, {0, -1, 0}, hl, fsize), "negative flag");
        // n > cap is not expressible through the counters (n = min(played, cap)): a len tensor of
        // more than cap games fails the n check above; 1000 games played hold cap = 6
        c = cnt; c[0] = 1000; c[1] = 5000;
        long long n = 0;
        expect(mzsnap::check_counters(c.data(), 6, 10, &n).empty() && n == 6, "n clamps to cap");
        // empty sets
        std::vector<int32_t> offs;
        expect(mzsnap::check_lens(nullptr, 0, 10, 1, &offs).empty() && offs.size() == 1 && offs[0] == 0, "empty len");
    }
    // metadata that is not a geometry
    const char* bad_T[] = {"", "-3", "1", "x", "99999999999999999999", "1e3", " 10", "10 ", "4294967296"};
    for (const char* t : bad_T) {
        mzst::JV r;
        if (parse_exact(meta(mzsnap::kFormat, t, "5") + "}", &r)) {
            mzsnap::Geometry g;
            expect(!mzsnap::parse_geometry(r, &g).empty(), t);
        }
    }
    const char* bad_seed[] = {"", "-1", "0x5", "123456789012345678901", "5 "};
    for (const char* s : bad_seed) {
        mzst::JV r;
        if (parse_exact(meta(mzsnap::kFormat, "10", s) + "}", &r)) {
            mzsnap::Geometry g;
            expect(!mzsnap::parse_geometry(r, &g).empty(), s);
        }
    }
    {
        mzst::JV r;
        mzsnap::Geometry g;
        expect(parse_exact(meta("libmz-checkpoint-1", "10", "5") + "}", &r) && !mzsnap::parse_geometry(r, &g).empty(),
               "a checkpoint is not a snapshot");
        expect(parse_exact("{}", &r) && !mzsnap::parse_geometry(r, &g).empty(), "no metadata");
        expect(parse_exact("{\"__metadata__\":[1]}", &r) && !mzsnap::parse_geometry(r, &g).empty(), "metadata not an object");
        expect(parse_exact("{\"__metadata__\":{\"format\":7}}", &r) && !mzsnap::parse_geometry(r, &g).empty(), "format not a string");
    }
    // every truncation of the valid header, then random byte mutations, each walked like a real load
    for (size_t n = 0; n < valid.size(); ++n) {
        mzst::JV r;
        if (parse_exact(valid.substr(0, n), &r)) (void)walk(r, eg, cnt, len, rean, n, fsize);
    }
    std::mt19937 rng(4321);
    const char alphabet[] = "{}[]\":,\\u0123456789-+.eEtrufalsn \x01\xff";
    int parsed = 0, passed = 0;
    for (int it = 0; it < 100000; ++it) {
        std::string h = valid;
        const int edits = 1 + (int)(rng() % 3);
        for (int k = 0; k < edits && !h.empty(); ++k) {
            const size_t pos = rng() % h.size();
            switch (rng() % 3) {
                case 0: h[pos] = alphabet[rng() % (sizeof(alphabet) - 1)]; break;
                case 1: h.erase(pos, 1 + rng() % 8); break;
                default: h.insert(pos, 1, alphabet[rng() % (sizeof(alphabet) - 1)]); break;
            }
        }
        mzst::JV r;
        if (!parse_exact(h, &r)) continue;
        ++parsed;
        // random arrays of the size the (possibly mutated) counters imply
        std::vector<long long> c = cnt;
        if (rng() % 4 == 0) c[rng() % 8] = (long long)(int32_t)rng();
        std::vector<int32_t> l = len, f = rean;
        if (rng() % 4 == 0) l[rng() % 3] = (int32_t)(rng() % 24) - 6;
        if (rng() % 8 == 0) { l.push_back(1); f.push_back(0); }
        passed += walk(r, eg, c, l, f, h.size(), fsize);
    }
    std::printf("snap_layout_asan: %d failures, %d of 100000 mutations parsed, %d passed every check\n", failures,
                parsed, passed);
    return failures ? 1 : 0;
}
