// mz_snapshot.hip — snapshots: mz_snapshot_save / _load, the exact
// resume of self-play, the replay shard and the learner.
//
// The reference keeps its buffer in memory only (games/tictactoe/main.jl:21,
// "Start saving Buffer to disk at periodic intervals" is a TODO).  A snapshot
// is one safetensors file, a superset of a checkpoint (mz_checkpoint.cpp):
// mz_checkpoint_load reads the learner's nets and ADAM state from it by name.
//
// Tensors (R = Σ len of the n held games, Rh = Σ len of the G games in
// progress; rows of game i start at the exclusive prefix sum of len):
//   "<net>.<i>", "adam.m", "adam.v", "adam.beta_pow"   as in a checkpoint;
//   "shard.counters" I64 [8]   num_played_games, num_played_steps, total_samples,
//                     num_reanalysed_games, the Reanalyse cursor, its last round's
//                     header {first game number, games, rows};
//   "shard.len" I32 [n], "shard.rean" I32 [n] (bit 1: rrv, bit 2: rcv valid),
//   "shard.gprio" F32 [n] (PER)      the held games, oldest first;
//   "shard.obs" U8 [R, osz], "shard.act" I32 [R], "shard.rew" F32 [R],
//   "shard.tp" I32 [R], "shard.cv" F32 [R, A], "shard.rv" F32 [R],
//   "shard.rrv" F32 [R], "shard.rcv" F32 [R, A] (if the engine had allocated it),
//   "shard.prio" F32 [R] (PER)       their live rows;
//   "slots.len" I32 [G], "slots.obs" U8 [Rh, osz], "slots.act" I32 [Rh],
//   "slots.rew" F32 [Rh], "slots.tp" I32 [Rh], "slots.cv" F32 [Rh, A],
//   "slots.rv" F32 [Rh]              the games in progress, slot order;
//   "slots.board" U8 [G, osz], "slots.player" I32 [G], "slots.over" U8 [G],
//   "slots.ekey" U32 [G], "slots.tgame" F32 [G], "slots.eval" I64 [4],
//   "slots.flags" I32 [1] (bit 1: the Atari-like env's initial games are still to
//                     be drawn at the first move);
//   "train.state" I64 [3] {batch size, learner step t, actor refreshes},
//   "train.actor" F32 [nflat], "train.queued" F32 [nflat]   only after mz_train_init.
// __metadata__: format "libmz-snapshot-1", network, training_step, config (as a
// checkpoint), env, G, cap, T, osz, A, PER, rcv, train, rng_seed, and `settings`
// (the saving handle's mz_train_set_reanalyse / mz_selfplay_mode /
// mz_learner_set_mode / mz_debug_enable / networks-path settings, for
// information: the loading host applies its own).
//
// Rows past len and ring slots that hold no game are not state.  The live
// rows are packed on the device (mz_snap_scan, mz_snap_pack) and streamed
// through one bounded staging pair, device + pinned host; load is the inverse
// (mz_snap_unpack) after the whole file has been validated on the host
// (mz_snap_layout.h).  No kernel waits on another.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mz_snap_iface.h"

#define SNAP_TRY(h, expr)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return mz_set_error(h, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------ kernels
// the packed image of a record range in the staging buffer; a null section is not part of the set
struct SnapStage {
    uint8_t* obs; int32_t* act; float* rew; int32_t* tp; float* cv; float* rv; float* rrv; float* rcv; float* prio;
    int32_t* len; int32_t* rean; float* gprio; uint8_t* board;
};
struct SnapParams {
    SpHist rec;                 // the record set: the ring, or the games in progress
    uint8_t* board;             // [n][osz] (games in progress), or null
    int ring;                   // 1: record i is the i-th held game, oldest first; 0: slot i
    int cap, T, osz, A, n;
    const long long* counters;
    const int32_t* offs;        // [n + 1] exclusive prefix sums of the records' live rows
    int r0, r1;                 // the record range of this launch
    int rows_cap, rec_cap;      // the staging buffer's capacity
    SnapStage st;
};

// record i of the set -> its slot
__device__ __forceinline__ int snap_slot(int ring, const long long* counters, int cap, int n, int i) {
    if (!ring) return i;
    const long long played = counters[0];
    const long long oldest = played - n + 1;                       // game number of record 0
    const long long s = (oldest + i - 1) % cap;
    return (int)(s < 0 ? s + cap : s);
}

// offs[0 .. n] = exclusive prefix sums of the records' len, clamped to [0, T], in record order.  One
// workgroup walks the records in chunks of its size: an inclusive scan of the chunk in LDS, the
// running total carried in a register every thread holds.
extern "C" __global__ __launch_bounds__(1024) void mz_snap_scan(const int32_t* len, const long long* counters, int cap,
                                                                 int T, int n, int ring, int32_t* offs) {
    __shared__ int cnt[1024];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        int v = 0;
        if (i < n) {
            v = len[snap_slot(ring, counters, cap, n, i)];
            v = v < 0 ? 0 : v > T ? T : v;
        }
        cnt[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = tid >= o ? cnt[tid - o] : 0;
            __syncthreads();
            cnt[tid] += t;
            __syncthreads();
        }
        if (i < n) offs[i] = carry + cnt[tid] - v;
        carry += cnt[1023];
        __syncthreads();
    }
    if (tid == 0) offs[n] = carry;
}

// `bytes` by the workgroup, in the widest unit source and destination are aligned alike to: 16-byte
// vectors (the Atari-like env's 7,056-byte frames, every 4-byte field when the offsets agree), 4-byte
// words, or bytes (the board games' 27- and 126-byte observations); head and tail go bytewise
template <typename U>
__device__ __forceinline__ void snap_copy_as(char* dst, const char* src, size_t bytes, int tid, int nt) {
    size_t head = (sizeof(U) - ((size_t)src & (sizeof(U) - 1))) & (sizeof(U) - 1);
    if (head > bytes) head = bytes;
    const size_t nu = (bytes - head) / sizeof(U), tail0 = head + nu * sizeof(U);
    for (size_t k = tid; k < head; k += nt) dst[k] = src[k];
    U* du = reinterpret_cast<U*>(dst + head);
    const U* su = reinterpret_cast<const U*>(src + head);
    for (size_t k = tid; k < nu; k += nt) du[k] = su[k];
    for (size_t k = tail0 + tid; k < bytes; k += nt) dst[k] = src[k];
}
__device__ __forceinline__ void snap_copy(void* dst, const void* src, size_t bytes, int tid, int nt) {
    const size_t x = (size_t)dst ^ (size_t)src;
    char* d = static_cast<char*>(dst);
    const char* s = static_cast<const char*>(src);
    if ((x & 15) == 0) snap_copy_as<uint4>(d, s, bytes, tid, nt);
    else if ((x & 3) == 0) snap_copy_as<uint32_t>(d, s, bytes, tid, nt);
    else snap_copy_as<uint8_t>(d, s, bytes, tid, nt);
}

// One workgroup per record of [r0, r1): PACK copies the record's live rows of every field of the set
// to the staging sections at row offs[r] - offs[r0] (and its len / flags / game priority / board to
// entry r - r0); !PACK is the inverse, from the staging sections into the record's slot.  A record that
// would not fit the staging buffer is skipped (the host sizes the ranges so that none is).
template <bool PACK>
__device__ __forceinline__ void snap_move(const SnapParams& P) {
    const int i = P.r0 + (int)blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (i >= P.r1 || i >= P.n) return;
    const int j = i - P.r0;
    const long long row0 = (long long)P.offs[i] - P.offs[P.r0];
    long long rows = (long long)P.offs[i + 1] - P.offs[i];
    if (j >= P.rec_cap || row0 < 0 || rows < 0 || rows > P.T || row0 + rows > P.rows_cap) return;
    const int slot = snap_slot(P.ring, P.counters, P.cap, P.n, i);
    const size_t src = (size_t)slot * (size_t)P.T, dst = (size_t)row0, n = (size_t)rows;
    const size_t osz = (size_t)P.osz, A = (size_t)P.A;
#define SNAP_FIELD(stage, field, elem_bytes)                                                                      \
    if (P.st.stage) {                                                                                             \
        char* a = reinterpret_cast<char*>(P.st.stage) + dst * (elem_bytes);                                       \
        char* b = reinterpret_cast<char*>(P.rec.field) + src * (elem_bytes);                                      \
        if (PACK) snap_copy(a, b, n * (elem_bytes), tid, nt); else snap_copy(b, a, n * (elem_bytes), tid, nt);    \
    }
    SNAP_FIELD(obs, obs, osz)
    SNAP_FIELD(act, act, (size_t)4)
    SNAP_FIELD(rew, rew, (size_t)4)
    SNAP_FIELD(tp, tp, (size_t)4)
    SNAP_FIELD(cv, cv, A * 4)
    SNAP_FIELD(rv, rv, (size_t)4)
    SNAP_FIELD(rrv, rrv, (size_t)4)
    SNAP_FIELD(rcv, rcv, A * 4)
    SNAP_FIELD(prio, prio, (size_t)4)
#undef SNAP_FIELD
    if (P.st.board) {
        uint8_t* a = P.st.board + (size_t)j * osz;
        uint8_t* b = P.board + (size_t)slot * osz;
        if (PACK) snap_copy(a, b, osz, tid, nt); else snap_copy(b, a, osz, tid, nt);
    }
    if (tid == 0) {
        if (PACK) {
            P.st.len[j] = (int32_t)rows;
            if (P.st.rean) P.st.rean[j] = P.rec.rean[slot];
            if (P.st.gprio) P.st.gprio[j] = P.rec.gprio[slot];
        } else {
            P.rec.len[slot] = (int32_t)rows;
            if (P.st.rean) P.rec.rean[slot] = P.st.rean[j];
            if (P.st.gprio) P.rec.gprio[slot] = P.st.gprio[j];
        }
    }
}
extern "C" __global__ __launch_bounds__(256) void mz_snap_pack(SnapParams P) { snap_move<true>(P); }
extern "C" __global__ __launch_bounds__(256) void mz_snap_unpack(SnapParams P) { snap_move<false>(P); }

// --------------------------------------------------------------------- host
namespace {

std::string esc(const std::string& s) {
    std::string o;
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o;
}

// one tensor of the file
struct Entry {
    std::string name, dtype;
    std::vector<int64_t> shape;
    size_t bytes = 0, off = 0;               // off: from the start of the data section
    const void* data = nullptr;              // host data written as a whole, or null (streamed)
};

// a packed field: rows of `row_bytes` (a row field) or one entry of `row_bytes` per record (a record field)
enum { F_OBS, F_ACT, F_REW, F_TP, F_CV, F_RV, F_RRV, F_RCV, F_PRIO, F_LEN, F_REAN, F_GPRIO, F_BOARD, F_N };
struct Field {
    const char* name; const char* dtype; size_t esz;
    bool per_rec = false, on = false;
    size_t row_bytes = 0, elems = 1;         // elems: the tensor's second dimension (1: none)
    size_t stage_off = 0;
    int entry = -1;                          // its Entry
};

// a record set and its staging layout
struct Set {
    const char* prefix;
    Field f[F_N];
    int n = 0;
    std::vector<int32_t> offs;
};

void set_fields(Set& S, int osz_, int A_, bool per, bool rcv, bool ring) {
    const size_t osz = (size_t)osz_, A = (size_t)A_;
    const Field proto[F_N] = {
        {"obs", "U8", 1, false, true, osz, osz},        {"act", "I32", 4, false, true, 4, 1},
        {"rew", "F32", 4, false, true, 4, 1},           {"tp", "I32", 4, false, true, 4, 1},
        {"cv", "F32", 4, false, true, A * 4, A},        {"rv", "F32", 4, false, true, 4, 1},
        {"rrv", "F32", 4, false, ring, 4, 1},           {"rcv", "F32", 4, false, ring && rcv, A * 4, A},
        {"prio", "F32", 4, false, ring && per, 4, 1}, {"len", "I32", 4, true, true, 4, 1},
        {"rean", "I32", 4, true, ring, 4, 1},           {"gprio", "F32", 4, true, ring && per, 4, 1},
        {"board", "U8", 1, true, !ring, osz, osz}};
    for (int k = 0; k < F_N; ++k) S.f[k] = proto[k];
}

// the bounded staging pair.  rows_cap >= T and rec_cap >= 1 whatever the budget, so every record fits.
struct Stage {
    char* dev = nullptr; char* host = nullptr;
    size_t bytes = 0;
    int rows_cap = 0, rec_cap = 0;
    ~Stage() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
    }
};

const size_t kStageBytes = (size_t)64 << 20;   // DESIGN §16; MZ_SNAP_STAGE_BYTES overrides (tests: many ranges)

// sizes the staging buffer for the larger of the two sets and lays out each set's sections in it
int stage_alloc(mz_handle* h, Stage& st, Set* sets, int nsets, int T) {
    size_t budget = kStageBytes;
    if (const char* e = std::getenv("MZ_SNAP_STAGE_BYTES")) budget = (size_t)std::strtoull(e, nullptr, 10);
    size_t row_b = 0, rec_b = 0;
    for (int s = 0; s < nsets; ++s) {
        size_t a = 0, b = 0;
        for (const Field& f : sets[s].f)
            if (f.on) (f.per_rec ? b : a) += f.row_bytes;
        row_b = std::max(row_b, a);
        rec_b = std::max(rec_b, b);
    }
    const size_t rows = std::min<size_t>(std::max<size_t>((size_t)T, budget / 8 * 7 / row_b), 0x7fffffff);
    const size_t recs = std::min<size_t>(std::max<size_t>(1, budget / 8 / rec_b), 0x7fffffff);
    st.rows_cap = (int)rows; st.rec_cap = (int)recs;
    for (int s = 0; s < nsets; ++s) {
        size_t off = 0;
        for (Field& f : sets[s].f) {
            if (!f.on) continue;
            f.stage_off = off;
            off += ((f.per_rec ? recs : rows) * f.row_bytes + 15) / 16 * 16;
        }
        st.bytes = std::max(st.bytes, off);
    }
    SNAP_TRY(h, hipMalloc(reinterpret_cast<void**>(&st.dev), st.bytes));
    SNAP_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&st.host), st.bytes));
    return 0;
}

SnapParams snap_params(const MzSnapView& v, const Set& S, bool ring, const int32_t* d_offs, const Stage& st) {
    SnapParams P;
    std::memset(&P, 0, sizeof(P));
    P.rec = ring ? v.ring : v.hist;
    P.board = ring ? nullptr : v.board;
    P.ring = ring; P.cap = v.cap; P.T = v.T; P.osz = v.osz; P.A = v.A; P.n = S.n;
    P.counters = v.counters; P.offs = d_offs;
    P.rows_cap = st.rows_cap; P.rec_cap = st.rec_cap;
    auto sec = [&](int k) -> char* { return S.f[k].on ? st.dev + S.f[k].stage_off : nullptr; };
    P.st.obs = reinterpret_cast<uint8_t*>(sec(F_OBS)); P.st.act = reinterpret_cast<int32_t*>(sec(F_ACT));
    P.st.rew = reinterpret_cast<float*>(sec(F_REW)); P.st.tp = reinterpret_cast<int32_t*>(sec(F_TP));
    P.st.cv = reinterpret_cast<float*>(sec(F_CV)); P.st.rv = reinterpret_cast<float*>(sec(F_RV));
    P.st.rrv = reinterpret_cast<float*>(sec(F_RRV)); P.st.rcv = reinterpret_cast<float*>(sec(F_RCV));
    P.st.prio = reinterpret_cast<float*>(sec(F_PRIO)); P.st.len = reinterpret_cast<int32_t*>(sec(F_LEN));
    P.st.rean = reinterpret_cast<int32_t*>(sec(F_REAN)); P.st.gprio = reinterpret_cast<float*>(sec(F_GPRIO));
    P.st.board = reinterpret_cast<uint8_t*>(sec(F_BOARD));
    return P;
}

// the end of the record range that starts at r0 and fits the staging buffer
int range_end(const Set& S, const Stage& st, int r0) {
    int r1 = r0;
    while (r1 < S.n && r1 - r0 < st.rec_cap && (long long)S.offs[r1 + 1] - S.offs[r0] <= st.rows_cap) ++r1;
    return r1;
}

bool pwrite_all(int fd, const void* p, size_t n, size_t off) {
    const char* c = static_cast<const char*>(p);
    while (n) {
        const ssize_t w = ::pwrite(fd, c, n, (off_t)off);
        if (w <= 0) return false;
        c += w; n -= (size_t)w; off += (size_t)w;
    }
    return true;
}
bool pread_all(int fd, void* p, size_t n, size_t off) {
    char* c = static_cast<char*>(p);
    while (n) {
        const ssize_t r = ::pread(fd, c, n, (off_t)off);
        if (r <= 0) return false;
        c += r; n -= (size_t)r; off += (size_t)r;
    }
    return true;
}

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) ::close(fd); }
};
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// the entries of a set's fields: shapes from its prefix sums
void set_entries(Set& S, std::vector<Entry>& ents) {
    const int64_t R = S.offs[S.n];
    for (Field& f : S.f) {
        if (!f.on) continue;
        Entry e;
        e.name = std::string(S.prefix) + "." + f.name; e.dtype = f.dtype;
        const int64_t lead = f.per_rec ? S.n : R;
        e.shape = f.elems > 1 ? std::vector<int64_t>{lead, (int64_t)f.elems} : std::vector<int64_t>{lead};
        e.bytes = (size_t)lead * f.row_bytes;
        f.entry = (int)ents.size();
        ents.push_back(e);
    }
}

}  // namespace

extern "C" {

int mz_snapshot_save(mz_handle* h, const char* path, int64_t training_step) {
    if (!h) return -2;
    if (!path) return mz_set_error(h, "null path");
    MzSnapView v;
    if (int rc = mz_snap_view(h, &v)) return rc;            // MZ_SYNC first
    if ((long long)v.cap * v.T > 0x7fffffffLL) return mz_set_error(h, "snapshot: shard too large");
    // the checkpoint part
    const size_t nf = mz_flat_count(h);
    std::vector<float> flat(nf), m(nf), mv(nf);
    double bp[2];
    if (mz_state_get(h, flat.data(), m.data(), mv.data(), bp)) return -1;
    std::vector<Entry> ents;
    auto dense = [&](const std::string& name, const char* dtype, std::vector<int64_t> shape, const void* data,
                     size_t bytes) {
        Entry e;
        e.name = name; e.dtype = dtype; e.shape = std::move(shape); e.bytes = bytes; e.data = data;
        ents.push_back(e);
    };
    for (const MzParamDesc& d : mz_param_table(h))
        dense(d.name, "F32", std::vector<int64_t>(d.jshape.rbegin(), d.jshape.rend()), flat.data() + d.off, d.count * 4);
    dense("adam.m", "F32", {(int64_t)nf}, m.data(), nf * 4);
    dense("adam.v", "F32", {(int64_t)nf}, mv.data(), nf * 4);
    dense("adam.beta_pow", "F64", {2}, bp, 16);
    // the counters, then the two sets' prefix sums: the only read-backs before the copies
    long long cnt[MZ_SP_COUNTERS];
    SNAP_TRY(h, hipMemcpy(cnt, v.counters, sizeof(cnt), hipMemcpyDeviceToHost));
    Set sets[2];
    sets[0].prefix = "shard"; sets[1].prefix = "slots";
    set_fields(sets[0], v.osz, v.A, v.per != 0, v.ring.rcv != nullptr, true);
    set_fields(sets[1], v.osz, v.A, v.per != 0, false, false);
    sets[0].n = (int)std::max<long long>(0, std::min<long long>(cnt[0], v.cap));
    sets[1].n = v.G;
    DevBuf d_offs[2];
    for (int s = 0; s < 2; ++s) {
        Set& S = sets[s];
        SNAP_TRY(h, hipMalloc(&d_offs[s].p, ((size_t)S.n + 1) * 4));
        hipLaunchKernelGGL(mz_snap_scan, dim3(1), dim3(1024), 0, v.stream, (s == 0 ? v.ring : v.hist).len,
                           (const long long*)v.counters, v.cap, v.T, S.n, s == 0 ? 1 : 0, (int32_t*)d_offs[s].p);
        SNAP_TRY(h, hipGetLastError());
        S.offs.resize((size_t)S.n + 1);
        SNAP_TRY(h, hipMemcpyAsync(S.offs.data(), d_offs[s].p, S.offs.size() * 4, hipMemcpyDeviceToHost, v.stream));
    }
    SNAP_TRY(h, hipStreamSynchronize(v.stream));
    dense("shard.counters", "I64", {MZ_SP_COUNTERS}, cnt, sizeof(cnt));
    set_entries(sets[0], ents);
    set_entries(sets[1], ents);
    // the slots' dense arrays and the train section (network-sized, not shard-sized)
    const size_t G = (size_t)v.G;
    std::vector<int32_t> player(G);
    std::vector<uint8_t> over(G);
    std::vector<uint32_t> ekey(G);
    std::vector<float> tgame(G);
    long long eval[4];
    SNAP_TRY(h, hipMemcpy(player.data(), v.player, G * 4, hipMemcpyDeviceToHost));
    SNAP_TRY(h, hipMemcpy(over.data(), v.over, G, hipMemcpyDeviceToHost));
    SNAP_TRY(h, hipMemcpy(ekey.data(), v.ekey, G * 4, hipMemcpyDeviceToHost));
    SNAP_TRY(h, hipMemcpy(tgame.data(), v.tgame, G * 4, hipMemcpyDeviceToHost));
    SNAP_TRY(h, hipMemcpy(eval, v.eval, sizeof(eval), hipMemcpyDeviceToHost));
    const int32_t flags = v.reset_pending ? 1 : 0;
    dense("slots.player", "I32", {(int64_t)G}, player.data(), G * 4);
    dense("slots.over", "U8", {(int64_t)G}, over.data(), G);
    dense("slots.ekey", "U32", {(int64_t)G}, ekey.data(), G * 4);
    dense("slots.tgame", "F32", {(int64_t)G}, tgame.data(), G * 4);
    dense("slots.eval", "I64", {4}, eval, sizeof(eval));
    dense("slots.flags", "I32", {1}, &flags, 4);
    std::vector<float> actor, queued;
    if (v.train) {
        actor.resize(nf); queued.resize(nf);
        SNAP_TRY(h, hipMemcpy(actor.data(), v.actor, nf * 4, hipMemcpyDeviceToHost));
        SNAP_TRY(h, hipMemcpy(queued.data(), v.queued, nf * 4, hipMemcpyDeviceToHost));
        dense("train.state", "I64", {3}, v.tr, sizeof(v.tr));
        dense("train.actor", "F32", {(int64_t)nf}, actor.data(), nf * 4);
        dense("train.queued", "F32", {(int64_t)nf}, queued.data(), nf * 4);
    }
    // the header: every size is known
    auto kv = [](const char* k, const std::string& val) { return std::string(",\"") + k + "\":\"" + val + "\""; };
    std::string hdr = std::string("{\"__metadata__\":{\"format\":\"") + mzsnap::kFormat + "\"" +
                      kv("network", mz_net_kind(h)) + kv("training_step", std::to_string((long long)training_step)) +
                      kv("config", esc(mz_describe(h))) + kv("env", std::to_string(v.env)) +
                      kv("G", std::to_string(v.G)) + kv("cap", std::to_string(v.cap)) + kv("T", std::to_string(v.T)) +
                      kv("osz", std::to_string(v.osz)) + kv("A", std::to_string(v.A)) +
                      kv("PER", std::to_string(v.per)) + kv("rcv", v.ring.rcv ? "1" : "0") +
                      kv("train", v.train ? "1" : "0") + kv("rng_seed", std::to_string((unsigned long long)v.seed)) +
                      kv("settings", esc(v.settings)) + "}";
    size_t off = 0;
    for (Entry& e : ents) {
        e.off = off;
        hdr += ",\"" + e.name + "\":{\"dtype\":\"" + e.dtype + "\",\"shape\":[";
        for (size_t i = 0; i < e.shape.size(); ++i) hdr += (i ? "," : "") + std::to_string((long long)e.shape[i]);
        hdr += "],\"data_offsets\":[" + std::to_string(off) + "," + std::to_string(off + e.bytes) + "]}";
        off += e.bytes;
    }
    hdr += "}";
    while (hdr.size() % 8) hdr += ' ';
    Stage st;
    if (int rc = stage_alloc(h, st, sets, 2, v.T)) return rc;
    const std::string tmp = std::string(path) + ".tmp";
    Fd f;
    f.fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return mz_set_error(h, std::string("cannot write ") + tmp);
    auto fail_io = [&](const std::string& msg) {
        ::close(f.fd); f.fd = -1;
        std::remove(tmp.c_str());
        return mz_set_error(h, msg);
    };
    const uint64_t hl = hdr.size();
    const size_t base = 8 + hdr.size();
    bool ok = pwrite_all(f.fd, &hl, 8, 0) && pwrite_all(f.fd, hdr.data(), hdr.size(), 8);
    for (const Entry& e : ents)
        if (e.data) ok = ok && pwrite_all(f.fd, e.data, e.bytes, base + e.off);
    if (!ok) return fail_io(std::string("writing ") + path + " failed");
    // the packed fields: record ranges through the staging pair
    for (int s = 0; s < 2; ++s) {
        const Set& S = sets[s];
        SnapParams P = snap_params(v, S, s == 0, (const int32_t*)d_offs[s].p, st);
        for (int r0 = 0; r0 < S.n;) {
            const int r1 = range_end(S, st, r0);
            if (r1 == r0) return fail_io("snapshot: a record does not fit the staging buffer");
            P.r0 = r0; P.r1 = r1;
            hipLaunchKernelGGL(mz_snap_pack, dim3(r1 - r0), dim3(256), 0, v.stream, P);
            hipError_t e = hipGetLastError();
            const size_t rows = (size_t)(S.offs[r1] - S.offs[r0]), recs = (size_t)(r1 - r0);
            for (const Field& fl : S.f) {
                const size_t nb = (fl.per_rec ? recs : rows) * fl.row_bytes;
                if (!fl.on || !nb || e != hipSuccess) continue;
                e = hipMemcpyAsync(st.host + fl.stage_off, st.dev + fl.stage_off, nb, hipMemcpyDeviceToHost, v.stream);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
            if (e != hipSuccess) return fail_io(std::string("snapshot pack: ") + hipGetErrorString(e));
            for (const Field& fl : S.f) {
                if (!fl.on) continue;
                const size_t nb = (fl.per_rec ? recs : rows) * fl.row_bytes;
                const size_t at = (fl.per_rec ? (size_t)r0 : (size_t)S.offs[r0]) * fl.row_bytes;
                if (nb && !pwrite_all(f.fd, st.host + fl.stage_off, nb, base + ents[fl.entry].off + at))
                    return fail_io(std::string("writing ") + path + " failed");
            }
            r0 = r1;
        }
    }
    // an empty trailing tensor writes nothing: the file still has to reach its full size
    if (::ftruncate(f.fd, (off_t)(base + off)) != 0) return fail_io(std::string("writing ") + path + " failed");
    const int crc = ::close(f.fd);
    f.fd = -1;
    if (crc != 0 || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return mz_set_error(h, std::string("writing ") + path + " failed");
    }
    return 0;
}

int mz_snapshot_load(mz_handle* h, const char* path, int64_t* training_step) {
    if (!h) return -2;
    if (!path) return mz_set_error(h, "null path");
    Fd f;
    f.fd = ::open(path, O_RDONLY);
    if (f.fd < 0) return mz_set_error(h, std::string("cannot open ") + path);
    const long long fsize = (long long)::lseek(f.fd, 0, SEEK_END);
    uint64_t hl = 0;
    if (fsize < 8 || !pread_all(f.fd, &hl, 8, 0) || hl > (1u << 28)) return mz_set_error(h, "not a safetensors file");
    if ((long long)hl + 8 > fsize) return mz_set_error(h, "truncated header");
    std::string hdr(hl, '\0');
    if (!pread_all(f.fd, &hdr[0], hl, 8)) return mz_set_error(h, "truncated header");
    mzst::JV root;
    const std::string perr = mzst::parse_header(hdr.data(), hdr.size(), &root);
    if (!perr.empty()) return mz_set_error(h, perr);
    // ---- validation: nothing below touches the engine until every check has passed
    mzsnap::Geometry g;
    mzsnap::EngineGeometry eg;
    mz_snap_engine_geometry(h, &eg);
    std::string err = mzsnap::parse_geometry(root, &g);
    if (err.empty()) err = mzsnap::check_engine(g, eg);
    if (!err.empty()) return mz_set_error(h, err);
    // span: the entry's place in the file, checked against the expected dtype and shape
    auto span = [&](const std::string& name, const char* dtype, size_t esz, const std::vector<int64_t>& shape,
                    long long* off) -> int {
        const std::string e = mzst::entry_span(root, name, dtype, esz, shape, hl, fsize, off);
        return e.empty() ? 0 : mz_set_error(h, e);
    };
    auto read = [&](const std::string& name, const char* dtype, size_t esz, const std::vector<int64_t>& shape,
                    void* dst) -> int {
        long long off = 0;
        if (int rc = span(name, dtype, esz, shape, &off)) return rc;
        size_t cnt = 1;
        for (int64_t d : shape) cnt *= (size_t)d;
        if (cnt && !pread_all(f.fd, dst, cnt * esz, (size_t)off)) return mz_set_error(h, name + ": short read");
        return 0;
    };
    const size_t nf = mz_flat_count(h);
    std::vector<float> flat(nf), m(nf), mv(nf);
    double bp[2];
    for (const MzParamDesc& d : mz_param_table(h))
        if (int rc = read(d.name, "F32", 4, std::vector<int64_t>(d.jshape.rbegin(), d.jshape.rend()), flat.data() + d.off))
            return rc;
    if (int rc = read("adam.m", "F32", 4, {(int64_t)nf}, m.data())) return rc;
    if (int rc = read("adam.v", "F32", 4, {(int64_t)nf}, mv.data())) return rc;
    if (int rc = read("adam.beta_pow", "F64", 8, {2}, bp)) return rc;
    long long cnt[MZ_SP_COUNTERS], n_held = 0;
    if (int rc = read("shard.counters", "I64", 8, {MZ_SP_COUNTERS}, cnt)) return rc;
    err = mzsnap::check_counters(cnt, g.cap, g.T, &n_held);
    if (!err.empty()) return mz_set_error(h, err);
    Set sets[2];                             // laid out from the file's geometry
    sets[0].prefix = "shard"; sets[1].prefix = "slots";
    set_fields(sets[0], (int)g.osz, (int)g.A, g.per != 0, g.rcv != 0, true);
    set_fields(sets[1], (int)g.osz, (int)g.A, g.per != 0, false, false);
    sets[0].n = (int)n_held; sets[1].n = (int)g.G;
    std::vector<long long> foff[2];          // the fields' absolute file offsets
    for (int s = 0; s < 2; ++s) {
        Set& S = sets[s];
        std::vector<int32_t> len((size_t)S.n);
        if (int rc = read(std::string(S.prefix) + ".len", "I32", 4, {(int64_t)S.n}, len.data())) return rc;
        err = mzsnap::check_lens(len.data(), len.size(), g.T, s == 0 ? 1 : 0, &S.offs);
        if (!err.empty()) return mz_set_error(h, err);
        if (s == 0) {
            std::vector<int32_t> rean((size_t)S.n);
            if (int rc = read("shard.rean", "I32", 4, {(int64_t)S.n}, rean.data())) return rc;
            err = mzsnap::check_shard(cnt, S.offs, rean.data(), g.rcv != 0);
            if (!err.empty()) return mz_set_error(h, err);
        }
        std::vector<Entry> ents;
        set_entries(S, ents);                // the expected shapes: the prefix sums of len
        foff[s].assign(F_N, 0);
        for (int k = 0; k < F_N; ++k) {
            const Field& fl = S.f[k];
            if (!fl.on) continue;
            const Entry& e = ents[fl.entry];
            if (int rc = span(e.name, fl.dtype, fl.esz, e.shape, &foff[s][k])) return rc;
        }
    }
    const size_t G = (size_t)g.G;
    std::vector<int32_t> player(G);
    std::vector<uint8_t> over(G);
    std::vector<uint32_t> ekey(G);
    std::vector<float> tgame(G);
    long long eval[4], tr[3] = {0, 0, 0};
    int32_t flags = 0;
    if (int rc = read("slots.player", "I32", 4, {(int64_t)G}, player.data())) return rc;
    if (int rc = read("slots.over", "U8", 1, {(int64_t)G}, over.data())) return rc;
    if (int rc = read("slots.ekey", "U32", 4, {(int64_t)G}, ekey.data())) return rc;
    if (int rc = read("slots.tgame", "F32", 4, {(int64_t)G}, tgame.data())) return rc;
    if (int rc = read("slots.eval", "I64", 8, {4}, eval)) return rc;
    if (int rc = read("slots.flags", "I32", 4, {1}, &flags)) return rc;
    if (flags & ~1) return mz_set_error(h, "snapshot: unknown slot flags");
    for (size_t i = 0; i < G; ++i)                   // (a pending reset: the slots are still zeroed)
        if (player[i] < ((flags & 1) ? 0 : 1) || player[i] > 2 || over[i] > 1)
            return mz_set_error(h, "snapshot: bad player / over in a slot");
    if ((flags & 1) && g.env != MZ_ENV_ATARI) return mz_set_error(h, "snapshot: pending reset outside the Atari-like env");
    std::vector<float> actor, queued;
    if (g.train) {
        actor.resize(nf); queued.resize(nf);
        if (int rc = read("train.state", "I64", 8, {3}, tr)) return rc;
        if (int rc = read("train.actor", "F32", 4, {(int64_t)nf}, actor.data())) return rc;
        if (int rc = read("train.queued", "F32", 4, {(int64_t)nf}, queued.data())) return rc;
        if (tr[0] < 1 || tr[0] > 0x7fffffffLL || tr[1] < 0 || tr[2] < 0) return mz_set_error(h, "snapshot: bad train state");
    }
    // ---- every check passed: the engine takes the file's state
    if (mz_state_set(h, flat.data(), m.data(), mv.data(), bp)) return -1;
    MzSnapView v;
    if (int rc = mz_snap_restore_begin(h, (int)g.env, (int)g.G, (int)g.cap, g.rcv != 0, g.train != 0, &v)) return rc;
    SNAP_TRY(h, hipMemcpy(v.counters, cnt, sizeof(cnt), hipMemcpyHostToDevice));
    Stage st;
    if (int rc = stage_alloc(h, st, sets, 2, v.T)) return rc;
    for (int s = 0; s < 2; ++s) {
        const Set& S = sets[s];
        DevBuf d_offs;
        SNAP_TRY(h, hipMalloc(&d_offs.p, S.offs.size() * 4));
        SNAP_TRY(h, hipMemcpy(d_offs.p, S.offs.data(), S.offs.size() * 4, hipMemcpyHostToDevice));
        SnapParams P = snap_params(v, S, s == 0, (const int32_t*)d_offs.p, st);
        for (int r0 = 0; r0 < S.n;) {
            const int r1 = range_end(S, st, r0);
            if (r1 == r0) return mz_set_error(h, "snapshot: a record does not fit the staging buffer");
            const size_t rows = (size_t)(S.offs[r1] - S.offs[r0]), recs = (size_t)(r1 - r0);
            for (int k = 0; k < F_N; ++k) {
                const Field& fl = S.f[k];
                if (!fl.on) continue;
                const size_t nb = (fl.per_rec ? recs : rows) * fl.row_bytes;
                const size_t at = (fl.per_rec ? (size_t)r0 : (size_t)S.offs[r0]) * fl.row_bytes;
                if (!nb) continue;
                if (!pread_all(f.fd, st.host + fl.stage_off, nb, (size_t)foff[s][k] + at))
                    return mz_set_error(h, std::string(S.prefix) + "." + fl.name + ": short read");
                SNAP_TRY(h, hipMemcpyAsync(st.dev + fl.stage_off, st.host + fl.stage_off, nb, hipMemcpyHostToDevice,
                                           v.stream));
            }
            P.r0 = r0; P.r1 = r1;
            hipLaunchKernelGGL(mz_snap_unpack, dim3(r1 - r0), dim3(256), 0, v.stream, P);
            SNAP_TRY(h, hipGetLastError());
            SNAP_TRY(h, hipStreamSynchronize(v.stream));      // the pinned half is reused by the next range
            r0 = r1;
        }
    }
    SNAP_TRY(h, hipMemcpy(v.player, player.data(), G * 4, hipMemcpyHostToDevice));
    SNAP_TRY(h, hipMemcpy(v.over, over.data(), G, hipMemcpyHostToDevice));
    SNAP_TRY(h, hipMemcpy(v.ekey, ekey.data(), G * 4, hipMemcpyHostToDevice));
    SNAP_TRY(h, hipMemcpy(v.tgame, tgame.data(), G * 4, hipMemcpyHostToDevice));
    SNAP_TRY(h, hipMemcpy(v.eval, eval, sizeof(eval), hipMemcpyHostToDevice));
    if (g.train) {
        SNAP_TRY(h, hipMemcpy(v.actor, actor.data(), nf * 4, hipMemcpyHostToDevice));
        SNAP_TRY(h, hipMemcpy(v.queued, queued.data(), nf * 4, hipMemcpyHostToDevice));
    }
    if (int rc = mz_snap_restore_end(h, cnt, flags & 1, g.train ? tr : nullptr)) return rc;
    if (training_step) *training_step = g.training_step;
    return 0;
}

}  // extern "C"
