// mz_expert.hip — the rules-search expert opponent of evaluation play
// (DESIGN §18): mz_expert_move, one launch between the search and mz_sp_commit
// in MZ_SP_EVAL with MZ_OPP_EXPERT, and the kernel behind mz_expert_eval.
//
// One wave per row.  The rules and the subtree search are mz_expert_rules.h
// (shared with the host and the CPU sanitizer harness); this file spreads the
// A² two-ply prefixes (a1, a2) of a row over the 64 lanes, folds their results
// with shuffles and picks the move.  No LDS, no barrier: no wave waits on
// another.  Host mirror: games/expert.py, selfplay.BatchedSelfPlay.
// Also here: the solved TicTacToe table's kernels (§18.1: the lookup
// mz_expert_table_move and the two small kernels of the fill) and the judge
// mode of both move kernels (§20.1).
#include "mz_internal.h"
#include "mz_selfplay_params.h"
#include "mz_expert_rules.h"

static_assert(MZX_TICTACTOE == MZ_ENV_TICTACTOE && MZX_CONNECT4 == MZ_ENV_CONNECT4, "env ids");

// the result of prefix i = a1·A + a2 as seen by the mover of a2 (the root's
// opponent): score(s', a2, D − 1); when a1 itself decides (it ends the game, or
// D = 1) every a2 carries −score(s, a1, D); MZX_ILLEGAL for a dead prefix
__device__ int expert_prefix(const ExpertPos& root, uint32_t legal1, int A, int D, int i) {
    const int a1 = i / A, a2 = i - a1 * A;
    if (i >= A * A || !((legal1 >> a1) & 1u)) return MZX_ILLEGAL;
    ExpertPos pos = root;
    uint64_t cell;
    const int out1 = mzx_play(pos, a1, &cell);
    if (out1 != MZX_CONT) return -(out1 * D);
    if (D == 1) return 0;
    if (!((mzx_legal(pos) >> a2) & 1u)) return MZX_ILLEGAL;
    return mzx_score(pos, a2, D - 1);
}

// self-play mode: what a row's wave does.  MuZero's rows (its turns; every row with MZ_OPP_SELF) are
// judged when X.judge is set and left alone otherwise; the other rows get the expert's move with
// MZ_OPP_EXPERT only.  With X.judge null (every launch outside a judging evaluation) this is the one
// test `player == muzero_player -> return` of an MZ_OPP_EXPERT move.
enum { EXPERT_SKIP = 0, EXPERT_PICK = 1, EXPERT_JUDGE = 2 };
__device__ int expert_role(const SpParams& S, const ExpertArgs& X, int player) {
    if (S.opponent == MZ_OPP_SELF || player == S.muzero_player) return X.judge ? EXPERT_JUDGE : EXPERT_SKIP;
    return S.opponent == MZ_OPP_EXPERT ? EXPERT_PICK : EXPERT_SKIP;
}

// the tail both kernels share: lane a < A holds score(s, a + 1, D) (MZX_ILLEGAL where !ok).
// EXPERT_PICK: the k-th (ascending) of the best legal actions replaces act[g].
// EXPERT_JUDGE: the chosen action act[g] adds {1, c == b, sgn(c) < sgn(b), b - c} to the audit row
// (c its score, b the best): integer atomics, so the sums are exact in any order.
__device__ void expert_tail(const SpParams& S, const ExpertArgs& X, int g, int lane, int role, bool ok, int score) {
    int best = score;
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(best, o);
        best = v > best ? v : best;
    }
    if (role == EXPERT_JUDGE) {
        const int a = X.act[g] - 1;                                // 0..A-1: the search's (or the caller's) action
        const int c = __shfl(score, a & 63);
        if (lane < 4 && c != MZX_ILLEGAL) {
            const int sc = (c > 0) - (c < 0), sb = (best > 0) - (best < 0);
            const long long term = lane == 0 ? 1 : lane == 1 ? c == best : lane == 2 ? sc < sb : best - c;
            atomicAdd(reinterpret_cast<unsigned long long*>(X.judge) + lane, (unsigned long long)term);
        }
        return;
    }
    const uint64_t set = __ballot(ok && score == best);           // the best legal actions
    if (lane == 0 && set) {
        const uint32_t r = mz_rng_u32(S.seed, MZ_RNG_OPPONENT, S.game_offset + (uint32_t)g, S.step, 0);
        uint64_t k = set;
        for (int n = (int)mz_rng_below(r, (uint32_t)__builtin_popcountll(set)); n > 0; --n) k &= k - 1;
        X.act[g] = __builtin_ctzll(k) + 1;
    }
}

extern "C" __global__ __launch_bounds__(256) void mz_expert_move(SpParams S, ExpertArgs X) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;                           // test worker: the slot's game is over
    const int player = S.player[g];
    const int role = X.scores ? EXPERT_PICK : expert_role(S, X, player);
    if (role == EXPERT_SKIP) return;                               // MuZero's own turn: the search's action stands
    const int A = S.A, cells = S.osz / 3;
    const uint8_t* b = S.board + (size_t)g * S.osz;
    const bool in = lane < cells;                                  // cells <= 42
    const uint64_t p1 = __ballot(in && b[in ? lane : 0] != 0);
    const uint64_t p2 = __ballot(in && b[in ? cells + lane : 0] != 0);
    const ExpertPos root = mzx_pos_from_bits(S.env, p1, p2, player);
    const uint32_t legal1 = mzx_legal(root);
    const int D = X.depth;
    // prefixes lane and lane + 64 (A² = 49 or 81 <= 128)
    const int t0 = expert_prefix(root, legal1, A, D, lane);
    const int t1 = expert_prefix(root, legal1, A, D, lane + 64);
    // lane a1 < A: max over a2, negated
    const int a1 = lane < A ? lane : A - 1;
    int m = MZX_ILLEGAL;
    for (int a2 = 0; a2 < A; ++a2) {
        const int i = a1 * A + a2;
        const int v0 = __shfl(t0, i & 63), v1 = __shfl(t1, i & 63);
        const int v = i < 64 ? v0 : v1;
        m = v > m ? v : m;
    }
    const bool ok = lane < A && ((legal1 >> a1) & 1u);
    const int score = ok ? -m : MZX_ILLEGAL;
    if (X.scores) {
        if (lane < A) X.scores[(size_t)g * A + lane] = score;
        return;
    }
    expert_tail(S, X, g, lane, role, ok, score);
}

// ---- the solved TicTacToe table
// The lookup in place of the search at depth 9: the same rows, early returns and tail as
// mz_expert_move, so the action is bit for bit the search kernel's.  Lanes below 9 form their cell's
// base-3 digit from the two plane bytes and the mover, a wave sum gives the code, and the same lanes
// load their score byte.  One wave per row; no LDS, no barrier.
extern "C" __global__ __launch_bounds__(256) void mz_expert_table_move(SpParams S, ExpertArgs X) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;
    const int player = S.player[g];
    const int role = expert_role(S, X, player);
    if (role == EXPERT_SKIP) return;
    const uint8_t* b = S.board + (size_t)g * S.osz;                // osz = 27: planes [p1, p2, empty]
    const bool in = lane < 9;
    int code = 0;
    if (in) {
        const bool s1 = b[lane] != 0, s2 = b[9 + lane] != 0;
        const bool me = player == 1 ? s1 : s2, opp = player == 1 ? s2 : s1;
        int w = 1;
        for (int c = 0; c < lane; ++c) w *= 3;
        code = w * (me ? 1 : opp ? 2 : 0);                         // a digit is 0..2: the code stays inside the table
    }
    for (int o = 8; o > 0; o >>= 1) code += __shfl_xor(code, o);  // lanes 0..15 hold the sum of lanes 0..8
    code = __shfl(code, 0);
    const int score = in ? (int)X.table[(size_t)code * MZX_TTT_ENTRY + lane] : MZX_ILLEGAL;
    expert_tail(S, X, g, lane, role, in && score != MZX_ILLEGAL, score);
}

// the fill's staging rows: the plane bytes and the player (1: the planes are then {me, opp, empty})
// of codes [c0, c0 + n), one thread per code
extern "C" __global__ __launch_bounds__(256) void mz_expert_table_rows(uint8_t* boards, int32_t* players, int c0,
                                                                        int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ExpertPos pos = mzx_ttt_decode(c0 + i);
    uint8_t* b = boards + (size_t)i * 27;
    for (int c = 0; c < 9; ++c) {
        const int me = (int)((pos.me >> c) & 1ull), opp = (int)((pos.opp >> c) & 1ull);
        b[c] = (uint8_t)me; b[9 + c] = (uint8_t)opp; b[18 + c] = (uint8_t)(1 - me - opp);
    }
    players[i] = 1;
}

// mz_expert_move's scores [n][9] of those rows -> the entries of codes [c0, c0 + n), one thread per byte
extern "C" __global__ __launch_bounds__(256) void mz_expert_table_pack(const int32_t* scores, int8_t* table, int c0,
                                                                        int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * MZX_TTT_ENTRY) return;
    const int e = i / MZX_TTT_ENTRY, k = i % MZX_TTT_ENTRY;
    table[(size_t)(c0 + e) * MZX_TTT_ENTRY + k] = k < 9 ? (int8_t)scores[(size_t)e * 9 + k] : (int8_t)MZX_ILLEGAL;
}
