// mz_expert.hip — the rules-search expert opponent of evaluation play
// (DESIGN §18): mz_expert_move, one launch between the search and mz_sp_commit
// in MZ_SP_EVAL with MZ_OPP_EXPERT, and the kernel behind mz_expert_eval.
//
// One wave per row.  The rules and the subtree search are mz_expert_rules.h
// (shared with the host and the CPU sanitizer harness); this file spreads the
// A² two-ply prefixes (a1, a2) of a row over the 64 lanes, folds their results
// with shuffles and picks the move.  No LDS, no barrier: no wave waits on
// another.  Host mirror: games/expert.py, selfplay.BatchedSelfPlay.
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

extern "C" __global__ __launch_bounds__(256) void mz_expert_move(SpParams S, ExpertArgs X) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;                           // test worker: the slot's game is over
    const int player = S.player[g];
    if (!X.scores && player == S.muzero_player) return;           // MuZero's own turn: the search's action stands
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
    int best = score;
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(best, o);
        best = v > best ? v : best;
    }
    const uint64_t set = __ballot(ok && score == best);           // the best legal actions
    if (lane == 0 && set) {
        const uint32_t r = mz_rng_u32(S.seed, MZ_RNG_OPPONENT, S.game_offset + (uint32_t)g, S.step, 0);
        uint64_t k = set;
        for (int n = (int)mz_rng_below(r, (uint32_t)__builtin_popcountll(set)); n > 0; --n) k &= k - 1;
        X.act[g] = __builtin_ctzll(k) + 1;
    }
}
