// mz_mcts_opp.hip — the rules-MCTS opponent of evaluation play:
// mz_mcts_move, one launch between the search and mz_sp_commit in MZ_SP_EVAL
// with MZ_OPP_MCTS, and the kernel behind mz_mcts_eval.
//
// One wave per row, X.games rows per workgroup.  The definition, the edge
// score and the rollout are mz_mcts_rules.h (shared with the host and the CPU
// sanitizer harness); this file spreads a node's edges over lanes 0..A-1 for
// the select, the R rollouts of a new node over lanes 0..R-1, and the path's
// edges over lanes 0..depth-1 for the backup.  The tree is a wave-private
// region of (S + 1)·A edge records in dynamic LDS; the path is one register
// per lane (lane d holds level d's edge).  The descent itself is wave-uniform:
// the position, the node and the chosen action are the same in every lane.
// No atomic, no workgroup barrier, no wait on another wave, and every loop is
// bounded by S, R or the cell count.  Host mirror: games/mcts_rules.py,
// selfplay.BatchedSelfPlay.
#include "mz_internal.h"
#include "mz_selfplay_params.h"
#include "mz_mcts_rules.h"

static_assert(MZM_MAX_DEPTH <= 64, "the path holds one level per lane");
static_assert(MZ_OPP_MCTS == 4, "the opponent id of the C ABI");

// the wave's own LDS writes are visible to its other lanes' later reads
__device__ __forceinline__ void mcts_wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

extern "C" __global__ __launch_bounds__(256) void mz_mcts_move(SpParams S, MctsArgs X) {
    extern __shared__ int32_t mcts_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * X.games + wave;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;                           // test worker: the slot's game is over
    const int player = S.player[g];
    if (!X.n && (S.opponent != MZ_OPP_MCTS || player == S.muzero_player)) return;   // MuZero's own turn
    const int A = S.A, cells = S.osz / 3, R = X.rollouts;
    const uint8_t* b = S.board + (size_t)g * S.osz;
    const bool in = lane < cells;                                  // cells <= 42
    const uint64_t p1 = __ballot(in && b[in ? lane : 0] != 0);
    const uint64_t p2 = __ballot(in && b[in ? cells + lane : 0] != 0);
    const ExpertPos root = mzx_pos_from_bits(S.env, p1, p2, player);
    const uint32_t legal0 = mzx_legal(root);
    const uint32_t id = S.game_offset + (uint32_t)g;
    MctsEdge* tree = reinterpret_cast<MctsEdge*>(mcts_lds) + (size_t)wave * (X.sims + 1) * A;
    const bool edge = lane < A;
    if (edge) tree[lane] = MctsEdge{0, 0, 0};
    mcts_wave_sync();
    int nodes = 1;
    for (int i = 0; i < X.sims && legal0; ++i) {
        ExpertPos pos = root;
        int v = 0, depth = 0, z = 0, mine = 0;                     // mine: the path's edge of level `lane`
        for (int level = 0; level < MZM_MAX_DEPTH; ++level) {
            // select: lane a < A scores edge (v, a); wave arg-max, ties to the lowest action
            const uint32_t lg = mzx_legal(pos);
            const int L = __builtin_popcount(lg);
            const bool ok = edge && ((lg >> lane) & 1u);
            const MctsEdge e = edge ? tree[v * A + lane] : MctsEdge{0, 0, 0};
            int N = e.n;                                           // lanes 0..15 cover the node: A <= 9
            for (int o = 8; o > 0; o >>= 1) N += __shfl_xor(N, o);
            N = __builtin_amdgcn_readfirstlane(N);
            double bs = ok ? mzm_edge_score(e.n, e.w, R, X.sqrt_tab[N], L) : -1.0e30;
            int ba = lane;
            for (int o = 8; o > 0; o >>= 1) {
                const double os = __shfl_xor(bs, o);
                const int oa = __shfl_xor(ba, o);
                if (os > bs || (os == bs && oa < ba)) { bs = os; ba = oa; }
            }
            const int a = __builtin_amdgcn_readfirstlane(ba);
            const int child = __builtin_amdgcn_readfirstlane(__shfl(e.child, a));
            // play
            uint64_t cell;
            const int out = mzx_play(pos, a, &cell);
            const int ei = v * A + a;
            if (lane == depth) mine = ei;
            ++depth;
            if (out != MZX_CONT) { z = out * R; break; }           // the move ends the game: no node
            if (child) { v = child; continue; }
            const int c = nodes++;                                 // one new node per simulation: c <= S
            if (lane == 0) tree[ei].child = c;
            if (edge) tree[c * A + lane] = MctsEdge{0, 0, 0};
            int r = lane < R ? mzm_rollout(pos, S.seed, id, S.step, i, lane) : 0;
            for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
            z = -__builtin_amdgcn_readfirstlane(r);
            break;
        }
        // backup: lane d < depth owns level d's edge (the path's edges are distinct)
        if (lane < depth) {
            tree[mine].n += 1;
            tree[mine].w += (depth - 1 - lane) & 1 ? -z : z;
        }
        mcts_wave_sync();
    }
    const bool ok0 = edge && ((legal0 >> lane) & 1u);
    const int n = ok0 ? tree[lane].n : -1;
    if (X.n) {
        if (edge) {
            X.n[(size_t)g * A + lane] = n;
            X.w[(size_t)g * A + lane] = ok0 ? tree[lane].w : 0;
        }
        return;
    }
    int best = n;
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(best, o);
        best = t > best ? t : best;
    }
    const uint64_t set = __ballot(ok0 && n == best);               // the most-visited legal actions
    if (lane == 0 && set) {
        const uint32_t r = mz_rng_u32(S.seed, MZ_RNG_OPPONENT, id, S.step, 0);
        uint64_t k = set;
        for (int m = (int)mz_rng_below(r, (uint32_t)__builtin_popcountll(set)); m > 0; --m) k &= k - 1;
        X.act[g] = __builtin_ctzll(k) + 1;
    }
}
