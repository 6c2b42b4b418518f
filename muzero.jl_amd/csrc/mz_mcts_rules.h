// mz_mcts_rules.h — the rules-MCTS opponent: vanilla UCT with
// uniform random rollouts over the board envs' true rules (mz_expert_rules.h).
// Plain C++17 and HIP: the edge score and the rollout run in mz_mcts_move
// (mz_mcts_opp.hip), and the serial mcts_root_stats below is the same search
// on one thread, for mz_mcts_eval's host-side validation and the CPU sanitizer
// harness (tests/sanitize/mcts_rules_main.cpp).  Python mirror:
// games/mcts_rules.py.
//
// Definition (S simulations, R rollouts per simulation, live position s):
//   tree    node 0 = s; an edge (v, a) is a legal action a at node v with
//           n (simulations through it), w (the sum of their outcomes for the
//           player to move at v, in rollouts: one simulation adds -R..+R) and a
//           child node or none.  N_v = Σ_a n(v, a), L_v = the legal actions at v.
//   select  score(v, a) = q + u in float64, no contraction:
//             q = n > 0 ? (double)w / (double)(n·R) : 0
//             u = sqrt_tab[N_v] / (double)((1 + n)·L_v)      sqrt_tab[k] = sqrt(k)
//           the largest score, ties to the lowest action.
//   play    a ends the game with outcome o for the mover: z = o·R, no node is
//           made.  Else the edge's child: select there.  Else a new child (one
//           per simulation: at most S + 1 nodes) and R rollouts from its
//           position s'; rollout j draws the k-th (ascending) legal action with
//           k = mz_rng_below(mz_rng_u32(seed, MZ_RNG_ROLLOUT, id, rng_step,
//           (i·64 + j)·64 + ply), popcount(legal)), ply = 0 at s', until the
//           game ends; r_j = the outcome for the player to move at s';
//           z = −Σ_j r_j.
//   backup  the path's last edge: n += 1, w += z; z changes sign at every
//           level going up.
// Every quantity inside a simulation is an integer sum or a comparison of the
// values above: nothing depends on the order lanes are visited in.
#pragma once
#include <vector>

#include "mz_expert_rules.h"
#include "../../include/mz_detmath.h"

enum { MZM_MAX_SIMS = 1024, MZM_MAX_ROLLOUTS = 64, MZM_DEF_SIMS = 64, MZM_DEF_ROLLOUTS = 16 };
enum { MZM_MAX_DEPTH = 42 };                               // a path plays one stone per level: <= the cell count

struct MctsEdge { int32_t n, w, child; };                  // child: node index, 0 = none (node 0 is the root)

// score(v, a) of an edge with n, w at a node with N_v = N and L_v = L; sqrt_n = sqrt_tab[N]
MZX_HD double mzm_edge_score(int n, int w, int R, double sqrt_n, int L) {
    const double q = n > 0 ? (double)w / (double)(n * R) : 0.0;
    const double u = sqrt_n / (double)((1 + n) * L);
    return q + u;
}

// the k-th (0-based, ascending) set bit of m; k < popcount(m)
MZX_HD int mzm_kth_bit(uint32_t m, uint32_t k) {
    for (; k > 0; --k) m &= m - 1;
    return __builtin_ctz(m);
}

// rollout j of simulation i from the live position pos: the outcome for the player to move at pos
MZX_HD int mzm_rollout(ExpertPos pos, uint64_t seed, uint32_t id, uint32_t rng_step, int i, int j) {
    const uint32_t base = ((uint32_t)i * 64u + (uint32_t)j) * 64u;
    const int cells = mzx_cells(pos.env);
    for (int ply = 0; ply < cells; ++ply) {
        const uint32_t lg = mzx_legal(pos);
        if (!lg) return 0;                                 // a live position always has a move: unreachable from one
        const uint32_t r = mz_rng_u32(seed, MZ_RNG_ROLLOUT, id, rng_step, base + (uint32_t)ply);
        const int a0 = mzm_kth_bit(lg, mz_rng_below(r, (uint32_t)__builtin_popcount(lg)));
        uint64_t cell;
        const int out = mzx_play(pos, a0, &cell);
        if (out != MZX_CONT) return ply & 1 ? -out : out;  // the mover of an odd ply is the other player
    }
    return 0;
}

// The whole search on one host thread: n_out / w_out [A] of the root's edges, n = -1 (w = 0) for an
// illegal action.  sqrt_tab: S + 1 doubles.  root: not finished.
static inline void mcts_root_stats(const ExpertPos& root, int S, int R, uint64_t seed, uint32_t id, uint32_t rng_step,
                                   const double* sqrt_tab, int32_t* n_out, int32_t* w_out) {
    const int A = mzx_actions(root.env);
    const uint32_t legal0 = mzx_legal(root);
    std::vector<MctsEdge> tree((size_t)(S + 1) * A, MctsEdge{0, 0, 0});
    int nodes = 1;
    int path[MZM_MAX_DEPTH];
    for (int i = 0; i < S && legal0; ++i) {
        ExpertPos pos = root;
        int v = 0, depth = 0, z = 0;
        for (;;) {
            const uint32_t lg = mzx_legal(pos);
            const int L = __builtin_popcount(lg);
            int N = 0;
            for (int a = 0; a < A; ++a) N += tree[v * A + a].n;
            int best = -1;
            double bs = 0.0;
            for (int a = 0; a < A; ++a) {
                if (!((lg >> a) & 1u)) continue;
                const MctsEdge& e = tree[v * A + a];
                const double sc = mzm_edge_score(e.n, e.w, R, sqrt_tab[N], L);
                if (best < 0 || sc > bs) { best = a; bs = sc; }
            }
            uint64_t cell;
            const int out = mzx_play(pos, best, &cell);
            MctsEdge& e = tree[v * A + best];
            path[depth++] = v * A + best;
            if (out != MZX_CONT) { z = out * R; break; }
            if (e.child) { v = e.child; continue; }
            const int c = nodes++;
            e.child = c;
            int sum = 0;
            for (int j = 0; j < R; ++j) sum += mzm_rollout(pos, seed, id, rng_step, i, j);
            z = -sum;
            break;
        }
        for (int d = depth - 1; d >= 0; --d) {
            tree[path[d]].n += 1;
            tree[path[d]].w += z;
            z = -z;
        }
    }
    for (int a = 0; a < A; ++a) {
        const bool ok = (legal0 >> a) & 1u;
        n_out[a] = ok ? tree[a].n : -1;
        w_out[a] = ok ? tree[a].w : 0;
    }
}
