// mz_expert_rules.h — the rules-search expert opponent: the board
// envs' rules on bitboards and a fixed-depth exhaustive negamax over them.
// Plain C++17 and HIP: the same code runs in mz_expert_move (mz_expert.hip), in
// mz_expert_eval's host-side validation and in the CPU sanitizer harness
// (tests/sanitize/expert_rules_main.cpp).  Python mirror: games/expert.py.
//
// A position is {me, opp}: the stones of the player to move and of the other
// player.  TicTacToe: bit c = cell c.  Connect4: bit w + 7h (w the row, 0 =
// bottom, h the column); bit 6 of every column and the bits from 49 on stay
// zero, so shifted run tests cannot wrap from one column into the next.
//
// play + the terminal test equal env_step + game_winner (mz_selfplay.hip):
//   TicTacToe (Q14): after a move the game is over when the player now to move
//     holds a line (that player wins: the mover has lost) or the board is full
//     (a draw); the mover's own new line does not end the game.
//   Connect4: the stone lands on the lowest empty cell of its column; four in a
//     row through that stone wins for the mover; a full board is a draw.
//
// Definition (mover p, depth d >= 1): score(s, a, d) = d * outcome if a ends
// the game (outcome +1 / 0 / -1 for the mover), else -V(s', d - 1); V(s, 0) = 0,
// V(s, d) = max over legal a of score(s, a, d).  Exhaustive: no pruning.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define MZX_HD __host__ __device__ __forceinline__
#else
#define MZX_HD static inline
#endif

enum { MZX_TICTACTOE = 0, MZX_CONNECT4 = 1 };             // = MZ_ENV_TICTACTOE / MZ_ENV_CONNECT4 (mz.h)
enum { MZX_CONT = 2 };                                     // play: the game goes on (else +1 / 0 / -1 for the mover)
enum { MZX_ILLEGAL = -128, MZX_MAX_DEPTH = 9 };

struct ExpertPos { uint64_t me, opp; int env; };

MZX_HD int mzx_actions(int env) { return env == MZX_TICTACTOE ? 9 : 7; }
MZX_HD int mzx_cells(int env) { return env == MZX_TICTACTOE ? 9 : 42; }
MZX_HD uint64_t mzx_full(int env) { return env == MZX_TICTACTOE ? 0x1FFull : 0xFDFBF7EFDFBFull; }

// cell-indexed stones (bit k = cell k of a plane, the byte planes' order) -> the position of `player`
MZX_HD ExpertPos mzx_pos_from_bits(int env, uint64_t p1, uint64_t p2, int player) {
    if (env == MZX_CONNECT4) {                             // 6 rows per column -> 7 bits per column
        uint64_t a = 0, b = 0;
        for (int h = 0; h < 7; ++h) {
            a |= ((p1 >> (6 * h)) & 63ull) << (7 * h);
            b |= ((p2 >> (6 * h)) & 63ull) << (7 * h);
        }
        p1 = a; p2 = b;
    }
    ExpertPos pos;
    pos.me = player == 1 ? p1 : p2;
    pos.opp = player == 1 ? p2 : p1;
    pos.env = env;
    return pos;
}

// the [p1, p2, empty] byte planes -> position; false when a cell is set in no
// plane or in more than one, or the player is not 1 or 2
MZX_HD bool mzx_pos_from_planes(int env, const uint8_t* planes, int player, ExpertPos* pos) {
    const int cells = mzx_cells(env);
    uint64_t p1 = 0, p2 = 0;
    if (player != 1 && player != 2) return false;
    for (int k = 0; k < cells; ++k) {
        const int a = planes[k] != 0, b = planes[cells + k] != 0, e = planes[2 * cells + k] != 0;
        if (a + b + e != 1) return false;
        p1 |= (uint64_t)a << k;
        p2 |= (uint64_t)b << k;
    }
    *pos = mzx_pos_from_bits(env, p1, p2, player);
    return true;
}

// The solved TicTacToe table's index: code = Σ_cell 3^cell · d,
// d = 0 empty / 1 the mover's stone / 2 the other player's; 3^9 = 19683 codes.
// The scores read {me, opp, env} only, so one entry serves both players.
enum { MZX_TTT_CODES = 19683, MZX_TTT_ENTRY = 16 };       // an entry: nine int8 scores padded to 16 bytes
MZX_HD int mzx_ttt_code(const ExpertPos& pos) {
    int code = 0;
    for (int c = 8; c >= 0; --c)
        code = 3 * code + (int)((pos.me >> c) & 1ull) + 2 * (int)((pos.opp >> c) & 1ull);
    return code;
}
MZX_HD ExpertPos mzx_ttt_decode(int code) {
    ExpertPos pos;
    pos.me = 0; pos.opp = 0; pos.env = MZX_TICTACTOE;
    for (int c = 0; c < 9; ++c) {
        const int d = code % 3;
        code /= 3;
        pos.me |= (uint64_t)(d == 1) << c;
        pos.opp |= (uint64_t)(d == 2) << c;
    }
    return pos;
}

// legal actions of a position that is not finished: bit a - 1 for action a
MZX_HD uint32_t mzx_legal(const ExpertPos& pos) {
    const uint64_t e = ~(pos.me | pos.opp);
    if (pos.env == MZX_TICTACTOE) return (uint32_t)(e & 0x1FFull);
    uint32_t m = 0;
    for (int h = 0; h < 7; ++h) m |= (uint32_t)((e >> (7 * h + 5)) & 1ull) << h;   // the column's top cell is empty
    return m;
}

MZX_HD bool mzx_ttt_line(uint64_t x) {
    const uint32_t v = (uint32_t)x;
    return (v & 0x007u) == 0x007u || (v & 0x038u) == 0x038u || (v & 0x1C0u) == 0x1C0u || (v & 0x049u) == 0x049u ||
           (v & 0x092u) == 0x092u || (v & 0x124u) == 0x124u || (v & 0x111u) == 0x111u || (v & 0x054u) == 0x054u;
}

// four in a row of stones x through the cell `bit` (c4_wins: vertical, horizontal, both diagonals)
MZX_HD uint64_t mzx_c4_runs(uint64_t x, int s) {        // the cells of x in a run of four along stride s
    const uint64_t t = x & (x >> s);
    const uint64_t q = t & (t >> (2 * s));                 // the lowest cell of every such run
    return q | (q << s) | (q << (2 * s)) | (q << (3 * s));
}
MZX_HD bool mzx_c4_four(uint64_t x, uint64_t bit) {
    return ((mzx_c4_runs(x, 1) | mzx_c4_runs(x, 7) | mzx_c4_runs(x, 8) | mzx_c4_runs(x, 6)) & bit) != 0;
}

// the mover (pos.me) plays legal action a0 (0-based); the position passes to
// the other player; *cell = the stone's bit; returns the outcome for the mover
MZX_HD int mzx_play(ExpertPos& pos, int a0, uint64_t* cell) {
    const uint64_t occ = pos.me | pos.opp;
    uint64_t bit;
    if (pos.env == MZX_TICTACTOE) {
        bit = 1ull << a0;
    } else {
        const uint64_t col = ~occ & (0x3Full << (7 * a0));
        bit = col & (0 - col);                             // the lowest empty cell of the column
    }
    const uint64_t mine = pos.me | bit;
    pos.me = pos.opp;
    pos.opp = mine;
    *cell = bit;
    const bool full = (occ | bit) == mzx_full(pos.env);
    if (pos.env == MZX_TICTACTOE) {
        if (mzx_ttt_line(pos.me)) return -1;               // Q14: the player now to move holds a line and wins
        return full ? 0 : MZX_CONT;
    }
    if (mzx_c4_four(mine, bit)) return 1;
    return full ? 0 : MZX_CONT;
}

MZX_HD void mzx_undo(ExpertPos& pos, uint64_t cell) {
    const uint64_t mine = pos.opp & ~cell;
    pos.opp = pos.me;
    pos.me = mine;
}

MZX_HD int mzx_action_of_cell(int env, int cell) { return env == MZX_TICTACTOE ? cell : cell / 7; }

// V(pos, d) of a position that is not finished, without recursion: the path's
// cells (6 bits a level) and the levels' running maxima (5 bits a level, biased
// by 16) live in two 64-bit words, so nothing is indexed dynamically
MZX_HD int mzx_value(ExpertPos pos, int d) {
    if (d <= 0) return 0;
    uint64_t path = 0, bests = 0;
    int level = 0, best = -16;
    int from = 0;                                          // first action (0-based) still to try at this level
    for (;;) {
        const uint32_t lg = mzx_legal(pos) & (0xFFFFFFFFu << from);
        if (!lg) {                                         // this level is done: hand -best to the parent
            if (level == 0) return best == -16 ? 0 : best;
            --level;
            const int cell = (int)((path >> (6 * level)) & 63ull);
            mzx_undo(pos, 1ull << cell);
            const int up = (int)((bests >> (5 * level)) & 31ull) - 16;
            best = up > -best ? up : -best;
            from = mzx_action_of_cell(pos.env, cell) + 1;
            continue;
        }
        const int a0 = __builtin_ctz(lg);
        uint64_t cell;
        const int out = mzx_play(pos, a0, &cell);
        const int rem = d - level;
        if (out != MZX_CONT || rem == 1) {
            const int sc = out == MZX_CONT ? 0 : out * rem;
            mzx_undo(pos, cell);
            best = best > sc ? best : sc;
            from = a0 + 1;
            continue;
        }
        path = (path & ~(63ull << (6 * level))) | ((uint64_t)__builtin_ctzll(cell) << (6 * level));
        bests = (bests & ~(31ull << (5 * level))) | ((uint64_t)(best + 16) << (5 * level));
        ++level;
        best = -16;
        from = 0;
    }
}

// score(pos, a, D) of action a (0-based) that is legal in pos
MZX_HD int mzx_score(ExpertPos pos, int a0, int D) {
    uint64_t cell;
    const int out = mzx_play(pos, a0, &cell);
    if (out != MZX_CONT) return out * D;
    return D == 1 ? 0 : -mzx_value(pos, D - 1);
}

// all A scores of a position that is not finished, MZX_ILLEGAL for an illegal action
MZX_HD void expert_scores(const ExpertPos& pos, int D, int32_t* out) {
    const uint32_t lg = mzx_legal(pos);
    const int A = mzx_actions(pos.env);
    for (int a0 = 0; a0 < A; ++a0) out[a0] = (lg >> a0) & 1u ? mzx_score(pos, a0, D) : MZX_ILLEGAL;
}
