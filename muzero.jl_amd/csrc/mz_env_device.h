// mz_env_device.h — the board envs' rules that read nothing but a board: one
// definition for device self-play (mz_selfplay.hip, the live board of a slot)
// and for the reanalyse search (mz_reanalyse.hip, the board bytes stored with
// a position).  Boards are 0/1 bytes, planes [p1, p2, empty], col-major cells.
#pragma once
#include "mz_internal.h"

static __constant__ int8_t c_ttt_lines[8][3] = {{0, 3, 6}, {1, 4, 7}, {2, 5, 8}, {0, 1, 2},
                                                 {3, 4, 5}, {6, 7, 8}, {0, 4, 8}, {6, 4, 2}};

// TicTacToe (game.jl:102-115, Q14): a line on the plane of player p
__device__ __forceinline__ bool ttt_line(const uint8_t* b, int p) {
    const uint8_t* pl = b + 9 * (p - 1);
    bool any = false;
#pragma unroll
    for (int l = 0; l < 8; ++l) any |= pl[c_ttt_lines[l][0]] && pl[c_ttt_lines[l][1]] && pl[c_ttt_lines[l][2]];
    return any;
}

// legal actions (1..A) of `player` on board b as a bit mask; `over`: the game
// has ended (Connect4 keeps it beside the board; TicTacToe reads it off the
// board, Q14)
__device__ __forceinline__ uint32_t env_legal_board(int env, const uint8_t* b, int player, int over, int W, int H,
                                                    int A) {
    uint32_t m = 0;
    if (env == MZ_ENV_ATARI) return A >= 32 ? 0xFFFFFFFFu : (1u << A) - 1u;
    if (env == MZ_ENV_TICTACTOE) {                      // game.jl:37-43
        if (ttt_line(b, player)) return 0;
        for (int c = 0; c < 9; ++c) m |= (uint32_t)b[18 + c] << c;
    } else {
        if (over) return 0;
        const int cells = W * H;
        for (int h = 0; h < H; ++h) m |= (uint32_t)b[2 * cells + (W - 1) + W * h] << h;
    }
    return m;
}
