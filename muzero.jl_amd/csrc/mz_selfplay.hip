// mz_selfplay.hip — device self-play loop body and device replay shard
// (SURVEY §8f-1, §8f-2).  One move of G lockstep games (play_game's loop body,
// SelfPlay.jl:343-380) is: mz_sp_prepare (observation append, stacked
// observations, legal mask, to_play) -> the batched search -> mz_sp_commit
// (env step, history append, finish test) -> mz_sp_order (ring slots of the
// finished games in slot order, replay counters) -> mz_sp_store (finished
// game -> replay ring, slot reset).  Nothing crosses PCIe.  MZ_OPP_NETWORK
// searches twice and mz_sp_pick chooses per slot before the commit.  mz_rp_sample is
// get_batch + make_target on the ring, writing an mz_batch in HBM.  The test
// worker plays its own slots with the same prepare / pick / commit
// in their one-game mode (S.frozen), between mz_test_begin and, per move,
// mz_test_tally in place of mz_sp_order / mz_sp_store.  The run log (DESIGN
// §21) folds the shard's new games, the learner's loss rows and the records
// with mz_log_games / mz_log_steps / mz_log_commit.
//
// Env rules: TicTacToe exactly as games/tictactoe/game.jl with quirk Q14 (the
// win test looks at the plane of the player TO MOVE; reward ±1 by the mover's
// id), Connect4 as games/connect4.py, the synthetic Atari-like env of
// configs[4] as games/atari_synth.py (Philox-keyed frames, one frame per move
// in the records, a four-frame stack as the observation).  Host mirrors:
// muzero.jl_amd/games/{tictactoe,connect4,atari_synth}.py, selfplay.py,
// replay_buffer.py.
#include "mz_internal.h"
#include "mz_selfplay_params.h"
#include "mz_replay_device.h"
#include "mz_env_device.h"

// ------------------------------------------------------------------- envs
// (ttt_line and the legal-action rule on a board: mz_env_device.h)
__device__ __forceinline__ bool c4_wins(const uint8_t* stones, int w, int h, int W, int H) {
    const int dw[4] = {1, 0, 1, 1}, dh[4] = {0, 1, 1, -1};
    for (int d = 0; d < 4; ++d) {
        int n = 1;
        for (int s = 1; s >= -1; s -= 2) {
            int ww = w + s * dw[d], hh = h + s * dh[d];
            while (ww >= 0 && ww < W && hh >= 0 && hh < H && stones[ww + W * hh]) {
                ++n;
                ww += s * dw[d];
                hh += s * dh[d];
            }
        }
        if (n >= 4) return true;
    }
    return false;
}

// ---- synthetic Atari-like env (games/atari_synth.py): the frame of key
// `key` (osz = 84·84 bytes = 441 Philox blocks of 16 bytes), written by the
// 64 lanes of one wave
__device__ void atari_frame(const SpParams& S, int g, uint32_t key, int lane) {
    uint4* f = reinterpret_cast<uint4*>(S.board + (size_t)g * S.osz);
    for (int j = lane; j < (S.osz >> 4); j += 64) {
        const mz_u32x4 r = mz_philox((uint32_t)j, key, 0u, MZ_RNG_FRAME, (uint32_t)S.seed, (uint32_t)(S.seed >> 32));
        f[j] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    }
}
// reset: key = u32(seed, ENV, global game id = game_offset + slot, step, ~0)
__device__ void atari_reset(const SpParams& S, int g, uint32_t step, int lane) {
    const uint32_t key = mz_rng_u32(S.seed, MZ_RNG_ENV, S.game_offset + (uint32_t)g, step, 0xFFFFFFFFu);
    atari_frame(S, g, key, lane);
    if (lane == 0) { S.ekey[g] = key; S.player[g] = 1; S.over[g] = 0; }
}

// legal actions (1..A) as a bit mask
__device__ uint32_t env_legal(const SpParams& S, int g) {
    return env_legal_board(S.env, S.board + (size_t)g * S.osz, S.player[g], S.env == MZ_ENV_CONNECT4 ? S.over[g] : 0,
                           S.W, S.H, S.A);
}

// env(action) (game.jl:45-52) + is_terminated / reward (:85-100): returns the
// reward recorded for the mover, sets *done
__device__ float env_step(const SpParams& S, int g, int a, bool* done) {
    uint8_t* b = S.board + (size_t)g * S.osz;
    const int p = S.player[g];
    if (S.env == MZ_ENV_TICTACTOE) {
        const int c = a - 1;
        b[18 + c] = 0;
        b[9 * (p - 1) + c] = 1;
        const int np = p % 2 + 1;
        S.player[g] = np;
        const bool win = ttt_line(b, np);
        bool full = true;
        for (int k = 0; k < 9; ++k) full &= b[18 + k] == 0;
        *done = full || win;
        return (*done && win) ? (p == 1 ? 1.0f : -1.0f) : 0.0f;
    }
    const int W = S.W, cells = S.W * S.H, h = a - 1;
    int w = 0;
    while (w < W && !b[2 * cells + w + W * h]) ++w;
    const int cell = w + W * h;
    b[2 * cells + cell] = 0;
    b[(p - 1) * cells + cell] = 1;
    const bool win = c4_wins(b + (p - 1) * cells, w, h, W, S.H);
    bool full = true;
    for (int k = 0; k < cells; ++k) full &= b[2 * cells + k] == 0;
    *done = win || full;
    S.over[g] = *done;
    S.player[g] = 3 - p;
    return win ? 1.0f : 0.0f;
}

// Winner of a finished game from its last move (0 = draw / unfinished).
// TicTacToe (Q14): the win test after a move looks at the plane of the player
// now to move, so a nonzero reward means THAT player (3 - mover) holds a line;
// Connect4: a nonzero reward is the mover's own four in a row.
__device__ __forceinline__ int game_winner(const SpParams& S, float last_reward, int last_mover) {
    if (last_reward == 0.0f) return 0;
    return S.env == MZ_ENV_TICTACTOE ? 3 - last_mover : last_mover;
}

__device__ void env_reset(const SpParams& S, int g, int lane) {
    if (S.env == MZ_ENV_ATARI) { atari_reset(S, g, S.step, lane); return; }
    uint8_t* b = S.board + (size_t)g * S.osz;
    const int cells = S.osz / 3;
    for (int k = lane; k < S.osz; k += 64) b[k] = k >= 2 * cells;
    if (lane == 0) { S.player[g] = 1; S.over[g] = 0; }
}

// ------------------------------------------------------------ self-play move
// one wave per game slot
extern "C" __global__ __launch_bounds__(256) void mz_sp_prepare(SpParams S) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) {                                 // test worker: the game is over, the dummy row
        for (int k = lane; k < S.F; k += 64) S.obs[(size_t)g * S.F + k] = 0.0f;
        for (int a = lane; a < S.A; a += 64) S.legal[(size_t)g * S.A + a] = 1;
        if (lane == 0) {
            S.tp[g] = 1;
            if (S.temp_g) S.temp_g[g] = 0.0f;
        }
        return;
    }
    const int t = S.hist.len[g];                                   // moves so far
    uint8_t* ho = S.hist.obs + ((size_t)g * S.T + t) * S.osz;     // observation_history append (:352)
    const uint8_t* b = S.board + (size_t)g * S.osz;
    for (int k = lane; k < S.osz; k += 64) ho[k] = b[k];
    if (S.frames)                                                  // the env's frame stack (same lanes wrote ho)
        frame_stack_obs(S.obs + (size_t)g * S.F, S.hist.obs + (size_t)g * S.T * S.osz, t + 1, S.osz, S.frames, lane);
    else
        stacked_obs(S.obs + (size_t)g * S.F, b, S.hist.obs + (size_t)g * S.T * S.osz, S.hist.act + (size_t)g * S.T,
                    t + 1, S.osz, S.P, S.stacked, lane);            // :355
    if (lane == 0) {
        const uint32_t m = env_legal(S, g);
        for (int a = 0; a < S.A; ++a) S.legal[(size_t)g * S.A + a] = (m >> a) & 1u;
        S.tp[g] = S.player[g];                                     // :351
        float tg = S.temperature;
        if (S.tgame) {                                             // one temperature per game (:396-407)
            if (t == 0) S.tgame[g] = S.temperature;
            tg = S.tgame[g];
        }
        if (S.temp_g)                                              // :344-346
            S.temp_g[g] = S.temp_threshold >= 0 && t >= S.temp_threshold ? 0.0f : tg;
    }
}

// MZ_OPP_NETWORK: both sides searched every slot; a slot whose
// mover is not muzero_player takes the opponent search's whole result, so
// mz_sp_commit records and plays the mover's own.  One wave per slot.
extern "C" __global__ __launch_bounds__(256) void mz_sp_pick(SpParams S, PickArgs X) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;
    if (S.player[g] == S.muzero_player) return;
    for (int a = lane; a < S.A; a += 64) X.cv[(size_t)g * S.A + a] = X.cv2[(size_t)g * S.A + a];
    if (lane == 0) { X.act[g] = X.act2[g]; X.rv[g] = X.rv2[g]; }
}

extern "C" __global__ __launch_bounds__(256) void mz_sp_commit(SpParams S) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= S.G) return;
    if (S.frozen && S.frozen[g]) return;                           // test worker: nothing of a finished game is recorded
    const int t = S.hist.len[g];
    const size_t r = (size_t)g * S.T + t;
    for (int a = lane; a < S.A; a += 64) S.hist.cv[r * S.A + a] = S.cv[(size_t)g * S.A + a];   // :375-379
    if (S.env == MZ_ENV_ATARI) {                                   // every lane steps the env (the frame is wave work)
        const int a = S.act[g];
        const uint32_t key = S.ekey[g];
        const mz_u32x4 v = mz_philox(0u, key, (uint32_t)a, MZ_RNG_ENV, (uint32_t)S.seed, (uint32_t)(S.seed >> 32));
        atari_frame(S, g, v.v[2], lane);
        if (lane == 0) {
            S.ekey[g] = v.v[2];
            S.hist.act[r] = a;
            S.hist.rew[r] = (int)mz_rng_below(v.v[0], (uint32_t)S.A) == a - 1 ? 1.0f : 0.0f;
            S.hist.tp[r] = S.player[g];
            S.hist.rv[r] = S.rv[g];
            S.hist.len[g] = t + 1;
            S.done[g] = (v.v[1] & 127u) == 0 || t + 1 > S.max_moves;
        }
        return;
    }
    if (lane == 0) {
        int a = S.act[g];
        const int mover = S.player[g];
        if (S.eval && S.opponent == MZ_OPP_RANDOM && mover != S.muzero_player) {   // :319-321
            uint32_t legal = 0;
            for (int b = 0; b < S.A; ++b) legal |= (uint32_t)(S.legal[(size_t)g * S.A + b] != 0) << b;
            const int n = __builtin_popcount(legal);
            if (n > 0) {
                const uint32_t r = mz_rng_u32(S.seed, MZ_RNG_OPPONENT, S.game_offset + (uint32_t)g, S.step, 0);
                uint32_t m = legal;
                for (int k = (int)mz_rng_below(r, (uint32_t)n); k > 0; --k) m &= m - 1;
                a = __builtin_ctz(m) + 1;
            }
        }
        bool done = false;
        const float rew = env_step(S, g, a, &done);                // :366-368
        S.hist.act[r] = a;
        S.hist.rew[r] = rew;
        S.hist.tp[r] = mover;
        S.hist.rv[r] = S.rv[g];
        S.hist.len[g] = t + 1;
        S.done[g] = done || t + 1 > S.max_moves;                  // :343 (> max_moves)
    }
}

// initial games of the synthetic Atari-like env (mz_selfplay_init's slots, at
// the first mz_selfplay_move: S.game_offset is that move's), one wave per slot
extern "C" __global__ __launch_bounds__(256) void mz_sp_reset(SpParams S) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g < S.G) atari_reset(S, g, S.reset_step, lane);
}

// ------------------------------------------------------------ test worker
// (mz_test_play): E test slots play one evaluation game each with
// the kernels above in their one-game mode (S.frozen).  mz_test_begin starts
// every slot's game as mz_selfplay_init plus the first move would (boards:
// empty, player 1; the Atari-like env: mz_sp_reset's draw) and opens the
// evaluation's record; one wave per slot.
extern "C" __global__ __launch_bounds__(256) void mz_test_begin(SpParams S, TestRec R) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x < 8)
        R.counts[threadIdx.x] = threadIdx.x == 0 ? R.training_step : threadIdx.x == 7 ? (long long)R.rng_step0 : 0ll;
    if (blockIdx.x == 0 && threadIdx.x < 3) R.sums[threadIdx.x] = 0.0;
    if (g >= S.G) return;
    if (S.env == MZ_ENV_ATARI) atari_reset(S, g, S.reset_step, lane);
    else env_reset(S, g, lane);
    if (lane == 0) { S.hist.len[g] = 0; S.done[g] = 0; R.frozen[g] = 0; }
}

// Behind mz_sp_commit, in place of mz_sp_order / mz_sp_store: the games that
// ended on this move go into the record and their slots freeze.  One
// workgroup, 1024 slots per pass.  Every lane sums its own game's records
// serially in f64 (+0, then + (double)x in record order); wave 0 then adds the
// finished games to the record in ascending slot order — a ballot per 64 slots
// finds them, every lane reads the same LDS entry, so each lane's chain of adds
// is the serial one and lane 0 stores it.  No float atomics: the host mirror
// (selfplay.evaluation_record) is exact.
extern "C" __global__ __launch_bounds__(1024) void mz_test_tally(SpParams S, TestRec R) {
    __shared__ double gs[3][1024];
    __shared__ int gi[3][1024];                    // 0 not finished | 1 MuZero won | 2 the opponent | 3 draw; length; MuZero's moves
    const int tid = threadIdx.x, lane = tid & 63;
    const bool every = S.opponent == MZ_OPP_SELF || R.players == 1;   // every record is MuZero's
    long long games = 0, won = 0, lost = 0, draws = 0, moves = 0, vmoves = 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (tid < 64) {
        games = R.counts[1]; won = R.counts[2]; lost = R.counts[3]; draws = R.counts[4];
        moves = R.counts[5]; vmoves = R.counts[6];
        s0 = R.sums[0]; s1 = R.sums[1]; s2 = R.sums[2];
    }
    for (int base = 0; base < S.G; base += 1024) {
        const int g = base + tid;
        int cls = 0, len = 0, vm = 0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (g < S.G && !R.frozen[g] && S.done[g]) {
            len = S.hist.len[g];                   // 1..T (mz_sp_commit)
            const size_t r0 = (size_t)g * S.T;
            for (int k = 0; k < len; ++k) {
                const float rew = S.hist.rew[r0 + k];
                if (every || S.hist.tp[r0 + k] == S.muzero_player) {
                    a0 = a0 + (double)rew;
                    a2 = a2 + (double)S.hist.rv[r0 + k];
                    ++vm;
                } else {
                    a1 = a1 + (double)rew;
                }
            }
            const int w = game_winner(S, S.hist.rew[r0 + len - 1], S.hist.tp[r0 + len - 1]);
            cls = w == 0 ? 3 : w == S.muzero_player ? 1 : 2;
            R.frozen[g] = 1;
        }
        gs[0][tid] = a0; gs[1][tid] = a1; gs[2][tid] = a2;
        gi[0][tid] = cls; gi[1][tid] = len; gi[2][tid] = vm;
        __syncthreads();
        if (tid < 64) {
            for (int ch = 0; ch < 1024 && base + ch < S.G; ch += 64) {
                uint64_t m = __ballot(gi[0][ch + lane] != 0);
                while (m) {
                    const int k = ch + __builtin_ctzll(m);
                    m &= m - 1;
                    const int c = gi[0][k];
                    games += 1; won += c == 1; lost += c == 2; draws += c == 3;
                    moves += gi[1][k]; vmoves += gi[2][k];
                    s0 = s0 + gs[0][k]; s1 = s1 + gs[1][k]; s2 = s2 + gs[2][k];
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        R.counts[1] = games; R.counts[2] = won; R.counts[3] = lost; R.counts[4] = draws;
        R.counts[5] = moves; R.counts[6] = vmoves;
        R.sums[0] = s0; R.sums[1] = s1; R.sums[2] = s2;
    }
}

// ------------------------------------------------------------ run log
// (mz_train_set_log).  mz_log_games, behind mz_sp_store of a
// training move: the shard games numbered max(logged_upto, played - held) + 1
// .. played go into the accumulators (game n lives in ring slot (n - 1) mod
// cap); the games between logged_upto and that range were evicted unseen and
// count as missed.  One workgroup, 1024 games per pass.  Every thread sums its
// own game serially in f64 (+0, then + (double)x in record order); thread 0
// then adds the pass's games in ascending game number.  No float atomics: the
// host mirror (learning.run_log_record) is exact.
extern "C" __global__ __launch_bounds__(1024) void mz_log_games(SpParams S, LogAcc* acc) {
    __shared__ double gs[3][1024];
    __shared__ int gi[2][1024];                    // 0 player 1 won | 1 player 2 | 2 draw; length
    const int tid = threadIdx.x;
    const long long played = S.counters[0];
    const long long held = played < S.cap ? played : S.cap;
    const long long upto = acc->logged_upto;
    if (upto >= played) {                          // nothing new
        if (tid == 0) acc->logged_upto = played;
        return;
    }
    const long long oldest = played - held;        // the newest game number no longer held
    const long long first = (upto > oldest ? upto : oldest) + 1;
    const long long n = played - first + 1;        // 1..cap
    long long games = 0, moves = 0, w0 = 0, w1 = 0, w2 = 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (tid == 0) {
        games = acc->games; moves = acc->moves; w0 = acc->wins[0]; w1 = acc->wins[1]; w2 = acc->wins[2];
        s0 = acc->gsum[0]; s1 = acc->gsum[1]; s2 = acc->gsum[2];
    }
    for (long long base = 0; base < n; base += 1024) {
        const long long k = base + tid;
        int cls = 2, len = 0;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (k < n) {
            const int slot = (int)((first + k - 1) % S.cap);
            len = S.ring.len[slot];
            len = len < 0 ? 0 : len > S.T ? S.T : len;
            const size_t r0 = (size_t)slot * S.T;
            for (int j = 0; j < len; ++j) {
                a0 = a0 + (double)S.ring.rew[r0 + j];
                a1 = a1 + (double)S.ring.rv[r0 + j];
                const float* cv = S.ring.cv + (r0 + j) * S.A;
                float mx = cv[0];
                for (int a = 1; a < S.A; ++a) mx = cv[a] > mx ? cv[a] : mx;
                a2 = a2 + (double)mx;
            }
            const int w = len > 0 ? game_winner(S, S.ring.rew[r0 + len - 1], S.ring.tp[r0 + len - 1]) : 0;
            cls = w == 1 ? 0 : w == 2 ? 1 : 2;
        }
        gs[0][tid] = a0; gs[1][tid] = a1; gs[2][tid] = a2;
        gi[0][tid] = cls; gi[1][tid] = len;
        __syncthreads();
        if (tid == 0) {
            const int m = (int)(n - base < 1024 ? n - base : 1024);
            for (int j = 0; j < m; ++j) {
                const int c = gi[0][j];
                games += 1; moves += gi[1][j]; w0 += c == 0; w1 += c == 1; w2 += c == 2;
                s0 = s0 + gs[0][j]; s1 = s1 + gs[1][j]; s2 = s2 + gs[2][j];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        acc->games = games; acc->moves = moves; acc->wins[0] = w0; acc->wins[1] = w1; acc->wins[2] = w2;
        acc->gsum[0] = s0; acc->gsum[1] = s1; acc->gsum[2] = s2;
        acc->missed += first - 1 - upto;
        acc->logged_upto = played;
    }
}

// Behind a learner chunk: its n <= 256 loss rows, in ascending step, into the
// six sums; the last row is kept.  One wave, lane j < 6 owns loss j.
extern "C" __global__ __launch_bounds__(64) void mz_log_steps(LogArgs L) {
    const int j = threadIdx.x;
    if (L.n < 1) return;
    if (j < 6) {
        double s = L.acc->loss[j];
        for (int i = 0; i < L.n; ++i) s = s + (double)L.rows[8 * i + j];
        L.acc->loss[j] = s;
        L.acc->last[j] = (double)L.rows[8 * (L.n - 1) + j];
    }
    if (j == 6) L.acc->steps += L.n;
}

// One record from the accumulators and the shard's counters as they stand at
// this point of the stream (layout: mz.h); the accumulators start over,
// logged_upto stays.  One thread per word of the record.
extern "C" __global__ __launch_bounds__(64) void mz_log_commit(LogArgs L) {
    const int i = threadIdx.x;
    LogAcc* a = L.acc;
    long long c = 0;
    double s = 0.0;
    if (i < 16) {
        const long long played = L.counters[0];
        switch (i) {
            case 0: c = L.t1; break;
            case 1: c = a->steps; break;
            case 2: c = played; break;
            case 3: c = L.counters[1]; break;
            case 4: c = L.counters[2]; break;
            case 5: c = played < L.cap ? played : L.cap; break;
            case 6: c = L.counters[3]; break;
            case 7: c = a->games; break;
            case 8: c = a->moves; break;
            case 9: case 10: case 11: c = a->wins[i - 9]; break;
            case 12: c = L.refreshes; break;
            case 13: c = a->missed; break;
            default: break;
        }
        s = i < 6 ? a->loss[i] : i < 12 ? a->last[i - 6] : i == 12 ? L.eta : a->gsum[i - 13];
    }
    __syncthreads();                               // every word is read before the accumulators are zeroed
    if (i < 16) { L.counts[i] = c; L.sums[i] = s; }
    if (i < 6) { a->loss[i] = 0.0; a->last[i] = 0.0; }
    if (i < 3) { a->wins[i] = 0; a->gsum[i] = 0.0; }
    if (i == 0) { a->steps = 0; a->games = 0; a->moves = 0; a->missed = 0; }
}

// Ring slots of this move's finished games in slot order (the host driver
// saves them in ascending slot order) and the replay counters (save_game,
// ReplayBuffer.jl:133-161).  One workgroup.
extern "C" __global__ __launch_bounds__(1024) void mz_sp_order(SpParams S) {
    __shared__ int cnt[1024];
    __shared__ long long red[3][1024];
    const int tid = threadIdx.x, per = (S.G + 1023) / 1024;
    const int g0 = tid * per, g1 = min(S.G, g0 + per);
    int n = 0;
    for (int g = g0; g < g1; ++g) n += S.done[g] != 0;
    cnt[tid] = n;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                           // inclusive scan
        const int v = tid >= o ? cnt[tid - o] : 0;
        __syncthreads();
        cnt[tid] += v;
        __syncthreads();
    }
    if (S.eval) {                                                   // tally; nothing is saved
        long long t[4] = {0, 0, 0, 0};
        for (int g = g0; g < g1; ++g) {
            S.ring_pos[g] = -1;
            if (!S.done[g]) continue;
            const size_t last = (size_t)g * S.T + S.hist.len[g] - 1;
            const int w = game_winner(S, S.hist.rew[last], S.hist.tp[last]);
            t[0] += 1;
            t[w == 0 ? 3 : w == S.muzero_player ? 1 : 2] += 1;
        }
        for (int k = 0; k < 4; ++k)                                 // integer sums: any order is exact
            if (t[k]) atomicAdd(reinterpret_cast<unsigned long long*>(S.eval_counts + k), (unsigned long long)t[k]);
        return;
    }
    const long long played = S.counters[0];
    long long rank = cnt[tid] - n, steps = 0, evicted = 0;
    for (int g = g0; g < g1; ++g) {
        if (!S.done[g]) { S.ring_pos[g] = -1; continue; }
        const long long num = played + rank + 1;                   // game number (1-based)
        const int slot = (int)((num - 1) % S.cap);
        const int len = S.hist.len[g];
        if (num > S.cap) evicted += S.ring.len[slot];              // the game it replaces
        S.ring_pos[g] = slot;
        steps += len;
        ++rank;
    }
    red[0][tid] = n; red[1][tid] = steps; red[2][tid] = evicted;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        S.counters[0] = played + red[0][0];
        S.counters[1] += red[1][0];
        S.counters[2] += red[1][0] - red[2][0];
    }
}

// finished game -> its ring slot; the slot starts a new game (one workgroup per slot)
extern "C" __global__ __launch_bounds__(256) void mz_sp_store(SpParams S) {
    const int g = blockIdx.x;
    if (!S.done[g]) return;
    const int slot = S.ring_pos[g], len = S.hist.len[g], tid = threadIdx.x;
    const size_t src = (size_t)g * S.T, dst = (size_t)(slot < 0 ? 0 : slot) * S.T;
    if (slot < 0) {                                // evaluation: the slot just restarts
        __syncthreads();
        if (tid == 0) { S.hist.len[g] = 0; S.done[g] = 0; }
        if (tid < 64) env_reset(S, g, tid);
        return;
    }
    for (int k = tid; k < len * S.osz; k += blockDim.x) S.ring.obs[dst * S.osz + k] = S.hist.obs[src * S.osz + k];
    for (int k = tid; k < len * S.A; k += blockDim.x) S.ring.cv[dst * S.A + k] = S.hist.cv[src * S.A + k];
    for (int k = tid; k < len; k += blockDim.x) {
        S.ring.act[dst + k] = S.hist.act[src + k];
        S.ring.rew[dst + k] = S.hist.rew[src + k];
        S.ring.tp[dst + k] = S.hist.tp[src + k];
        S.ring.rv[dst + k] = S.hist.rv[src + k];
    }
    __syncthreads();                               // every thread has read len and done
    if (S.per) {                                   // save_game's initial priorities (:136-143)
        SpHist ring = S.ring;
        per_init_slot(ring, slot, len, S.T, S.td, S.disc_pow, S.per_alpha, tid, blockDim.x);
        __syncthreads();
        if (tid == 0) per_game_max(ring, slot, len, S.T);
    }
    // the game that held the slot may have been reanalysed: this one starts as `nothing`
    if (tid == 0) { S.ring.len[slot] = len; S.ring.rean[slot] = 0; S.hist.len[g] = 0; S.done[g] = 0; }
    if (tid < 64) env_reset(S, g, tid);
}

// ------------------------------------------------------------------- PER
// initial priorities of one ring slot written by mz_replay_save_game
extern "C" __global__ void mz_rp_per_init(SpHist ring, int slot, int len, int Tmax, int td, const float* disc_pow,
                                          int alpha) {
    per_init_slot(ring, slot, len, Tmax, td, disc_pow, alpha, threadIdx.x, blockDim.x);
    __syncthreads();
    if (threadIdx.x == 0) per_game_max(ring, slot, len, Tmax);
}

// sample_n_games' game probabilities (:91-99): the held games oldest first
// (the Dict's game-number order), p_i = gprio_i / S with S the ascending f32
// sum, cum_i the ascending f32 running sum of p; total_samples = Σ len.  One
// lane: the f32 sums are sequential by definition.
extern "C" __global__ void mz_rp_per_prep(SpHist ring, const long long* counters, int cap, float* cum, float* prob,
                                          long long* total) {
    if (threadIdx.x != 0) return;
    const long long played = counters[0];
    const int n = (int)(played < cap ? played : cap);
    const long long oldest = played - n + 1;
    float S = 0.0f;
    long long tot = 0;
    for (int i = 0; i < n; ++i) {
        const int slot = (int)((oldest + i - 1) % cap);
        S = S + ring.gprio[slot];
        tot += ring.len[slot];
    }
    float c = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float p = ring.gprio[(int)((oldest + i - 1) % cap)] / S;
        c = c + p;
        prob[i] = p;
        cum[i] = c;
    }
    *total = tot;
}

// weight_batch ./= maximum(weight_batch) (:215)
extern "C" __global__ void mz_rp_per_norm(float* w, int B) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int i = tid; i < B; i += blockDim.x) m = w[i] > m ? w[i] : m;
    red[tid] = m;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
        __syncthreads();
    }
    const float mx = red[0];
    for (int i = tid; i < B; i += blockDim.x) w[i] = w[i] / mx;
}

// update_priorities! (ReplayBuffer.jl:168-183, Learning.jl:400-404) in its
// intended reading (the reference's `minimum(a, b)` and its K+2-element slice
// cannot run): for sample i in batch order, if game index[i] is still held,
// positions pos..min(pos+K, len) get |pv − tv|^alpha of steps 0.., then the
// game priority is their max.  Samples run in order (later ones overwrite),
// lanes over the steps of one sample.
extern "C" __global__ void mz_rp_per_update(SpHist ring, const long long* counters, int cap, int Tmax, int B, int K,
                                            int alpha, const int32_t* index, const float* pv, const float* tv) {
    const int lane = threadIdx.x;
    const long long played = counters[0];
    const long long held_from = played - (played < cap ? played : cap) + 1;
    for (int i = 0; i < B; ++i) {
        const long long num = index[2 * i];
        const int pos = index[2 * i + 1];
        if (num < held_from) continue;                     // evicted since it was sampled
        const int slot = (int)((num - 1) % cap), len = ring.len[slot];
        const int end = pos + K < len ? pos + K : len;     // 1-based, inclusive
        float* pr = ring.prio + (size_t)slot * Tmax;
        for (int k = pos + lane; k <= end; k += blockDim.x)
            pr[k - 1] = per_priority(pv[(size_t)i * (K + 1) + (k - pos)] - tv[(size_t)i * (K + 1) + (k - pos)], alpha);
        __syncthreads();
        if (lane == 0) per_game_max(ring, slot, len, Tmax);
        __syncthreads();
    }
}

// ------------------------------------------------------------- replay sample
// one wave per sample (get_batch, :188-217); the body is shared with the
// fused sample + unroll kernel (mz_replay_device.h)
extern "C" __global__ __launch_bounds__(256) void mz_rp_sample(RpSampleParams Q) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b < Q.B) rp_sample_one(Q, b, lane);
}

// mz_batch_symmetry: row b of a batch under element sym[b] of the env's group, one wave per row, through
// the sampler's row transform (sym_put_board / sym_action / sym_put_pol of mz_replay_device.h); an id
// outside 0..n-1 copies the row and reads no table
extern "C" __global__ __launch_bounds__(256) void mz_rp_symmetry(RpSymParams Y) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= Y.B) return;
    const int K1 = Y.K + 1, A = Y.A;
    const int s = __builtin_amdgcn_readfirstlane(Y.sym[b]);
    const bool on = (unsigned)s < (unsigned)Y.n;
    const int32_t* cp = Y.cell + (size_t)(on ? s : 0) * Y.P;
    const int32_t* ap = Y.act + (size_t)(on ? s : 0) * A;
    const float* x = Y.obs + (size_t)b * Y.F;
    float* y = Y.o_obs + (size_t)b * Y.F;
    const float* pi = Y.tpol + (size_t)b * K1 * A;
    float* po = Y.o_tpol + (size_t)b * K1 * A;
    if (on) {
        // the row is a run of planes of P cells (Q15): C board planes per observation, one action plane
        // (the raw id in every cell, 0 in the all-zero block before the first move) before each past one
        const int blk = (Y.C + 1) * Y.P;
        sym_put_board(y, x, Y.C, Y.P, cp, lane);
        for (int o = Y.C * Y.P; o + blk <= Y.F; o += blk) {
            for (int c = lane; c < Y.P; c += 64) y[o + cp[c]] = sym_action(ap, A, x[o + c]);
            sym_put_board(y + o + Y.P, x + o + Y.P, Y.C, Y.P, cp, lane);
        }
        for (int e = lane; e < K1 * A; e += 64) sym_put_pol(po, e, pi[e], A, ap);
    } else {
        for (int f = lane; f < Y.F; f += 64) y[f] = x[f];
        for (int e = lane; e < K1 * A; e += 64) po[e] = pi[e];
    }
    for (int k = lane; k < K1; k += 64) {
        const float a = Y.actions[(size_t)b * K1 + k];
        Y.o_actions[(size_t)b * K1 + k] = on ? sym_action(ap, A, a) : a;
        Y.o_tv[(size_t)b * K1 + k] = Y.tv[(size_t)b * K1 + k];
        Y.o_tr[(size_t)b * K1 + k] = Y.tr[(size_t)b * K1 + k];
    }
    if (lane == 0) {
        Y.o_gscale[b] = Y.gscale[b];
        if (Y.weights) Y.o_weights[b] = Y.weights[b];
    }
}
