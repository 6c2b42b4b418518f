// mz_selfplay_params.h — device self-play and the device
// replay shard (§8f-2): parameters shared by the host (mz_engine.hip) and the
// kernels (mz_selfplay.hip).
//
// Per game slot g (G slots played in lockstep, SelfPlay.jl:330-382):
//   env      board[g][osz] (0/1 bytes: planes [p1, p2, empty], col-major cells),
//            player[g] (1 or 2), over[g]; the synthetic Atari-like env
//            (frames = 4): board[g] = the current 84x84 frame, ekey[g] its key;
//   history  GameHistory (Constructors.jl:6-16) of the game in progress, up to
//            T = max_moves + 1 moves: obs[g][T][osz] bytes (one frame per move
//            when frames > 0: the observation stacks the last `frames`), act / rew / tp /
//            rv [g][T], cv [g][T][A], len[g] = moves recorded.
// Replay shard (ReplayBuffer.jl:133-161, PER = false): a FIFO ring of `cap`
// finished games with the same per-game layout; game number n (1-based, the
// Dict key of save_game) lives in ring slot (n - 1) mod cap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct SpHist {                 // a set of game records: [n][T] ...
    uint8_t* obs;               // [n][T][osz]
    int32_t* act;               // [n][T] 1-based actions
    float* rew;                 // [n][T]
    int32_t* tp;                // [n][T] to_play before the move
    float* cv;                  // [n][T][A] child visit distributions
    float* rv;                  // [n][T] root values
    int32_t* len;               // [n] moves
    float* prio;                // [n][T] PER position priorities (ring only, conf.PER)
    float* gprio;               // [n] PER game priority = max(prio) (ring only)
    // Reanalyse (ReplayBuffer.jl:8, 56-67; mz_reanalyse.hip), ring only (null in `hist`)
    float* rrv;                 // [n][T] reanalysed_predicted_root_values
    int32_t* rean;              // [n] bit mask, 0 = `nothing`: bit 1 = rrv, bit 2 = rcv hold the slot's whole game
    float* rcv;                 // [n][T][A] reanalysed child_visits (mz_replay_reanalyse_search; null before its first call)
};

enum { MZ_REAN_VALUES = 1, MZ_REAN_POLICIES = 2 };                  // SpHist.rean bits
enum { MZ_REAN_DEAD = 0, MZ_REAN_LIVE = 1, MZ_REAN_EMPTY = 2 };     // ReanParams.stage_state

// mz_replay_reanalyse on the shard's games first .. first+count-1 (0 = oldest
// held; games past the held range are skipped on the device)
struct ReanParams {
    int first, count;           // count < 0: every held game
    int T, osz, P, F, stacked, cap;
    SpHist ring;
    long long* counters;        // [0] num_played_games (read), [3] num_reanalysed_games (bumped once per game)
    // FC engines (mz_reanalyse_fc): the root plan on the tile16 images
    const int* plan_root; const float* Wp; const float* Bp;
    int x_rep, v_out, v_act, lds_total;
    // ResNet engines: positions [p0, p0 + pn) of the flattened (game, pos) grid, T per game
    int p0, pn;
    float* stage_x;             // [pn][F] gathered stacked observations
    const float* stage_v;       // [pn] value-head outputs
    // mz_replay_reanalyse_search: rows [p0, p0 + pn) of the same grid are the games of one batched
    // search (stage_x = its obs); the env rules of mz_env_device.h rebuild each row's legal mask
    int env, W, H, A, players;
    uint8_t* stage_legal;       // [pn][A]
    int32_t* stage_tp;          // [pn]
    int32_t* stage_state;       // [pn] MZ_REAN_DEAD (pos >= len, or past the held range), _LIVE, _EMPTY (no legal action)
    const float* stage_cv;      // [pn][A] the search's child_visits
    const float* stage_rv;      // [pn] the search's root_value
    // mz_replay_reanalyse_next: a round's packed rows.  null: the grid above.  Set: row p is the
    // (ring slot, 0-based pos) pair rows[p] that mz_reanalyse_pack wrote, dead from n_rows =
    // counters[MZ_REAN_HDR + 2] on; first / count are not read.  R = the round's capacity in rows.
    const int32_t* rows;        // [R][2]
    int R;
};

// the words behind the shard's four counters: the reanalyse cursor (the game number, in save_game's
// 1-based numbering, of the next game mz_replay_reanalyse_next takes) and the last round's header
// {first game number, games taken, n_rows}
enum { MZ_REAN_CURSOR = 4, MZ_REAN_HDR = 5, MZ_SP_COUNTERS = 8 };

struct SpParams {
    int G, env, W, H, osz, P, A, F, stacked, T, max_moves;
    int frames;                 // > 0: the env stacks its last `frames` frames (atari_synth), 0: board games
    uint8_t* board; int32_t* player; uint8_t* over;
    uint32_t* ekey;             // [G] synthetic Atari-like env state
    uint32_t reset_step;        // mz_sp_reset: the step key of the initial games
    SpHist hist;                // [G] games in progress
    SpHist ring;                // [cap] replay shard
    int cap;
    long long* counters;        // [0] num_played_games, [1] num_played_steps, [2] total_samples
    // search io (device buffers of the engine)
    float* obs; uint8_t* legal; int32_t* tp; const float* cv; const float* rv; const int32_t* act;
    int32_t* done;              // [G] finished this move
    int32_t* ring_pos;          // [G] ring slot of the finished game
    // evaluation play (competitive_play!, SelfPlay.jl:421-435): finished games
    // are tallied, not saved; with opponent = MZ_OPP_RANDOM the moves of the
    // player != muzero_player are uniform legal actions (select_opponent_action
    // :311-325) from the Philox OPPONENT stream keyed (game id, move step)
    int eval, opponent, muzero_player;
    uint32_t step, game_offset;
    uint64_t seed;
    long long* eval_counts;     // [4] games, muzero wins, opponent wins, draws
    // PER (conf.PER): initial priorities of a stored game (save_game, ReplayBuffer.jl:133-145)
    int per, per_alpha, td;
    const float* disc_pow;
    // temperature_threshold (SelfPlay.jl:344-346): a game with >= temp_threshold
    // moves recorded plays at temperature 0 (-1 = nothing: every slot at `temperature`)
    float temperature; int temp_threshold; float* temp_g;   // temp_g [G]
    // actor-learner loop (mz_train_run): each game keeps the temperature of its first move,
    // as play_game(env, temperature, ...) takes it once per game (SelfPlay.jl:396-407);
    // tgame [G] holds it (nullptr: every move uses `temperature`)
    float* tgame;
    // the test worker's one-game mode (mz_test_play): frozen[g] != 0 marks a slot whose
    // game of this evaluation has ended.  Its search row is the dummy row of mz_reanalyse_sgather
    // (zero observation, every action legal, to_play 1) and mz_sp_commit / mz_expert_move / mz_sp_pick
    // leave it alone.  nullptr (every other launch): no slot is frozen.
    const int32_t* frozen;
};

// mz_test_begin / mz_test_tally (mz_selfplay.hip): the evaluation's record in the handle's ring
struct TestRec {
    long long* counts;          // [8] training_step, games, muzero wins, opponent wins, draws, moves, value_moves,
                                //     rng_step0
    double* sums;               // [3] reward_muzero, reward_opponent, value_sum
    long long training_step;    // mz_test_begin stamps these two
    uint32_t rng_step0;
    int32_t* frozen;            // [G] the slots' flags (SpParams::frozen, writable)
    int players;                // conf.players: with 1 every record is MuZero's
};

// The run log (mz_log_games / mz_log_steps / mz_log_commit in mz_selfplay.hip): the
// device accumulators between two records.  Sums and counts, never means.
struct LogAcc {
    long long steps;            // learner steps folded
    long long games, moves;     // shard games folded, Σ length
    long long wins[3];          // player 1, player 2, draws (game_winner on the last record)
    long long missed;           // games that entered the shard and left it before a fold reached them
    long long logged_upto;      // the highest game number already folded (mz_log_commit keeps it)
    double loss[6];             // Σ (double) of {value, reward, policy, l2_repr, l2_pred, l2_dyn}, ascending step
    double last[6];             // the same six of the last folded step
    double gsum[3];             // Σ rewards, Σ root values, Σ_positions max_a child_visits[a]
};

struct LogArgs {
    LogAcc* acc;
    // mz_log_steps: n loss rows of 8 floats (the first six are the losses), ascending step
    const float* rows; int n;
    // mz_log_commit: the record's ring slot, the shard's counters, and the host's words
    long long* counts;          // [16]
    double* sums;               // [16]
    const long long* counters;  // [MZ_SP_COUNTERS]
    int cap;
    long long t1, refreshes;
    double eta;
};

// mz_expert_move (mz_expert.hip): the rules-search expert opponent.  The rows are SpParams'
// (G, env, A, osz, board, player; in self-play mode also muzero_player, seed, step, game_offset).
struct ExpertArgs {
    int depth;                  // D, 1..9
    int32_t* act;               // self-play mode (scores == null): [G] the search's actions; the rows whose
                                // mover is not muzero_player get the expert's
    int32_t* scores;            // eval mode: [G][A] score(s, a, D) of every row, -128 for an illegal action
    // mz_expert_table_move only: the solved TicTacToe table, [19683] entries of 16 bytes,
    // the first nine of each = score(s, a, 9) as int8 (mz_expert_rules.h: mzx_ttt_code)
    const int8_t* table;
    // judge mode, self-play mode only; null in every launch outside a judging evaluation
    // and mz_expert_judge: the audit row {moves judged, in the best set, outcome given away, score
    // deficit}.  MuZero's rows (mover == muzero_player, every row with MZ_OPP_SELF) add the four terms
    // of act[g]; the other rows get the expert's move only with MZ_OPP_EXPERT.
    long long* judge;
};

// mz_mcts_move (mz_mcts_opp.hip): the rules-MCTS opponent.  The rows are SpParams' (G, env,
// A, osz, board, player, seed, step, game_offset; in self-play mode also muzero_player, frozen).
struct MctsArgs {
    int sims, rollouts;         // S 1..1024, R 1..64
    int games;                  // rows (waves) per workgroup: the grid is ceil(G / games) blocks of 64 * games lanes,
                                // each wave with (S + 1) * A edge records of dynamic LDS
    const double* sqrt_tab;     // [S + 1] IEEE sqrt(k), built on the host
    int32_t* act;               // self-play mode (n == null): [G] the search's actions; the rows whose mover is
                                // not muzero_player get the opponent's
    int32_t* n; int32_t* w;     // eval mode: [G][A] the root's statistics, n = -1 (w = 0) for an illegal action
};

// mz_sp_pick (mz_selfplay.hip): MZ_OPP_NETWORK's choice between the two searches of one move.
// The rows are SpParams' (G, A, player, muzero_player).
struct PickArgs {
    float* cv; float* rv; int32_t* act;                         // [G][A], [G], [G] the engine's nets' search; the rows
                                                                // whose mover is not muzero_player get ...
    const float* cv2; const float* rv2; const int32_t* act2;    // ... the opponent's nets' search of the same rows
};

// mz_prior_fc / mz_prior_pick (mz_prior.hip): the network-only player.  Row g's result
// (π, v, action) goes where a search row has its visit fractions, root value and action.
struct PriorParams {
    int G, A, obs_feat;
    uint32_t rng_step, game_offset;
    uint64_t seed;
    float temperature;
    const float* temp_g;        // [G] per-row temperatures (self-play temperature_threshold) or null
    const float* obs;           // mz_prior_fc: [G][obs_feat] stacked observations
    const uint8_t* legal;       // [G][A]
    float* policy; float* value; int32_t* action;               // [G][A], [G], [G] (1-based)
    // mz_prior_fc: the root plan (representation, then prediction from h_out) on the tile16 images
    const int* plan_root; const float* Wp; const float* Bp;
    int x_rep, v_out, p_out, v_act, lds_total;
    // mz_prior_pick: what the two mz_rnet_forward_kernel launches wrote
    const float* p;             // [G][A] the policy head's softmax
    const float* v;             // [G] the value head's output
};

// get_batch + make_target (ReplayBuffer.jl:5-50, 73-107, 188-217) on the shard
struct RpSampleParams {
    int B, K, A, osz, P, F, stacked, T, td, cap;
    int frames;                 // the env's frame stack (0: stacked observations, Q15)
    // board symmetry (mz_replay_set_symmetry): sample b is written under element
    // s_b = rng_below(SYMMETRY stream (b, step), sym_n) of the env's group.  The three fields sit in
    // the struct's alignment holes, so every kernel argument keeps its offset (§23's resource table);
    // the tables follow disc_pow in its buffer, named by their offsets from it in 4-byte words
    int sym_n;                  // the group's order, 0: off
    uint64_t seed; uint32_t step;
    int sym_cell;               // [sym_n][P] at (int32_t*)disc_pow + sym_cell: cell c moves to [s][c]
    SpHist ring;
    const long long* counters;
    const float* disc_pow;      // [td + 2]: f32(discount^n) as Julia's Float32^Int
    float* obs; float* actions; float* tv; float* tr; float* tpol; float* gscale;
    int32_t* index;             // [B][2]: (game number, position) — index_batch
    // PER (conf.PER): sample_n_games / sample_position by priority (:73-107)
    // from the cumulative game probabilities of mz_rp_per_prep; raw IS weights
    // 1/(total_samples·p_game·p_pos), normalised by mz_rp_per_norm (:211-215)
    int per;
    int sym_act;                // [sym_n][A] at (int32_t*)disc_pow + sym_act: 0-based action a becomes [s][a]
    const float* per_cum;       // [n held] cumulative f32 game probabilities (oldest first)
    const float* per_p;         // [n held] game probabilities
    const long long* per_total; // total_samples of the held games
    float* weights;             // [B]
};
static_assert(sizeof(RpSampleParams) == 272, "RpSampleParams: the symmetry fields belong in the alignment holes");

// mz_rp_symmetry (mz_selfplay.hip): mz_batch_symmetry's transform of a device batch, row b under
// element sym[b] of the group (an id outside 0..n-1: the row is copied)
struct RpSymParams {
    int B, K, A, P, C, F;       // C = board planes of one observation (osz / P)
    int n;
    const int32_t* cell; const int32_t* act;                    // the tables: [n][P], [n][A]
    const int32_t* sym;         // [B]
    const float* obs; const float* actions; const float* tv; const float* tr; const float* tpol;
    const float* gscale; const float* weights;                  // weights: null without PER
    float* o_obs; float* o_actions; float* o_tv; float* o_tr; float* o_tpol; float* o_gscale; float* o_weights;
};

// ---- kernel prototypes (mz_selfplay.hip, mz_reanalyse.hip)
extern "C" __global__ void mz_sp_prepare(SpParams S);
extern "C" __global__ void mz_sp_commit(SpParams S);
extern "C" __global__ void mz_sp_order(SpParams S);
extern "C" __global__ void mz_sp_store(SpParams S);
extern "C" __global__ void mz_sp_reset(SpParams S);
extern "C" __global__ void mz_expert_move(SpParams S, ExpertArgs X);
extern "C" __global__ void mz_expert_table_move(SpParams S, ExpertArgs X);
extern "C" __global__ void mz_expert_table_rows(uint8_t* boards, int32_t* players, int c0, int n);
extern "C" __global__ void mz_expert_table_pack(const int32_t* scores, int8_t* table, int c0, int n);
extern "C" __global__ void mz_mcts_move(SpParams S, MctsArgs X);
extern "C" __global__ void mz_sp_pick(SpParams S, PickArgs X);
extern "C" __global__ void mz_prior_fc(PriorParams Q);
extern "C" __global__ void mz_prior_pick(PriorParams Q);
extern "C" __global__ void mz_prior_pick32(PriorParams Q);
extern "C" __global__ void mz_test_begin(SpParams S, TestRec R);
extern "C" __global__ void mz_test_tally(SpParams S, TestRec R);
extern "C" __global__ void mz_log_games(SpParams S, LogAcc* acc);
extern "C" __global__ void mz_log_steps(LogArgs L);
extern "C" __global__ void mz_log_commit(LogArgs L);
extern "C" __global__ void mz_rp_sample(RpSampleParams Q);
extern "C" __global__ void mz_rp_symmetry(RpSymParams Y);
extern "C" __global__ void mz_rp_per_init(SpHist ring, int slot, int len, int Tmax, int td, const float* disc_pow,
                                          int alpha);
extern "C" __global__ void mz_rp_per_prep(SpHist ring, const long long* counters, int cap, float* cum, float* prob,
                                          long long* total);
extern "C" __global__ void mz_rp_per_norm(float* w, int B);
extern "C" __global__ void mz_rp_per_update(SpHist ring, const long long* counters, int cap, int Tmax, int B, int K,
                                            int alpha, const int32_t* index, const float* pv, const float* tv);
extern "C" __global__ void mz_reanalyse_fc(ReanParams Q);
extern "C" __global__ void mz_reanalyse_gather(ReanParams Q);
extern "C" __global__ void mz_reanalyse_scatter(ReanParams Q);
extern "C" __global__ void mz_reanalyse_clear(int32_t* rean, int cap);
extern "C" __global__ void mz_reanalyse_sgather(ReanParams Q);
extern "C" __global__ void mz_reanalyse_sscatter(ReanParams Q);
extern "C" __global__ void mz_reanalyse_pack(ReanParams Q, int32_t* rows);
extern "C" __global__ void mz_reanalyse_seek(long long* counters, long long game_number);
