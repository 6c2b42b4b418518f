/*
 * mz.h — C ABI of libmz, the MI355X-native MuZero self-play + learner engine.
 *
 * This is the drop-in boundary for the reference's hot path.
 * The reference (deveshjawla/MuZero.jl) is Julia; a maintainer binds these
 * symbols with `ccall`; tests bind them with ctypes.
 *
 * Conventions (SURVEY §8b "Conventions"):
 *   - every entry point returns int status: 0 = OK, < 0 = error; the message
 *     is in mz_last_error(h) (the reference raises Julia exceptions / @assert,
 *     e.g. src/SelfPlay.jl:243-244);
 *   - host buffers are caller-owned and borrowed for the duration of the call;
 *     `_dev` variants take device pointers and a hipStream_t (as void*);
 *   - one handle per GPU, one host thread per handle; calls are synchronous
 *     at return (the `_dev` variants are stream-ordered instead); a
 *     host-synchronous call (weights, state, checkpoints, replay / debug
 *     read-outs, the host-buffer search and learner step) first waits for all
 *     of the process's work on the device, so `_dev` work queued on a caller
 *     stream is complete before it reads or overwrites engine memory
 *     (mz_set_sync_stream narrows that wait to one caller stream);
 *   - action ids are 1-based (Julia convention), arrays are column-major with
 *     the reference's shapes (W,H,C,N): feature index = w + W*h + W*H*c.
 */
#ifndef MZ_H
#define MZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZ_MAX_ACTIONS 32

/* Config — field names and defaults of src/Constructors.jl:18-52.
 * Julia `dirichlet_α`/`exploration_ϵ` are spelled dirichlet_alpha /
 * exploration_eps; `temperature_threshold = nothing` is -1; `action_space`
 * is 1:action_space_size; `players` is 1:players.                         */
typedef struct mz_config {
    int32_t seed;                    /* 1337 (Constructors.jl:19, never used by the reference) */
    int32_t observation_shape[3];    /* (W,H,C) per observation, e.g. (3,3,3) */
    int32_t action_space_size;       /* |action_space| = 9 for TicTacToe */
    int32_t players;                 /* |players| = 2 */
    int32_t stacked_observations;    /* 1 */
    int32_t muzero_player;           /* 1 */
    int32_t intermediate_rewards;    /* false */
    int32_t num_workers;
    int32_t selfplay_on_gpu;
    int32_t max_moves;               /* 9 */
    int32_t temperature_threshold;   /* -1 = nothing */
    float dirichlet_alpha;           /* 0.25 */
    float exploration_eps;           /* 0.25 */
    int32_t pb_c_base;               /* 19652 */
    float pb_c_init;                 /* 1.25 */
    float discount;                  /* 0.997 */
    int32_t num_iters;               /* simulations per move */
    int32_t replay_buffer_size;      /* 10000 */
    int32_t num_unroll_steps;        /* K = 5 */
    int32_t td_steps;                /* 5 */
    int32_t PER;                     /* false */
    int32_t PER_alpha;               /* 1 */
    int32_t training_steps;          /* 10000 */
    int32_t batch_size;              /* 32 */
    int32_t checkpoint_interval;     /* 10 */
    float value_loss_weight;         /* 0.25 (never applied by the reference, Q11) */
} mz_config;

enum { MZ_ACT_IDENTITY = 0, MZ_ACT_RELU = 1, MZ_ACT_TANH = 2 };

/* FeedForwardHP — src/Constructors.jl:62-75 */
typedef struct mz_ffhp {
    int32_t width_hidden;            /* 64 */
    int32_t depth_representation;    /* 3 */
    int32_t depth_prediction;        /* 3 */
    int32_t depth_dynamics;          /* 3 */
    int32_t depth_policy;            /* 1 */
    int32_t depth_value;             /* 1 */
    int32_t depth_reward;            /* 1 */
    int32_t depth_state_head;        /* 3 */
    int32_t use_batch_norm;          /* false; true: make_dense = Dense then BatchNorm(out, relu) in test mode (Learning.jl:70-78) */
    float batch_norm_momentum;       /* 0.6 */
    int32_t hidden_state_size;       /* 27 = prod(observation_shape) */
    int32_t reward_activation;       /* MZ_ACT_TANH */
} mz_ffhp;

/* ResNetHP — src/Constructors.jl:77-90, the residual conv towers of
 * Learning.jl:148-255.  The reference's ResNet constructors cannot run
 * (SURVEY §2.1 Q12); the engine builds their intended architecture
 * (DESIGN.md §9): stride-1 zero-padded Conv (Flux convolution, kernel
 * flipped), BatchNorm in test mode (the reference's forward runs outside the
 * pullback) with its running statistics, residual blocks
 * conv-BN-relu-conv-BN-(+x)-relu, 1x1 convs in prediction / dynamics, and the
 * heads' Dense layers of width `width_hidden` (a field the reference reads
 * from ResNetHP but never declares).                                       */
typedef struct mz_resnet_hp {
    int32_t num_blocks;              /* residual blocks per tower */
    int32_t num_filters;             /* nf */
    int32_t conv_kernel_size[2];     /* representation kernel (odd), e.g. (3,3) */
    int32_t num_second_head_filters; /* 2: policy head 1x1 conv channels */
    int32_t num_first_head_filters;  /* 1: value / reward head 1x1 conv channels */
    float batch_norm_momentum;       /* 0.6 (unused in test mode) */
    int32_t downsample;              /* false; true = the Atari downsampler of Learning.jl:175-187
                                        (BASELINE configs[4]): Conv(k, C=>C, stride 2), 2 blocks,
                                        Conv(k, C=>2C, stride 2), 3 blocks, MeanPool((3,3), stride 2,
                                        pad 1), 3 blocks, MeanPool, then the representation's
                                        Conv(k, 2C=>nf) + blocks: 84x84 -> 6x6.  The hidden board
                                        (representation_output_size) is then 6x6, and the
                                        downsampler's params lead the representation's Flux.params */
    int32_t depth_policy;            /* hidden Dense layers (the reference reuses depth_value, kept) */
    int32_t depth_value;             /* hidden Dense layers of the value / reward / policy heads */
    int32_t width_hidden;            /* 64: Dense width of the heads */
    int32_t reward_activation;       /* MZ_ACT_TANH */
} mz_resnet_hp;

/* The three networks of the `NNs` NamedTuple (SelfPlay.jl:230). */
enum { MZ_NET_REPR = 0, MZ_NET_PRED = 1, MZ_NET_DYN = 2 };

typedef struct mz_handle mz_handle;

/* Create an engine on HIP device `device` (replaces init_* + the Julia
 * process setup of games/tictactoe/main.jl:15-28).  `max_games` bounds the
 * batch G of mz_mcts_search; `rng_seed` keys every Philox stream.         */
int mz_engine_create(const mz_config* conf, const mz_ffhp* hyper, int device,
                     int max_games, uint64_t rng_seed, mz_handle** out);
/* Same engine with the ResNet networks (ResNetHP, configs 3-5).  Hidden
 * state = (W, H, num_filters) on the observation board (W, H), or on the
 * downsampled board with ResNetHP.downsample; the dynamics input is
 * (W, H, num_filters+1).  action_space_size <= 32 (the FC engine: <= 16). */
int mz_engine_create_resnet(const mz_config* conf, const mz_resnet_hp* hyper, int device,
                            int max_games, uint64_t rng_seed, mz_handle** out);
void mz_engine_destroy(mz_handle* h);
const char* mz_last_error(const mz_handle* h);
/* message of the last failed mz_engine_create (no handle exists then) */
const char* mz_create_error(void);

/* Parameter counts and exchange in Flux order: for every Dense, W (out,in)
 * column-major then b; Chain order, Split paths in order
 * (Learning.jl:87-142).  FC TicTacToe: 18331 / 23242 / 33308 floats.      */
int mz_net_param_count(const mz_handle* h, int net, size_t* n);
int mz_weights_set(mz_handle* h, int net, const float* flat, size_t n);
int mz_weights_get(mz_handle* h, int net, float* flat, size_t n);

/* Batched forward of one net (the Flux Chain call, Learning.jl:87-142).
 *   REPR: x = stacked obs (W,H,Cs,n) -> out0 = h (hidden,n)
 *   PRED: x = h (hidden,n)          -> out0 = value (1,n), out1 = policy probs (A,n)
 *   DYN : x = state-action (W,H,C+1,n) -> out0 = h' (hidden,n), out1 = reward (1,n) */
int mz_net_forward(mz_handle* h, int net, const float* x, int n, float* out0, float* out1);

/* Batched run_mcts + select_action + store_search_stats! for G games
 * (SelfPlay.jl:230-306, 115-122).
 *   obs        (W,H,Cs,G) stacked observations (get_stacked_observations)
 *   legal_mask (A,G) uint8, nonzero = legal (legal_action_space), >= 1 per game
 *   to_play    (G) current player, 1-based
 *   exploration  add Dirichlet noise at the root (SelfPlay.jl:247-249)
 *   rng_step   move counter keying the Philox streams; game_offset = global id
 *              of game 0 (shard offset on multi-GPU)
 *   temperature  visit_softmax_temperature (0 = argmax, INFINITY = uniform)
 * outputs: child_visits (A,G) = N_a / sum N, root_value (G) = node_value(root),
 *          action_out (G) in 1..A.                                         */
int mz_mcts_search(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask,
                   const int32_t* to_play, int exploration, uint32_t rng_step,
                   uint32_t game_offset, float temperature,
                   float* child_visits, float* root_value, int32_t* action_out);

/* Same, all buffers in device memory, stream-ordered on `stream` (hipStream_t). */
int mz_mcts_search_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask,
                       const int32_t* to_play, int exploration, uint32_t rng_step,
                       uint32_t game_offset, float temperature,
                       float* child_visits, float* root_value, int32_t* action_out,
                       void* stream);

/* Host-synchronous calls wait for ALL of the process's device work by
 * default (hipDeviceSynchronize), which is always safe.  A caller that
 * orders its own `_dev` work can narrow that wait with narrow = 1: the calls
 * then wait only for `stream` (a hipStream_t as void*; NULL = the legacy
 * default stream) and the handle's own stream.  narrow = 0 restores the
 * device-wide wait.                                                        */
int mz_set_sync_stream(mz_handle* h, void* stream, int narrow);

/* Debug/parity: flags & 1 = keep a copy of every search's final tree in HBM
 * (the LDS-resident tree is otherwise discarded at kernel exit); flags & 2 =
 * time the ResNet search's network launches, flags & 4 = the ResNet
 * learner's unroll launches and the unroll launch of each
 * mz_learner_train_multi_dev (mz_learn_multi*) (mz_debug_kernel_time). */
int mz_debug_enable(mz_handle* h, int flags);

/* Debug/parity: copy the last search's tree statistics to host.  Per game,
 * expanded-node slots e = 0..S (0 = root, e = s+1 expanded by simulation s)
 * and child slots a = 0..A-1:
 *   edge_N/edge_W/edge_P/edge_R: (A, S+1, G), edge_child: expanded slot or -1,
 *   node_to_play (S+1, G); any pointer may be NULL.                        */
int mz_debug_tree(mz_handle* h, int G, int32_t* edge_N, float* edge_W, float* edge_P,
                  float* edge_R, int32_t* edge_child, int32_t* node_to_play);

/* Debug/parity: with mz_debug_enable(h, 1) the small-batch search kernels
 * (mz_search_small*) count, per game of the last search, the simulations whose
 * leaf the constant-depth ballot select found (fast) and those that entered
 * the serial level walk (walked); fast + walked = num_iters.  Any other search
 * kernel leaves both at 0.  Either pointer may be NULL.                    */
int mz_debug_select_stats(mz_handle* h, int G, int32_t* fast, int32_t* walked);

/* Measurement: with mz_debug_enable(h, 2) every network launch of the
 * ResNet search (mz_rsearch_nets, its dominant kernel), with flag 4 every
 * learner unroll launch (mz_runroll_*, mz_learn_multi*), is bracketed by HIP events on
 * its stream; this returns the summed duration and the launch count since
 * the previous call, and resets them.                                      */
int mz_debug_kernel_time(mz_handle* h, double* total_ms, int* launches);

/* Debug/parity: the last learner unroll's read-outs (Learning.jl:347-370)
 * for its first B samples: values (K+1, B) and rewards (K+1, B) after their
 * activations, policies (A, K+1, B) as probabilities — the predictions the
 * loss reads (Q10 alignment: step 0 and step 1 both predict from h0,
 * reward 0 at step 0).  Any pointer may be NULL.                          */
int mz_debug_unroll(mz_handle* h, int B, float* values, float* policies, float* rewards);
/* The same read-outs of step step0 + i of the last mz_learner_train_multi_dev
 * that ran its multi-step form, 0 <= i < L; the per-step scratch is a ring of
 * at least 33 steps (the largest multiple of the chain-launch length <= 64),
 * so steps older than that are refused.                                     */
int mz_debug_unroll_step(mz_handle* h, int i, int B, float* values, float* policies, float* rewards);

/* Debug/parity: the plan of the FC corrected learner (MZ_LEARN_CORRECTED,
 * mz_bp_tile_lv), built if it is not yet; nothing is launched.  A plan the
 * engine refuses (its level schedule exceeds the LDS) is an error with that
 * message, as from the learner calls; so is a ResNet engine, and n below
 * MZ_BP_PLAN_FIELDS.  out[0..MZ_BP_PLAN_FIELDS):
 *   0 applications (dense and concat) of the unroll
 *   1 forward levels                  2 backward levels
 *   3 floats of one LDS cache slot    4 cache slots (0: the kernel runs without the cache)
 *   5 dynamic LDS bytes of the kernel
 *   6 applications reading from the arena an input that an earlier application produced
 *   7 produced tensors that are read later and got no forward slot
 *   8 applications accumulating dL/dx in the arena for a tensor that has a producer
 *   9 forward levels ending in a full barrier (the arena's stores drained)
 *  10 backward levels ending in one                                          */
enum { MZ_BP_PLAN_FIELDS = 11 };
int mz_debug_bp_plan(mz_handle* h, int32_t* out, int n);

/* One learner batch, the tuple returned by get_batch (ReplayBuffer.jl:216),
 * column-major as in the reference:
 *   observation (W,H,Cs,B), actions (K+1,B) as float action ids,
 *   target_values (K+1,B), target_rewards (K+1,B), target_policies (A,K+1,B),
 *   gradient_scale (B), weights (B): PER importance-sampling weights
 *   (weight_batch, ReplayBuffer.jl:211-215), NULL = all 1 (PER = false).     */
typedef struct mz_batch {
    int32_t batch_size;
    const float* observation;
    const float* actions;
    const float* target_values;
    const float* target_rewards;
    const float* target_policies;
    const float* gradient_scale;
    const float* weights;
} mz_batch;

/* Learner step in ref_semantics (Learning.jl:327-413, quirks Q10/Q11):
 * K-step unroll forward, losses, gradient 2θ, ADAM(β=(0.9,0.999), ϵ=1e-8)
 * with learning rate `eta` (the host evaluates Cos(λ0=1e-4, λ1=1e-1,
 * period=10) and passes it; Learning.jl:319,382).
 * losses_out[6] = {value, reward, policy, l2_repr, l2_pred, l2_dyn}; the
 * reference's three reported losses are value+reward+policy+l2_net.
 * Single-GPU form; data-parallel training uses the split form below.      */
int mz_learner_step(mz_handle* h, const mz_batch* batch, double eta, float* losses_out);

/* Learner mode.  MZ_LEARN_REF_SEMANTICS (default): the reference as written
 * — its pullbacks see only sum(sqnorm, params), so ∇ = 2θ (quirk Q11), and
 * the reported policy loss is Q11's broadcast.  MZ_LEARN_CORRECTED (every
 * net: FC with or without BatchNorm, ResNet with or without the downsampler): the loss
 * Learning.jl:261-288 means, differentiated through the unroll (real
 * backpropagation on MFMA, mz_backprop.hip), as a per-sample mean so a
 * data-parallel all-reduce-mean equals the global batch:
 *   L = (1/B) Σ_b (w_b/g_b) [Σ_k (v−z)² + Σ_k CE(logits, π) + ir·Σ_k (r−u)²] + Σθ²
 * (CE = logitcrossentropy on the policy head's logits).  Every learner entry
 * point follows the mode; losses_out = {value, reward, policy, Σθ² ×3}.    */
enum { MZ_LEARN_REF_SEMANTICS = 0, MZ_LEARN_CORRECTED = 1 };
int mz_learner_set_mode(mz_handle* h, int mode);

/* Split learner step for data-parallel training: (1) forward + losses +
 * the DATA TERM of the gradient into grad_dev (device, mz_grad_count
 * floats): ∂/∂θ of the loss without Σθ² — zero in ref_semantics (Q11),
 * the backpropagated term in the corrected mode; (2) the caller all-reduces
 * (sum) grad_dev across ranks; (3) mz_learner_apply_dev runs ADAM on
 * ∇ = grad_dev · grad_scale + 2θ (grad_scale = 1/world).  The rank-invariant
 * 2θ = ∂Σθ²/∂θ is added after the exchange, so the update equals the
 * single-GPU update bit for bit at every world size in ref_semantics (an
 * exchanged 2θ would be summed in f32 and round differently at world 8).
 * Stream-ordered on `stream`.                                              */
int mz_grad_count(const mz_handle* h, size_t* n);
int mz_learner_grad_dev(mz_handle* h, const mz_batch* dev_batch, float* grad_dev,
                        float* losses_dev, void* stream);
int mz_learner_apply_dev(mz_handle* h, const float* grad_dev, float grad_scale,
                         double eta, void* stream);

/* ---- Data-parallel learner over RCCL -------------------------
 * For hosts without torch.distributed (the Julia binding): one RCCL
 * communicator per handle, one handle per GPU.  Rank 0 calls
 * mz_dp_unique_id and hands the 128-byte id to every rank out of band (the
 * RemoteChannel / Distributed.jl of the reference host); each rank calls
 * mz_dp_init.  mz_dp_allreduce sums the gradient bucket (mz_grad_count
 * floats, grad_dev or the handle's gradient if NULL) in place over RCCL on
 * `stream`; mz_learner_train_dp = mz_learner_grad_sampled_dev (data term)
 * + that all-reduce + mz_learner_apply_dev(1/world, + 2θ).  librccl.so.1 is loaded on
 * first use (the copy already in the process if any).                      */
#define MZ_DP_ID_BYTES 128
int mz_dp_unique_id(uint8_t* id);
int mz_dp_init(mz_handle* h, int rank, int world, const uint8_t* id);
int mz_dp_allreduce(mz_handle* h, float* grad_dev, void* stream);
int mz_learner_train_dp(mz_handle* h, int32_t B, uint32_t step, double eta, float* losses_dev, void* stream);

/* ---- Device self-play and replay shard ------------
 * The loop body of play_game (SelfPlay.jl:330-382) and the replay buffer
 * (ReplayBuffer.jl) kept in HBM: no host round trip per move or per batch. */
enum { MZ_ENV_TICTACTOE = 0, MZ_ENV_CONNECT4 = 1, MZ_ENV_ATARI = 2 };

/* Device self-play state for G <= max_games game slots: env boards
 * (games/tictactoe/game.jl with quirk Q14, or the Connect4 env of BASELINE
 * configs[3], rules in muzero.jl_amd/games/connect4.py), each slot's
 * GameHistory (Constructors.jl:6-16) in HBM, and a replay shard: FIFO of
 * replay_games >= G finished games (ReplayBuffer.jl:133-161, PER = false;
 * the RemoteBufferChannel Dict keyed by game number).  Every slot starts a
 * new game.  The conf must match the env (TicTacToe (3,3,3)/9 actions,
 * Connect4 (6,7,3)/7 actions, the synthetic Atari-like env of configs[4]
 * (84,84,4)/18 actions with stacked_observations = 0: Philox-keyed frames,
 * rules in muzero.jl_amd/games/atari_synth.py; the records and the shard
 * hold one 84x84 byte frame per move and the observation is the env's
 * four-frame stack; its slots' initial games are drawn at the first
 * mz_selfplay_move, keyed by that move's global game ids game_offset + slot).
 * Calling it again discards the state.                                      */
int mz_selfplay_init(mz_handle* h, int env_kind, int G, int replay_games);

/* One move of every slot, on the device, stream-ordered: observation append
 * and stacked observations (SelfPlay.jl:351-355, Q15), legal mask, to_play,
 * the batched search (as mz_mcts_search_dev with exploration on), env step
 * and GameHistory append (:359-379).  Games that end (terminal, or more than
 * max_moves moves, :343) go to the replay shard in slot order (save_game)
 * and their slot starts a new game.  rng_step = the global move counter.   */
int mz_selfplay_move(mz_handle* h, uint32_t rng_step, uint32_t game_offset, float temperature,
                     void* stream);

/* Evaluation play (competitive_play!, SelfPlay.jl:421-435; play_game with
 * an opponent, :330-382; select_opponent_action, :311-325).  mode
 * MZ_SP_EVAL: finished games are not saved (competitive_play! keeps no
 * buffer) but tallied for mz_eval_results; with opponent MZ_OPP_RANDOM the
 * player != muzero_player (1 or 2) plays a uniform legal action (the Philox
 * OPPONENT stream keyed (game id, rng_step)) instead of the search's, the
 * intended reading of :321 (the reference reads `las`, defined only in the
 * "human" branch); MZ_OPP_SELF: MuZero plays both sides.  Pass
 * temperature 0 to mz_selfplay_move for competitive play.  MZ_SP_TRAIN
 * (default): self_play! (:384-419).  Applies to the following moves; the
 * games in progress continue.
 * MZ_OPP_EXPERT (board envs only): on the same turns, from the same stream,
 * the opponent is a rules search on the device, one extra launch per move
 * and no network.  With p to move, score(s, a, d) of a legal action a is 0 /
 * +d / -d when a ends the game in a draw / a win of p / a win of the other
 * player (the env's own finish test and winner, Q14 included), else
 * -V(s', d - 1); V(s, 0) = 0 and V(s, d) = max over the legal a of
 * score(s, a, d), exhaustive to depth D = mz_expert_depth.  The expert plays
 * the k-th (ascending) of the actions with the maximal score(s, a, D),
 * k = mz_rng_below(draw, their count).  The reference's Config.opponent
 * defaults to "expert" and its expert_agent() is a stub
 * (games/AbstractGame.jl:91-93): this is the opponent that default asks for.
 * MZ_OPP_NETWORK (board envs only): net against net.  On the
 * same turns the opponent is the same search run with the opponent's weight
 * set (mz_opponent_*, below).  Each move searches all G slots twice, first
 * with the engine's nets, then with the opponent's, with the same inputs,
 * rng_step, game_offset, per-slot temperatures and exploration flag (the
 * Philox id of slot g is game_offset + g in both), and one launch
 * (mz_sp_pick) gives every slot whose mover is not muzero_player the
 * opponent search's child_visits, root value and action; the history then
 * holds the mover's own search statistics.  Nothing crosses PCIe.  With
 * mz_debug_enable(h, 1) the dumped tree is the second (the opponent's)
 * search's.  Refused until the opponent set is complete, and on the
 * one-player frame-stack env.  No other mode launches or allocates anything
 * for it.
 * MZ_OPP_MCTS (board envs only): on the same turns the opponent
 * is a vanilla MCTS over the true rules with uniform random rollouts, one
 * extra launch per move and no network: S simulations of R rollouts each
 * (mz_mcts_opponent), UCT with exploration constant 1, every draw from the
 * Philox ROLLOUT stream keyed (game id, rng_step).  It plays the k-th
 * (ascending) of the root actions with the most simulations, k =
 * mz_rng_below(the OPPONENT stream's draw, their count).  Its strength grows
 * with S at a cost linear in S.  The launch is issued in this mode only.    */
enum { MZ_SP_TRAIN = 0, MZ_SP_EVAL = 1 };
enum { MZ_OPP_SELF = 0, MZ_OPP_RANDOM = 1, MZ_OPP_EXPERT = 2, MZ_OPP_NETWORK = 3 };
enum { MZ_OPP_MCTS = MZ_OPP_NETWORK + 1 };                /* 4: the next opponent id */
int mz_selfplay_mode(mz_handle* h, int mode, int opponent, int muzero_player);

/* The opponent's weight set of MZ_OPP_NETWORK: a second set of the three
 * nets (flat parameters and their search images), allocated by the first
 * call that fills it.  A handle setting like mz_expert_depth:
 * mz_selfplay_init, mz_snapshot_load and mz_weights_set leave it alone, and
 * snapshots do not carry it.  It is complete once all three nets have been
 * given: by three mz_opponent_weights_set, one mz_opponent_from or one
 * mz_opponent_load.
 *   _weights_set: host floats in mz_weights_set's layout; an n other than
 *     mz_net_param_count is refused.  The set's search images are rebuilt
 *     when the last missing net arrives and on every later call.
 *     Synchronises.
 *   _weights_get: one net of the set (refused if that net was never given).
 *     Synchronises.
 *   _from: a device copy, stream-ordered on `stream`, no host
 *     synchronisation: MZ_TRAIN_LEARNER = the engine's current nets (needs
 *     no mz_train_init), MZ_TRAIN_ACTOR / MZ_TRAIN_QUEUED = the actor-learner
 *     loop's sets (refused before mz_train_init).
 *   _load: the three nets' arrays, by name, from a file mz_checkpoint_save
 *     or mz_snapshot_save wrote.  The network kind and every shape are
 *     checked against this engine first, and a refused file leaves the set
 *     as it was.  The learner's nets and ADAM state are not touched.
 *     *training_step (may be NULL) = the file's.  Synchronises.              */
int mz_opponent_weights_set(mz_handle* h, int net, const float* flat, size_t n);
int mz_opponent_weights_get(mz_handle* h, int net, float* flat, size_t n);
int mz_opponent_from(mz_handle* h, int which, void* stream);
int mz_opponent_load(mz_handle* h, const char* path, int64_t* training_step);

/* Depth D of the expert opponent, 1..9; 0 (default) = the env's default:
 * 9 for TicTacToe (perfect play under the env's rules), 4 for Connect4
 * (1 takes an immediate win, 2 also blocks one).  A handle setting like
 * mz_selfplay_mode's: mz_selfplay_init and mz_snapshot_load keep it.        */
int mz_expert_depth(mz_handle* h, int depth);

/* The expert's scores of G >= 1 given positions, by the kernel evaluation
 * play runs: boards [G][W*H*3] 0/1 bytes (planes [p1, p2, empty]), players
 * [G] (1 or 2, the player to move), depth 1..9 -> scores [G][A]
 * score(s, a, depth), -128 for an illegal action.  Host buffers;
 * synchronises; needs no mz_selfplay_init.  env_kind must fit the conf as
 * for mz_selfplay_init.  The positions are taken as not finished.  Refused:
 * a cell set in no plane or in more than one, a player outside 1..2.        */
int mz_expert_eval(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players, int depth,
                   int32_t* scores);

/* The solved TicTacToe table: score(s, a, 9) of every board,
 * so the depth-9 expert's move is a lookup, not a search.  The scores depend
 * on the mover-relative position only: entry code = Σ_cell 3^cell · d, d = 0
 * for an empty cell, 1 for the mover's stone, 2 for the other player's, cells
 * in the byte planes' order; 3^9 = 19683 entries of nine int8 scores, -128
 * for an illegal action (on the device each entry is padded to 16 bytes).
 * Every code is filled, unreachable and finished boards with what the search
 * kernel says of them: the fill is mz_expert_move's own depth-9 output over
 * all codes, so table and search agree by construction.
 *   mz_expert_table: a handle setting like mz_expert_depth (default off;
 *     mz_selfplay_init and mz_snapshot_load keep it, snapshots do not carry
 *     it).  on = 1 builds the table if the handle has none (host-synchronous,
 *     once per handle; the table lives as long as the handle) and is refused
 *     on a conf that cannot be TicTacToe (observation_shape (3,3,3), 9
 *     actions); on = 0 stores the flag and frees nothing.
 *     The lookup kernel replaces the search kernel's launch of an
 *     MZ_OPP_EXPERT move (mz_selfplay_move in MZ_SP_EVAL, mz_test_play, the
 *     test worker in mz_train_run) exactly when the switch is on, the env is
 *     MZ_ENV_TICTACTOE and the effective depth is 9 (mz_expert_depth 0 or 9).
 *     Same rows, same draw, same tie-break: the moves are bit for bit the
 *     search kernel's.  mz_expert_eval always runs the search kernel.
 *   mz_expert_table_get (parity): scores [19683][9] int8 (refused while no
 *     table is built), *built 0|1, *in_use = 1 when the lookup would be
 *     launched for the current env and depth.  Any pointer may be NULL.
 *     Synchronises.                                                          */
int mz_expert_table(mz_handle* h, int on);
int mz_expert_table_get(mz_handle* h, void* scores, int32_t* built, int32_t* in_use);

/* The judge's rule on given positions: row g is the move
 * actions[g] (1-based) of players[g] on boards[g], judged at `depth`.  With
 * c = score(s, a, depth) and b = the maximum over the legal actions' scores,
 * a move adds {1, c == b, sgn(c) < sgn(b), b - c} to out4 = {moves judged,
 * moves inside the expert's best set, moves that give away a win or a draw,
 * total score deficit}.  Integers throughout: exact in any order.  Buffers
 * and refusals as mz_expert_eval, plus an action that is not legal on its
 * board.  Always the search kernel, in the judge mode evaluations use;
 * synchronises; needs no mz_selfplay_init.  A host can judge any games it
 * holds with it, e.g. those of mz_replay_get_game.                          */
int mz_expert_judge(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players,
                    const int32_t* actions, int depth, int64_t* out4);

/* The rules-MCTS opponent's budget (MZ_OPP_MCTS): sims 1..1024 simulations
 * a move, rollouts 1..64 random playouts per simulation; 0 = the default
 * (64 simulations, 16 rollouts).  A handle setting like mz_expert_depth:
 * mz_selfplay_init and mz_snapshot_load keep it, snapshots do not carry it.  */
int mz_mcts_opponent(mz_handle* h, int sims, int rollouts);

/* The rules-MCTS opponent's root statistics of G >= 1 given positions, by
 * the kernel evaluation play runs (the parity entry point): boards, players
 * as mz_expert_eval; sims 1..1024, rollouts 1..64; row g searches with the
 * Philox id game_offset + g and the step rng_step -> n_out, w_out [G][A]:
 * the simulations through each root action and the sum of their outcomes for
 * the player to move, in rollouts (|w| <= n * rollouts); n = -1, w = 0 for an
 * illegal action.  Host buffers; synchronises; needs no mz_selfplay_init.
 * Buffers, validation and refusals are mz_expert_eval's.                     */
int mz_mcts_eval(mz_handle* h, int env_kind, int G, const uint8_t* boards, const int32_t* players, int sims,
                 int rollouts, uint32_t rng_step, uint32_t game_offset, int32_t* n_out, int32_t* w_out);

/* ---- The network-only player (AlphaZero.jl's NetworkOnly) -------
 * A row's move from the policy head alone, with no tree.  For a row with
 * observation obs, a non-empty legal set, temperature T and the Philox key
 * (seed, game_offset + row, rng_step):
 *   (v, p) = prediction(representation(obs)), bit for bit what
 *     mz_net_forward(MZ_NET_REPR) then mz_net_forward(MZ_NET_PRED) return: v
 *     the value head's post-activation, p the policy head's softmax over all A
 *     actions (the distribution the learner trains; not the Q3 double softmax);
 *   s = the ascending f32 sum of p[a] over the legal a; π[a] = p[a] / s for a
 *     legal a and 0 for an illegal one; with s == 0, π[a] = 1 / n_legal;
 *   the action follows select_action on π with the draw r select_action takes
 *     for the same row (the ACTION stream; no new stream): T == 0 the first
 *     maximum of π, T == +inf the mz_rng_below(r, n_legal)-th legal action,
 *     else weights w[a] = π[a] (T == 1) or (float)det_exp(det_log((double)π[a])
 *     · (double)(1.0f / T)) where π[a] > 0, else 0; S = their ascending f32 sum,
 *     u = (float)(r >> 8) · 2^-24 · S, the first legal b whose running f32 sum
 *     exceeds u, else the last legal action.
 * The row's result (π, v, action) stands where a search row has (child_visits,
 * root_value, action).  Serial restatement: csrc/mz_prior_rules.h (mzp_row);
 * Python mirror: selfplay.prior_move.
 *   mz_eval_players: which player produces a network side's rows in evaluation
 *     play.  muzero_kind: the rows with to_play == muzero_player, on the
 *     handle's nets.  other_kind: the other rows where the other side is a
 *     network player (MZ_OPP_SELF: the same nets; MZ_OPP_NETWORK: the opponent
 *     weight set); the rules opponents (RANDOM, EXPERT, MCTS) do not consult
 *     it.  A handle setting like mz_expert_depth, default (SEARCH, SEARCH):
 *     mz_selfplay_init and mz_snapshot_load keep it, snapshots do not carry
 *     it.  Read by mz_selfplay_move in MZ_SP_EVAL and by mz_test_play (so by
 *     the test worker inside mz_train_run); MZ_SP_TRAIN never consults it.
 *     Every env.  Each move issues MuZero's kind on the handle's nets first
 *     (into the engine's search io), then, only where it differs in kind or in
 *     weights, the other side's kind into second outputs followed by
 *     mz_sp_pick.  With (PRIOR, ·) against a rules opponent, or (PRIOR, PRIOR)
 *     with MZ_OPP_SELF, a move launches no search.  Refused: a kind outside
 *     {0, 1} ("eval players: ...").
 *   mz_prior_eval: G rows (0..max_games) on host buffers, as mz_mcts_search's:
 *     obs [G][stacked features], legal_mask [G][A] -> policy [G][A] = π, value
 *     [G] = v, action [G] (1-based).  opponent_set 0: the handle's nets; 1: the
 *     opponent weight set (refused until it is complete).  Refused: a row
 *     without a legal action, a temperature that is negative or NaN.
 *     Synchronises; needs no mz_selfplay_init.
 *   mz_prior_eval_dev: the same on device pointers, stream-ordered on
 *     `stream`, no validation of the rows.                                     */
enum { MZ_PLAYER_SEARCH = 0, MZ_PLAYER_PRIOR = 1 };
int mz_eval_players(mz_handle* h, int muzero_kind, int other_kind);
int mz_prior_eval(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, int opponent_set,
                  uint32_t rng_step, uint32_t game_offset, float temperature, float* policy, float* value,
                  int32_t* action);
int mz_prior_eval_dev(mz_handle* h, int G, const float* obs, const uint8_t* legal_mask, int opponent_set,
                      uint32_t rng_step, uint32_t game_offset, float temperature, float* policy, float* value,
                      int32_t* action, void* stream);

/* Evaluation tally since mz_selfplay_init: {games finished, MuZero wins,
 * opponent wins, draws}; the winner is read from the last move's reward
 * (TicTacToe with quirk Q14: the player to move after it; Connect4: the
 * mover).  Synchronises.                                                    */
int mz_eval_results(mz_handle* h, int64_t* out4);

/* ---- The test worker (the reference's muzero.jl:29-31 leaves it
 * as "Launch the test worker to get performance metrics") -------------------
 * Evaluation games on a second, independent set of E game slots of the
 * handle, so a training job can be measured while it runs: the self-play
 * slots, their histories, the shard, its counters and PER state, the batch
 * drawn ahead, the train loop's weight sets and mz_eval_results are not
 * touched.  What an evaluation uses is what every search on the stream uses:
 * the engine's tree buffers and search io.  Nothing crosses PCIe.
 *   mz_test_config: a handle setting like mz_expert_depth (mz_selfplay_init
 *     and mz_snapshot_load keep it): E = games test slots (1..max_games; 0 =
 *     off, which frees nothing until the next mz_selfplay_init), the opponent
 *     MZ_OPP_* and muzero_player 1|2.  Refused as mz_selfplay_mode refuses:
 *     before mz_selfplay_init, an unknown opponent, muzero_player outside
 *     1..2, EXPERT / NETWORK / MCTS on the frame-stack env, NETWORK before
 *     the opponent set is complete.
 *   mz_test_play: one evaluation, stream-ordered, no host synchronisation.
 *     Every test slot g starts a new game as mz_selfplay_init plus the first
 *     mz_selfplay_move would start slot g (boards: empty, player 1; the
 *     Atari-like env: mz_sp_reset's draw keyed by game_offset + g), then
 *     T = max_moves + 1 moves are enqueued.  Move m is what
 *     mz_selfplay_move(rng_step0 + m, game_offset, temperature) does in
 *     MZ_SP_EVAL mode with the configured opponent and muzero_player, with the
 *     weights mz_net_forward would use at this point of the stream
 *     (temperature_threshold applies as there).  A slot whose game has ended
 *     (done, or more than max_moves moves) is frozen for the rest of the
 *     evaluation: neither restarted nor stored, nothing more of it recorded;
 *     its search row is the dummy row of the Reanalyse rounds (zero
 *     observation, every action legal, to_play 1).  The host never learns when
 *     every slot is done: it always enqueues T moves, each followed by one
 *     launch of mz_test_tally in place of mz_sp_order / mz_sp_store.  So slot
 *     g's game is, bit for bit, the first game slot g plays after
 *     mz_selfplay_init(env, E, E) + mz_selfplay_mode(MZ_SP_EVAL, opponent,
 *     muzero_player) + those moves, and what the host mirror's
 *     BatchedSelfPlay(...).play_games() returns.  With mz_debug_enable(h, 1)
 *     the dumped tree is the evaluation's last search's.  The test slots are
 *     allocated by the first call after each mz_selfplay_init /
 *     mz_snapshot_load.  Refused before mz_selfplay_init and with games == 0;
 *     mz_test_config's refusals are checked again.
 *     Each evaluation appends one record, kept in slot e % MZ_TEST_RECORDS of
 *     a device ring that lives with the handle (mz_selfplay_init keeps it):
 *       counts[8] = {training_step, games finished, MuZero wins, opponent
 *                    wins, draws, moves, value_moves, rng_step0}
 *       sums[3]   = {reward_muzero, reward_opponent, value_sum}
 *     Winner and draw as mz_eval_results reads them; moves = the sum of the
 *     game lengths.  MuZero's moves of a game are its records with to_play ==
 *     muzero_player, and every record when the opponent is MZ_OPP_SELF or
 *     players == 1: reward_muzero sums their rewards, value_sum their stored
 *     root values (value_moves counts them), reward_opponent the other
 *     records' rewards.  The numerics are part of the contract: each game's
 *     three sums are f64, start at +0 and add (double)x in record order, and
 *     the record adds the finished games' sums in (move, ascending slot)
 *     order; selfplay.evaluation_record is the exact host mirror.
 *   mz_test_results: the latest min(max_records, held) records, oldest first
 *     (held = min(total, MZ_TEST_RECORDS)); *total = evaluations since create
 *     / mz_test_clear; counts [n][8], sums [n][3]; any pointer may be NULL.
 *     Synchronises.  mz_test_clear: total back to 0.
 *   mz_test_get_game (parity): test slot `slot`'s game of the last evaluation,
 *     layouts of mz_replay_get_game; synchronises.
 *   mz_test_audit: judge MuZero's moves of the following
 *     evaluations by the expert's scores, the rule of mz_expert_judge at depth
 *     D = mz_expert_depth (0: the env's default).  A handle setting, default
 *     off, kept by mz_selfplay_init and mz_snapshot_load; refused on the
 *     frame-stack env, and checked again by mz_test_play.  Judged: MuZero's
 *     moves as above (to_play == muzero_player; every move with MZ_OPP_SELF)
 *     of the slots that are not frozen, each by the action the search left
 *     before mz_sp_commit, i.e. after temperature sampling.  One launch per
 *     move: the expert's own launch with MZ_OPP_EXPERT (it judges MuZero's
 *     turns and moves on the others), one more otherwise; the lookup kernel
 *     where the solved table is in use, else the search kernel.  Games and
 *     records are those of the same evaluation with judging off, bit for bit.
 *     The sums {moves judged, in the expert's best set, win or draw given
 *     away, score deficit} go to row e % MZ_TEST_RECORDS of a second device
 *     ring int64 [MZ_TEST_RECORDS][4], allocated by the first evaluation that
 *     judges and zeroed on the stream at its start.  An evaluation with
 *     judging off issues no launch or memset it did not issue before.
 *   mz_test_audit_results: audit [n][4], the rows of the evaluations
 *     mz_test_results returns, in its order: row i of both belongs to the same
 *     evaluation.  An evaluation run with judging off reads {-1, 0, 0, 0}.
 *     total and audit may be NULL.  Synchronises.  mz_test_clear resets both
 *     rings.                                                                  */
enum { MZ_TEST_RECORDS = 1024 };
int mz_test_config(mz_handle* h, int32_t games, int opponent, int muzero_player);
int mz_test_play(mz_handle* h, int64_t training_step, uint32_t rng_step0, uint32_t game_offset,
                 float temperature, void* stream);
int mz_test_results(mz_handle* h, int64_t* total, int64_t* counts, double* sums, int32_t max_records);
int mz_test_clear(mz_handle* h);
int mz_test_audit(mz_handle* h, int on);
int mz_test_audit_results(mz_handle* h, int64_t* total, int64_t* audit, int32_t max_records);
int mz_test_get_game(mz_handle* h, int32_t slot, int32_t* T, uint8_t* obs, int32_t* actions, float* rewards,
                     int32_t* to_play, float* child_visits, float* root_values);

/* The shard's counters {num_played_games, num_played_steps, total_samples}
 * (ReplayBuffer.jl:133-161) and the games it holds; synchronises.          */
int mz_replay_counts(mz_handle* h, int64_t* counts, int32_t* games_in_buffer);

/* save_game of a host GameHistory of T moves (obs as 0/1 bytes (T, W*H*C),
 * actions / rewards / to_play / root_values (T), child_visits (A, T)).     */
int mz_replay_save_game(mz_handle* h, int32_t T, const uint8_t* obs, const int32_t* actions,
                        const float* rewards, const int32_t* to_play, const float* child_visits,
                        const float* root_values);

/* get_batch with make_target (ReplayBuffer.jl:5-50, 73-107, 188-217) on the
 * device: B samples drawn with the Philox streams of learner step `step`
 * (engine seed; sample_n_games uniform with replacement, sample_position
 * uniform, absorbing-state actions uniform).  Fills *batch with device
 * arrays owned by the handle (valid until the next call; feed them to
 * mz_learner_grad_dev) and, if index_batch != NULL, copies the (game
 * number, 1-based position) pairs to it (B x 2, synchronises).             */
int mz_replay_sample(mz_handle* h, int32_t B, uint32_t step, mz_batch* batch, int32_t* index_batch,
                     void* stream);

/* Board-symmetry augmentation of get_batch.  The board envs have
 * exact symmetries: TicTacToe the eight of the square (id s: transpose
 * (i, j) -> (j, i) if s >= 4, then s & 3 quarter turns (a, b) -> (b, 2 - a);
 * cell i + 3j, action a <-> cell a - 1), Connect4 the left-right mirror (id 1:
 * cell (w, h) -> (w, H-1 - h), action a -> H + 1 - a).  id 0 is the identity.
 *
 *   mz_replay_set_symmetry: a handle setting like mz_expert_depth (default 0 =
 *     off; mz_selfplay_init of the same env and mz_snapshot_load keep it,
 *     snapshots do not carry it).  on = 1: sample b of every device get_batch
 *     at learner step `step` (mz_replay_sample, mz_learner_grad_sampled_dev /
 *     _train_dev / _train_multi_dev / _train_dp, mz_train_run / _learn) is
 *     the stored position replayed under element
 *       s_b = rng_below(rng_u32(seed, MZ_RNG_SYMMETRY, b, step, 0), n)
 *     of the env's group: every board plane of the stacked observation is
 *     permuted, the action planes, `actions` (absorbing-state actions
 *     included, drawn as ever and then permuted) hold the permuted id,
 *     target_policies moves with the actions; target_values / _rewards,
 *     gradient_scale, the index batch, the PER weights and the priority
 *     update are those of the plain sample.  Needs mz_selfplay_init; the
 *     Atari-like env has no group and is refused; on must be 0 or 1.  A toggle
 *     drops a batch drawn ahead.
 *   mz_replay_symmetry_get: the group order n, the tables as the device holds
 *     them (cell_perm [n][W*H]: cell c moves to cell_perm[s][c]; action_perm
 *     [n][A], 0-based) and the setting; any output may be NULL.  n <= 8.
 *   mz_batch_symmetry: the same transform of a device batch of in->batch_size
 *     rows assembled by the caller, row b under element sym_dev[b] (device
 *     int32 [B]; an id outside 0..n-1 copies the row) into the arrays of *out
 *     (device, the caller's, writable, the same sizes; weights are copied
 *     when both batches have them).  No array of *out may overlap one of *in.
 *     Works with the setting on or off.                                      */
int mz_replay_set_symmetry(mz_handle* h, int on);
int mz_replay_symmetry_get(mz_handle* h, int32_t* n, int32_t* cell_perm, int32_t* action_perm, int32_t* on);
int mz_batch_symmetry(mz_handle* h, const mz_batch* in_dev, const int32_t* sym_dev, mz_batch* out_dev,
                      void* stream);

/* One learner iteration on a batch drawn from this GPU's replay shard:
 * get_batch (as mz_replay_sample(step)) + learning! (Learning.jl:327-404).
 * The sampling runs inside the FC unroll kernel (its own launch otherwise).
 * _grad_sampled_dev: results of mz_replay_sample + mz_learner_grad_dev (for
 * a gradient exchange before mz_learner_apply_dev).  _train_dev (one GPU,
 * world = 1): also the ADAM step with learning rate eta, fused into the loss
 * kernel — results of the three calls with grad_scale 1.  The batch arrays
 * of _grad_sampled_dev are left in the handle's mz_replay_sample buffers.
 * _train_dev on the one-launch FC path (PER off) also draws step + 1's batch
 * into a second batch set, which the next call uses only while the shard
 * (games stored), the step, B and every other sampling call since still
 * match — identical results, the sampler off the next step's critical path
 * (env MZ_NO_BATCH_PREFETCH=1 turns it off).  Replaces, per step,
 * the learner's fetch of the buffer + get_batch + learning! iteration
 * (Learning.jl:329-404).                                                    */
int mz_learner_grad_sampled_dev(mz_handle* h, int32_t B, uint32_t step, float* grad_dev,
                                float* losses_dev, void* stream);
int mz_learner_train_dev(mz_handle* h, int32_t B, uint32_t step, double eta, float* losses_dev,
                         void* stream);

/* L consecutive learner iterations (Learning.jl:327-404) at steps step0 ..
 * step0+L-1, eta[i] the learning rate of step step0+i (host array): the
 * results of L mz_learner_train_dev calls, bit for bit.  In ref_semantics
 * (Q11) the update θ_{s+1} = ADAM(θ_s, 2θ_s) does not read the data, and with
 * PER off step s's batch is keyed by s, so the engine runs the ADAM
 * iterations of many steps in one launch and their unrolls + losses side by
 * side (L·B workgroups instead of B).  losses_dev:
 * NULL or [L][8] (per step the six losses of mz_learner_train_dev);
 * theta_dev: NULL or [L][nflat], the flat parameters (Flux order, the
 * mz_weights_get layout of all three nets back to back) after each step.
 * 1 <= L <= 256.  FC: chain launches (mz_learn_chain: the ADAM iterations,
 * each step's θ scattered into its own image in a bank, Σθ² per step, the
 * batches) of up to 32 steps, each followed by unroll launches
 * (mz_learn_multi*) of up to 32 steps side by side (mz_learn_multi4; 16 on
 * the one- and two-sample kernels); ResNet: the same chain
 * launches feeding the mz_runroll_* launches with the steps on gridDim.z
 * (rlearner_multi).  The corrected mode and PER run the L steps one after
 * another.  Replaces L iterations of the learner loop.                      */
int mz_learner_train_multi_dev(mz_handle* h, int32_t B, uint32_t step0, int32_t L, const double* eta,
                               float* losses_dev, float* theta_dev, void* stream);

/* PER (conf.PER, ReplayBuffer.jl:133-145, 168-183; Learning.jl:400-404).
 * With PER the shard keeps per-position priorities (initialised by
 * save_game: |root_value − target_value|^PER_alpha, game priority = max),
 * get_batch samples games and positions by priority and fills
 * batch->weights, and the learner weights its losses.  The fused learner
 * calls (mz_learner_train_dev / _grad_sampled_dev) then update the sampled
 * positions' priorities from the unroll's values; after mz_replay_sample +
 * mz_learner_grad_dev call mz_replay_update_priorities (it uses the batch of
 * the last sample and the last unroll).  The reference's update_priorities!
 * cannot run (`minimum(a, b)`, a K+2-element slice); this is its intended
 * reading: positions pos..min(pos+K, len), samples in batch order.          */
int mz_replay_update_priorities(mz_handle* h, void* stream);
/* Debug/parity: priorities of game i of the shard (0 = oldest held), T of
 * them, and its game priority; synchronises.                                */
int mz_replay_get_priorities(mz_handle* h, int32_t i, float* priorities, float* game_priority);

/* Debug/parity: game i of the shard (0 = oldest held), buffers sized for
 * max_moves + 1 moves (layouts as mz_replay_save_game); any pointer may be
 * NULL.  And the slots' games in progress: moves recorded, boards (G, W*H*C)
 * as 0/1 bytes, player to move.  Both synchronise.                         */
int mz_replay_get_game(mz_handle* h, int32_t i, int32_t* T, uint8_t* obs, int32_t* actions,
                       float* rewards, int32_t* to_play, float* child_visits, float* root_values);
int mz_selfplay_slots(mz_handle* h, int32_t* history_len, uint8_t* board, int32_t* player);

/* Reanalyse (ReplayBuffer.jl:8, 56-67; muzero.jl:15-19): games first ..
 * first+count-1 of the shard (0 = oldest held, as mz_replay_get_game;
 * count < 0 = all held; games past the held range are skipped on the device)
 * get reanalysed_predicted_root_values = value head of prediction(
 * representation(stacked obs)) at every position, with the weights
 * mz_net_forward would use at this point of the stream.  Stream-ordered, no
 * host synchronisation.  Targets drawn afterwards (mz_replay_sample and
 * every learner call that samples) bootstrap from them instead of the
 * search's root_values; a game stored into a slot later (self-play or
 * mz_replay_save_game) starts as `nothing` again, and PER's initial
 * priorities stay on root_values (save_game runs before any reanalysis).
 * FC engines: one launch (mz_reanalyse_fc); ResNet board engines: gather /
 * representation / prediction / scatter launches per chunk of positions.
 * The frame-stack env (MZ_ENV_ATARI) is refused.
 * Ordering is the caller's: reanalyse reads the shard and the weights, so it
 * and mz_selfplay_move / the learner calls on DIFFERENT streams must be
 * ordered by the caller (events); on one stream nothing is needed.  In the
 * split actor-learner loop the place for the call is between mz_train_move
 * and mz_train_learn, on their stream; mz_train_run never makes this call
 * (the reference's loop has no reanalyse worker) — what it can run every move
 * is the worker's round, mz_replay_reanalyse_next, once mz_train_set_reanalyse
 * turns it on.
 * _clear_reanalysed: every held game back to `nothing`.  _reanalysed_count:
 * num_reanalysed_games, one per game per mz_replay_reanalyse since
 * mz_selfplay_init; synchronises.  _get_reanalysed (parity): game i's flag
 * and, if set, its T values (buffer sized for max_moves + 1); synchronises. */
int mz_replay_reanalyse(mz_handle* h, int32_t first, int32_t count, void* stream);
int mz_replay_clear_reanalysed(mz_handle* h, void* stream);
int mz_replay_reanalysed_count(mz_handle* h, int64_t* n);
int mz_replay_get_reanalysed(mz_handle* h, int32_t i, int32_t* is_set, float* values);

/* Reanalyse by search — the other half of MuZero Reanalyze, the worker the
 * reference leaves as a TODO (muzero.jl:15-19): the stored positions of games
 * first .. first+count-1 (selected as above) are searched again with the
 * current networks.  Their child_visits become the games' policy targets and
 * the search's root values their bootstrap values (they replace what
 * mz_replay_reanalyse wrote; a later mz_replay_reanalyse keeps the policies
 * and overwrites the values).  The selection is flattened as p = gi*T + pos
 * (gi = index inside the selection, T = max_moves + 1); position p is searched
 * exactly as mz_mcts_search_dev searches the game with Philox id
 * game_offset + p: obs = the stacked observation at pos, to_play = the stored
 * to_play, legal_mask = the env's legal actions on the stored board for that
 * player (what self-play's search saw), `exploration` and rng_step as given,
 * temperature 0 with the action discarded.  The result does not depend on how
 * the rows are cut into launches: max_games rows per round of mz_reanalyse_sgather
 * -> the engine's search launches -> mz_reanalyse_sscatter; rows with
 * pos >= len and rows past the held range ride along as dummy games whose
 * outputs are dropped.  A stored position with no legal action, or a to_play
 * outside 1..players (only mz_replay_save_game can store either), is not
 * searched: it keeps copies of its stored child_visits and root_values.
 * Stream-ordered, no host synchronisation; num_reanalysed_games goes up by
 * one per game.  The search's io buffers and the shard's reanalysed
 * child_visits are allocated by the first call that has work.  Ordering and
 * the place in the split loop are as for mz_replay_reanalyse: between
 * mz_train_move and mz_train_learn, on their stream (the search uses the
 * engine's one set of tree buffers, as mz_selfplay_move does); mz_train_run
 * never makes this call either: its reanalysis is the worker's round below
 * (mz_train_set_reanalyse, off by default).  The frame-stack env is refused.
 * _get_reanalysed_policies (parity): game i's policy flag and, if set, its
 * (A, T) child_visits in mz_replay_get_game's layout (buffer sized for
 * max_moves + 1 positions); synchronises.  mz_replay_clear_reanalysed and a
 * game stored into the slot reset both fields.                              */
int mz_replay_reanalyse_search(mz_handle* h, int32_t first, int32_t count, int exploration, uint32_t rng_step,
                               uint32_t game_offset, void* stream);
int mz_replay_get_reanalysed_policies(mz_handle* h, int32_t i, int32_t* is_set, float* child_visits);

/* The Reanalyse worker: rounds whose selection is made on the device, so a
 * rolling pass needs no read-back of the counters.  The shard keeps a cursor,
 * the game number (save_game's 1-based numbering) of the next game to
 * reanalyse; mz_selfplay_init sets it to 1.  One round (kernel
 * mz_reanalyse_pack), with played = num_played_games, n = min(played,
 * capacity), oldest = played - n + 1: nothing if played == 0; else a cursor
 * outside [oldest, played] moves to oldest (the wrap, or the games evicted
 * since), and games cursor, cursor + 1, ... are taken while they are <= played
 * and their lengths sum to <= R.  R = max_games rows with MZ_REAN_BY_SEARCH,
 * 4096 with MZ_REAN_BY_VALUE.  A round never wraps: one that reaches `played`
 * ends there and the next starts at the oldest game.  The cursor becomes the
 * first game not taken.  Only the taken games' stored positions become rows,
 * in (game, position) order; a round that did not end at `played` has fewer
 * than max_moves + 1 unused rows.
 * _next: one round, pack -> (mz_reanalyse_fc | gather, nets, scatter) or
 *   (sgather, the search, sscatter) on the packed rows, stream-ordered, no host
 *   synchronisation, with the weights and tree buffers an explicit reanalyse
 *   call would use at this point of the stream; flags, counter and targets as
 *   for mz_replay_reanalyse / _search.  Search mode: row i is searched exactly
 *   as mz_mcts_search_dev searches game i of a G = max_games launch with
 *   Philox id game_offset + i (temperature 0, the action dropped); the rows
 *   from n_rows on ride along as the dummy game.  Value mode ignores
 *   exploration, rng_step and game_offset.  Refused: the frame-stack env, and
 *   search mode with max_games < max_moves + 1 (a round could not hold one
 *   full game).
 * _cursor (parity, synchronises): the cursor and the last round's {first game
 *   number, games taken, rows}; either pointer may be NULL.
 * _seek: stream-ordered, sets the cursor to any value; the next round
 *   normalises it as above.                                                  */
enum { MZ_REAN_OFF = 0, MZ_REAN_BY_VALUE = 1, MZ_REAN_BY_SEARCH = 2 };
int mz_replay_reanalyse_next(mz_handle* h, int mode, int exploration, uint32_t rng_step,
                             uint32_t game_offset, void* stream);
int mz_replay_reanalyse_cursor(mz_handle* h, int64_t* next_game, int64_t* last_round3);
int mz_replay_reanalyse_seek(mz_handle* h, int64_t game_number, void* stream);

/* ---- Actor–learner loop (self_play! ‖ learning!) -----
 * The reference runs self_play! (SelfPlay.jl:384-419) and learning!
 * (Learning.jl:306-438) as two processes coupled by RemoteChannels (quirk
 * Q16): self-play take!s the training step once per game, the learner put!s
 * it once per step, and every checkpoint_interval steps the learner queues
 * its nets on remote_NNs (capacity 1, starting with the initial nets) which
 * self-play then take!s — the actors run one checkpoint behind.  On the
 * device, for the G lockstep slots of mz_selfplay_init:
 *   mz_train_init: the actors' weight set and the queue start as copies of
 *     the engine's current (initial) nets; learner step t = 0; B = batch.
 *   mz_train_init_at: the same from learner step t0 (a resume: pass the
 *     training_step mz_checkpoint_load returned; the Cos η phase, the
 *     training_steps bound, the temperature and the checkpoint cadence then
 *     continue from t0).  Checkpoints hold the learner's nets and ADAM state,
 *     not the actors' or queued sets, so a resume restarts the one-checkpoint
 *     lag: actors and queue start as copies of the loaded learner nets.
 *     That restart applies to checkpoints; a snapshot (mz_snapshot_save /
 *     _load, below) holds both sets and resumes exactly, without this call.
 *   mz_train_run: `moves` times: one self-play move of every slot with the
 *     ACTORS' nets (mz_selfplay_move, move key move0 + m); each game plays
 *     at the temperature visit_softmax_temperature_fn(t) of the step t at
 *     which it started (play_game takes T once per game, SelfPlay.jl:396-407;
 *     games in progress at mz_train_init_at take that of t0); then one
 *     learner step per game saved by that move (mz_learner_train_dev with
 *     step t+1, eta = Cos(t+1)) while t <= training_steps; after step t with
 *     t % checkpoint_interval == 0 and t > 1 the actors take the queued nets
 *     and the learner's nets are queued, and — when a networks path is set and
 *     t > round(0.9 training_steps) — the learner's state is written to
 *     <networks_path>/<t>.safetensors (mz_checkpoint_save; Learning.jl:416-432).
 *     Deliberate deviation: the G games run in lockstep on one weight set, so
 *     a refresh reaches every slot at once, games in progress included; the
 *     reference's single actor takes new nets only between games
 *     (SelfPlay.jl:399-401).  Reads the shard's game counter back once per
 *     move (one kernel stores it into pinned host memory and the host spins
 *     on it, bounded; the stream's work up to that move is then complete).
 *     state_out[4] = {t, num_played_games, actor refreshes,
 *     learner steps of this call}; losses_dev (device, 6 floats, or NULL) =
 *     the last step's.  The learner steps of one move run as one
 *     mz_learner_train_multi_dev chunk across the refresh points (the chain
 *     launch copies out θ of the last two refresh steps for the actors' and
 *     queued sets, and writes the actors' search images; with a networks path
 *     the chunks end at each refresh).
 *     Data parallel (after mz_dp_init, world > 1): the move's finished-game
 *     count is summed over the ranks (RCCL) and every rank takes that many
 *     learner steps on its own shard, so the ref_semantics replicas stay
 *     bit-identical.
 *   mz_train_move / mz_train_learn: the two halves of one mz_train_run move,
 *     for a host that exchanges the count itself (torch.distributed, a Julia
 *     Distributed host): mz_train_move plays one move and returns the games it
 *     saved on this rank (*nfin); mz_train_learn takes `steps` learner steps
 *     (capped at training_steps) with the refreshes, state_out as above.
 *   mz_train_set_reanalyse: the Reanalyse worker inside mz_train_run.  With
 *     mode MZ_REAN_BY_VALUE or MZ_REAN_BY_SEARCH every move runs
 *     `rounds_per_move` rounds of mz_replay_reanalyse_next after its self-play
 *     and before its learner steps, with the learner's nets; round r of move
 *     key m has rng_step = m and game_offset = (the call's game_offset) +
 *     r * max_games.  The rounds are issued behind the move's launches and
 *     before the host waits for the move's finished-game count, so that wait
 *     overlaps them.  The results are those of the split loop with the same
 *     mz_replay_reanalyse_next calls between mz_train_move and mz_train_learn;
 *     mz_train_move / mz_train_learn themselves never reanalyse.  At world > 1
 *     every rank reanalyses its own shard, nothing is exchanged.  MZ_REAN_OFF
 *     (the default): no round, every launch as without the call.  Refused:
 *     rounds_per_move < 0, an unknown mode, and what mz_replay_reanalyse_next
 *     refuses.  The setting stays with the handle.
 *   mz_train_set_test: the test worker inside mz_train_run.  With interval > 0,
 *     after a move's learner steps took the learner from step t0 to t1 with
 *     t1 / interval > t0 / interval, the loop runs one evaluation:
 *     mz_test_play(h, t1, (uint32_t)t1 * (uint32_t)(max_moves + 1),
 *     game_offset, temperature, stream).  The move's learner steps run as one
 *     chunk and the chunk is not cut: the evaluation sees the nets after the
 *     move's last step (the latest-weights behaviour of an asynchronous test
 *     worker), at the point of the stream where the next move's Reanalyse
 *     rounds search with them too.  mz_train_move / mz_train_learn never
 *     evaluate; the split-loop host calls mz_test_play itself.  At world > 1
 *     every rank evaluates its own games: the condition is rank-invariant and
 *     nothing is exchanged.  interval 0 (the default): no evaluation, every
 *     launch as without the call.  Refused: a negative interval, and an
 *     interval > 0 with no test slots configured (mz_test_config; checked
 *     again by the evaluation).  The setting stays with the handle.
 *   mz_train_set_networks_path: conf.networks_path (Constructors.jl:47) for
 *     the periodic checkpoints; NULL or "" (the default) writes none.
 *   mz_train_weights_get: the learner's, actors' or queued nets (Flux order).
 * oracle/mz_oracle.c ora_train_loop restates it.                            */
enum { MZ_TRAIN_LEARNER = 0, MZ_TRAIN_ACTOR = 1, MZ_TRAIN_QUEUED = 2 };
int mz_train_init(mz_handle* h, int32_t batch_size);
int mz_train_init_at(mz_handle* h, int32_t batch_size, int64_t t0);
int mz_train_set_networks_path(mz_handle* h, const char* networks_path);
int mz_train_set_reanalyse(mz_handle* h, int mode, int rounds_per_move, int exploration);
int mz_train_set_test(mz_handle* h, int64_t interval, uint32_t game_offset, float temperature);
int mz_train_run(mz_handle* h, int32_t moves, uint32_t move0, uint32_t game_offset, int64_t* state_out,
                 float* losses_dev, void* stream);
int mz_train_move(mz_handle* h, uint32_t move, uint32_t game_offset, int64_t* nfin, void* stream);
int mz_train_learn(mz_handle* h, int64_t steps, float* losses_dev, int64_t* state_out, void* stream);
int mz_train_weights_get(mz_handle* h, int which, int net, float* flat, size_t n);

/* ---- The run log: per-interval loss and self-play records ------
 * The shared storage of the reference's job sketch (src/muzero.jl:11-33, "Write
 * everything in TensorBoard"; Learning.jl:416-424 prints the three losses at
 * every checkpoint), kept on the device: nothing is read back, nothing waits
 * on the host, and a job with the log on is bit for bit the job without it.
 *   mz_train_set_log: interval > 0 switches the log on, 0 (the default) off.
 *     A handle setting like mz_train_set_test's: mz_selfplay_init and
 *     mz_snapshot_load keep it, snapshots do not carry it.  The first interval
 *     > 0 allocates the accumulators, the loss rows of one learner chunk and
 *     the record ring; they live with the handle.  Switching the log on (from
 *     off) zeroes the accumulators and takes the games the shard has seen so
 *     far as not this log's; so do mz_selfplay_init and a passing
 *     mz_snapshot_load (the file's games are not this log's).  The ring and
 *     the record count survive all three.  Refused: a negative interval.
 *     With the log on, every move of mz_train_run / mz_train_move in
 *     MZ_SP_TRAIN mode is followed by one launch of mz_log_games, which folds
 *     the shard games numbered max(logged_upto, played - held) + 1 .. played
 *     (its own saves, and games mz_replay_save_game put in since the last
 *     move); games that were evicted before a fold reached them are counted as
 *     missed.  Every learner chunk of mz_train_run / mz_train_learn (up to 256
 *     steps) writes each step's six losses to the handle's rows and is
 *     followed by one launch of mz_log_steps; losses_dev gets a copy of the
 *     last row.  After a move's (mz_train_run) or a call's (mz_train_learn)
 *     learner steps took the learner from t0 to t1 with t1 / interval > t0 /
 *     interval, one launch of mz_log_commit writes one record and zeroes the
 *     accumulators (the chunk is not cut).  So the split loop gets the records
 *     mz_train_run gets.  At world > 1 every rank logs its own shard and
 *     steps; nothing is exchanged.  Off: none of the three is launched and
 *     every pointer is the caller's as without the call.
 *     Record e is kept in slot e % MZ_LOG_RECORDS of the ring.  Sums and
 *     counts, never means: the host divides.
 *       counts[16] = {training step t1 at the commit, learner steps folded
 *                     since the previous record, num_played_games,
 *                     num_played_steps, positions held (total_samples), games
 *                     held, the count mz_replay_reanalysed_count reads, games
 *                     folded since the previous record, their moves (Σ
 *                     length), wins of player 1, wins of player 2, draws,
 *                     actor refreshes (state_out[2]), games missed, 0, 0}
 *       sums[16]   = {Σ over the folded steps of value, reward, policy,
 *                     l2_repr, l2_pred, l2_dyn [0..5], the same six of the
 *                     last folded step alone [6..11] (zeros when no step was
 *                     folded), η = Cos(t1) [12], Σ rewards [13], Σ stored root
 *                     values [14] and Σ over the positions of max_a
 *                     child_visits[a] [15] of the folded games}
 *     counts[2..6] are the shard's words at the commit's point of the stream.
 *     Winner and draw: the engine's rule on each game's last record, as
 *     mz_eval_results reads them (TicTacToe, Q14: a nonzero reward is a win of
 *     3 - mover; every other env: of the mover; zero: a draw).  The numerics
 *     are part of the contract: the loss sums add (double) of each f32 loss in
 *     ascending step; a game's three sums start at +0 and add (double)x in
 *     record order, the maximum taken in f32; the accumulator adds the games'
 *     sums in ascending game number.  No float atomics.
 *     learning.run_log_record is the exact host mirror.
 *   mz_train_log_flush: one record now from whatever is accumulated (zero fold
 *     counts when nothing is), stream-ordered.  Refused before mz_train_init
 *     and with the log off.
 *   mz_train_log_results: the latest min(max_records, held) records, oldest
 *     first (held = min(total, MZ_LOG_RECORDS)); *total = records since create
 *     / mz_train_log_clear; counts [n][16], sums [n][16]; any pointer may be
 *     NULL.  Synchronises.  Refused: max_records < 0.
 *   mz_train_log_clear: total back to 0 and the accumulators zeroed (the games
 *     already folded stay folded).  Synchronises when the log was ever on.   */
enum { MZ_LOG_RECORDS = 1024 };
int mz_train_set_log(mz_handle* h, int64_t interval);
int mz_train_log_flush(mz_handle* h, void* stream);
int mz_train_log_results(mz_handle* h, int64_t* total, int64_t* counts, double* sums, int32_t max_records);
int mz_train_log_clear(mz_handle* h);

/* ---- Checkpoints -------------------------------------------
 * Replace serialize(joinpath(networks_path, "$(step)_<net>.bin"), net)
 * (Learning.jl:424-431) and play.jl's deserialize: one safetensors file with
 * the three nets' Flux.params arrays ("<net>.<i>", Julia column-major bytes,
 * shape = the Julia shape reversed), the ADAM moments and βp state, and
 * metadata (training_step, network kind, config).  Load checks every shape
 * against this engine and restores weights + optimiser state (resume).      */
int mz_checkpoint_save(mz_handle* h, const char* path, int64_t training_step);
int mz_checkpoint_load(mz_handle* h, const char* path, int64_t* training_step);

/* ---- Snapshots: exact resume ----------------------------------
 * A checkpoint holds the learner only.  A snapshot also holds the replay shard
 * (the held games' live rows, PER priorities, reanalysed values / policies and
 * flags, every counter word with the Reanalyse cursor and round header), the
 * games in progress (histories, boards, players, the Atari-like env's keys,
 * per-game temperatures, the evaluation tally, a still-pending initial reset)
 * and, after mz_train_init, the train loop (batch size, learner step, refresh
 * count, the actors' and the queued weight sets).  Every random draw is keyed
 * by (seed, step, game id), so a run cut in two by mz_snapshot_save -> any
 * engine of the same config and rng_seed -> mz_snapshot_load continues bit for
 * bit as the uncut run.  The reference has no counterpart (its buffer lives in
 * memory only; games/tictactoe/main.jl:21 leaves saving it as a TODO).
 *   mz_snapshot_save: one safetensors file (written to path + ".tmp", then
 *     renamed), a superset of a checkpoint: mz_checkpoint_load reads the
 *     learner's nets, ADAM state and training_step from it.  Only live rows
 *     are written: new kernels pack them on the device and the host streams
 *     them through one bounded staging buffer.  Tensor names: mz_snapshot.hip.
 *   mz_snapshot_load: parses and validates the whole file first (header, every
 *     game length, the row tensors' shapes against the lengths' prefix sums,
 *     the counters, network kind and shapes, env, observation_shape, actions,
 *     max_moves, PER, rng_seed, G <= max_games); a refused load leaves the
 *     engine exactly as it was.  Then it performs what mz_selfplay_init(env, G,
 *     cap) performs with the file's env, G and cap, restores the state and, if
 *     the file has a train section, what mz_train_init allocates; without one
 *     mz_train_run is refused until mz_train_init.  *training_step = the value
 *     given to mz_snapshot_save.
 * Both synchronise first and are valid between calls only, never inside a move.
 * Handle settings are NOT state: mz_train_set_reanalyse, mz_selfplay_mode,
 * mz_train_set_networks_path, mz_learner_set_mode and mz_debug_enable are
 * written into the metadata for information, and the loading host applies its
 * own (its mz_selfplay_mode, mz_expert_depth and opponent weight set survive
 * the load; the depth and the opponent set are not written to the file).
 * The test worker's settings (mz_test_config, mz_train_set_test,
 * mz_test_audit) and its record and audit rings are handle settings too, as
 * are mz_expert_table's switch and table: not written, and they survive the
 * load; the test slots are re-created by the next mz_test_play.  The run log
 * (mz_train_set_log) likewise: its setting, ring and record count survive the
 * load, its accumulators start over.
 * At world > 1 each rank saves
 * and loads its own file; the host orders the calls.                          */
int mz_snapshot_save(mz_handle* h, const char* path, int64_t training_step);
int mz_snapshot_load(mz_handle* h, const char* path, int64_t* training_step);

/* Name of the search kernel variant the last search launched (for profiles):
 * mz_search_small{1,2,4} (T games per workgroup, G <= 4 x #CUs) or the
 * 16-game MFMA tile kernel mz_search_kernel_{lds,hbm}[_res].  Environment
 * MZ_SEARCH_KERNEL=tile16|small (read at create) forces a family.          */
const char* mz_search_variant(const mz_handle* h);

/* The learner unroll's kernels of the last ResNet learner step, "+"-joined
 * (e.g. mz_runroll_chain_r+mz_runroll_pred_n1), for profiles; "none" before. */
const char* mz_learner_variant(const mz_handle* h);

/* Games per tile of the ResNet network kernels (rn_ng: the widest of 16, 8, 4,
 * 2, 1 whose three plans fit the LDS with their k tables below LDS offset
 * 32768, chosen at create); 0 for the FC nets.                              */
int mz_resnet_tile_games(const mz_handle* h);

/* Whether mz_downsample_kernel stages the observation in LDS for its first
 * layer (DsPlan.stage_in, chosen at create: 1 when the observation's floats
 * are a multiple of 4, two activation buffers plus every conv's parameters
 * fit in them, and the staged layout fits the LDS; 0 when layer 0 reads the
 * observation from HBM); -1 without a downsampler (ResNetHP.downsample unset,
 * or the FC nets).                                                           */
int mz_downsample_staged(const mz_handle* h);

/* Wait for the engine's work (the device, or the pair mz_set_sync_stream
 * named) and report a device fault.  A kernel that gives up waiting for a
 * cross-workgroup publish (a bounded poll, 2 s) sets a fault word instead of
 * hanging; this and every host-synchronous call then fail once with the
 * message.  What it invalidates: the outputs of the launches since the last
 * synchronisation — search results, the games self-play stored from them in
 * the replay shard, losses and read-outs.  The ref_semantics weights and
 * ADAM state stay valid (their update does not read those outputs, Q11);
 * after a fault re-create the shard (mz_selfplay_init) before training on it. */
int mz_sync(mz_handle* h);

#ifdef __cplusplus
}
#endif

#endif /* MZ_H */
