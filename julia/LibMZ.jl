# LibMZ.jl — the Julia binding of libmz (include/mz.h) a MuZero.jl maintainer
# adds to the reference (deveshjawla/MuZero.jl), next to src/SelfPlay.jl and
# src/Learning.jl.  Every `ccall` matches include/mz.h: Cint status (0 = OK),
# 1-based actions, column-major arrays in the reference's own shapes, so Julia
# arrays pass with no transpose.  The executable mirror of this file is
# muzero.jl_amd/abi.py (ctypes); this image has no Julia toolchain, so the file
# is reviewed, not run (INTEGRATION.md).
module LibMZ

using Flux: params, relu, tanh

const libmz = get(ENV, "LIBMZ", joinpath(@__DIR__, "..", "muzero.jl_amd", "lib", "libmz.so"))

# ---- PODs: field order and types exactly as include/mz.h --------------------
struct MzConfig                         # Config, src/Constructors.jl:18-52
    seed::Int32; observation_shape::NTuple{3,Int32}; action_space_size::Int32; players::Int32
    stacked_observations::Int32; muzero_player::Int32; intermediate_rewards::Int32
    num_workers::Int32; selfplay_on_gpu::Int32; max_moves::Int32; temperature_threshold::Int32
    dirichlet_alpha::Float32; exploration_eps::Float32; pb_c_base::Int32; pb_c_init::Float32
    discount::Float32; num_iters::Int32; replay_buffer_size::Int32; num_unroll_steps::Int32
    td_steps::Int32; PER::Int32; PER_alpha::Int32; training_steps::Int32; batch_size::Int32
    checkpoint_interval::Int32; value_loss_weight::Float32
end
struct MzFFHP                           # FeedForwardHP, src/Constructors.jl:62-75
    width_hidden::Int32; depth_representation::Int32; depth_prediction::Int32; depth_dynamics::Int32
    depth_policy::Int32; depth_value::Int32; depth_reward::Int32; depth_state_head::Int32
    use_batch_norm::Int32; batch_norm_momentum::Float32; hidden_state_size::Int32; reward_activation::Int32
end
struct MzResNetHP                       # ResNetHP, src/Constructors.jl:77-90 (+ the fields its heads read, Q12)
    num_blocks::Int32; num_filters::Int32; conv_kernel_size::NTuple{2,Int32}
    num_second_head_filters::Int32; num_first_head_filters::Int32; batch_norm_momentum::Float32
    downsample::Int32; depth_policy::Int32; depth_value::Int32; width_hidden::Int32; reward_activation::Int32
end
struct MzBatch                          # the tuple of get_batch, src/ReplayBuffer.jl:216
    batch_size::Int32
    observation::Ptr{Float32}; actions::Ptr{Float32}; target_values::Ptr{Float32}
    target_rewards::Ptr{Float32}; target_policies::Ptr{Float32}; gradient_scale::Ptr{Float32}
    weights::Ptr{Float32}               # weight_batch (:211-215); C_NULL without PER
end

const NET_REPR, NET_PRED, NET_DYN = Cint(0), Cint(1), Cint(2)
const ACT_IDENTITY, ACT_RELU, ACT_TANH = Int32(0), Int32(1), Int32(2)
const ENV_TICTACTOE, ENV_CONNECT4, ENV_ATARI = Cint(0), Cint(1), Cint(2)   # ENV_ATARI: the synthetic frame-stacked env of configs[4]
const SP_TRAIN, SP_EVAL, OPP_SELF, OPP_RANDOM, OPP_EXPERT = Cint(0), Cint(1), Cint(0), Cint(1), Cint(2)
const OPP_NETWORK = Cint(3)
const OPP_MCTS = OPP_NETWORK + Cint(1)          # 4 = MZ_OPP_MCTS: the next opponent id
const PLAYER_SEARCH, PLAYER_PRIOR = Cint(0), Cint(1)   # mz_eval_players: the search, the network-only player
const LEARN_REF_SEMANTICS, LEARN_CORRECTED = Cint(0), Cint(1)
const TRAIN_LEARNER, TRAIN_ACTOR, TRAIN_QUEUED = Cint(0), Cint(1), Cint(2)
const REAN_OFF, REAN_BY_VALUE, REAN_BY_SEARCH = Cint(0), Cint(1), Cint(2)

act_code(f) = f === tanh ? ACT_TANH : f === relu ? ACT_RELU : ACT_IDENTITY

MzConfig(c) = MzConfig(c.seed, Int32.(c.observation_shape), length(c.action_space), length(c.players),
    c.stacked_observations, c.muzero_player, c.intermediate_rewards, c.num_workers, c.selfplay_on_gpu,
    c.max_moves, something(c.temperature_threshold, -1), c.dirichlet_α, c.exploration_ϵ, c.pb_c_base,
    c.pb_c_init, c.discount, c.num_iters, c.replay_buffer_size, c.num_unroll_steps, c.td_steps, c.PER,
    c.PER_alpha, c.training_steps, c.batch_size, c.checkpoint_interval, c.value_loss_weight)
MzFFHP(h) = MzFFHP(h.width_hidden, h.depth_representation, h.depth_prediction, h.depth_dynamics,
    h.depth_policy, h.depth_value, h.depth_reward, h.depth_state_head, h.use_batch_norm,
    h.batch_norm_momentum, h.hidden_state_size, act_code(h.reward_activation))
# ResNetHP declares neither width_hidden nor reward_activation although its heads read them (Q12)
MzResNetHP(h; width_hidden=64, reward_activation=tanh) = MzResNetHP(h.num_blocks, h.num_filters,
    Int32.(h.conv_kernel_size), h.num_second_head_filters, h.num_first_head_filters, h.batch_norm_momentum,
    h.downsample, h.depth_policy, h.depth_value, width_hidden, act_code(reward_activation))

mutable struct Engine
    h::Ptr{Cvoid}
end

last_error(e::Engine) = unsafe_string(ccall((:mz_last_error, libmz), Cstring, (Ptr{Cvoid},), e.h))
check(e::Engine, rc) = rc == 0 || error("libmz: ", last_error(e))

"""Engine(conf, hyper; device, max_games, rng_seed) — replaces init_representation /
init_prediction / init_dynamics (src/Learning.jl:87-142, 148-255) and the process
setup of games/tictactoe/main.jl:15-28.  One engine per GPU."""
function Engine(conf, hyper; device=0, max_games=512, rng_seed=UInt64(1234))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if hasproperty(hyper, :num_filters)            # ResNetHP
        ccall((:mz_engine_create_resnet, libmz), Cint,
              (Ref{MzConfig}, Ref{MzResNetHP}, Cint, Cint, UInt64, Ref{Ptr{Cvoid}}),
              MzConfig(conf), MzResNetHP(hyper), device, max_games, rng_seed, out)
    else
        ccall((:mz_engine_create, libmz), Cint,
              (Ref{MzConfig}, Ref{MzFFHP}, Cint, Cint, UInt64, Ref{Ptr{Cvoid}}),
              MzConfig(conf), MzFFHP(hyper), device, max_games, rng_seed, out)
    end
    rc == 0 || error("libmz: ", unsafe_string(ccall((:mz_create_error, libmz), Cstring, ())))
    e = Engine(out[])
    finalizer(x -> ccall((:mz_engine_destroy, libmz), Cvoid, (Ptr{Cvoid},), x.h), e)
    return e
end

# ---- weights: vcat(vec.(Flux.params(net))...) (Dense: W (out,in) column-major, then b)
function set_weights!(e::Engine, net::Cint, chain)
    flat = reduce(vcat, vec.(collect(params(chain))))
    check(e, ccall((:mz_weights_set, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t),
                   e.h, net, flat, length(flat)))
end
function get_weights(e::Engine, net::Cint)
    n = Ref{Csize_t}(0)
    check(e, ccall((:mz_net_param_count, libmz), Cint, (Ptr{Cvoid}, Cint, Ref{Csize_t}), e.h, net, n))
    flat = Vector{Float32}(undef, n[])
    check(e, ccall((:mz_weights_get, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t), e.h, net, flat, n[]))
    flat
end
set_nets!(e::Engine, NNs) = (set_weights!(e, NET_REPR, NNs.representation);
                             set_weights!(e, NET_PRED, NNs.prediction); set_weights!(e, NET_DYN, NNs.dynamics))

# the Chain call (src/Learning.jl:87-142): x (W,H,C,N) -> out0 (and out1 for PRED / DYN)
forward!(e::Engine, net::Cint, x::Array{Float32}, out0::Array{Float32}, out1=nothing) =
    check(e, ccall((:mz_net_forward, libmz), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Float32}, Cint, Ptr{Float32}, Ptr{Float32}),
                   e.h, net, x, size(x, ndims(x)), out0, out1 === nothing ? C_NULL : out1))

"""mcts_search!(e, obs (W,H,Cs,G), legal (A,G) UInt8, to_play (G)) — G × (run_mcts +
select_action + store_search_stats!), src/SelfPlay.jl:230-306, 115-122."""
function mcts_search!(e::Engine, obs::Array{Float32,4}, legal::Matrix{UInt8}, to_play::Vector{Int32};
                      exploration=true, rng_step::Integer, game_offset::Integer=0, temperature::Float32=1f0)
    G = size(obs, 4); A = size(legal, 1)
    child_visits = Matrix{Float32}(undef, A, G); root_value = Vector{Float32}(undef, G)
    action = Vector{Int32}(undef, G)
    check(e, ccall((:mz_mcts_search, libmz), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{UInt8}, Ptr{Int32}, Cint, UInt32, UInt32, Float32,
                    Ptr{Float32}, Ptr{Float32}, Ptr{Int32}),
                   e.h, G, obs, legal, to_play, exploration, rng_step, game_offset, temperature,
                   child_visits, root_value, action))
    return child_visits, root_value, action
end

"""debug_select_stats(e, G) — per game of the last small-kernel search (after
mz_debug_enable flag 1): simulations whose leaf the ballot select found, and
simulations that entered the serial walk."""
debug_enable!(e::Engine, flags::Integer=1) =
    check(e, ccall((:mz_debug_enable, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, flags))
function debug_select_stats(e::Engine, G::Integer)
    fast = Vector{Int32}(undef, G); walked = Vector{Int32}(undef, G)
    check(e, ccall((:mz_debug_select_stats, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}, Ptr{Int32}),
                   e.h, G, fast, walked))
    return fast, walked
end

# ParameterSchedulers 0.2.3 Cos(λ0=1e-4, λ1=1e-1, period=10) under Stateful (src/Learning.jl:319, 382);
# the caller keeps the schedule (`next!(schedule)`) and passes eta
cos_eta(t) = abs(1e-4 - 1e-1) * (1 + cos(2π * (t - 1) / 10)) / 2 + min(1e-4, 1e-1)

"""learner_step!(e, batch, eta) — one learning! iteration (src/Learning.jl:327-413) on
batch = get_batch(buffer)[2]; eta = next!(schedule) (:382).  Returns the losses
(value, reward, policy, Σθ² of repr / pred / dyn)."""
function learner_step!(e::Engine, batch, eta::Real)
    obs, acts, tv, tr, tp, w, gs = batch
    acts32 = Float32.(acts)
    losses = Vector{Float32}(undef, 6)
    GC.@preserve obs acts32 tv tr tp w gs begin
        b = MzBatch(size(obs, 4), pointer(obs), pointer(acts32), pointer(tv), pointer(tr), pointer(tp),
                    pointer(gs), w === nothing ? C_NULL : pointer(w))
        check(e, ccall((:mz_learner_step, libmz), Cint, (Ptr{Cvoid}, Ref{MzBatch}, Float64, Ptr{Float32}),
                       e.h, b, Float64(eta), losses))
    end
    return losses
end

"""learner_mode!(e, LEARN_CORRECTED) — real backpropagation through the unroll
(FC nets with or without BatchNorm, ResNet nets with or without the downsampler) instead of the reference's
∇ = 2θ (quirk Q11)."""
learner_mode!(e::Engine, mode::Cint) =
    check(e, ccall((:mz_learner_set_mode, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, mode))

"""downsample_staged(e) — 1 / 0: the downsampler stages the observation in LDS for its first layer or reads it
from HBM (chosen at create); -1 without a downsampler."""
downsample_staged(e::Engine) = ccall((:mz_downsample_staged, libmz), Cint, (Ptr{Cvoid},), e.h)

# ---- device self-play and replay shard (play_game's loop body + ReplayBuffer.jl on the GPU)
selfplay_init!(e::Engine, env::Cint, G, replay_games) =
    check(e, ccall((:mz_selfplay_init, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Cint), e.h, env, G, replay_games))
selfplay_move!(e::Engine, step; offset=0, temperature=1f0) =
    check(e, ccall((:mz_selfplay_move, libmz), Cint, (Ptr{Cvoid}, UInt32, UInt32, Float32, Ptr{Cvoid}),
                   e.h, step, offset, temperature, C_NULL))
selfplay_mode!(e::Engine, mode::Cint; opponent=OPP_SELF, mzp=1) =
    check(e, ccall((:mz_selfplay_mode, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Cint), e.h, mode, opponent, mzp))
# OPP_EXPERT (Config.opponent = "expert"): the rules search on the device; depth 1..9, 0 = the env's default
expert_depth!(e::Engine, depth=0) =
    check(e, ccall((:mz_expert_depth, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, depth))
"""expert_eval(e, env, boards (W*H*3, G) UInt8 planes [p1, p2, empty], players (G), depth) — the expert's
scores (A, G), -128 for an illegal action: what would the expert play here."""
function expert_eval(e::Engine, env::Cint, boards::Matrix{UInt8}, players::Vector{Int32}, depth::Integer, A::Integer)
    scores = Matrix{Int32}(undef, A, size(boards, 2))
    check(e, ccall((:mz_expert_eval, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ptr{Int32}, Cint, Ptr{Int32}),
                   e.h, env, size(boards, 2), boards, players, depth, scores))
    scores
end
# the solved TicTacToe table (DESIGN §18.1): a handle setting; on: built once, and the depth-9 TicTacToe
# expert's move is a lookup (bit for bit the search's)
expert_table!(e::Engine, on::Bool=true) =
    check(e, ccall((:mz_expert_table, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, on ? 1 : 0))
"""expert_table_get(e) — (scores Int8 (9, 19683) or nothing, built, in_use): column code + 1, code = Σ 3^cell · d
(d = 0 empty, 1 the mover's stone, 2 the other's), holds score(s, a, 9), -128 for an illegal action."""
function expert_table_get(e::Engine)
    built = Ref{Int32}(0); in_use = Ref{Int32}(0)
    check(e, ccall((:mz_expert_table_get, libmz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ref{Int32}),
                   e.h, C_NULL, built, in_use))
    built[] == 0 && return (nothing, false, in_use[] != 0)
    scores = Matrix{Int8}(undef, 9, 19683)
    check(e, ccall((:mz_expert_table_get, libmz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int32}, Ref{Int32}),
                   e.h, scores, built, in_use))
    (scores, true, in_use[] != 0)
end
"""expert_judge(e, env, boards (W*H*3, G), players (G), actions (G, 1-based), depth) — the judge's rule on given
moves: (moves judged, in the expert's best set, win or draw given away, score deficit)."""
function expert_judge(e::Engine, env::Cint, boards::Matrix{UInt8}, players::Vector{Int32}, actions::Vector{Int32},
                      depth::Integer)
    out = zeros(Int64, 4)
    check(e, ccall((:mz_expert_judge, libmz), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Cint, Ptr{Int64}),
                   e.h, env, size(boards, 2), boards, players, actions, depth, out))
    out
end
# OPP_MCTS (DESIGN §22): vanilla MCTS over the true rules with random rollouts on the device; sims 1..1024,
# rollouts 1..64 per simulation, 0 = the default (64, 16); a handle setting like expert_depth!
mcts_opponent!(e::Engine, sims=0, rollouts=0) =
    check(e, ccall((:mz_mcts_opponent, libmz), Cint, (Ptr{Cvoid}, Cint, Cint), e.h, sims, rollouts))
"""mcts_eval(e, env, boards (W*H*3, G), players (G), sims, rollouts, A; rng_step, game_offset) — the MCTS
opponent's root statistics (n, w), each (A, G): the simulations through every root action and the sum of their
outcomes for the player to move, in rollouts; n = -1 for an illegal action."""
function mcts_eval(e::Engine, env::Cint, boards::Matrix{UInt8}, players::Vector{Int32}, sims::Integer,
                   rollouts::Integer, A::Integer; rng_step=0, game_offset=0)
    n = Matrix{Int32}(undef, A, size(boards, 2)); w = Matrix{Int32}(undef, A, size(boards, 2))
    check(e, ccall((:mz_mcts_eval, libmz), Cint,
                   (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ptr{Int32}, Cint, Cint, UInt32, UInt32, Ptr{Int32}, Ptr{Int32}),
                   e.h, env, size(boards, 2), boards, players, sims, rollouts, rng_step, game_offset, n, w))
    (n, w)
end
# The network-only player (DESIGN §24; AlphaZero.jl's NetworkOnly): a handle setting like expert_depth!; which
# player (PLAYER_SEARCH / PLAYER_PRIOR) produces MuZero's rows and the other network side's rows in evaluation play
eval_players!(e::Engine, muzero_kind::Cint=PLAYER_SEARCH, other_kind::Cint=PLAYER_SEARCH) =
    check(e, ccall((:mz_eval_players, libmz), Cint, (Ptr{Cvoid}, Cint, Cint), e.h, muzero_kind, other_kind))
"""prior_eval(e, obs (features, G), legal (A, G) UInt8; opponent_set, rng_step, game_offset, temperature) — the
policy head's move with no tree: (policy (A, G) = its softmax renormalised over the legal actions, value (G),
action (G) 1-based).  opponent_set = 1: the opponent weight set's nets."""
function prior_eval(e::Engine, obs::Matrix{Float32}, legal::Matrix{UInt8}; opponent_set=0, rng_step=0,
                    game_offset=0, temperature=0f0)
    A, G = size(legal)
    policy = Matrix{Float32}(undef, A, G); value = Vector{Float32}(undef, G); action = Vector{Int32}(undef, G)
    check(e, ccall((:mz_prior_eval, libmz), Cint,
                   (Ptr{Cvoid}, Cint, Ptr{Float32}, Ptr{UInt8}, Cint, UInt32, UInt32, Float32, Ptr{Float32},
                    Ptr{Float32}, Ptr{Int32}),
                   e.h, G, obs, legal, opponent_set, rng_step, game_offset, temperature, policy, value, action))
    (policy, value, action)
end
# Board-symmetry augmentation of the device get_batch (DESIGN §23): a handle setting like expert_depth!;
# on: every sample of every device get_batch is drawn under a random element of the env's symmetry group
# (TicTacToe 8, Connect4 2), keyed by the Philox SYMMETRY stream
replay_set_symmetry!(e::Engine, on::Bool=true) =
    check(e, ccall((:mz_replay_set_symmetry, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, on ? 1 : 0))
"""replay_symmetry_get(e, P, A) — (cell_perm (P, n), action_perm (A, n) 0-based, on): column s + 1 = where
each cell / action goes under element s."""
function replay_symmetry_get(e::Engine, P::Integer, A::Integer)
    n = Ref{Int32}(0); on = Ref{Int32}(0)
    check(e, ccall((:mz_replay_symmetry_get, libmz), Cint,
                   (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}, Ptr{Int32}, Ref{Int32}), e.h, n, C_NULL, C_NULL, on))
    cell = Matrix{Int32}(undef, P, n[]); act = Matrix{Int32}(undef, A, n[])
    check(e, ccall((:mz_replay_symmetry_get, libmz), Cint,
                   (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}, Ptr{Int32}, Ref{Int32}), e.h, n, cell, act, on))
    (cell, act, on[] != 0)
end
# the same transform of a device batch the caller assembled: row b under element ids[b] (a device Int32
# vector) into the distinct device arrays of `dst`
batch_symmetry!(e::Engine, src::MzBatch, ids::Ptr{Int32}, dst::MzBatch) =
    check(e, ccall((:mz_batch_symmetry, libmz), Cint, (Ptr{Cvoid}, Ref{MzBatch}, Ptr{Int32}, Ref{MzBatch}, Ptr{Cvoid}),
                   e.h, src, ids, dst, C_NULL))
# OPP_NETWORK: the opponent's weight set (a handle setting; complete after all three nets, one
# opponent_from! or one opponent_load!), then selfplay_mode!(e, SP_EVAL; opponent=OPP_NETWORK, mzp=...)
function opponent_set_weights!(e::Engine, net::Cint, chain)
    flat = reduce(vcat, vec.(collect(params(chain))))
    check(e, ccall((:mz_opponent_weights_set, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t),
                   e.h, net, flat, length(flat)))
end
function opponent_get_weights(e::Engine, net::Cint)
    flat = similar(get_weights(e, net))
    check(e, ccall((:mz_opponent_weights_get, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Float32}, Csize_t),
                   e.h, net, flat, length(flat)))
    flat
end
opponent_from!(e::Engine, which::Cint) =       # TRAIN_LEARNER | TRAIN_ACTOR | TRAIN_QUEUED, a device copy
    check(e, ccall((:mz_opponent_from, libmz), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}), e.h, which, C_NULL))
function opponent_load!(e::Engine, path)       # a checkpoint or snapshot file's nets; the learner is not touched
    step = Ref{Int64}(0)
    check(e, ccall((:mz_opponent_load, libmz), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), e.h, path, step))
    step[]
end
function eval_results(e::Engine)              # competitive_play!: (games, MuZero wins, opponent wins, draws)
    r = zeros(Int64, 4)
    check(e, ccall((:mz_eval_results, libmz), Cint, (Ptr{Cvoid}, Ptr{Int64}), e.h, r))
    Tuple(r)
end
function replay_counts(e::Engine)              # (num_played_games, num_played_steps, total_samples), held
    c = zeros(Int64, 3); held = Ref{Int32}(0)
    check(e, ccall((:mz_replay_counts, libmz), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int32}), e.h, c, held))
    Tuple(c), held[]
end
learner_train!(e::Engine, B, step, eta; losses=C_NULL) =  # get_batch + learning! on the device shard
    check(e, ccall((:mz_learner_train_dev, libmz), Cint, (Ptr{Cvoid}, Int32, UInt32, Float64, Ptr{Float32}, Ptr{Cvoid}),
                   e.h, B, step, eta, losses, C_NULL))
# length(etas) consecutive learning! iterations from step0 (ref_semantics, Q11: the ADAM chain in one
# launch, the unrolls side by side in a second); losses: C_NULL or a device [8, L] buffer
learner_train_multi!(e::Engine, B, step0, etas::Vector{Float64}; losses=C_NULL) =
    check(e, ccall((:mz_learner_train_multi_dev, libmz), Cint,
                   (Ptr{Cvoid}, Int32, UInt32, Int32, Ptr{Float64}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
                   e.h, B, step0, length(etas), etas, losses, C_NULL, C_NULL))

# Reanalyze (src/ReplayBuffer.jl:8, 56-67; the worker src/muzero.jl:15-19 leaves unbuilt) on the device shard:
# games first .. first+count-1 (0 = oldest held, count < 0 = all held) get reanalysed_predicted_root_values from
# the current networks, stream-ordered; targets drawn afterwards bootstrap from them.  In the split loop call it
# between train_move! and train_learn!.
reanalyse!(e::Engine; first=0, count=-1) =
    check(e, ccall((:mz_replay_reanalyse, libmz), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}), e.h, first, count, C_NULL))
clear_reanalysed!(e::Engine) =                 # every held game back to `nothing`
    check(e, ccall((:mz_replay_clear_reanalysed, libmz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), e.h, C_NULL))
function reanalysed_count(e::Engine)           # num_reanalysed_games
    n = Ref{Int64}(0)
    check(e, ccall((:mz_replay_reanalysed_count, libmz), Cint, (Ptr{Cvoid}, Ref{Int64}), e.h, n))
    n[]
end
function get_reanalysed(e::Engine, i, max_moves)   # shard game i: `nothing`, or max_moves + 1 values (the game's first T hold)
    set = Ref{Int32}(0); v = zeros(Float32, max_moves + 1)
    check(e, ccall((:mz_replay_get_reanalysed, libmz), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float32}), e.h, i, set, v))
    set[] == 0 ? nothing : v
end

# The other half of Reanalyze: the selected games' stored positions are searched again with the current networks;
# their child_visits become the policy targets and the search's root values the bootstrap values.  Position pos of
# selected game gi is searched as the game with Philox id game_offset + gi*(max_moves+1) + pos at rng_step.
reanalyse_search!(e::Engine; first=0, count=-1, exploration=false, rng_step=0, game_offset=0) =
    check(e, ccall((:mz_replay_reanalyse_search, libmz), Cint,
                   (Ptr{Cvoid}, Int32, Int32, Cint, UInt32, UInt32, Ptr{Cvoid}),
                   e.h, first, count, exploration ? 1 : 0, rng_step, game_offset, C_NULL))
function get_reanalysed_policies(e::Engine, i, A, max_moves)   # shard game i: `nothing`, or (A, max_moves + 1) child_visits
    set = Ref{Int32}(0); cv = zeros(Float32, A, max_moves + 1)
    check(e, ccall((:mz_replay_get_reanalysed_policies, libmz), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Float32}),
                   e.h, i, set, cv))
    set[] == 0 ? nothing : cv
end

# The Reanalyse worker: one round of whole games from the shard's cursor (a game number; the device picks as many
# games as fit max_games rows in search mode, 4096 in value mode, and packs only their stored positions), stream-ordered
# with no read-back.  Search mode: row i of the round is the game with Philox id game_offset + i at rng_step.
reanalyse_next!(e::Engine, mode::Cint; exploration=false, rng_step=0, game_offset=0) =
    check(e, ccall((:mz_replay_reanalyse_next, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, UInt32, UInt32, Ptr{Cvoid}),
                   e.h, mode, exploration ? 1 : 0, rng_step, game_offset, C_NULL))
function reanalyse_cursor(e::Engine)           # (next game number, (first game number, games, rows) of the last round)
    c = Ref{Int64}(0); r = zeros(Int64, 3)
    check(e, ccall((:mz_replay_reanalyse_cursor, libmz), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}), e.h, c, r))
    c[], Tuple(r)
end
reanalyse_seek!(e::Engine, game_number) =
    check(e, ccall((:mz_replay_reanalyse_seek, libmz), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}), e.h, game_number, C_NULL))
# train_run! then runs `rounds_per_move` such rounds every move, after its self-play and before its learner steps
# (REAN_OFF, the default: none)
train_set_reanalyse!(e::Engine, mode::Cint; rounds_per_move=1, exploration=false) =
    check(e, ccall((:mz_train_set_reanalyse, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Cint),
                   e.h, mode, rounds_per_move, exploration ? 1 : 0))

# ---- the test worker (muzero.jl:29-31's TODO; DESIGN §20): evaluation games on their own slots while a job trains
test_config!(e::Engine, games; opponent::Cint=OPP_SELF, muzero_player=1) =
    check(e, ccall((:mz_test_config, libmz), Cint, (Ptr{Cvoid}, Int32, Cint, Cint), e.h, games, opponent, muzero_player))
# one evaluation with the current nets: every test slot plays one game, one record is appended (stream-ordered)
test_play!(e::Engine, training_step, rng_step0; game_offset=0, temperature=0f0) =
    check(e, ccall((:mz_test_play, libmz), Cint, (Ptr{Cvoid}, Int64, UInt32, UInt32, Float32, Ptr{Cvoid}),
                   e.h, training_step, rng_step0, game_offset, temperature, C_NULL))
# (evaluations so far, counts (8, n): training_step, games, MuZero wins, opponent wins, draws, moves, value_moves,
#  rng_step0; sums (3, n): reward_muzero, reward_opponent, value_sum), the latest n records, oldest first
function test_results(e::Engine; max_records=1024)
    total = Ref{Int64}(0); counts = zeros(Int64, 8, max_records); sums = zeros(Float64, 3, max_records)
    check(e, ccall((:mz_test_results, libmz), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Int32),
                   e.h, total, counts, sums, max_records))
    n = min(max_records, total[], 1024)
    total[], counts[:, 1:n], sums[:, 1:n]
end
test_clear!(e::Engine) = check(e, ccall((:mz_test_clear, libmz), Cint, (Ptr{Cvoid},), e.h))
# judge MuZero's moves of the following evaluations by the expert's scores (DESIGN §20.1): a handle setting
test_audit!(e::Engine, on::Bool=true) =
    check(e, ccall((:mz_test_audit, libmz), Cint, (Ptr{Cvoid}, Cint), e.h, on ? 1 : 0))
# (evaluations so far, audit (4, n): moves judged, in the best set, win or draw given away, score deficit) of the
# records test_results returns, column for column; (-1, 0, 0, 0): that evaluation ran with judging off
function test_audit_results(e::Engine; max_records=1024)
    total = Ref{Int64}(0); audit = zeros(Int64, 4, max_records)
    check(e, ccall((:mz_test_audit_results, libmz), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Int32),
                   e.h, total, audit, max_records))
    total[], audit[:, 1:min(max_records, total[], 1024)]
end
function test_get_game(e::Engine, slot, osz, A, max_moves)   # test slot `slot`'s game of the last evaluation
    T = Ref{Int32}(0); M = max_moves + 1
    obs = zeros(UInt8, osz, M); act = zeros(Int32, M); rew = zeros(Float32, M); tp = zeros(Int32, M)
    cv = zeros(Float32, A, M); rv = zeros(Float32, M)
    check(e, ccall((:mz_test_get_game, libmz), Cint,
                   (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Float32},
                    Ptr{Float32}), e.h, slot, T, obs, act, rew, tp, cv, rv))
    n = T[]
    (obs[:, 1:n], act[1:n], rew[1:n], tp[1:n], cv[:, 1:n], rv[1:n])
end
# train_run! then evaluates after every move whose learner steps crossed a multiple of `interval` (0, the default: never)
train_set_test!(e::Engine, interval; game_offset=0, temperature=0f0) =
    check(e, ccall((:mz_train_set_test, libmz), Cint, (Ptr{Cvoid}, Int64, UInt32, Float32),
                   e.h, interval, game_offset, temperature))

# ---- the run log (DESIGN §21): per-interval loss and self-play records kept on the device.  train_run! /
# train_learn! then commit one record after every move / call whose learner steps crossed a multiple of `interval`
# (0, the default: the log is off)
train_set_log!(e::Engine, interval) =
    check(e, ccall((:mz_train_set_log, libmz), Cint, (Ptr{Cvoid}, Int64), e.h, interval))
# one record now from whatever is accumulated (stream-ordered)
train_log_flush!(e::Engine) = check(e, ccall((:mz_train_log_flush, libmz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), e.h, C_NULL))
# (records so far, counts (16, n), sums (16, n)), the latest n records, oldest first; the rows: include/mz.h.
# Sums and counts, never means: the host divides
function train_log_results(e::Engine; max_records=1024)
    total = Ref{Int64}(0); counts = zeros(Int64, 16, max_records); sums = zeros(Float64, 16, max_records)
    check(e, ccall((:mz_train_log_results, libmz), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Int32),
                   e.h, total, counts, sums, max_records))
    n = min(max_records, total[], 1024)
    total[], counts[:, 1:n], sums[:, 1:n]
end
train_log_clear!(e::Engine) = check(e, ccall((:mz_train_log_clear, libmz), Cint, (Ptr{Cvoid},), e.h))

"""The actor–learner loop of self_play! ‖ learning! (src/SelfPlay.jl:384-419,
src/Learning.jl:306-438; quirk Q16) on one GPU: `moves` self-play moves with the
actors' nets, one learner step per finished game, the actors one checkpoint behind.
Returns (learner step t, games played, actor refreshes, steps of this call)."""
train_init!(e::Engine, B) = check(e, ccall((:mz_train_init, libmz), Cint, (Ptr{Cvoid}, Int32), e.h, B))
function train_run!(e::Engine, moves; move0=0, offset=0)
    st = zeros(Int64, 4)
    check(e, ccall((:mz_train_run, libmz), Cint, (Ptr{Cvoid}, Int32, UInt32, UInt32, Ptr{Int64}, Ptr{Float32}, Ptr{Cvoid}),
                   e.h, moves, move0, offset, st, C_NULL, C_NULL))
    Tuple(st)
end
# the two halves of one train_run! move, for a Distributed.jl host that sums `nfin` over the workers itself:
# every worker then takes the global count of learner steps (the replicas stay identical, SURVEY §8e)
function train_move!(e::Engine, move; offset=0)
    n = zeros(Int64, 1)
    check(e, ccall((:mz_train_move, libmz), Cint, (Ptr{Cvoid}, UInt32, UInt32, Ptr{Int64}, Ptr{Cvoid}),
                   e.h, move, offset, n, C_NULL))
    n[1]
end
function train_learn!(e::Engine, steps)
    st = zeros(Int64, 4)
    check(e, ccall((:mz_train_learn, libmz), Cint, (Ptr{Cvoid}, Int64, Ptr{Float32}, Ptr{Int64}, Ptr{Cvoid}),
                   e.h, steps, C_NULL, st, C_NULL))
    Tuple(st)
end
function train_weights(e::Engine, which::Cint, net::Cint)
    flat = similar(get_weights(e, net))
    check(e, ccall((:mz_train_weights_get, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float32}, Csize_t),
                   e.h, which, net, flat, length(flat)))
    flat
end

# host-synchronous calls wait only for `stream` (a HIP stream handle) and the engine's own; narrow=false: all work
set_sync_stream!(e::Engine, stream::Ptr{Cvoid}; narrow=true) =
    check(e, ccall((:mz_set_sync_stream, libmz), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), e.h, stream, Cint(narrow)))

# ---- data-parallel learner over RCCL without torch (one engine per GPU / Distributed.jl worker)
function dp_unique_id()                        # on rank 0; send the 128 bytes to the other workers
    id = zeros(UInt8, 128)
    ccall((:mz_dp_unique_id, libmz), Cint, (Ptr{UInt8},), id) == 0 || error("mz_dp_unique_id")
    id
end
dp_init!(e::Engine, rank, world, id) =
    check(e, ccall((:mz_dp_init, libmz), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), e.h, rank, world, id))
learner_train_dp!(e::Engine, B, step, eta; losses=C_NULL) =   # data term, RCCL all-reduce, ADAM(1/world, + 2θ)
    check(e, ccall((:mz_learner_train_dp, libmz), Cint, (Ptr{Cvoid}, Int32, UInt32, Float64, Ptr{Float32}, Ptr{Cvoid}),
                   e.h, B, step, eta, losses, C_NULL))

# ---- checkpoints (the safetensors file replacing serialize(...), src/Learning.jl:424-431)
checkpoint_save(e::Engine, path, step) =
    check(e, ccall((:mz_checkpoint_save, libmz), Cint, (Ptr{Cvoid}, Cstring, Int64), e.h, path, step))
function checkpoint_load!(e::Engine, path)
    step = Ref{Int64}(0)
    check(e, ccall((:mz_checkpoint_load, libmz), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), e.h, path, step))
    step[]
end

# ---- snapshots: the learner, the replay shard, the games in progress and the train loop (exact resume)
snapshot_save(e::Engine, path, step) =
    check(e, ccall((:mz_snapshot_save, libmz), Cint, (Ptr{Cvoid}, Cstring, Int64), e.h, path, step))
function snapshot_load!(e::Engine, path)
    step = Ref{Int64}(0)
    check(e, ccall((:mz_snapshot_load, libmz), Cint, (Ptr{Cvoid}, Cstring, Ref{Int64}), e.h, path, step))
    step[]
end

end # module
