/*
 * aigar.h -- C-ABI of the MI355X agar.io environment stepper (libaigar_hip.so).
 *
 * Drop-in boundary for the reference's hot path.  The
 * reference has no FFI: its boundary is the Python object API of
 * src/model/{field,model,player,cell,bot}.py.  Each entry point below names the
 * reference call it replaces; the Python facade in aigar_amd/ binds them with
 * ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - Every call returns int: 0 = OK, < 0 = error; aigar_last_error() gives the
 *    message (thread-local).  No C++ exception crosses the ABI.
 *  - One handle = one HIP device + one HIP stream.  Calls on a handle are
 *    serialised by the caller.  Handles on different devices may run
 *    concurrently (one process per GPU).
 *  - A handle owns n_arenas independent arenas ("fields") of bots_per_arena
 *    players each; arrays that span all arenas are arena-major:
 *    index = arena * bots_per_arena + player.
 *  - on_device = 0: caller passes host pointers (copied during the call);
 *    on_device = 1: device pointers on the handle's stream (e.g. torch tensors
 *    via data_ptr(); adopt torch's stream with aigar_set_stream()).
 *  - All state is fp64, like the reference (Python floats / numpy float64).
 */
#ifndef AIGAR_H
#define AIGAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIGAR_ABI_VERSION 7

/* random number stream of the world (spawns, explosion angles) */
#define AIGAR_RNG_PHILOX 0   /* Philox4x64-10 keyed by (seed, site, index): device + oracle */
#define AIGAR_RNG_MT19937 1  /* numpy legacy MT19937 stream, reference-exact: oracle only */

/* observation channels, in the reference's stacking order (bot.py:459-495) */
#define AIGAR_OBS_PELLET     0x001u  /* PELLET_GRID: pellet mass sum      */
#define AIGAR_OBS_SELF       0x002u  /* SELF_GRID: biggest own cell mass  */
#define AIGAR_OBS_WALL       0x004u  /* WALL_GRID: wall fraction (3 dp)   */
#define AIGAR_OBS_ENEMY      0x008u  /* ENEMY_GRID: biggest enemy mass    */
#define AIGAR_OBS_ALL        0x010u  /* ALL_PLAYER_GRID                   */
#define AIGAR_OBS_VIRUS      0x020u  /* VIRUS_GRID                        */
#define AIGAR_OBS_SELF_SLF   0x040u  /* SELF_GRID_SLF  (second-last frame)*/
#define AIGAR_OBS_SELF_LF    0x080u  /* SELF_GRID_LF   (last frame)       */
#define AIGAR_OBS_ENEMY_SLF  0x100u  /* ENEMY_GRID_SLF                    */
#define AIGAR_OBS_ENEMY_LF   0x200u  /* ENEMY_GRID_LF                     */
/* GRID_VIEW_ENABLED = False (networkParameters.py:119): getSimpleStateRepresentation
 * (bot.py:511-547) instead of the grids -- 12 values per bot (first own cell,
 * closest enemy cell, closest pellet, visible field edges); no grids, no extras */
#define AIGAR_OBS_SIMPLE     0x400u
/* extra inputs, in getAdditionalFeatures order (bot.py:302-323) */
#define AIGAR_EX_LAST_FOV    0x01u
#define AIGAR_EX_FOV         0x02u
#define AIGAR_EX_MASS        0x04u
#define AIGAR_EX_LAST_ACT    0x08u
#define AIGAR_EX_2LAST_ACT   0x10u

/* event codes (tick-ordered the way the reference performs them) */
#define AIGAR_EV_MERGE           1  /* (bigger seq, smaller seq)     field.py:372  */
#define AIGAR_EV_VIRUS_EAT_BLOB  2  /* (virus seq, blob seq)         field.py:316  */
#define AIGAR_EV_VIRUS_SPLIT     3  /* (virus seq, new virus seq)    field.py:318  */
#define AIGAR_EV_CELL_EAT_VIRUS  4  /* (cell seq, virus seq)         field.py:333  */
#define AIGAR_EV_EXPLODE         5  /* (cell seq, n new cells)       field.py:350  */
#define AIGAR_EV_CELL_EAT_PELLET 6  /* (cell seq, pellet seq)        field.py:327  */
#define AIGAR_EV_CELL_EAT_BLOB   7  /* (cell seq, blob seq)          field.py:330  */
#define AIGAR_EV_CELL_EAT_CELL   8  /* (eater seq, eaten seq)        field.py:346  */
#define AIGAR_EV_PLAYER_DEATH    9  /* (player index, last cell seq) field.py:386  */
#define AIGAR_EV_RESPAWN        10  /* (player index, new cell seq)  field.py:277  */

#define AIGAR_FLAG_EVENTS 0x1       /* record the event log of each step */
/* per-player mass history statistics, sampled on the device at the start of every
 * tick (aigar_score*; untiled handles only).  Without it no tick launches anything more */
#define AIGAR_FLAG_SCORE 0x2
/* tile_flags: decide only the cells this tile owns (the others wait for their
 * owners' messages) -- the strictest exchange pattern, used by the tests */
#define AIGAR_TILE_OWNED_ONLY 0x1
/* a 1 x 1 "tiled" handle: the whole field is one tile that still runs the tile
 * passes and the exchange (a 1-rank RCCL communicator: the one-GPU test of the
 * C4 exchange path) */
#define AIGAR_TILE_FORCE 0x2

typedef struct aigar_handle aigar_handle;

typedef struct aigar_config {
  int32_t n_arenas;        /* independent fields per handle (batched-env mode)        */
  int32_t bots_per_arena;  /* players per field                                       */
  int32_t field_size;      /* 0 -> int(75 * sqrt(bots)) (field.py:58)                 */
  int32_t virus_enabled;   /* Field(virusEnabled) (field.py:30, VIRUS_SPAWN)          */
  double max_pellets;      /* < 0 -> size*size*0.015 (field.py:65, parameters.py:16)  */
  double max_viruses;      /* < 0 -> size*size*5e-5 (field.py:66, parameters.py:17)   */
  int32_t grid_squares;    /* GRID_SQUARES_PER_FOV (networkParameters.py:97), or the CNN
                            * grid view's CNN_INPUT_DIM_* (bot.py:103-111: 42 / 84);
                            * 0 -> 11; at most 127                                     */
  uint32_t obs_channels;   /* AIGAR_OBS_* mask (networkParameters.py:76-96)           */
  uint32_t obs_extras;     /* AIGAR_EX_* mask (networkParameters.py:91-95)            */
  int32_t rng_mode;        /* AIGAR_RNG_*                                             */
  int32_t device;          /* HIP device ordinal                                      */
  int32_t pellet_cap;      /* 0 -> max_pellets + blob_cap + 64                        */
  int32_t blob_cap;        /* 0 -> 4 * bots + 256                                     */
  int32_t virus_cap;       /* 0 -> 2 * max_viruses + 64                               */
  int32_t event_cap;       /* events kept per arena per step (0 -> 65536)             */
  int32_t flags;           /* AIGAR_FLAG_*                                            */
  /* C4: one arena tiled 2-D over tile_x * tile_y handles, one per GPU (SURVEY.md
   * §8e).  1 x 1 (or 0 x 0) = untiled.  A tiled handle needs n_arenas == 1.     */
  int32_t tile_x, tile_y;  /* tiles along x and y                                     */
  int32_t tile_id;         /* this handle's tile, row-major: ty * tile_x + tx         */
  int32_t tile_halo;       /* pellets held beyond the tile, field units (0 -> 400;    *
                            * at least 140: an owned cell's reach; 370 covers any view) */
  int32_t tile_cap;        /* records per exchange message (0 -> 2048)                */
  int32_t tile_flags;      /* AIGAR_TILE_*                                            */
} aigar_config;

/*
 * Snapshot of one arena, the unit of parity.  Record layouts (row-major):
 *   players_f [n_players][2]  command point x, y          (player.py:99-102)
 *   players_i [n_players][5]  alive, respawnTime, doSplit, doEject, #cells
 *   cells_f   [n_cells][9]    x y mass radius vx vy svx svy mergeTime (cell.py:21-45)
 *   cells_i   [n_cells][4]    owner, splitVelocityCounter, seq, in_player_hash
 *             cells are grouped by owner in player order, each group in the
 *             player's cell-list order
 *   pellets_f [n_pellets][4]  x y mass radius, sorted by seq
 *   pellets_seq [n_pellets]
 *   blobs_f   [n_blobs][8]    x y mass radius vx vy svx svy (list order)
 *   blobs_i   [n_blobs][3]    svc, seq, ejecter cell seq
 *   viruses_f [n_viruses][8]  as blobs
 *   viruses_i [n_viruses][3]  svc, seq, in_virus_hash
 *   dead      [n_dead]        deadPlayers list (player indices, in order)
 * seq = creation sequence number of the Cell object (canonical order).
 * aigar_get_state: with NULL arrays only the counts are filled; otherwise the
 * n_* fields give the capacities of the caller's arrays on input.
 */
typedef struct aigar_state {
  int32_t n_players, field_size, virus_enabled, rng_mode;
  int64_t seq_next, tick;
  double max_pellets, max_viruses;
  uint64_t philox_key[2];
  uint64_t ctr_pellet, ctr_virus;
  uint32_t mt_key[624];
  int32_t mt_pos;
  int32_t n_cells, n_pellets, n_blobs, n_viruses, n_dead;
  double *players_f;
  int64_t *players_i;
  double *cells_f;
  int64_t *cells_i;
  double *pellets_f;
  int64_t *pellets_seq;
  double *blobs_f;
  int64_t *blobs_i;
  double *viruses_f;
  int64_t *viruses_i;
  int64_t *dead;
  /* optional (NULL: not exported / -1 on import): the player whose colour the
   * object carries -- an ejected blob its ejecting player's (field.py:141,
   * cell.py:219), a pellet made from a blob the blob's (field.py:110) -- or -1
   * for a pellet's / orphan blob's colour of its own (cell.py:31) */
  int64_t *pellets_col;  /* [n_pellets], in pellets_seq order */
  int64_t *blobs_col;    /* [n_blobs] */
} aigar_state;

const char *aigar_last_error(void);
int aigar_abi_version(void);

/* Field(virusEnabled) + Model bookkeeping: allocate all device buffers.
 * replaces model.py:51-73 / field.py:30-46 */
int aigar_create(const aigar_config *cfg, aigar_handle **out);
int aigar_destroy(aigar_handle *h);

/* Field.initialize()/Field.reset(): spawn every player, pellets, viruses.
 * replaces field.py:57-83 (model.py:90-98) */
int aigar_reset(aigar_handle *h, uint64_t seed);

/* Field.reset() of the listed arenas only (field.py:69-83) + every bot's reset in
 * those arenas; all other arenas are untouched.  Afterwards arena arenas[k] is the
 * world of a one-arena handle of the same config after aigar_reset(seeds[k]),
 * Philox key included (its arena word is 0, whatever the arena's index), and its
 * bots restart as after aigar_load_state: history grids, lastFovSize and
 * currentAction cleared, lastMass None, commands -1.  The arenas must be distinct;
 * n == 0 does nothing; tiled handles are refused.  Stream-ordered, no host round
 * trip: the lists are copied before the call returns, device errors surface at the
 * next call that checks them (aigar_step, aigar_get_state).  Captured graphs stay valid. */
int aigar_reset_arenas(aigar_handle *h, const int32_t *arenas, const uint64_t *seeds, int n);

/* Player.setCommands(x, y, split, eject) for every player: cmd[A*B][4].
 * replaces player.py:99-102 (called from bot.py:550-577) */
int aigar_set_commands(aigar_handle *h, const double *cmd, int on_device);

/* Synthetic bot population on the device (benchmark / smoke driver): every
 * alive player draws an action in [0,1]^2 mapped through the reference's
 * set_command_point (bot.py:550-577) and splits/ejects with p_split/p_eject.
 * The draws are Philox-keyed by (world key, seed, tick, player): a function of
 * the state, not of how many times the policy was called. */
int aigar_policy_random(aigar_handle *h, double p_split, double p_eject, uint64_t seed);

/* Model.takeBotActions for Greedy bots (bot.py:252-269 -> make_greedy_bot_move
 * bot.py:579-633 -> set_command_point bot.py:550-577): sets the command of every
 * alive player whose mask byte is non-zero (mask NULL: every player).
 * greedy_split = ENABLE_GREEDY_SPLIT (networkParameters.py:17).  Random draws
 * (fallback target, split dice) come from the Philox stream. */
int aigar_policy_greedy(aigar_handle *h, int greedy_split, const uint8_t *mask, int on_device);
/* Greedy bots' splitLikelihood (bot.py:93), [bots_per_arena] for one arena;
 * NULL: derive them from the Philox key (the default). */
int aigar_set_split_likelihood(aigar_handle *h, int arena, const int32_t *lh);

/* External (learner) actions for every player: act[A*B][n_act], n_act = 2, 3 or 4,
 * mapped through set_command_point (bot.py:550-577).  skipping: a frame-skip
 * frame, split/eject dropped (bot.py:266-267); record: a decision frame, the
 * observation's last / second-last action extras advance (bot.py:180-193) and
 * the live NN players' lastMass becomes their total mass (bot.py:228-230). */
int aigar_apply_actions(aigar_handle *h, const double *act, int n_act, int enable_split, int skipping, int record,
                        int on_device);

/* Bot.getReward (bot.py:654-667) for every player into out[A*B] (NaN = None);
 * update_last: lastMass <- total mass for live players (end of move_NN). */
typedef struct aigar_reward_params {
  int32_t mass_as_reward;  /* MASS_AS_REWARD (networkParameters.py:50) */
  int32_t pad;
  double reward_term;      /* REWARD_TERM  */
  double death_term;       /* DEATH_TERM   */
  double death_factor;     /* DEATH_FACTOR */
  double reward_scale;     /* REWARD_SCALE */
} aigar_reward_params;
int aigar_rewards(aigar_handle *h, double *out, const aigar_reward_params *p, int update_last, int on_device);

/* One learner decision for every player -- the NN bots' move_NN / updateRewards
 * / frame skipping (bot.py:166-233) batched, as aigar.py:performModelSteps
 * drives them: act[A*B][n_act] (n_act 2..4, DEVICE pointer) goes through
 * set_command_point (as aigar_apply_actions) and is held for skip + 1 ticks
 * (FRAME_SKIP_RATE; split/eject dropped on the skipped ticks), reward_out[A*B]
 * (DEVICE) gets the window's summed getReward (nothing is added for a player
 * without a lastMass, bot.py:167, also when the mass is the reward; lastMass is
 * set for the live NN players at the decision and advances for every live player
 * at the end), obs_out (DEVICE, as aigar_observe) every bot's observation.  The
 * whole decision is one hipGraph replay (re-captured when a pointer or a
 * parameter changes). */
int aigar_env_step(aigar_handle *h, const double *act, int n_act, int enable_split, int skip,
                   const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype);

/* n_ticks x Field.update() with the current commands (field.py:85-92). */
int aigar_step(aigar_handle *h, int n_ticks);

/* One whole batched env step, n_steps times: the bot policy (Model.takeBotActions,
 * model.py:100-105), Field.update() (field.py:85-92) and, when obs_out is not
 * NULL, every bot's getStateRepresentation (bot.py:272-299) into the DEVICE
 * buffer obs_out[A*B][aigar_obs_len()] (dtype as aigar_observe).  The step is
 * captured once as a single hipGraph (re-captured when the parameters or the
 * buffer change) and replayed, so no host round trip separates the phases;
 * a second graph holds AIGAR_RUN_UNROLL copies of the step (environment,
 * read at aigar_create; default 4) and carries n_steps / 4 of them (the rest
 * one step per replay) -- the same kernels in the same order, one graph launch
 * per 4 steps.
 * policy: AIGAR_POLICY_NONE keeps the current commands; RANDOM is
 * aigar_policy_random(p_split, p_eject, seed);
 * GREEDY is aigar_policy_greedy for every player.  With AIGAR_FLAG_EVENTS the
 * event log holds the events of all n_steps of the call. */
/* player roles of a batched population (aigar_set_roles) */
#define AIGAR_ROLE_NN     0  /* actions from the caller (learner): aigar_apply_actions / aigar_env_step */
#define AIGAR_ROLE_GREEDY 1  /* Greedy bot on the device (bot.py:579-633)                              */
#define AIGAR_ROLE_RANDOM 2  /* Random bot on the device (bot.py:243-249)                              */
#define AIGAR_POLICY_NONE   0
#define AIGAR_POLICY_RANDOM 1
#define AIGAR_POLICY_GREEDY 2
typedef struct aigar_run_params {
  int32_t policy;        /* AIGAR_POLICY_*                                   */
  int32_t greedy_split;  /* ENABLE_GREEDY_SPLIT (networkParameters.py:17)    */
  double p_split;        /* RANDOM: split probability per bot-tick           */
  double p_eject;        /* RANDOM: eject probability per bot-tick           */
  uint64_t seed;         /* RANDOM: Philox salt                              */
} aigar_run_params;
int aigar_run(aigar_handle *h, int n_steps, const aigar_run_params *p, void *obs_out, int dtype);

/* Bot.getStateRepresentation() for every player (bot.py:272-497):
 * out[A*B][aigar_obs_len()] (dtype 0 = float64, 1 = float32); dead players get NaN.
 * Updates each bot's last-frame history grids like the reference does. */
int aigar_obs_len(aigar_handle *h);
int aigar_observe(aigar_handle *h, void *out, int dtype, int on_device);
/* The same for the players whose mask byte is non-zero only (mask on the host, or on
 * the device when mask_on_device): the others' rows stay as they are in out and
 * their last-frame history does not advance -- the reference computes a state only
 * for the NN bots that are not skipping a frame (bot.py:195-202). */
int aigar_observe_masked(aigar_handle *h, void *out, int dtype, int on_device, const uint8_t *mask,
                         int mask_on_device);

/* Mixed populations (aigar.py:767-780: NN bots trained among Greedy and Random
 * bots): roles[A*B] of AIGAR_ROLE_* (NULL: every player NN).  aigar_env_step then
 * moves the Greedy and Random bots itself every tick (the learner's actions apply to
 * the NN players only) and observes the NN players only. */
int aigar_set_roles(aigar_handle *h, const uint8_t *roles, int on_device);
typedef struct aigar_env_params {
  int32_t greedy_split;   /* ENABLE_GREEDY_SPLIT (networkParameters.py:17)            */
  int32_t random_skip;    /* Random bots draw a new action every FRAME_SKIP_RATE moves */
  int32_t random_split;   /* ENABLE_SPLIT: Random bots draw a split value             */
  int32_t random_eject;   /* ENABLE_EJECT: Random bots draw an eject value            */
  uint64_t salt;          /* Philox salt of the Random bots' draws                    */
} aigar_env_params;
int aigar_env_config(aigar_handle *h, const aigar_env_params *p);
/* One Model.takeBotActions for the Random bots only (make_random_bot_move +
 * set_command_point, bot.py:243-269), with the aigar_env_config parameters. */
int aigar_policy_random_bots(aigar_handle *h);
/* RGBGenerator.get_cnn_inputRGB (rgbGenerator.py:95-110) for every player: a
 * side x side frame (side <= 84; CNN_INPUT_DIM_* of networkParameters.py) of
 * the player's FOV, objects drawn in stable mass order with SDL_gfx circle
 * primitives.  dtype 2: uint8 RGB out[A*B][side][side][3] in pygame surfarray
 * order [x][y][rgb]; 0 / 1: float64 / float32 grayscale out[A*B][side][side]
 * (numpy.average with weights 0.298, 0.587, 0.114).  color_seed picks the
 * per-player / per-pellet colours (the reference draws them from numpy RNG,
 * cell.py:31, player.py:39).  Dead players get zeros (uint8) / NaN (gray). */
int aigar_observe_pixels(aigar_handle *h, void *out, int side, uint64_t color_seed, int dtype, int on_device);
/* The pixel state of a CNN learner (CNN_P_REPR, bot.py:276-282): the frame above
 * through the reference's (rgb_values - 255) / 100, written by the kernel itself.
 * Grayscale (1 channel): (gray - 255) / 100 in fp64.  AIGAR_PIX_RGB (3 channels): the
 * reference subtracts from a uint8 array, which wraps, so a byte b becomes
 * ((b + 1) & 255) / 100 (white 255 -> 0.0, black 0 -> 0.01).  AIGAR_PIX_LAST doubles
 * the channels, [current C | previous C]: the previous channels are the current
 * channels of this bot's previous pixel-state observation, and the zero state (the
 * white frame) before its first one.  (The reference's own CNN_LAST_GRID code cannot
 * run, bot.py:102, 281-282; this is what its networks are built for, network.py:156-165.)
 * The history advances only for the bots a call observes (alive, mask != 0), and is
 * cleared wherever the grid history is: aigar_reset, aigar_reset_arenas,
 * aigar_load_state, aigar_reset_bots.
 *
 * aigar_pixel_config sets the mode of the handle (NULL or side 0: off), allocates and
 * clears the history, and drops the captured decision graph; side must be in [1, 84];
 * tiled handles are refused.  aigar_pixel_state_len: side * side * channels (0: off).
 * aigar_observe_pixel_state: out[A*B][side][side][channels] (surfarray order [x][y],
 * channels last; a device out must be 16-byte aligned), for the players with
 * mask[i] != 0 (NULL: all): the other rows of out and those bots' history are left
 * as they are.  Dead players get NaN rows (all channels) and keep their history.
 * While a pixel config is set, aigar_env_step writes this state (obs_out
 * [A*B][side][side][channels], the NN players' rows in a mixed population) instead of
 * the grid row, still in its one graph. */
#define AIGAR_PIX_RGB  0x1   /* CNN_P_RGB: 3 channels, else 1 (grayscale)          */
#define AIGAR_PIX_LAST 0x2   /* + the bot's previous frame (CNN_LAST_GRID's intent) */
typedef struct aigar_pixel_params {
  int32_t side;          /* CNN_INPUT_DIM_1/2/3 (rgbGenerator.py:16-21)            */
  int32_t flags;         /* AIGAR_PIX_*                                            */
  uint64_t color_seed;   /* as aigar_observe_pixels                                */
} aigar_pixel_params;
int aigar_pixel_config(aigar_handle *h, const aigar_pixel_params *p);
int aigar_pixel_state_len(aigar_handle *h);
int aigar_observe_pixel_state(aigar_handle *h, void *out, int dtype, int on_device, const uint8_t *mask,
                              int mask_on_device);
/* The learners' experience replay memory (replay_buffer.py: ReplayBuffer and
 * PrioritizedReplayBuffer over common/segment_tree.py; driven by aigar.py:1109-1125,
 * 1174-1177, 1075-1086), owned by the handle: a ring of `capacity` transitions
 * (state, action[4], reward, next state, done) and, prioritized, the sum and min trees
 * of 2 * it_cap doubles (it_cap: the next power of two >= capacity), all on the device.
 *
 * aigar_exp_config allocates and clears it (NULL or capacity 0: frees it) and drops the
 * captured decision graph.  The state width is aigar_pixel_state_len() when a pixel
 * config is set, else aigar_obs_len(); capacity must be at least n_arenas *
 * bots_per_arena (one decision's transitions); tiled handles are refused.  While a
 * memory is set, aigar_pixel_config is refused (the rows keep their width) and so is an
 * aigar_env_step whose dtype differs from state_dtype.  A failed allocation is an error
 * return.
 *
 * Transitions.  Every player carries an old state (Bot.oldState, bot.py:186): the last
 * state an observation call computed for it while it was alive -- set by aigar_observe*,
 * aigar_observe_pixel_state (for the players they observe) and aigar_env_step, cleared
 * by a NaN state (a dead player: the reference's None) and wherever the bots' history
 * is: aigar_reset, aigar_reset_arenas, aigar_load_state, aigar_reset_bots.  After its
 * observation, aigar_env_step appends, still in its one graph, one transition for every
 * NN player that had an old state (bot.py:204-217): the old state, this call's action
 * padded with zeros to 4 values, this call's window reward, the new state row (NaN if
 * the player is dead) and done = the player is dead; the new state then becomes the old
 * state (none if dead).  So a player dead at decision time contributes nothing, no
 * transition bridges a death or a reset, and a time-limit end is not marked done
 * (aigar.py:851-887).  Greedy and Random players never contribute.  Slots are given in
 * ascending player index starting at next_idx and wrap at capacity; size = min(size + n,
 * capacity) -- ReplayBuffer.add once per transition in that order (replay_buffer.py:24-31).
 * A new slot's leaf is pow(max_priority, alpha) (max_priority starts at 1.0).
 *
 * aigar_exp_add: the same add for caller rows i < n with mask[i] != 0 (NULL: all), in
 * row order: s, s2 [n][width] of state_dtype, a [n][4], r [n], done [n]; host pointers
 * (copied during the call) or, on_device, device pointers on the handle's stream.  Of
 * more than capacity rows the last capacity remain, as in the reference.
 * aigar_exp_info (synchronises): capacity, size, next_idx, transitions ever added.
 *
 * aigar_exp_sample: ALL pointers are DEVICE pointers; stream-ordered, no host round trip
 * (size is read on the device, so the call can sit in a caller's graph).  u[batch] are
 * the draws in [0, 1); u NULL: the device draws u_k as the top 53 bits of Philox keyed
 * by (seed, number of sample calls so far, k).  Uniform: idx = floor(u * size), w = 1.0.
 * Prioritized, replay_buffer.py:114-171 bit for bit, quirks included: mass = u *
 * sum(0, size - 1), which reduces the leaves [0, size - 2] (the newest-indexed item is
 * left out of the mass), associated the way _reduce_helper nests a prefix range
 * (v[left] + (v[left'] + ...)); then find_prefixsum_idx (> goes left, else subtract and
 * go right); w = pow(leaf / total * size, -beta) / pow(min / total * size, -beta) with
 * total and min the tree roots; every pow is glibc's (aigar_selftest_pow).  Row k of
 * s, a, r, s2, done (each may be NULL) gets transition idx[k].  A memory too small to
 * draw from (size 0; size < 2 when prioritized, where the reference recurses forever)
 * gives idx = -1 and w = NaN and leaves the rows as they are; no error is raised.
 * aigar_exp_gather: the same row fetch for the caller's idx[batch] (DEVICE pointers);
 * rows whose index is outside [0, size) are left untouched.
 *
 * aigar_exp_update_priorities (replay_buffer.py:173-195, batched; DEVICE pointers,
 * stream-ordered): leaf idx[j] becomes pow(prio[j], alpha) in both trees; of several
 * entries with one index the last in idx order wins; max_priority becomes the max of
 * itself and every given priority, overwritten duplicates included.  Entries with
 * prio <= 0 or an index outside [0, size) are skipped.  Nothing happens in uniform mode. */
#define AIGAR_EXP_PRIORITIZED 0x1   /* PRIORITIZED_EXP_REPLAY_ENABLED */
#define AIGAR_EXP_EXTRA       0x2   /* the tuple's fifth field (aigar_exp_extra_get / _set) */
typedef struct aigar_exp_params {
  int64_t capacity;     /* MEMORY_CAPACITY: transitions kept, a ring; >= n_arenas * bots_per_arena */
  int32_t state_dtype;  /* 0 float64, 1 float32: how states are stored and handed out            */
  int32_t flags;        /* AIGAR_EXP_*                                                            */
  double alpha, beta;   /* MEMORY_ALPHA (>= 0), MEMORY_BETA (> 0)                                 */
  uint64_t seed;        /* Philox salt of the memory's own sampling draws                         */
} aigar_exp_params;
int aigar_exp_config(aigar_handle *h, const aigar_exp_params *p);
int aigar_exp_info(aigar_handle *h, int64_t info[4]);
int aigar_exp_add(aigar_handle *h, const void *s, const double *a, const double *r, const void *s2,
                  const uint8_t *done, const uint8_t *mask, int n, int on_device);
int aigar_exp_sample(aigar_handle *h, int batch, const double *u, void *s, double *a, double *r, void *s2,
                     uint8_t *done, double *w, int64_t *idx);
int aigar_exp_gather(aigar_handle *h, const int64_t *idx, int batch, void *s, double *a, double *r, void *s2,
                     uint8_t *done);
int aigar_exp_update_priorities(aigar_handle *h, const int64_t *idx, const double *prio, int n);

/* The Q-learning bots' action selection (qLearning.py:208-243 decideMove; DESIGN.md §4h;
 * tests/decide_model.py is the specification in plain Python).  The learner's network
 * gives one value per discrete action; the device turns every live NN player's row
 * q[n_out] (float32 or float64, widened exactly) into an action index and applies that
 * row of the action table as a 4-value action of aigar_apply_actions.  All arithmetic is
 * float64 in the reference's operation order.
 *
 * aigar_decide_config: the table actions[n_out][4] (HOST pointer; network.py:26-65,
 * aigar_amd/actions.py), copied to the device; p NULL: off.  Configuring or
 * un-configuring drops the captured decision graph.  A tiled handle is refused.
 *
 * Per call: explore = {epsilon, temperature} is read from DEVICE memory (a decay schedule
 * needs no re-capture); all players of a decision see the same two values.  u: DEVICE
 * [A*B][3] draws in [0, 1), or NULL: u0, u1, u2 are the top 53 bits of the first three
 * words of Philox keyed by the arena, at (global player, stream 10, the arena's tick, seed).
 *   strategy 0, e-Greedy: u0 < epsilon explores: idx = floor(u1 * n_out), value NaN;
 *     else greedy.
 *   greedy: numpy.argmax, the first index of the maximum; value q[idx].
 *   strategy 1, Boltzmann (no coin): temperature == 0 is greedy.  Else m = max(q),
 *     d_i = pow(e, (q_i - m) / temperature) (glibc's pow), s = numpy.sum(d) in numpy's
 *     pairwise association, p_i = d_i / s, cdf = cumsum(p) left to right, cdf_i /= cdf[n-1],
 *     k = #{cdf_i <= u2} clamped to n_out - 1, idx = the first j with p_j == p_k; the value
 *     is p[idx], the probability (the reference rebinds q_Values to the distribution).
 * Only live NN players decide: a dead or non-NN player gets idx -1, value NaN, and its
 * action row is left as it is -- in the handle's own action buffer (zeros at config time)
 * its last chosen row, by which a player that respawns on a skipped tick of the window
 * moves (bot.py:166-168 holds the bot's current action over the skipped frames).  A live player's row holding a NaN or an infinity is
 * outside the contract: idx 0, value q[0], and warn bit AIGAR_WARN_Q_NONFINITE of its
 * arena (aigar_warnings), no error.
 *
 * aigar_decide: the selection alone on the handle's stream (all DEVICE pointers): idx_out
 * [A*B] int32, val_out [A*B], act_out [A*B][4] (may be NULL) gets the chosen rows; no
 * command is set.  aigar_env_step_q: the selection and then aigar_env_step's whole
 * decision with the chosen rows as its 4-value actions, one graph replay (re-captured
 * when a pointer or a parameter changes).  With a replay memory configured the
 * transition's action row is [idx, 0, 0, 0] (bot.py:206 stores the index).  Both are
 * error returns without a config. */
typedef struct aigar_decide_params {
  int32_t n_out;      /* rows of the action table, 1..1024 */
  int32_t strategy;   /* 0 e-Greedy, 1 Boltzmann (EXPLORATION_STRATEGY) */
  int32_t q_dtype;    /* 0 float64, 1 float32 */
  int32_t pad;
  uint64_t seed;      /* Philox salt of the own draws */
} aigar_decide_params;
int aigar_decide_config(aigar_handle *h, const aigar_decide_params *p, const double *actions);
int aigar_decide(aigar_handle *h, const void *q, const double *explore, const double *u, int32_t *idx_out,
                 double *val_out, double *act_out);
int aigar_env_step_q(aigar_handle *h, const void *q, const double *explore, const double *u, int enable_split, int skip,
                     const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype, int32_t *idx_out,
                     double *val_out);
/* The actor-critic learners' exploration noise (actorCritic.py:922-966 applyNoise /
 * decideMove; tests/noise_model.py is the specification in plain Python).
 * The learner's actor gives n_act = 2..4 numbers in [0, 1] per player; the device perturbs
 * every live NN player's row mu[n_act] (float32 or float64, widened exactly) with Gaussian
 * or Ornstein-Uhlenbeck noise, clips it to [0, 1] and moves the player by it.  All
 * arithmetic is float64 in the reference's operation order; the only fused multiply-adds
 * are inside glibc's log (aigar_selftest_log).
 *
 * A standard-normal pair is numpy's legacy Gaussian (RandomState.normal, the polar
 * method): attempt t takes two uniforms (ua, ub) on numpy's 53-bit grid, x1 = 2 ua - 1,
 * x2 = 2 ub - 1, r2 = x1 x1 + x2 x2; it is rejected unless r2 < 1 and r2 != 0; else
 * f = sqrt(-2 log(r2) / r2) and the pair is (f x2, f x1), in numpy's order.  Values 0 and
 * 1 of a row take pair 0, values 2 and 3 pair 1; an odd n_act drops its leftover normal
 * (numpy would carry it into the next call).  At most T <= 16 attempts are made per pair;
 * a pair that exhausts them is (0.0, 0.0) and the row's arena gets the sticky bit
 * AIGAR_WARN_NOISE_EXHAUSTED (with own draws: about 2e-11 per pair).
 *   type 0, Gaussian:  a_i = mu_i + std z_i.
 *   type 1, Orn-Uhl:   noise_i = prev_i + theta (ou_mu - prev_i) dt + std sqrt(dt) z_i in
 *     Python's left-to-right association; prev_i = noise_i; a_i = mu_i + noise_i.
 *   Both end with numpy.clip(a, 0, 1) (a -0.0 stays -0.0, as numpy leaves it).
 * std is ONE double read from DEVICE memory at every call / replay (a decay schedule is a
 * write by the caller, no re-capture); all players of a decision see the same std.
 * Outside the contract, no error: a NaN or an infinity in a deciding row's mu is taken as
 * 0.0, a std that is negative, NaN or infinite as 0.0, an Orn-Uhl state that would become
 * NaN or infinite (a huge std, a non-finite prev of the caller) restarts at 0.0 with no noise
 * for that value, and the row's arena gets the sticky bit AIGAR_WARN_NOISE_NONFINITE.  (A
 * Gaussian mu + std z that overflows is clipped to 0 or 1 like any other value.)
 *
 * Draws.  u: DEVICE [rows][2][T][2] uniforms in [0, 1) (row, pair, attempt, {ua, ub}), T
 * given in the call (1..16); or NULL: the device's own, T = 16: attempts 2 b and 2 b + 1
 * of (row, pair) are the top 53 bits of words {0, 1} and {2, 3} of Philox4x64-10 keyed by
 * the arena's key at the counter (row, 11 | pair << 8 | b << 16, the arena's tick, seed);
 * 11 is the stream word ST_NOISE.  Row r belongs to arena (r / bots_per_arena) % n_arenas
 * (the player's arena when rows = n_arenas * bots_per_arena).  Nothing in the counter names
 * the call: own draws depend on (row, pair, attempt, tick, seed) alone, so two aigar_noise
 * calls between two ticks give row r the same normals, and so does an aigar_noise call and
 * the aigar_env_step_ac that follows it at the same tick, for rows below A*B.  A caller that
 * perturbs several batches per step (SPG's offline exploration) passes its own u, or gives
 * each batch other rows of one larger call.
 *
 * Differences from the reference (the device's choice first): the Orn-Uhl state is per
 * player, the reference keeps one on the shared learner; the stored raw action is the
 * actor's own output in float64, the reference's Orn-Uhl branch adds the noise into the
 * array it later stores as "raw" (and rounds to float32 in a float32 array); the
 * critic-guided OCACLA_ONLINE_SAMPLES stay with the caller, who has aigar_noise for them.
 *
 * aigar_noise_config: p NULL turns it off.  Allocates the handle's action, raw-action and
 * Orn-Uhl buffers ([A*B][n_act] each, zeros) and drops the captured decision graph; a
 * tiled handle is refused.  The Orn-Uhl state is zero at config time and cleared wherever
 * the bots' history is: aigar_reset, aigar_reset_arenas, aigar_load_state,
 * aigar_reset_bots (actorCritic.py:1121-1123).
 *
 * mu_dtype holds for aigar_noise and aigar_env_step_ac alike, and configuring again restarts
 * the Orn-Uhl state: a caller with rows of both dtypes configures float64 once and widens its
 * float32 rows (exact), as AgarVecEnv does.
 *
 * aigar_noise: the perturbation alone, stream-ordered, all DEVICE pointers, on any rows
 * >= 0 of mu [rows][n_act] into noisy_out [rows][n_act]; it ignores liveness and roles
 * (SPG's offline exploration, actorCritic.py:892-896, calls it on [batch x samples]
 * rows).  prev: the caller's Orn-Uhl state [rows][n_act], advanced in place; NULL with an
 * Orn-Uhl config is an error (ignored with a Gaussian config).  n_exhausted (may be NULL):
 * a DEVICE uint64 counter that every exhausted pair increments.
 *
 * aigar_env_step_ac: the noise for every live NN player and then aigar_env_step's whole
 * decision with the noisy rows as its n_act-value actions, one graph replay (re-captured
 * when a pointer or a parameter changes).  A dead or non-NN player keeps its row of the
 * handle's action buffer and its Orn-Uhl state; its noisy_out row (may be NULL;
 * [A*B][n_act]) is NaN.  With a replay memory the transition's action row is the noisy
 * action padded with zeros; with AIGAR_EXP_EXTRA see there.  All three are error returns
 * without a config. */
#define AIGAR_NOISE_GAUSSIAN 0   /* NOISE_TYPE == "Gaussian" */
#define AIGAR_NOISE_ORN_UHL  1   /* NOISE_TYPE == "Orn-Uhl"  */
typedef struct aigar_noise_params {
  int32_t n_act;      /* values per action: 2 + ENABLE_SPLIT + ENABLE_EJECT, 2..4         */
  int32_t type;       /* AIGAR_NOISE_*                                                   */
  int32_t mu_dtype;   /* 0 float64, 1 float32                                            */
  int32_t store_raw;  /* the replay memory's extra field gets the raw action (CACLA)     */
  double theta;       /* ORN_UHL_THETA                                                   */
  double ou_mu;       /* ORN_UHL_MU                                                      */
  double dt;          /* ORN_UHL_DT (>= 0)                                               */
  uint64_t seed;      /* Philox salt of the own draws                                    */
} aigar_noise_params;
int aigar_noise_config(aigar_handle *h, const aigar_noise_params *p);
int aigar_noise(aigar_handle *h, const void *mu, int rows, const double *std, const double *u, int T, double *prev,
                double *noisy_out, uint64_t *n_exhausted);
int aigar_env_step_ac(aigar_handle *h, const void *mu, const double *std, const double *u, int T, int enable_split,
                      int skip, const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype,
                      double *noisy_out);
/* The learners' acting network (network.py:207-241, actorCritic.py:219-330; DESIGN.md §4j;
 * tests/net_model.py is the specification in plain Python).  An MLP of n_layers dense
 * layers (1..5: up to four hidden layers and the head), layer l with kernel W[in][out] and
 * bias b[out] in float32, Keras' layout; units[l] <= 256 outputs each, n_in <= 16384 inputs.
 * One row: the input rounded once to float32 (a float32 row is taken as it is); per unit
 * acc = +0.0f, acc = fmaf(x_k, W[k][j], acc) for k = 0, 1, ..., in - 1 as ONE chain, then
 * y_j = acc + b_j as one float32 add; hidden layers relu (y > 0 ? y : +0.0f) or linear; the
 * head linear (y widened to float64) or the sigmoid in float64: t = max(-|y|, -750),
 * z = pow(e, t) (glibc's pow), y >= 0 ? 1 / (1 + z) : z / (1 + z).  A row whose first value
 * is a NaN is not evaluated: its output row is NaN.  Any other NaN or infinity in a row is
 * outside the contract: the result is what the arithmetic gives, and the head's
 * AIGAR_WARN_Q_NONFINITE / AIGAR_WARN_NOISE_NONFINITE handling catches it.  Keras' own
 * float32 sigmoid and summation order are not reproducible; this definition is the
 * project's.  Every other activation code is refused.
 *
 * aigar_net_config: p NULL turns it off.  Allocates the zero-padded weights (all zero until
 * aigar_net_set_weights) and the output buffer [A*B][units[n_layers - 1]] float64, and
 * drops the captured decision graph.  A tiled handle is refused.  The parameters are
 * checked before the handle, so a bad set is reported with its own message.
 *
 * aigar_net_set_weights: layer's W[in][out] and b[out], float32, both host or (on_device)
 * both DEVICE pointers; stream-ordered (host pointers are read before it returns).  It
 * re-packs into the handle's own padded copy, which the captured graph reads: no
 * re-capture, and the next decision uses the new weights.  This is the trainer's push.
 *
 * aigar_net_forward: the network alone, stream-ordered, on rows >= 1 rows of the DEVICE
 * buffer x [rows][n_in] (x_dtype: 0 float64, 1 float32, independent of the config's) into
 * the DEVICE buffer out [rows][n_out] float64.  Liveness and roles are ignored.
 *
 * aigar_env_step_net: the whole decision with the network in front, one graph replay per
 * decision: the network on obs_out, then aigar_env_step_q's selection (head
 * AIGAR_NET_HEAD_Q; needs an aigar_decide_config with q_dtype 0 and n_out == the network's
 * outputs; explore is [epsilon, temperature], u [A*B][3] or NULL, T ignored) or
 * aigar_env_step_ac's noise (head AIGAR_NET_HEAD_ACTOR; needs an aigar_noise_config with
 * mu_dtype 0 and n_act == the network's outputs; explore is [std], u [A*B][2][T][2] or
 * NULL) on the handle's output buffer, then the decision.  The network reads obs_out as the
 * previous decision, or the caller's aigar_observe, left it, and the decision overwrites it
 * at its end: THE BUFFER MUST HOLD THE CURRENT STATES BEFORE THE FIRST CALL.  dtype must be
 * the config's x_dtype and n_in the state length (aigar_obs_len; no pixel state).  Only
 * live NN players' rows are evaluated; a dead or non-NN player keeps its output row.
 * idx_out / val_out (head Q) and noisy_out (head actor, may be NULL) as in those calls.
 * n_decisions >= 1 replays the graph that many times with no host work in between;
 * explore is read from device memory at every replay (u, if given, is the same draws every
 * time).  aigar_net_output: a stream-ordered copy of the handle's output buffer (the last
 * decision's Q values / mu) into the DEVICE buffer out [A*B][n_out] float64. */
#define AIGAR_NET_MAX_LAYERS 5
#define AIGAR_NET_MAX_UNITS  256
#define AIGAR_NET_MAX_IN     16384
#define AIGAR_ACT_LINEAR  0
#define AIGAR_ACT_RELU    1
#define AIGAR_ACT_SIGMOID 2
#define AIGAR_ACT_ELU     3   /* refused */
#define AIGAR_ACT_TANH    4   /* refused */
#define AIGAR_NET_HEAD_Q     0
#define AIGAR_NET_HEAD_ACTOR 1
typedef struct aigar_net_params {
  int32_t n_layers;    /* dense layers, 1..AIGAR_NET_MAX_LAYERS                          */
  int32_t n_in;        /* the state length, 1..AIGAR_NET_MAX_IN                          */
  int32_t x_dtype;     /* the decision's state dtype: 0 float64, 1 float32               */
  int32_t hidden_act;  /* AIGAR_ACT_RELU or AIGAR_ACT_LINEAR                             */
  int32_t out_act;     /* AIGAR_ACT_LINEAR or AIGAR_ACT_SIGMOID                          */
  int32_t pad;
  int32_t units[8];    /* outputs of layer l, 1..AIGAR_NET_MAX_UNITS; [n_layers, 8) unused */
} aigar_net_params;
int aigar_net_config(aigar_handle *h, const aigar_net_params *p);
int aigar_net_set_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device);
int aigar_net_forward(aigar_handle *h, const void *x, int x_dtype, int rows, double *out);
int aigar_net_output(aigar_handle *h, double *out);
int aigar_env_step_net(aigar_handle *h, int head, const double *explore, const double *u, int T, int enable_split,
                       int skip, const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype,
                       int32_t *idx_out, double *val_out, double *noisy_out, int n_decisions);
/* The CNN learners' acting network (CNN_REPR with CNN_P_REPR: network.py:154-183,
 * actorCritic.py:122-136; tests/conv_model.py is the specification in plain
 * Python): a convolutional front end in front of the dense layers above.  The image is
 * x[side][side][channels] (the pixel state, channels last), rounded once to float32.  n_conv
 * (1..3) conv layers, layer l with a square kernel W[k][k][Cin][F] and bias b[F] in float32
 * (Keras' layout), valid padding, stride s, always relu; its output side is
 * (in - k) / s + 1 (floor).  One output (oy, ox, f): acc = +0.0f,
 * acc = fmaf(x[oy s + ky][ox s + kx][c], W[ky][kx][c][f], acc) as ONE chain in ascending
 * order of (ky k + kx) Cin + c, then acc + b[f] as one float32 add, then y > 0 ? y : +0.0f.
 * The last conv layer's output, flattened in (y, x, f) order (Keras' Flatten), is the dense
 * part's float32 input row.  A sample whose first image value is a NaN (a dead player's
 * pixel state) is not evaluated: its output row is NaN.
 *
 * aigar_net_config_cnn: both parameter sets are checked before the handle, each refusal with
 * its own message: side 1..128, channels 1..8, n_conv 1..3, k 1..8, stride 1..8, filters
 * 1..64, every layer's output side >= 1, the flattened length <= AIGAR_NET_MAX_IN, and
 * d->n_in == the flattened length; d->x_dtype is the image's dtype.  A tiled handle is
 * refused.  It allocates the padded filters (zero until aigar_net_set_conv_weights) and the
 * float32 activations and feature rows for max(A*B, 64) samples, all owned by the handle,
 * and drops the captured decision graph.  aigar_net_config (plain or NULL) turns the conv
 * part off again.
 *
 * aigar_net_set_conv_weights: conv layer's W[k][k][Cin][F] and b[F], host or (on_device)
 * DEVICE pointers, stream-ordered, re-packed into the handle's own copy: no re-capture
 * (aigar_net_set_weights goes on setting the dense layers).  With a conv part
 * aigar_net_forward takes x[rows][side][side][channels] and aigar_env_step_net requires a
 * configured pixel state (aigar_pixel_config) of the same side and channel count; it then
 * runs the conv layers, the dense layers and the head's selection or noise in the
 * decision's one graph.  Without a conv part a pixel state is refused as before. */
#define AIGAR_CONV_MAX_LAYERS  3
#define AIGAR_CONV_MAX_SIDE    128
#define AIGAR_CONV_MAX_CHANNELS 8
#define AIGAR_CONV_MAX_KERNEL  8
#define AIGAR_CONV_MAX_FILTERS 64
typedef struct aigar_conv_params {
  int32_t side;        /* the image's side, 1..AIGAR_CONV_MAX_SIDE                        */
  int32_t channels;    /* ... and channels, 1..AIGAR_CONV_MAX_CHANNELS                    */
  int32_t n_conv;      /* conv layers, 1..AIGAR_CONV_MAX_LAYERS                           */
  int32_t k[3];        /* kernel side of layer l, 1..AIGAR_CONV_MAX_KERNEL                */
  int32_t stride[3];   /* stride of layer l, 1..AIGAR_CONV_MAX_KERNEL                     */
  int32_t filters[3];  /* filters of layer l, 1..AIGAR_CONV_MAX_FILTERS                   */
} aigar_conv_params;
int aigar_net_config_cnn(aigar_handle *h, const aigar_conv_params *c, const aigar_net_params *d);
int aigar_net_set_conv_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device);
/* The replay memory's fifth field (bot.py:206-216; replay_buffer.py:197-209 update_dones;
 * aigar.py:1079-1086).  With AIGAR_EXP_EXTRA in aigar_exp_params.flags the ring also keeps
 * extra[capacity][4] doubles and a valid byte per slot.  aigar_env_step_ac's transition
 * then carries a = the noisy action padded with zeros and, when the noise config has
 * store_raw (CACLA), extra = the raw action padded with zeros, valid; without store_raw
 * (SPG, DPG) the slot's extra is invalid: NaN, valid 0 -- the reference's None.  Every
 * other add (aigar_env_step, aigar_env_step_q, aigar_exp_add) leaves the extra invalid.  A
 * ring wrap overwrites a slot's extra together with its transition; aigar_exp_config
 * clears them.  aigar_exp_sample, aigar_exp_gather and a memory without the flag are
 * unchanged.  Both calls below take DEVICE pointers, are stream-ordered and are error
 * returns on a memory without the flag.
 * aigar_exp_extra_get: out[batch][4] and valid[batch] (each may be NULL) of the slots
 * idx[batch]; rows whose index is outside [0, size) are left untouched.
 * aigar_exp_extra_set (update_dones): slot idx[j] gets rows[j][4] and becomes valid, j < n
 * <= capacity; of several entries with one index the last in order wins; indices outside
 * [0, size) are skipped. */
int aigar_exp_extra_get(aigar_handle *h, const int64_t *idx, int batch, double *out, uint8_t *valid);
int aigar_exp_extra_set(aigar_handle *h, const int64_t *idx, const double *rows, int n);
/* The Q-learning trainer on the device (qLearning.py:116-193 QLearn.train, network.py:378-392
 * trainOnBatch; tests/train_model.py is the specification in plain Python): the
 * reference's default discrete learner -- an MLP with a linear head, Keras 2.2.4 Adam
 * (amsgrad off) on loss='mse' with the memory's importance weights as sample weights, a
 * hard target-network copy every target_steps applied steps.  One step, for a batch of B
 * drawn transitions (s, a, rew, s2, done, w), a = [index, 0, 0, 0]:
 *   q = forward(s, online) with every layer's float32 activations kept; q2 = forward(s2, target);
 *   t = rew if done, else rew + discount * max_j q2[j] (float64: one multiply, one add);
 *   td = t - q[a]; with a prioritized memory |td| + 1e-4 becomes the priority of the drawn
 *   slot (aigar_exp_update_priorities: the last of a repeated index wins);
 *   delta_L[r][a_r] = float32(((2 w_r) (-td_r)) / (n_out B)), +0.0f elsewhere;
 *   for l = L ... 1 in float32: dW_l[k][j] = ONE fmaf chain over ascending r of
 *   h_{l-1}[r][k] delta_l[r][j] from +0.0f; db_l[j] = the plain sum over ascending r; and,
 *   with the weights as they are before the update, e[r][k] = ONE fmaf chain over ascending
 *   j of delta_l[r][j] W_l[k][j], delta_{l-1} = e where y_{l-1} > 0 (relu; else +0.0f) or e (linear);
 *   Adam per parameter, m and v float32, float64 arithmetic on the widened values with every
 *   operation rounding on its own: lr_t = lr * sqrt(1 - pow(beta2, t)) / (1 - pow(beta1, t))
 *   (glibc's pow; t counts applied steps from 1), m = f32(beta1 m + (1 - beta1) g),
 *   v = f32(beta2 v + (1 - beta2) (g g)), p = f32(p - lr_t m / (sqrt(v) + epsilon));
 *   after a step with t % target_steps == 0 (target_steps > 0) target <- online.
 * A step is skipped on the device -- no weight, counter t or priority changes -- while the
 * memory holds fewer than max(batch, min_size) transitions, and also when a TD error is not
 * finite or a stored action index lies outside the head; the latter sets the sticky bit
 * AIGAR_WARN_TRAIN_NONFINITE of arena 0.  Skipped steps are counted.
 *
 * aigar_train_config: the parameters are checked before the handle, each refusal with its own
 * message (batch 1..256, min_size >= 0, target_steps >= 0, lr > 0, betas in [0, 1),
 * epsilon > 0, discount in [0, 1]).  It needs a dense acting network with a linear head and no
 * conv part (aigar_net_config), a replay memory whose state length is the network's n_in, an
 * action selection (aigar_decide_config) of the network's n_out, and no tiled handle.  It
 * allocates the target network as a copy of the online one as it is NOW, zeroed Adam state,
 * the staging rows and the activation buffers.  NULL turns training off and frees them;
 * aigar_net_config* and aigar_exp_config drop the train configuration.
 * Training is in place on the acting network's packed weights: the next decision acts with
 * the trained weights.  aigar_net_set_weights overwrites the online weights only.
 *
 * aigar_train_step: n_steps >= 1 steps, one captured graph replayed n_steps times with no
 * host work in between.  u NULL: the memory's own Philox stream, as aigar_exp_sample; else
 * the DEVICE buffer u [n_steps][batch] of draws in [0, 1) (step i's row is copied on the
 * stream in front of its replay).  Stream-ordered.
 * aigar_train_info: {steps applied, steps skipped, steps since the last target copy, 0};
 * the one synchronising read.  aigar_train_td: stream-ordered copies of the last drawn
 * step's TD errors [batch] and memory indices [batch] into DEVICE buffers (each may be NULL).
 * aigar_train_sync_target: target <- online now.  aigar_train_reset: m, v and t to zero.
 * aigar_net_get_weights: layer's W[in][out] and b[out] in Keras' layout, into host or
 * (on_device) DEVICE buffers; which 0 the online network (needs no train configuration),
 * 1 the target network, 2 Adam's m, 3 Adam's v.  aigar_net_pad_check: a debug read, the
 * number of padded entries of which's packed copies whose bits are not +0.0f's (a host
 * round trip; 0 in every correct state). */
typedef struct aigar_train_params {
  int32_t batch;         /* transitions a step, 1..256                          */
  int32_t min_size;      /* NUM_EXPS_BEFORE_TRAIN: no step below this memory size */
  int32_t target_steps;  /* TARGET_NETWORK_STEPS; 0: never copied                */
  int32_t pad;
  double lr, beta1, beta2, epsilon;  /* Keras' Adam: 1e-4 (ALPHA), 0.9, 0.999, 1e-7 */
  double discount;                   /* DISCOUNT                                  */
} aigar_train_params;
int aigar_train_config(aigar_handle *h, const aigar_train_params *p);
int aigar_train_step(aigar_handle *h, int n_steps, const double *u);
int aigar_train_info(aigar_handle *h, int64_t info[4]);
int aigar_train_td(aigar_handle *h, double *td, int64_t *idx);
int aigar_train_sync_target(aigar_handle *h);
int aigar_train_reset(aigar_handle *h);
int aigar_net_get_weights(aigar_handle *h, int which, int layer, float *W, float *b, int on_device);
int aigar_net_pad_check(aigar_handle *h, int which, int64_t *count);
/* The Q-learning trainer of an acting network with a conv part (the pixel learner: CNN_REPR with
 * CNN_P_REPR; tests/cnn_train_model.py is the specification in plain Python, on
 * tests/conv_model.py and tests/train_model.py).  One step is the step above with the conv
 * layers around the dense part, in place on the packed filters and kernels the decision acts
 * with; s and s2 are images [side][side][channels] of the memory's dtype:
 *   every conv layer's post-relu output a_l is kept; feat = a_last flattened in (y, x, f) order is
 *   the dense part's float32 input, and the first dense layer's gradient is taken with h = feat;
 *   q2 comes from the target network, conv part included, on s2;
 *   e[r][i] = ONE float32 fmaf chain from +0.0f over ascending unit j of delta_1[r][j] W_dense0[i][j];
 *   delta_conv_last = e where feat > 0, else +0.0f, as [B][O][O][F];
 *   dW_l[ky][kx][c][f] = ONE fmaf chain from +0.0f over ascending m = (r O + oy) O + ox of
 *   h_{l-1}[r][oy s + ky][ox s + kx][c] delta_l[r][oy][ox][f]; db_l[f] = the plain float32 sum of
 *   delta_l[m][f] over ascending m;
 *   for l >= 2, e_{l-1}[r][iy][ix][c] = ONE chain from +0.0f over ALL k k F taps in ascending
 *   (ky k + kx) F + f of fmaf(x, W_l[ky][kx][c][f], acc) with x = delta_l[r][(iy - ky) / s][(ix - kx) / s][f]
 *   when both differences are >= 0, divisible by s and their quotients < O, else x = -0.0f (the
 *   padded steps are executed); delta_{l-1} = e where a_{l-1} > 0, else +0.0f;
 *   Adam on every conv W and b as on the dense ones, one lr_t and one t; every gradient is taken
 *   with the weights as they were before the step; the hard target copy takes the filters as well.
 * The skip rules, the warn bit and the counters are the dense trainer's.
 *
 * aigar_train_config_cnn: the same parameters, checked before the handle with the same messages
 * under its own name.  It needs an acting network with a conv part (aigar_net_config_cnn; on a
 * dense one it refuses and names aigar_train_config) and a linear head, a replay memory whose
 * state length is side * side * channels, and no tiled handle.  NULL turns it off.  It is dropped
 * by what drops a train configuration.  aigar_train_config on a network with a conv part is
 * refused as before.  aigar_train_step, aigar_train_info, aigar_train_td, aigar_train_sync_target
 * and aigar_train_reset serve both configurations.
 * aigar_net_get_conv_weights: conv layer's W[k][k][cin][F] and b[F] in Keras' layout, into host or
 * (on_device) DEVICE buffers; which as aigar_net_get_weights' 0..3 (1..3 need this configuration).
 * aigar_net_get_weights on such a network reads the dense layers; aigar_net_pad_check counts the
 * conv copies' padding too. */
int aigar_train_config_cnn(aigar_handle *h, const aigar_train_params *p);
int aigar_net_get_conv_weights(aigar_handle *h, int which, int layer, float *W, float *b, int on_device);
/* The CACLA learner's critic and trainer on the device (actorCritic.py ActorCritic.learn for
 * ALGORITHM == "CACLA": train_critic 1032-1065, train_actor_batch 791-858, the critic's hard
 * target copy 745-746; tests/cacla_model.py is the specification in plain Python).
 *
 * The critic V(s) is a second network of the handle.  aigar_critic_config: a dense MLP under
 * aigar_net_config's limits whose last layer is ONE unit with out_act AIGAR_ACT_LINEAR and
 * whose n_in is the acting network's; it needs a dense acting network without a conv part.
 * The parameters are checked before the handle, each refusal with its own message.  NULL turns
 * it off and frees it; aigar_net_config* drops it.  aigar_critic_set_weights: as
 * aigar_net_set_weights.  aigar_critic_forward: V(s) of rows >= 1 rows of the DEVICE buffer
 * x [rows][n_in] into the DEVICE buffer out [rows] float64, stream-ordered, the arithmetic of
 * aigar_net_forward.
 *
 * One training step on B drawn transitions (s, a[4], rew, s2, done, w); forward passes, the
 * backward pass and Adam are aigar_train_step's, in the same orders and roundings:
 *   v = forward(s, critic) with the activations kept; v2 = forward(s2, critic's target);
 *   t = rew if done, else rew + discount * v2 (float64: one multiply, one add); td = t - v;
 *   with a prioritized memory |td| + 1e-4 becomes the drawn slot's priority;
 *   critic: delta_L[r][0] = float32(((2 w_r) (-td_r)) / (1 B)), backward, Adam with critic_lr
 *   and the critic's own step counter t_c;
 *   selection, on the td above, float64, over ascending r, count[r] = the actor epochs of row r:
 *     var_epochs == 0: count[r] = 1 if td_r > 0, else 0;
 *     var_epochs = E >= 1: for EVERY row var = (1 - var_beta) var + var_beta (td_r td_r); then
 *     count[r] = 0 if td_r <= 0, else c = ceil(td_r / sqrt(var)) if 1 <= c <= E, else E (the
 *     row is counted as cut; a c that is not finite or below 1 is cut too).  The reference's
 *     epochs are unbounded: the cap E <= AIGAR_ACTRAIN_MAX_EPOCHS is this project's.  var
 *     persists across steps and starts at var_start;
 *   actor epochs e = 0 .. max_r count[r] - 1, rows with count[r] > e taking part, n_e of them:
 *     mu = the sigmoid head of forward(s, actor) with the weights as they are NOW;
 *     delta_L[r][j] = float32(((2 (mu_rj - a_rj)) / (n_out n_e)) (mu_rj (1 - mu_rj))) for the
 *     rows taking part, +0.0f for the others; backward; Adam with actor_lr and the actor's own
 *     counter t_a, which advances once an epoch.  No importance weights on the actor;
 *   t_c += 1; after a step with t_c % target_steps == 0 (target_steps > 0) the critic's target
 *   <- the critic.  CACLA keeps no actor target.
 * A step is skipped -- no weight, counter, priority or var changes -- while the memory holds
 * fewer than max(batch, min_size) transitions, and, with AIGAR_WARN_TRAIN_NONFINITE, when a td
 * is not finite.  An epoch whose delta_L has a non-finite entry is skipped with the same bit,
 * and so are the step's later epochs; each of them is counted.
 *
 * aigar_actrain_config: the parameters are checked before the handle, each refusal with its
 * own message (batch 1..256, min_size >= 0, target_steps >= 0, var_epochs 0..8, both lr > 0,
 * betas in [0, 1), epsilon > 0, discount in [0, 1], var_start > 0, var_beta in [0, 1)).  It
 * needs an acting network with a sigmoid head, 1..4 outputs and no conv part, a critic, a
 * replay memory whose state length is n_in, and no tiled handle.  It allocates the critic's
 * target as a copy of the critic as it is NOW, zeroed Adam state for both networks, staging
 * rows and activation buffers.  NULL turns it off; aigar_net_config*, aigar_critic_config and
 * aigar_exp_config drop it.  It and aigar_train_config exclude each other by their heads.
 * Training is in place on the acting network's packed weights.
 * aigar_actrain_step: as aigar_train_step.  aigar_actrain_info: {critic steps applied, steps
 * skipped, steps since the target copy, actor epochs applied (t_a), rows selected in the last
 * step, epochs of the last step, rows cut to var_epochs (total), actor epochs skipped (total)};
 * a synchronising read.  aigar_actrain_td: stream-ordered copies of the last drawn step's td
 * [batch], indices [batch] and count [batch] into DEVICE buffers (each may be NULL).
 * aigar_actrain_var: var into a host double, synchronising.  aigar_actrain_sync_target: the
 * critic's target <- the critic now.  aigar_actrain_reset: both networks' m and v, t_c and t_a
 * to zero, var to var_start.
 * aigar_net_get_weights / aigar_net_pad_check: which 4 the critic (needs only a critic), 5 its
 * target, 6 / 7 its Adam m / v; under an actrain configuration 2 / 3 are the actor's m / v and
 * 1 is refused (CACLA keeps no actor target). */
#define AIGAR_ACTRAIN_MAX_EPOCHS 8
typedef struct aigar_actrain_params {
  int32_t batch, min_size, target_steps, var_epochs;   /* 1..256, >=0, >=0, 0..8 */
  double critic_lr, actor_lr, beta1, beta2, epsilon, discount, var_start, var_beta;
} aigar_actrain_params;                                 /* 80 bytes */
int aigar_critic_config(aigar_handle *h, const aigar_net_params *p);
int aigar_critic_set_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device);
int aigar_critic_forward(aigar_handle *h, const void *x, int x_dtype, int rows, double *out);
int aigar_actrain_config(aigar_handle *h, const aigar_actrain_params *p);
int aigar_actrain_step(aigar_handle *h, int n_steps, const double *u);
int aigar_actrain_info(aigar_handle *h, int64_t info[8]);
int aigar_actrain_td(aigar_handle *h, double *td, int64_t *idx, int32_t *count);
int aigar_actrain_var(aigar_handle *h, double *var);
int aigar_actrain_sync_target(aigar_handle *h);
int aigar_actrain_reset(aigar_handle *h);
/* The DPG learner's critic and trainer on the device (actorCritic.py ActorCritic.learn for
 * ALGORITHM == "DPG": train_critic_DPG 986-1029, train_actor_DPG 751-789 on
 * createCombinedActorCritic 581-598, softlyUpdateTargetModel 366-373; DESIGN.md §4n;
 * tests/dpg_model.py is the specification in plain Python).
 *
 * aigar_qcritic_config: the critic Q(s, a) in the handle's critic slot.  aigar_critic_config's
 * checks, but n_in is the acting network's n_in + n_out (DPG_FEED_ACTION_IN_LAYER = 1: a row is
 * the state, then the action), and the acting network must be dense with a sigmoid head and
 * 1..4 outputs.  aigar_critic_set_weights, aigar_critic_forward (rows of the critic's own n_in)
 * and which 4..7 serve it unchanged.  NULL turns it off.  aigar_actrain_config refuses a
 * Q(s, a) critic, aigar_dpg_config a V(s) one.
 *
 * One training step on B drawn transitions (s, a[4], rew, s2, done, w); forward passes, the
 * backward pass and Adam are aigar_train_step's.  An action entering the critic is the float64
 * action rounded once to float32, as every input is.
 *   critic half: mu2 = forward(s2, actor's target); q2 = forward([s2, mu2], critic's target);
 *   q = forward([s, a], critic) with the activations kept; t = rew if done, else
 *   rew + discount * q2 (float64: one multiply, one add); td = t - q; a prioritized memory gets
 *   |td| + 1e-4; delta_L[r][0] = float32(((2 w_r) (-td_r)) / (1 B)), backward, Adam with
 *   critic_lr and the counter t_c;
 *   actor half, with the critic as just updated and both targets as before this step:
 *   mu = forward(s, actor) with the activations kept, mu- = forward(s, actor's target);
 *   qmu = forward([s, mu], critic) with the activations kept; qt = forward([s, mu-], critic's
 *   target); dq[r][0] = float32((2.0 (qmu_r - (qt_r + q_increase))) / (1 B)) on every row;
 *   backward through the critic's layers L-1 .. 1 to delta_0 (no critic gradient is formed);
 *   ea[r][k] = ONE fmaf chain over ascending unit j of delta_0[r][j] W_0[n_s + k][j] from
 *   +0.0f; the actor's delta_L[r][k] = float32((double)ea[r][k] (mu_rk (1.0 - mu_rk)));
 *   backward through the actor; Adam with actor_lr and the actor's own m, v and counter t_a;
 *   t_c += 1; tau > 0: both targets, every entry, theta- = float32(float32(theta- float32(1.0 -
 *   tau)) + float32(theta float32(tau))); tau == 0: both targets are copied after a step with
 *   t_c % target_steps == 0 (target_steps > 0).
 * A step is skipped -- nothing changes -- while the memory holds fewer than max(batch,
 * min_size) transitions, and, with AIGAR_WARN_TRAIN_NONFINITE, when a td is not finite.  A
 * non-finite dq or actor delta_L entry skips the actor half only, with the same bit: the critic's
 * update and the target update apply, t_a stays, the half is counted.
 *
 * aigar_dpg_config: the parameters are checked before the handle, each refusal with its own
 * message (batch 1..256, min_size >= 0, target_steps >= 0, reserved 0, both lr > 0, betas in
 * [0, 1), epsilon > 0, discount in [0, 1], tau in [0, 1], q_increase finite).  It needs a Q(s, a)
 * critic, a replay memory whose state length is the actor's n_in, no conv part and no tiled
 * handle.  It allocates both targets as copies of the networks as they are NOW and zeroed Adam
 * state.  NULL turns it off; aigar_net_config*, aigar_critic_config, aigar_qcritic_config and
 * aigar_exp_config drop it.  The three train configurations exclude one another by the head of
 * the acting network and the kind of the critic.
 * aigar_dpg_step: as aigar_actrain_step.  aigar_dpg_info: {critic steps applied, steps skipped,
 * steps since the hard copy, actor steps applied (t_a), actor halves skipped, 0, 0, 0}; a
 * synchronising read.  aigar_dpg_td: stream-ordered copies of the last drawn step's td [batch]
 * and indices [batch] into DEVICE buffers (each may be NULL).  aigar_dpg_sync_target: both
 * targets <- online now.  aigar_dpg_reset: both networks' m and v, t_c and t_a to zero.
 * aigar_net_get_weights / aigar_net_pad_check under a DPG configuration: which 1 is the actor's
 * target, 2 / 3 the actor's m / v, 5..7 the critic's target, m, v. */
typedef struct aigar_dpg_params {
  int32_t batch, min_size, target_steps, reserved;   /* 1..256, >=0, >=0, 0 */
  double critic_lr, actor_lr, beta1, beta2, epsilon, discount, tau, q_increase;
} aigar_dpg_params;                                   /* 80 bytes */
int aigar_qcritic_config(aigar_handle *h, const aigar_net_params *p);
int aigar_dpg_config(aigar_handle *h, const aigar_dpg_params *p);
int aigar_dpg_step(aigar_handle *h, int n_steps, const double *u);
int aigar_dpg_info(aigar_handle *h, int64_t info[8]);
int aigar_dpg_td(aigar_handle *h, double *td, int64_t *idx);
int aigar_dpg_sync_target(aigar_handle *h);
int aigar_dpg_reset(aigar_handle *h);
/* The SPG (Sampled Policy Gradient) learner's trainer on the device (actorCritic.py
 * ActorCritic.learn for OCACLA_ENABLED 730-733: train_critic_DPG(get_evals=True) 986-1029,
 * train_actor_OCACLA 860-919; tests/spg_model.py is the specification in plain
 * Python).  It trains the Q(s, a) critic of aigar_qcritic_config as aigar_dpg_step does and the
 * actor by regression towards the best action a per-row search finds.
 *
 * One training step on B drawn transitions (s, a[4], rew, s2, done, w, idx, extra[4], valid):
 *   critic half: aigar_dpg_step's, entry for entry (mu2, q2, q = Q([s, a]), td, delta_L, backward,
 *   Adam with critic_lr and t_c).  A prioritized memory gets |q_r| + 1e-4 with prio_evals = 1
 *   (the reference: get_evals hands Q(s, a) to the memory in the TD error's place) and
 *   |td_r| + 1e-4 with prio_evals = 0;
 *   search, every row on its own, with the critic as just updated and the actor as it is; every
 *   comparison is a float64 `>` (a NaN never wins); an action entering the critic is its float64
 *   value rounded once to float32:
 *     mu = forward(s, actor) with the activations kept; qmu = Q([s, mu]);
 *     best = a_r[:n_act], best_eval = q_r (the value from before the critic's update);
 *     when samples = K > 0: with replace and a valid extra, qe = Q([s, extra[:n_act]]) and the
 *     extra is taken if qe > best_eval; mu is taken if qmu > best_eval; then for x = 0 .. K-1:
 *     cand = clip(base + noise z, 0, 1), base = best when moving, else mu; z from numpy's legacy
 *     Gaussian as aigar_noise's (pair 0 gives values 0 and 1, pair 1 values 2 and 3, at most 16
 *     attempts a pair; an exhausted pair is (0, 0) and sets AIGAR_WARN_NOISE_EXHAUSTED on arena
 *     0; the clip leaves -0.0 alone); cand is taken if Q([s, cand]) > best_eval;
 *     the row is selected iff best_eval > qmu;
 *   actor half: count = the selected rows.  count == 0: nothing is trained, t_a stays, the half
 *   is counted as empty.  Else delta_L[r][j] = float32(((2.0 (mu_rj - best_rj)) / (n_out count))
 *   (mu_rj (1.0 - mu_rj))) for the selected rows and +0.0f for the others, backward, Adam with
 *   actor_lr and t_a.  No importance weights;
 *   write-back (replace): every drawn slot's extra becomes valid and holds best padded with zeros
 *   for a selected row and a_r otherwise; the last entry of a repeated index wins;
 *   tail: aigar_dpg_step's counters and target updates (soft with tau > 0, else the due hard copy
 *   of both targets), then noise <- noise * noise_decay, one float64 multiply on the device
 *   double that holds the search noise.
 * Skips are aigar_dpg_step's: a small memory or a non-finite td skips the whole step (nothing
 * changes, no extra is written, the noise does not decay; the latter with
 * AIGAR_WARN_TRAIN_NONFINITE); a non-finite actor delta skips the actor half only (counted; the
 * write-back stays).  A noise outside [0, inf) counts as 0 with AIGAR_WARN_NOISE_NONFINITE.
 * Differences from the reference: the actor trains from the first step (no
 * AC_ACTOR_TRAINING_START); both targets are updated (the reference's SPG actor target never
 * moves and its soft update is DPG-only); the write-back does not depend on the memory being
 * prioritized; Gaussian search noise only; the search's draws are the caller's or order-free
 * Philox, not numpy's stream; samples <= AIGAR_SPG_MAX_SAMPLES.
 *
 * aigar_spg_config: the parameters are checked before the handle, each refusal with its own
 * message (aigar_dpg_config's; samples 0..8; moving, replace, prio_evals, fused 0 or 1 -- fused = 1
 * runs the search in one kernel that evaluates the critic's first-layer chunks below the actions once a row, with
 * the same results bit for bit; pad 0; noise finite and >= 0;
 * noise_decay in (0, 1]; q_increase is unused but must be finite).  It needs what
 * aigar_dpg_config needs and, with replace, a memory with AIGAR_EXP_EXTRA.  It and
 * aigar_dpg_config exclude each other: configuring one drops the other, and whatever drops a
 * DPG configuration drops this one.  NULL turns it off.
 * aigar_spg_step: u as aigar_dpg_step's; zu NULL or the DEVICE buffer [n_steps][batch][samples]
 * [2][16][2] of the search's uniforms in [0, 1) (sample x of row r: pair, attempt, the two
 * values).  NULL: Philox4x64-10 under arena 0's key at the counter (row, 12 | pair << 8 |
 * b << 16 | x << 24, the ordinal of the step -- applied or skipped -- since the configuration
 * or the last aigar_spg_reset, seed); block b holds attempts 2 b and 2 b + 1.
 * aigar_spg_info: {critic steps applied, steps skipped, steps since the hard copy, actor steps
 * applied (t_a), actor halves skipped, actor halves empty, rows selected by the last applied
 * step, 0}; a synchronising read.  aigar_spg_td: as aigar_dpg_td (td either way).
 * aigar_spg_noise: the DEVICE address of the noise double (the caller may read and write it in
 * stream order).  aigar_spg_sync_target, aigar_spg_reset (both networks' m and v, t_c, t_a and
 * the steps' ordinal to zero; the noise stays): as DPG's.  aigar_net_get_weights /
 * aigar_net_pad_check and aigar_critic_forward behave as under a DPG configuration. */
#define AIGAR_SPG_MAX_SAMPLES 8
typedef struct aigar_spg_params {
  int32_t batch, min_size, target_steps, reserved;   /* 1..256, >=0, >=0, 0 */
  double critic_lr, actor_lr, beta1, beta2, epsilon, discount, tau, q_increase;
  int32_t samples, moving, replace, prio_evals, fused, pad;  /* 0..8, 0/1, 0/1, 0/1, 0/1, 0 */
  double noise, noise_decay;                          /* OCACLA_NOISE, OCACLA_NOISE_DECAY */
  uint64_t seed;                                      /* of the search's own draws */
} aigar_spg_params;                                   /* 128 bytes */
int aigar_spg_config(aigar_handle *h, const aigar_spg_params *p);
int aigar_spg_step(aigar_handle *h, int n_steps, const double *u, const double *zu);
int aigar_spg_info(aigar_handle *h, int64_t info[8]);
int aigar_spg_td(aigar_handle *h, double *td, int64_t *idx);
int aigar_spg_noise(aigar_handle *h, double **dev);
int aigar_spg_sync_target(aigar_handle *h);
int aigar_spg_reset(aigar_handle *h);
/* The sticky quirk bits of one arena since its last reset (a host round trip): 1 a virus
 * made this tick ate, 2 a dead virus was met, 4 a tile observed past its held pellets,
 * 8 AIGAR_WARN_Q_NONFINITE, 16 AIGAR_WARN_NOISE_NONFINITE, 32 AIGAR_WARN_NOISE_EXHAUSTED,
 * 64 AIGAR_WARN_TRAIN_NONFINITE (arena 0 only). */
#define AIGAR_WARN_TRAIN_NONFINITE 0x40
#define AIGAR_WARN_Q_NONFINITE 0x8
#define AIGAR_WARN_NOISE_NONFINITE 0x10
#define AIGAR_WARN_NOISE_EXHAUSTED 0x20
int aigar_warnings(aigar_handle *h, int arena, uint32_t *out);
/* bot.currentAction / bot.lastAction used by the action extras: [A*B][4] each (may be NULL). */
int aigar_set_actions(aigar_handle *h, const double *cur, const double *prev, int on_device);
/* Bot.reset (bot.py:125-164) for the players with mask[i] != 0 (NULL: all): the
 * NN bot's last / second-last self and enemy grids restart at zero and its
 * lastFovSize at 0, as model.resetBots() does between the collector's windows
 * (aigar.py:845-852, 833-838).  mask: NP bytes, host or (on_device) device. */
int aigar_reset_bots(aigar_handle *h, const uint8_t *mask, int on_device);

/* per-player summary [A*B][5]: alive, total mass (player.py:129), fov x, fov y, fov size
 * (player.py:156-167). */
int aigar_player_stats(aigar_handle *h, double *out, int on_device);

/* The bots' mass history (AIGAR_FLAG_SCORE).  Bot.makeMove appends
 * player.getTotalMass() at the start of every Model.update (bot.py:253); with the
 * flag every tick of aigar_step / aigar_run / aigar_env_step starts by taking that
 * sample of every player on the device: the player's total mass, 0.0 while it is
 * dead.  T ticks after a reset are T samples, the first the fresh world's mass; the
 * state after the last tick is not sampled.  aigar_reset, aigar_reset_arenas and
 * aigar_load_state clear the players they restart; aigar_reset_bots does not
 * (Bot.reset keeps totalMasses).
 *
 * aigar_score: out[A*B][4] = samples, sum, max, dead of Bot.getMassOverTime()
 * (bot.py:639-640) -- what aigar.py:531-535 reduces to meanMass (the mean over bots
 * of sum / samples) and maxMass (the max over bots of max).  sum is one fp64 add per
 * sample in tick order; max is 0.0 without samples; dead counts the samples taken
 * while the player was dead (one per death: stepsUntilRespawn = 1). */
int aigar_score(aigar_handle *h, double *out, int on_device);
/* Bot.resetMassList (bot.py:122-123) for the players with mask[i] != 0 (NULL: all):
 * the next sample is sample 0.  mask: NP bytes, host or (on_device) device.
 * Stream-ordered. */
int aigar_score_reset(aigar_handle *h, const uint8_t *mask, int on_device);
/* The list itself (bot.py:639-640): a DEVICE buffer buf[cap][A*B] (row = sample
 * index, column = player), NULL to detach.  Sample k of player i goes to
 * buf[k][i] while k < cap; later samples are counted but not stored.  Column i,
 * rows [0, min(samples, cap)), is that bot's getMassOverTime().  Stream-ordered;
 * the buffer's address is read from device memory, so captured graphs stay valid. */
int aigar_score_trace(aigar_handle *h, double *buf, int64_t cap);

/* Snapshot / restore one arena (parity harness, checkpoint/resume). */
int aigar_get_state(aigar_handle *h, int arena, aigar_state *st);
int aigar_load_state(aigar_handle *h, int arena, const aigar_state *st);

/* Event log of the last aigar_step (AIGAR_FLAG_EVENTS): rows of (tick, code, a, b)
 * in reference order.  *n gets the count; returns < 0 if cap is too small. */
int aigar_get_events(aigar_handle *h, int arena, int64_t *out, int cap, int *n);

/*
 * C4 tiled arena (field.py:85-92, 200-253, 256-313).  Every tile
 * handle replays the whole tick on its replica of the players, cells, blobs and
 * viruses; it holds only the pellets of its tile plus the halo.  The eat phase
 * (field.py:207-222) is resolved per tile; the cells a tile owns (centre bucket
 * in the tile) report their outcomes in ONE message per pass, and the caller's
 * transport all-gathers the messages (RCCL all-gather over xGMI; in-process
 * device copies for tests):
 *   [Greedy bots (bot.py:579-633): aigar_tile_policy(h, greedy_split), the
 *    all-gather, aigar_tile_apply_commands(h) -- each tile moves the bots it
 *    observes (it holds their whole view) and sends their commands]
 *   aigar_tile_begin(h, p)  policy (NONE / RANDOM; GREEDY once the commands of
 *                           this tick were applied) + the tick up to the first
 *                           eat pass; the outbox holds the message
 *   <all-gather every tile's outbox into every tile's inbox>
 *   aigar_tile_apply(h, &u) the other tiles' outcomes; u = owned cells still
 *                           undone on all tiles (same value on every tile)
 *   while (u > 0) { aigar_tile_resume(h); <all-gather>; aigar_tile_apply(h, &u); }
 *   aigar_tile_end(h, obs, dtype)  playerPlayerOverlap .. spawnStuff; then, if obs
 *                           (DEVICE) is given, the observations of the bots THIS
 *                           tile observes (bot.py:272-497; the other rows are left
 *                           as they are, dead bots get NaN on every tile)
 * Without host round trips: aigar_tile_apply(h, NULL) returns at once, and a
 * fixed number K of further (aigar_tile_resume, all-gather, aigar_tile_apply)
 * rounds follow; a resume pass does nothing on the device once no owned cell is
 * undone, and aigar_tile_end raises error bit 4096 if cells are still undone
 * after the K passes (K = 0 with the default halo in practice: one pass).
 * Observation: each bot is observed by ONE tile -- the one holding its
 * last-frame history grids (bot.py:480-495), else the tile of its view centre.
 * A bot whose view centre moved to another tile, or that died, has its history
 * handed off in the next tick's first message and every tile takes it, so the
 * next observation is made by the view centre's tile; a view the observing
 * tile does not hold sets error bit 2048.  aigar_tile_observers: per player,
 * the observing tile of the last observation (-1: dead), identical on every tile.
 * The spawn deficit is global: each tile's message carries its pellet kills.
 * aigar_tile_info: info[14] = ntiles, tile_id, owned bucket range x0, x1, y0, y1
 * (half-open), held range x0, x1, y0, y1, records per message, bitmap words,
 * hand-off slots per message, records per hand-off slot;
 * the device outbox / inbox and the bytes of one message (the inbox holds
 * ntiles messages, tile k at k * bytes).  A message is 32-byte records:
 * [header: kind 0, record count, undone owned cells, pellet kills as double,
 * hand-off slots as double] [records: kind 1 pellet kill (seq, x, y) | 2 blob
 * kill (slot, seq) | 3 cell outcome (pool index, seq, mass, radius)] and, in
 * the tick's first pass, [hand-off slots: kind 4 (player, lastFovSize) + the
 * bot's history grids as doubles], in later passes [bitmap: owned cells now final].
 * aigar_tile_set_buffers: use caller-owned device buffers instead (e.g. torch
 * tensors that RCCL fills); aigar_tile_exchange_local: the in-process transport
 * -- copies every handle's outbox into every handle's inbox (same process).
 * aigar_get_state on a tiled handle returns the pellets the tile OWNS; the
 * union over the tiles is the arena's pellet list.
 */
int aigar_tile_info(aigar_handle *h, int32_t *info, void **outbox, void **inbox, int64_t *msg_bytes);
int aigar_tile_set_buffers(aigar_handle *h, void *outbox, void *inbox);
/* bytes of the current pass's message: the first pass of a tick sends the header
 * and records only (no bitmap); the inbox then holds tile k's at k * these bytes */
int aigar_tile_msg_bytes(aigar_handle *h, int64_t *bytes);
int aigar_tile_begin(aigar_handle *h, const aigar_run_params *p);
/* Greedy moves of the bots this tile observes (the observation's rule: history
 * holder, else the view centre's tile) into a command message [header: kind 0,
 * count][kind 5 records: player, split | eject << 1, command x, y]; after the
 * all-gather aigar_tile_apply_commands takes the other tiles' commands.  Replaces
 * Bot.make_greedy_bot_move + set_command_point (bot.py:579-633, 550-577) for a
 * tiled arena, where no tile holds every pellet. */
int aigar_tile_policy(aigar_handle *h, int greedy_split);
int aigar_tile_apply_commands(aigar_handle *h);
int aigar_tile_apply(aigar_handle *h, int *undone);
int aigar_tile_resume(aigar_handle *h);
int aigar_tile_end(aigar_handle *h, void *obs_out, int dtype);
int aigar_tile_exchange_local(aigar_handle **hs, int n);
int aigar_tile_observers(aigar_handle *h, int32_t *out);

/* C4 over RCCL (xGMI): the tile's exchange as ncclAllGather(outbox -> inbox) on
 * the handle's stream, so a whole tiled step -- policy, the tick with its eat
 * passes and exchanges, the observation of this tile's bots -- is one hipGraph
 * replay with no host round trip (the rank-side loop of the aigar_tile_* calls
 * above, with the caller's transport replaced by RCCL).
 *   aigar_rccl_unique_id(path, id)   rank 0: a fresh ncclUniqueId (128 bytes),
 *                                    which the caller broadcasts to every rank
 *   aigar_tile_comm_init(h, path, id, nranks, rank)  ncclCommInitRank; nranks
 *                                    must be the tile count and rank the tile id
 *   aigar_tile_run(h, n, p, extra_passes, obs, dtype)  n tiled steps: per step
 *       (policy GREEDY: aigar_tile_policy, all-gather, aigar_tile_apply_commands)
 *       aigar_tile_begin, all-gather, aigar_tile_apply, extra_passes gated
 *       (resume, all-gather, apply) rounds, aigar_tile_end (obs: DEVICE buffer
 *       or NULL) -- captured once as a hipGraph (RCCL is captured with it),
 *       direct launches if the capture fails or while profiling
 * path: the librccl.so to bind (the one the process's torch loaded, so that one
 * HIP runtime serves both), or NULL for "librccl.so" on the loader path. */
int aigar_rccl_unique_id(const char *path, void *id);
int aigar_tile_comm_init(aigar_handle *h, const char *path, const void *id, int nranks, int rank);
int aigar_tile_run(aigar_handle *h, int n_steps, const aigar_run_params *p, int extra_passes, void *obs_out,
                   int dtype);
/* 1 if aigar_tile_run replays a captured graph, 0 if it launches directly */
int aigar_tile_run_graphed(aigar_handle *h);
/* Timing rehearsal only (tools/c4_solo.py): aigar_tile_run without a
 * communicator, the exchange replaced by a copy of this tile's message into its
 * own inbox slot, every other tile's slot an empty message.  The tile then steps
 * alone on its GPU -- the per-GPU cost of a tiled step without the all-gather;
 * its world is not the tiled arena's (no other tile's outcomes arrive). */
int aigar_tile_loopback(aigar_handle *h);

/* The event log as raw rows (key_hi = tick << 8 | phase, key_lo = order within the
 * phase, code, a, b), unsorted: tiled arenas merge their tiles' logs by key. */
int aigar_get_events_raw(aigar_handle *h, int arena, int64_t *out, int cap, int *n);

/* Stream control. */
int aigar_set_stream(aigar_handle *h, void *hip_stream);
int aigar_sync(aigar_handle *h);

/* Timing support for bench.py: HIP-event time of the named kernel's launches
 * on the handle's stream during the last step (ms total, launch count). */
int aigar_profile(aigar_handle *h, int enable);
int aigar_kernel_time(aigar_handle *h, const char *kernel, double *ms, int *launches);

/* Diagnostics: per-arena work counters accumulated since reset/load_state --
 * out[0..n) of: serial work-list entries of virusBlobOverlap, playerVirusOverlap,
 * pellet + blob eating (cells), pellets eaten, playerPlayerOverlap (players),
 * pellets respawned, ticks whose playerPlayerOverlap ran as independent
 * groups (see tick.hip pp_pass), ticks.  n <= 8. */
int aigar_counters(aigar_handle *h, int arena, int64_t *out, int n);

/* Diagnostics: evaluate the device's pow (aigar_math.h: glibc 2.35's pow, bit
 * for bit) on host arrays of n (x, y) pairs -- used by the parity tests. */
int aigar_selftest_pow(const double *x, const double *y, double *out, int n);
/* out[i] = log(x[i]) as the device computes it (glibc 2.35's, restated in aigar_math.h); host arrays. */
int aigar_selftest_log(const double *x, double *out, int n);

/* Diagnostics: evaluate the device's trig (aigar_glibc_trig.h: glibc 2.35's
 * __ieee754_atan2_fma / __sin_fma / __cos_fma, bit for bit) on host arrays:
 * out[0, n) = atan2(y, x), out[n, 2n) = sin(x), out[2n, 3n) = cos(x). */
int aigar_selftest_trig(const double *y, const double *x, double *out, int n);

/* Diagnostics: evaluate the device's per-entity helpers (aigar_sem.h) and exact integer
 * helpers (aigar_math.h) on host arrays, one element per thread, the header functions
 * themselves.  in is [in_cols][n] and out is [out_cols][n], both of 8-byte words: values
 * are doubles, integers come back as exact doubles, and the 64-bit words of the Philox op
 * are bit patterns.  Each op fixes its column counts (inputs -> outputs):
 *   MOD_POS        a, b                     -> mod_pos(a, b, 1.0 / b)
 *   TRUNC_DIV_POS  x, b                     -> trunc_div_pos(x, b, 1.0 / b)
 *   PY_MOD         a, b                     -> py_mod
 *   ROUND3         v                        -> py_round3
 *   SUM            16 terms, count (0..16)  -> np_sum, NpAcc fed term by term
 *   RADIUS         m                        -> radius_of, pellet_radius
 *   BUCKET         c, cols                  -> bucket_floor_s; where c >= 0 (else -1):
 *                                              bucket_floor, center_bucket_coord
 *   FOOTPRINT      px, py, rad, size        -> x0, x1, y0, y1
 *   MOVE           x, y, m, r, cpx, cpy     -> vx, vy, c, s of set_move_direction
 *   MOMENTUM       x, y, cpx, cpy, w, h, orig_r -> svx, svy of add_momentum
 *   MERGE_TIME     f, m                     -> merge_time_for
 *   PHILOX         c0..c3, k0, k1, lo, hi   -> the 4 output words, u01(out0),
 *                                              ph_randint(out0, lo, hi)
 *   TRIG_FORMS     y, x                     -> atan2_glibc, atan2_glibc_flat, sin_glibc(x),
 *                                              cos_glibc(x), sincos_glibc(x)'s sin and cos
 * An unknown op, column counts that are not the op's, a null pointer or a negative n
 * return < 0 with a message that names the argument; n == 0 succeeds. */
#define AIGAR_SEM_MOD_POS 0
#define AIGAR_SEM_TRUNC_DIV_POS 1
#define AIGAR_SEM_PY_MOD 2
#define AIGAR_SEM_ROUND3 3
#define AIGAR_SEM_SUM 4
#define AIGAR_SEM_RADIUS 5
#define AIGAR_SEM_BUCKET 6
#define AIGAR_SEM_FOOTPRINT 7
#define AIGAR_SEM_MOVE 8
#define AIGAR_SEM_MOMENTUM 9
#define AIGAR_SEM_MERGE_TIME 10
#define AIGAR_SEM_PHILOX 11
#define AIGAR_SEM_TRIG_FORMS 12
#define AIGAR_SEM_N_OPS 13
int aigar_selftest_sem(int op, const double *in, int in_cols, double *out, int out_cols, int n);

#ifdef __cplusplus
}
#endif
#endif /* AIGAR_H */
