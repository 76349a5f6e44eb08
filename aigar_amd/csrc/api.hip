// api.hip -- host implementation of include/aigar.h (libaigar_hip.so).
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/aigar.h"
#include "aigar_dev.h"
#include "aigar_sem.h"

namespace aigar {
void launch_tick(const Dev &d, hipStream_t s, int rounds, int64_t *scr_k, int *scr_v,
                 const RandomPolicy *rp = nullptr);
void launch_tick_pre(const Dev &d, hipStream_t s, int64_t *scr_k, int *scr_v, const RandomPolicy *rp);
void launch_tick_post(const Dev &d, hipStream_t s, int64_t *scr_k, int *scr_v);
void launch_tile_pass(const Dev &d, hipStream_t s, int rounds, int64_t *scr_k, int *scr_v, int first);
void launch_tile_policy(const Dev &d, hipStream_t s, int greedy_split, uint8_t *mask, int cap);
void launch_tile_cmd_apply(const Dev &d, hipStream_t s, int box_recs);
void launch_pel_gather(const Dev &d, hipStream_t s, int a);
void launch_tile_apply(const Dev &d, hipStream_t s, int box_recs, int first);
void launch_restart(const Dev &d, hipStream_t s, const ArenaSel &sel);
void launch_restart_bots(const Dev &d, hipStream_t s, const ArenaSel &sel);
void launch_observe(const Dev &d, hipStream_t s, void *out, int dtype, uint32_t epoch,
                    const uint8_t *mask = nullptr, int greedy_next = -1);
bool observe_fuses_greedy(const Dev &d);
void launch_policy_refrandom(const Dev &d, hipStream_t s, int skip_rate, int enable_split, int enable_eject,
                             uint64_t salt);
int launch_observe_pixels(const Dev &d, hipStream_t s, void *out, int dtype, int side, uint64_t seed, uint8_t *ovf);
int launch_observe_pixel_state(const Dev &d, hipStream_t s, void *out, int dtype, int side, int flags, uint64_t seed,
                               uint8_t *ovf, const uint8_t *mask, uint32_t *hist);
void launch_policy(const Dev &d, hipStream_t s, double ps, double pe, uint64_t salt);
void launch_player_stats(const Dev &d, hipStream_t s, double *out);
void launch_score_read(const Dev &d, hipStream_t s, double *out);
void launch_score_reset(const Dev &d, hipStream_t s, const uint8_t *mask);
void launch_score_trace(const Dev &d, hipStream_t s, double *buf, int64_t cap);
void launch_player_fov(const Dev &d, hipStream_t s, const ArenaSel &sel);
void launch_apply_actions(const Dev &d, hipStream_t s, const double *act, int n_act, int enable_split, int skipping,
                          int record);
void launch_rewards(const Dev &d, hipStream_t s, double *out, const aigar_reward_params &p, int update_last,
                    int mode);
void launch_policy_greedy(const Dev &d, hipStream_t s, int greedy_split, const uint8_t *mask, int want = -1);
void launch_set_commands(const Dev &d, hipStream_t s, const double *cmd);
}  // namespace aigar

using namespace aigar;

#include "replay.inc"
#include "decide.inc"
#include "noise.inc"
#include "net.inc"
#include "conv.inc"
#include "train.inc"
#include "convtrain.inc"
#include "actrain.inc"
#include "dpg.inc"
#include "spg.inc"

static thread_local std::string g_err;
static int fail(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}
#define HIPCHK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) return fail("%s failed: %s", #x, hipGetErrorString(e_));       \
  } while (0)

// librccl.so, bound at run time (C4 over RCCL, below)
namespace {
struct RcclId {
  char b[128];  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES)
};
constexpr int kNcclUint8 = 1;  // ncclDataType_t ncclUint8 (rccl.h)
struct Rccl {
  void *so = nullptr;
  int (*get_unique_id)(RcclId *) = nullptr;
  int (*comm_init_rank)(void **, int, RcclId, int) = nullptr;
  int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*comm_destroy)(void *) = nullptr;
  const char *(*error_string)(int) = nullptr;
};
Rccl g_rccl;
int rccl_load(const char *path) {
  if (g_rccl.so) return 0;
  void *so = dlopen(path && *path ? path : "librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!so) return fail("RCCL: dlopen(%s) failed: %s", path ? path : "librccl.so", dlerror());
  Rccl r;
  r.so = so;
  r.get_unique_id = (int (*)(RcclId *))dlsym(so, "ncclGetUniqueId");
  r.comm_init_rank = (int (*)(void **, int, RcclId, int))dlsym(so, "ncclCommInitRank");
  r.all_gather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(so, "ncclAllGather");
  r.comm_destroy = (int (*)(void *))dlsym(so, "ncclCommDestroy");
  r.error_string = (const char *(*)(int))dlsym(so, "ncclGetErrorString");
  if (!r.get_unique_id || !r.comm_init_rank || !r.all_gather || !r.comm_destroy || !r.error_string)
    return fail("RCCL: %s lacks an nccl* entry point", path ? path : "librccl.so");
  g_rccl = r;
  return 0;
}
}  // namespace

// ---- captured graphs
// A slot owns one executable graph.  Every entry point that replays a graph keeps
// it in a slot, and there is one rule for letting a graph go (drop): the handle's
// stream is synchronised first, since replays of the graph may still be queued.
struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  void drop(aigar_handle *h);
  hipError_t launch(const aigar_handle *h) const;
};
// ... together with the byte image of the key it was captured for: everything
// the captured launches bake in -- parameters by value, buffers by pointer.  A key
// is a plain struct built in cleared storage (key_clear), whose struct members are
// set with key_put, and it is stored and compared as bytes (memcpy, memcmp): the
// comparison reads no padding that the language leaves unspecified.
template <class K>
struct KeyedSlot : GraphSlot {
  static_assert(std::is_trivially_copyable_v<K>, "a graph key is moved and compared as bytes");
  unsigned char image[sizeof(K)] = {};
  bool holds(const K &k) const { return exec && memcmp(image, &k, sizeof(K)) == 0; }
  // the graph of k: captured from issue(stream) unless the slot holds it; false: the capture failed
  template <class F>
  bool ensure(aigar_handle *h, const K &k, F issue);
};
template <class K>
static void key_clear(K &k) {
  static_assert(std::is_trivially_copyable_v<K>, "a graph key is moved and compared as bytes");
  memset(&k, 0, sizeof k);
}
template <class T>
static void key_put(T &member, const T &v) {
  memcpy(&member, &v, sizeof(T));
}
struct StepKey {  // aigar_step: one Field.update
  int rounds;  // food_rounds
};
struct RunKey {  // aigar_run, aigar_tile_run: one whole step
  aigar_run_params p;
  void *out;
  int dtype;  // -1: no observation
  int extra;  // aigar_tile_run's extra passes
};
struct TileKey {  // aigar_tile_begin, aigar_tile_end: the tick before the first / after the last exchange
  aigar_run_params p;  // (tile_end: none)
  const void *box[2];  // the message buffers (aigar_tile_set_buffers)
  void *out;           // (tile_begin: none)
  int dtype;           // -1: no observation
};
struct TrainKey {  // aigar_*_step: one training step (every buffer is the train configuration's own)
  int kind;   // whose step it is: kTrainQ, kTrainCacla, kTrainDpg, kTrainSpg
  int has_u;  // the draws come from the handle's u row (the caller's draws are copied there)
  int has_zu;  // SPG: the search's uniforms come from the trainer's zu rows (the caller's are copied there)
  int pad;
  Conv conv;  // kTrainQ under aigar_train_config_cnn: the conv part the step runs through (n_conv 0: none)
};
enum { kTrainQ, kTrainCacla, kTrainDpg, kTrainSpg };
struct EnvKey {  // aigar_env_step*: one learner decision
  const double *act;
  int n_act, enable_split, skip, dtype;
  aigar_reward_params prm;
  double *reward;
  void *obs;
  aigar_env_params envp;
  int n_greedy, n_random;
  aigar_pixel_params pix;  // side 0: the grid row
  uint32_t *pix_hist;
  const void *exp;  // the replay memory the decision appends to (null: none)
  const double *exp_act;  // ... and the action rows it stores, [NP][exp_n_act]
  int exp_n_act;
  // aigar_env_step_q: the selection in front of the decision (q null: none)
  const void *q;
  const double *explore, *u;
  int32_t *idx_out;
  double *val_out;
  Decide dec;
  // aigar_env_step_ac: the exploration noise in front of the decision (mu null: none)
  const void *mu;
  const double *nstd, *nu;
  double *noisy;
  const double *exp_extra;  // the transitions' fifth field, [NP][exp_n_act] (null: invalid)
  int nT, pad;
  Noise noi;
  // aigar_env_step_net: the acting network in front of either (n_layers 0: none)
  Net net;
  // ... with a conv part in front of it (aigar_net_config_cnn; n_conv 0: none)
  Conv conv;
};

// A feature's device buffers, allocated one by one and freed together.
struct DevBlock {
  std::vector<void *> bufs;
  // null: out of device memory (the HIP error is cleared); zero: cleared on stream s
  void *alloc(size_t bytes, bool zero, hipStream_t s) {
    void *m = nullptr;
    if (hipMalloc(&m, bytes ? bytes : 1) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    bufs.push_back(m);
    if (zero) (void)hipMemsetAsync(m, 0, bytes, s);
    return m;
  }
  void release() {
    for (void *m : bufs) (void)hipFree(m);
    bufs.clear();
  }
};

struct aigar_handle {
  aigar_config cfg;
  Dev d;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  uint32_t obs_calls = 0;
  // reservation rounds of the eat phase before the serial fallback (food_rounds):
  // 0 = by population -- 1 until the handle's Greedy policy ran, then 2 (Greedy
  // bots crowd the same pellets: 18 cells per C3 tick failed a single round and
  // took the serial pass, 0.9 with two rounds, profiles/r05_v2g_*); an empty
  // round exits at once but costs a dependent launch
  int rounds = 0;
  bool greedy_seen = false;
  int64_t *scr_k = nullptr;
  int *scr_v = nullptr;
  double *d_cmd = nullptr, *d_stats = nullptr;
  double *d_score = nullptr;  // host-destination staging for aigar_score
  uint8_t *d_mask = nullptr;
  uint8_t *d_nnmask = nullptr;  // 1 for the players of role NN (the env step's observations)
  int n_greedy = 0, n_random = 0;  // role counts (aigar_set_roles)
  aigar_env_params envp{};
  void *d_obs = nullptr;
  // aigar_reset_arenas: the call's arena and seed lists, [n_arenas] each.  The
  // kernels read the device copies; the async copies read pinned host slots, a
  // slot reused only once the copy that read it last is done (its event)
  static constexpr int kResetSlots = 4;
  int *d_rlist = nullptr;
  uint64_t *d_rseed = nullptr;
  char *h_reset = nullptr;  // kResetSlots x 16 A bytes ([A] seeds, [A] arenas), pinned
  hipEvent_t ev_reset[kResetSlots] = {};
  unsigned reset_calls = 0;
  void *d_pix = nullptr;  // host-destination staging for aigar_observe_pixels
  uint8_t *d_pix_ovf = nullptr;  // per player: frame left to the pixel kernel's second pass
  size_t pix_bytes = 0;
  // aigar_pixel_config: the learner's pixel state (side 0: off) and, with AIGAR_PIX_LAST,
  // every bot's previous frame [NP][side * side] as ~0x00RRGGBB (cleared = the white frame)
  aigar_pixel_params pix{};
  uint32_t *d_pix_hist = nullptr;
  std::vector<void *> allocs;
  char *arena = nullptr;  // aigar_create's arrays (dalloc); freed through allocs
  size_t arena_size = 0, arena_used = 0;
  bool arena_sizing = false;
  int box_recs = 0;   // C4: TileRec slots of a full exchange message (header + records + bitmap)
  int pass_recs = 0;  // ... of the current pass's message (the first pass sends no bitmap)
  int first_pass = 0;  // the current pass is the tick's first (its message carries the history hand-off)
  hipEvent_t ev_x = nullptr;  // in-process transport: this handle's outbox is written / its inbox is filled
  // C4: the tick up to the first exchange and the tick after the last one, as
  // graphs (re-captured when the policy, the observation buffer or the message
  // buffers change)
  KeyedSlot<TileKey> tb, te;
  bool profile = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // timer name -> recorded (start, stop) event pairs, resolved lazily
  std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> marks;
  std::vector<hipEvent_t> event_pool;
  KeyedSlot<StepKey> step;  // aigar_step: one Field.update as a graph
  hipStream_t cap_stream = nullptr;  // private stream graphs are captured on (the caller's may be the null stream)
  bool use_graph = true;  // AIGAR_NO_GRAPH=1 disables (direct launches)
  // C4 tile phases as graphs (AIGAR_TILE_GRAPH=1): measured no faster than direct
  // launches on a tile's own GPU (tools/c4_tile_timing.py), and slower in the
  // 1-GPU gloo rehearsal, so off by default
  bool tile_graph = false;
  bool graph_failed = false;
  // C4 over RCCL (aigar_tile_comm_init / aigar_tile_run)
  void *rccl_comm = nullptr;
  int rccl_ranks = 0;
  bool rccl_bad = false;  // an all-gather failed while a graph was captured
  bool loopback = false;  // timing rehearsal: the exchange copies this tile's message to its own slot only
  bool cmd_ready = false;  // this tick's Greedy commands were exchanged and applied (aigar_tile_apply_commands)
  bool cmd_pending = false;  // aigar_tile_policy wrote a command message that was not applied yet
  KeyedSlot<RunKey> tr;
  bool tr_failed = false;
  // aigar_run: one whole env step (policy + Field.update + observation) as a graph
  KeyedSlot<RunKey> run;
  GraphSlot run_u;  // run_unroll steps in one graph (keyed off run's key: dropped with it)
  // AIGAR_RUN_UNROLL (default 4): each graph launch costs an inter-graph gap on
  // the device that a node boundary inside a graph does not (C3 A/B,
  // profiles/r05_ab_notes.txt v30: 1 -> 4 steps per graph 42.5 -> 44.4 M env-steps/s)
  int run_unroll = 4;
  bool run_u_tried = false;  // the unrolled graph of this key was captured (or its capture failed)
  // aigar_env_step: one learner decision (skip + 1 ticks) as a graph
  KeyedSlot<EnvKey> env;
  // aigar_decide_config: the Q-learning bots' action selection (decide.inc; n_out 0: off)
  Decide dec{};
  DevBlock dec_mem;
  // aigar_noise_config: the actor-critic learners' exploration noise (noise.inc; n_act 0: off)
  Noise noi{};
  DevBlock noi_mem;
  // aigar_net_config: the learners' acting network (net.inc; n_layers 0: off)
  Net net{};
  DevBlock net_mem;  // ... and the conv part's buffers
  float *net_stage = nullptr;  // aigar_net_set_weights' staging of host weights (one of net_mem)
  // aigar_net_config_cnn: the conv part in front of it (conv.inc; n_conv 0: off)
  Conv conv{};
  float *conv_stage = nullptr;  // aigar_net_set_conv_weights' staging (one of net_mem)
  // aigar_exp_config: the learners' replay memory (replay.inc; cap 0: off)
  Exp exp;
  DevBlock exp_mem;
  int *d_exp_off = nullptr;  // aigar_exp_add's slot offsets, [exp_off_n]
  size_t exp_off_n = 0;
  // aigar_critic_config: the actor-critic learners' critic, a second network (n_layers 0: off)
  Net crit{};
  DevBlock crit_mem;
  float *crit_stage = nullptr;  // aigar_critic_set_weights' staging of host weights (one of crit_mem)
  // aigar_qcritic_config: the critic is Q(s, a), its rows are [state, action]
  bool crit_q = false;
  // The trainer (batch 0: off).  At most one is configured -- each needs another head or critic --
  // so they share one block of buffers and one step graph (trainer_free).
  Train trn;     // aigar_train_config: Q-learning (train.inc)
  ConvTrain ctrn{};  // aigar_train_config_cnn: ... of a network with a conv part, trn its dense part (convtrain.inc)
  ACTrain act;   // aigar_actrain_config: CACLA (actrain.inc)
  DPGTrain dpg;  // aigar_dpg_config: DPG (dpg.inc)
  SPGTrain spg;  // aigar_spg_config: SPG on DPG's critic half (spg.inc)
  DevBlock trn_mem;
  KeyedSlot<TrainKey> train;
  GraphSlot *const slots[8] = {&step, &run, &run_u, &env, &tb, &te, &tr, &train};
};

void GraphSlot::drop(aigar_handle *h) {
  if (!exec) return;
  (void)hipStreamSynchronize(h->stream);  // (no replay of the graph is pending)
  (void)hipGraphExecDestroy(exec);
  exec = nullptr;
}
hipError_t GraphSlot::launch(const aigar_handle *h) const { return hipGraphLaunch(exec, h->stream); }

extern "C" const char *aigar_last_error(void) { return g_err.c_str(); }
extern "C" int aigar_abi_version(void) { return AIGAR_ABI_VERSION; }

// Device arrays.  aigar_create carves the world's ~120 arrays out of ONE
// allocation (arena_*: a sizing pass, one hipMalloc, a carving pass) instead of a
// hipMalloc each: one large allocation is mapped with large pages, so the tick's
// kernels, which touch tens of arrays per load round, need far fewer address
// translations.  Every array starts on a 256-byte boundary.  Later allocations
// (pixel buffers) are separate.
template <class T>
static T *dalloc(aigar_handle *h, size_t n) {
  void *p = nullptr;
  if (n == 0) n = 1;
  const size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
  if (h->arena_sizing) {  // sizing pass: a placeholder (never dereferenced)
    const size_t off = h->arena_used;
    h->arena_used += bytes;
    return (T *)(uintptr_t)(256 + off);
  }
  if (h->arena) {
    if (h->arena_used + bytes > h->arena_size) return nullptr;
    p = h->arena + h->arena_used;
    h->arena_used += bytes;
    return (T *)p;  // (zeroed with the whole arena)
  }
  if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) return nullptr;
  (void)hipMemset(p, 0, n * sizeof(T));
  h->allocs.push_back(p);
  return (T *)p;
}

static int obs_len_of(const aigar_config &c) {
  int G = c.grid_squares ? c.grid_squares : 11, n = 0, e = 0;
  if (c.obs_channels & AIGAR_OBS_SIMPLE) return 12;  // getSimpleStateRepresentation (bot.py:511-547)
  for (int b = 0; b < 10; b++) n += (c.obs_channels >> b) & 1;
  e += (c.obs_extras & AIGAR_EX_LAST_FOV) ? 1 : 0;
  e += (c.obs_extras & AIGAR_EX_FOV) ? 1 : 0;
  e += (c.obs_extras & AIGAR_EX_MASS) ? 1 : 0;
  e += (c.obs_extras & AIGAR_EX_LAST_ACT) ? 4 : 0;
  e += (c.obs_extras & AIGAR_EX_2LAST_ACT) ? 4 : 0;
  return G * G * n + e;
}

static void free_all(aigar_handle *h) {
  for (GraphSlot *g : h->slots) g->drop(h);
  for (void *p : h->allocs) (void)hipFree(p);
  h->allocs.clear();
  if (h->d_pix) (void)hipFree(h->d_pix);
  h->d_pix = nullptr;
  h->d_pix_ovf = nullptr;  // (one of allocs)
  h->pix_bytes = 0;
  if (h->d_pix_hist) (void)hipFree(h->d_pix_hist);
  h->d_pix_hist = nullptr;
  for (DevBlock *m : {&h->exp_mem, &h->dec_mem, &h->noi_mem, &h->net_mem, &h->trn_mem, &h->crit_mem}) m->release();
  if (h->d_exp_off) (void)hipFree(h->d_exp_off);
  h->d_exp_off = nullptr;
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev_x) (void)hipEventDestroy(h->ev_x);
  for (hipEvent_t &e : h->ev_reset)
    if (e) (void)hipEventDestroy(e);
  if (h->h_reset) (void)hipHostFree(h->h_reset);
  h->h_reset = nullptr;
  if (h->rccl_comm && g_rccl.comm_destroy) (void)g_rccl.comm_destroy(h->rccl_comm);
  h->rccl_comm = nullptr;
  for (auto &m : h->marks) {
    (void)hipEventDestroy(m.second.first);
    (void)hipEventDestroy(m.second.second);
  }
  for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
  if (h->stream && h->own_stream) (void)hipStreamDestroy(h->stream);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
}

static hipEvent_t pool_event(aigar_handle *h) {
  hipEvent_t e = nullptr;
  if (!h->event_pool.empty()) {
    e = h->event_pool.back();
    h->event_pool.pop_back();
  } else {
    (void)hipEventCreate(&e);
  }
  return e;
}
struct Mark {  // records a (start, stop) event pair around a launch group when profiling
  aigar_handle *h;
  const char *name;
  hipEvent_t a = nullptr;
  Mark(aigar_handle *hh, const char *n) : h(hh), name(n) {
    if (h->profile) {
      a = pool_event(h);
      (void)hipEventRecord(a, h->stream);
    }
  }
  ~Mark() {
    if (!a) return;
    hipEvent_t b = pool_event(h);
    (void)hipEventRecord(b, h->stream);
    h->marks.push_back({name, {a, b}});
  }
};

extern "C" int aigar_create(const aigar_config *cfg, aigar_handle **out) {
  if (!cfg || !out) return fail("aigar_create: null argument");
  if (cfg->n_arenas < 1 || cfg->bots_per_arena < 1) return fail("aigar_create: need n_arenas >= 1 and bots >= 1");
  if (cfg->rng_mode != AIGAR_RNG_PHILOX)
    return fail("aigar_create: the device stepper runs AIGAR_RNG_PHILOX only (MT19937 lives in the CPU oracle)");
  int G = cfg->grid_squares ? cfg->grid_squares : 11;
  if (G < 1 || G > 127) return fail("aigar_create: grid_squares must be in [1, 127]");
  if (cfg->obs_channels & AIGAR_OBS_ALL &&
      cfg->obs_channels & (AIGAR_OBS_SELF_LF | AIGAR_OBS_SELF_SLF | AIGAR_OBS_ENEMY_LF | AIGAR_OBS_ENEMY_SLF))
    return fail("aigar_create: ALL_PLAYER_GRID with last-frame grids is undefined in the reference");
  if ((cfg->flags & AIGAR_FLAG_SCORE) &&
      (std::max(1, cfg->tile_x) * std::max(1, cfg->tile_y) > 1 || (cfg->tile_flags & AIGAR_TILE_FORCE)))
    return fail("aigar_create: AIGAR_FLAG_SCORE (the mass history score) is not kept on a tiled handle");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail("aigar_create: device %d not present (%d devices)", cfg->device, ndev);
  HIPCHK(hipSetDevice(cfg->device));
  aigar_handle *h = new aigar_handle();
  h->cfg = *cfg;
  if (getenv("AIGAR_NO_GRAPH")) h->use_graph = false;
  if (const char *u = getenv("AIGAR_RUN_UNROLL")) h->run_unroll = std::max(1, std::min(64, atoi(u)));
  if (getenv("AIGAR_TILE_GRAPH")) h->tile_graph = true;
  h->d.pp_par = getenv("AIGAR_PP_SERIAL") ? 0 : 1;
  // tuning knob: a fixed number of reservation rounds for every population
  if (const char *r = getenv("AIGAR_FOOD_ROUNDS")) h->rounds = std::max(1, std::min(16, atoi(r)));
  Dev &d = h->d;
  d.A = cfg->n_arenas;
  d.B = cfg->bots_per_arena;
  d.NP = d.A * d.B;
  d.size = cfg->field_size > 0 ? cfg->field_size : (int)(75 * std::sqrt((double)d.B));
  d.cols = (int)std::ceil(d.size / 20.0);
  d.H = d.cols * d.cols;
  d.virus_enabled = cfg->virus_enabled ? 1 : 0;
  d.max_pellets = cfg->max_pellets >= 0 ? cfg->max_pellets : (double)d.size * d.size * 0.015;
  d.max_viruses = cfg->max_viruses >= 0 ? cfg->max_viruses : (double)d.size * d.size * 0.00005;
  if (!d.virus_enabled) d.max_viruses = 0;
  auto r64 = [](int v) { return (v + 63) / 64 * 64; };  // a wavefront never straddles two arenas
  d.Ecap = r64(cfg->blob_cap > 0 ? cfg->blob_cap : 4 * d.B + 256);
  d.Pcap = r64(cfg->pellet_cap > 0 ? cfg->pellet_cap : (int)std::ceil(d.max_pellets) + d.Ecap + 64);
  d.Vcap = r64(cfg->virus_cap > 0 ? cfg->virus_cap : 2 * (int)std::ceil(d.max_viruses) + 64);
  // the pellet row store (aigar_dev.h): per bucket row a home of PR slots, twice;
  // PR leaves a quarter of headroom over the row's share of Pcap (uniform spawns
  // put ~Pcap / cols pellets in a row) plus 64
  if (d.cols > 1024) {
    delete h;
    return fail("aigar_create: field size %d: more than 1024 bucket rows", d.size);
  }
  d.PR = r64((int)std::ceil(1.25 * d.Pcap / d.cols) + 64);
  d.PS = 2 * d.cols * d.PR;
  d.PD = d.PS + d.Pcap;
  d.PH1 = d.cols * (d.cols + 1) + 1;
  d.Wcap = std::max(kMaxCells * d.B, std::max(d.Ecap, 4096));
  d.EVcap = cfg->event_cap > 0 ? cfg->event_cap : 65536;
  d.G = G;
  d.L = obs_len_of(*cfg);
  d.obs_ch = cfg->obs_channels;
  d.obs_ex = cfg->obs_extras;
  d.flags = cfg->flags;
  d.occ_words = (d.H + 63) / 64;
  d.scan_tiles = (d.H + 2047) / 2048;
  d.pl_tiles = (d.B + 255) / 256;
  // C4 tiles: bucket-aligned tiles, ownership by centre bucket
  const int tx = std::max(1, cfg->tile_x), ty = std::max(1, cfg->tile_y);
  d.ntiles = tx * ty;
  d.tiled = d.ntiles > 1 || (cfg->tile_flags & AIGAR_TILE_FORCE);
  d.own_bx0 = d.own_by0 = d.loc_bx0 = d.loc_by0 = 0;
  d.own_bx1 = d.own_by1 = d.loc_bx1 = d.loc_by1 = d.cols;
  if (d.tiled) {
    auto bad = [&](const char *m) {
      delete h;
      return fail("aigar_create: %s", m);
    };
    if (d.A != 1) return bad("a tiled handle steps one arena (n_arenas must be 1)");
    if (cfg->tile_id < 0 || cfg->tile_id >= d.ntiles) return bad("tile_id out of range");
    if (tx > d.cols || ty > d.cols) return bad("more tiles than hash buckets along a side");
    const int ix = cfg->tile_id % tx, iy = cfg->tile_id / tx;
    const int halo = cfg->tile_halo > 0 ? cfg->tile_halo : 400;
    // an owned cell's boxes (pellet turn, blob turn, one bucket of food footprint)
    // reach <= 6 buckets from its centre bucket at the mass cap: with 7 its owner
    // holds every food it can touch, so every cell is decidable somewhere
    const int hb = std::max(7, (halo + kBucket - 1) / kBucket);
    if (d.ntiles > 64) return bad("at most 64 tiles");
    d.tile_id = cfg->tile_id;
    d.tile_flags = cfg->tile_flags;
    d.own_bx0 = ix * d.cols / tx;
    d.own_bx1 = (ix + 1) * d.cols / tx;
    d.own_by0 = iy * d.cols / ty;
    d.own_by1 = (iy + 1) * d.cols / ty;
    d.loc_bx0 = std::max(0, d.own_bx0 - hb);
    d.loc_bx1 = std::min(d.cols, d.own_bx1 + hb);
    d.loc_by0 = std::max(0, d.own_by0 - hb);
    d.loc_by1 = std::min(d.cols, d.own_by1 + hb);
  }
  d.tile_nx = tx;
  d.tile_ny = ty;
  d.tile_gate = 0;
  d.tcap = cfg->tile_cap > 0 ? cfg->tile_cap : 2048;
  d.bm_words = (int)(((size_t)kMaxCells * d.NP + 255) / 256 * 4);  // 16 * NP bits, whole TileRecs
  // observation-history hand-off: the grids the observation keeps per bot
  // (self / enemy, last / second-last frame), 4 doubles per 32-byte record
  {
    const uint32_t ch = cfg->obs_channels;
    d.nh = ((ch & (AIGAR_OBS_SELF_LF | AIGAR_OBS_SELF_SLF)) ? 1 : 0) + ((ch & AIGAR_OBS_SELF_SLF) ? 1 : 0) +
           ((ch & (AIGAR_OBS_ENEMY_LF | AIGAR_OBS_ENEMY_SLF)) ? 1 : 0) + ((ch & AIGAR_OBS_ENEMY_SLF) ? 1 : 0);
    d.hrec = 1 + (d.nh * G * G + 3) / 4;
    d.hcap = std::min(kHcapMax, std::max(16, d.tcap / 64));
  }
  h->box_recs = 1 + d.tcap + std::max(d.bm_words / 4, d.hcap * d.hrec);
  for (int k = 0; k <= kMaxCells; k++) d.pow_n032[k] = aigar_math::pow_glibc((double)k, 0.32);
  d.cshift = 3;  // coarse blob/virus grids: 160 x 160 field units per cell, <= 4096 cells (grid_small_build)
  while ((((d.cols + (1 << d.cshift) - 1) >> d.cshift) * ((d.cols + (1 << d.cshift) - 1) >> d.cshift)) > 4096)
    d.cshift++;
  d.cshift_c = 0;  // player-cell grid: as fine as one block's LDS histogram allows
  while ((((d.cols + (1 << d.cshift_c) - 1) >> d.cshift_c) * ((d.cols + (1 << d.cshift_c) - 1) >> d.cshift_c)) > 4096)
    d.cshift_c++;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return fail("hipStreamCreate failed");
  }
  const size_t A = d.A, NP = d.NP, C = (size_t)kMaxCells * NP, H1 = (size_t)d.H + 1, GG = (size_t)G * G;
  bool ok = true;
#define AL(field, T, n)                     \
  do {                                      \
    d.field = dalloc<T>(h, (n));            \
    ok = ok && d.field != nullptr;          \
  } while (0)
#ifndef AIGAR_NO_ARENA
  for (int pass = 0; pass < 2; pass++) {  // 0: size the arena, 1: carve it
    h->arena_sizing = pass == 0;
    if (pass == 1) {
      h->arena_size = h->arena_used;
      h->arena_used = 0;
      void *base = nullptr;
      if (hipMalloc(&base, h->arena_size) != hipSuccess) {
        ok = false;
        break;
      }
      h->allocs.push_back(base);
      (void)hipMemset(base, 0, h->arena_size);
      h->arena = (char *)base;
    }
#endif
  AL(ctl, ArenaCtl, A);
  AL(p_alive, int, NP); AL(p_respawn, int, NP); AL(p_ncells, int, NP); AL(p_split, int, NP); AL(p_eject, int, NP);
  AL(p_pend, int, NP); AL(p_cmdx, double, NP); AL(p_cmdy, double, NP); AL(p_list, uint8_t, C);
  AL(p_newc, int, NP); AL(p_heavy, int, NP); AL(p_newb, int, NP); AL(p_seqoff, int, NP); AL(p_bloboff, int, NP);
  AL(c_x, double, C); AL(c_y, double, C); AL(c_m, double, C); AL(c_r, double, C); AL(c_vx, double, C);
  AL(c_vy, double, C); AL(c_svx, double, C); AL(c_svy, double, C); AL(c_mt, double, C); AL(c_svc, int, C);
  AL(c_flags, uint32_t, C); AL(c_seq, int64_t, C); AL(c_active, uint8_t, C);
  AL(sp_r, double, C); AL(sp_svx, double, C); AL(sp_svy, double, C);
  AL(sb_x, double, C); AL(sb_y, double, C); AL(sb_svx, double, C); AL(sb_svy, double, C); AL(sb_slot, uint8_t, C);
  const size_t P = A * d.Pcap, PSA = A * d.PS, PDA = A * d.PD, PHA = A * d.PH1;
  AL(pel, PelRec, PSA); AL(pel_col, int, PSA);
  AL(pn, PelRec, P); AL(pn_col, int, P);
  AL(pel_dead, uint8_t, PDA); AL(pel_rank, int, P); AL(pncnt, int, PHA); AL(pstart, int, PHA);
  AL(pel_owner, uint64_t, PDA);
  const size_t E = A * d.Ecap, V = A * d.Vcap;
  AL(b_x, double, E); AL(b_y, double, E); AL(b_m, double, E); AL(b_r, double, E); AL(b_vx, double, E);
  AL(b_vy, double, E); AL(b_svx, double, E); AL(b_svy, double, E); AL(b_svc, int, E); AL(b_seq, int64_t, E);
  AL(b_ej, int64_t, E); AL(b_flags, uint32_t, E); AL(b_owner, uint64_t, E); AL(b_col, int, E);
  AL(bstart, int, A * H1); AL(bitems, int, E); AL(b_rank, int, E); AL(bmap, uint64_t, A * 64);
  AL(v_x, double, V); AL(v_y, double, V); AL(v_m, double, V); AL(v_r, double, V); AL(v_vx, double, V);
  AL(v_vy, double, V); AL(v_svx, double, V); AL(v_svy, double, V); AL(v_svc, int, V); AL(v_seq, int64_t, V);
  AL(v_flags, uint32_t, V); AL(v_active, int, V);
  AL(vcnt, int, A * H1); AL(vstart, int, A * H1); AL(vitems, int, V); AL(v_rank, int, V);
  AL(ccnt, int, A * H1); AL(cstart, int, A * H1); AL(citems, int, C); AL(c_rank, int, C);
  AL(cgcnt, int, A * 2 * 4100);
  AL(occ, unsigned long long, A * d.occ_words); AL(occ_cnt, int, A * d.H);
  AL(dead, int, NP); AL(work, int, A * d.Wcap); AL(work2, int, A * d.Wcap);
  AL(f_list, int, C * FCAP); AL(f_cnt, uint8_t, C); AL(f_done, uint8_t, C);
  AL(resp_slot, int, NP); AL(resp_list, int, NP);
  AL(ev, int64_t, A * d.EVcap * 5);
  AL(o_lastfov, double, NP); AL(o_self_lf, double, NP * GG); AL(o_self_slf, double, NP * GG);
  AL(o_en_lf, double, NP * GG); AL(o_en_slf, double, NP * GG); AL(o_act_cur, double, NP * 4);
  AL(o_act_prev, double, NP * 4);
  d.OBcap = (int)std::min<size_t>(std::max<size_t>(1u << 20, 64 * NP), (size_t)1 << 24);
  AL(scan_state, unsigned long long, 2 * A * d.scan_tiles);
  AL(pl_state, unsigned long long, A * d.pl_tiles);
  AL(ticket, int, 16);
  AL(kill_list, int, P); AL(spec_x, double, A * 64); AL(spec_y, double, A * 64); AL(spec_m, double, A * 64); 
  AL(ob_used, unsigned long long, 1);
  AL(ob_epoch, uint32_t, 1);
  AL(p_split_lh, int, NP);
  AL(p_role, uint8_t, NP);
  AL(p_time, int, NP);
  AL(o_last_mass, double, NP);
  if (d.tiled) {
    AL(t_holder, int, NP);
    AL(t_obsby, int, NP);
    AL(t_holive, int, NP);
    AL(t_hodefer, uint8_t, NP);
    AL(t_hoslot, int, d.hcap);
    AL(outbox, TileRec, h->box_recs);
    TileRec *ib = nullptr;
    ib = dalloc<TileRec>(h, (size_t)h->box_recs * d.ntiles);
    ok = ok && ib != nullptr;
    d.inbox = ib;
  }
  AL(p_fx, double, NP); AL(p_fy, double, NP); AL(p_fs, double, NP); AL(p_mass, double, NP); AL(ob_seq, int64_t, d.OBcap); AL(ob_m, double, d.OBcap); AL(ob_r, double, d.OBcap);
  AL(ob_mask, uint32_t, d.OBcap); AL(ob_own, uint8_t, d.OBcap); AL(ob_perm, int, d.OBcap);
  d.ob_wmask = nullptr;
  if (G > 16) AL(ob_wmask, uint64_t, 4 * (size_t)d.OBcap);
  d.sc = nullptr;
  d.sc_ctl = nullptr;
  if (cfg->flags & AIGAR_FLAG_SCORE) {  // (zeroed with the arena: no samples, no trace)
    AL(sc, double, 4 * NP);
    AL(sc_ctl, ScoreCtl, 1);
  }
#undef AL
  h->scr_k = dalloc<int64_t>(h, A * d.Wcap);
  h->scr_v = dalloc<int>(h, A * d.Wcap);
  h->d_cmd = dalloc<double>(h, NP * 4);
  h->d_mask = dalloc<uint8_t>(h, NP);
  h->d_nnmask = dalloc<uint8_t>(h, NP);
  h->d_stats = dalloc<double>(h, NP * 5);
  h->d_obs = dalloc<double>(h, NP * (size_t)d.L);
  h->d_rlist = dalloc<int>(h, A);
  h->d_rseed = dalloc<uint64_t>(h, A);
  if (d.sc) {
    h->d_score = dalloc<double>(h, NP * 4);
    ok = ok && h->d_score;
  }
  ok = ok && h->scr_k && h->scr_v && h->d_cmd && h->d_stats && h->d_obs && h->d_mask && h->d_nnmask && h->d_rlist &&
       h->d_rseed;
#ifndef AIGAR_NO_ARENA
  }
  h->arena_sizing = false;
  h->arena = nullptr;  // later dalloc calls (pixel buffers) allocate on their own
#endif
  if (ok) (void)hipMemset(h->d_nnmask, 1, NP);  // every player is NN until aigar_set_roles
  if (ok && !d.tiled) {  // (aigar_reset_arenas refuses tiled handles)
    ok = hipHostMalloc((void **)&h->h_reset, aigar_handle::kResetSlots * A * 2 * sizeof(uint64_t),
                       hipHostMallocDefault) == hipSuccess;
    for (hipEvent_t &e : h->ev_reset) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  }
  (void)hipEventCreate(&h->ev0);
  (void)hipEventCreate(&h->ev1);
  if (!ok) {
    free_all(h);
    delete h;
    return fail("aigar_create: device allocation failed");
  }
  if (hipDeviceSynchronize() != hipSuccess) {
    free_all(h);
    delete h;
    return fail("aigar_create: device synchronize failed");
  }
  *out = h;
  return 0;
}

extern "C" int aigar_destroy(aigar_handle *h) {
  if (!h) return 0;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  free_all(h);
  delete h;
  return 0;
}

static int check_device_errors(aigar_handle *h) {
  std::vector<ArenaCtl> ctl(h->d.A);
  HIPCHK(hipMemcpyAsync(ctl.data(), h->d.ctl, sizeof(ArenaCtl) * h->d.A, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int a = 0; a < h->d.A; a++)
    if (ctl[a].err)
      return fail("device error bits 0x%x in arena %d (1 pellet cap, 2 blob cap, 4 virus cap, 8 event cap, "
                  "16 worklist cap, 32 observation cap, 64 candidate cap, 128 slot, 256 pixel-frame object cap, "
                  "512 tile message cap, 1024 tile record lookup, 2048 tile view beyond the held pellets, "
                  "4096 tiled tick ended with undone cells, 8192 new-cell / blob counts not as predicted, "
                  "16384 more dead bots to hand off than hand-off slots)",
                  ctl[a].err, a);
  return 0;
}

static size_t pix_hist_bytes(const aigar_handle *h) {
  return (h->pix.flags & AIGAR_PIX_LAST) ? sizeof(uint32_t) * h->d.NP * (size_t)h->pix.side * h->pix.side : 0;
}
// the pixel history of the selected arenas' bots (row: the B * side * side words of one arena)
__global__ void __launch_bounds__(256) k_pix_hist_clear_arenas(uint32_t *hist, size_t row, ArenaSel sel) {
  uint32_t *p = hist + (size_t)sel.arena(blockIdx.y) * row;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < row; i += (size_t)gridDim.x * blockDim.x) p[i] = 0;
}
// ... of the players with mask[i] != 0 (null: all); LL = side * side words a player
__global__ void __launch_bounds__(256) k_pix_hist_clear_bots(uint32_t *hist, size_t LL, size_t n, const uint8_t *mask) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i / LL])) hist[i] = 0;
}

__global__ void k_fill_d(double *p, size_t n, double v) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// What a restart clears beside the Dev buffers, for the bots of the selected
// arenas: the pixel history, the replay memory's oldState marks (Bot.reset:
// oldState = None) and the Orn-Uhl noise state
static void restart_side_buffers(aigar_handle *h, const ArenaSel &sel) {
  const Dev &d = h->d;
  if (h->d_pix_hist) {
    const size_t row = (size_t)d.B * h->pix.side * h->pix.side;
    const unsigned nb = (unsigned)std::min<size_t>((row + 255) / 256, 256);
    hipLaunchKernelGGL(k_pix_hist_clear_arenas, dim3(nb, sel.n), dim3(256), 0, h->stream, h->d_pix_hist, row, sel);
  }
  if (h->exp.cap) hipLaunchKernelGGL(k_exp_clear_arenas, dim3(sel.n), dim3(256), 0, h->stream, h->exp.has_old, d.B, sel);
  if (h->noi.n_act)
    hipLaunchKernelGGL(k_noise_clear_arenas, dim3(sel.n), dim3(256), 0, h->stream, h->noi.ou, d.B * h->noi.n_act, sel);
}
// a tiled handle: every tile's history copy is current, and the hand-off priorities restart
static int tiles_restart(aigar_handle *h) {
  const Dev &d = h->d;
  if (!d.tiled) return 0;
  HIPCHK(hipMemsetAsync(d.t_holder, 0xFF, sizeof(int) * d.NP, h->stream));
  HIPCHK(hipMemsetAsync(d.t_obsby, 0xFF, sizeof(int) * d.NP, h->stream));
  HIPCHK(hipMemsetAsync(d.t_hodefer, 0, d.NP, h->stream));
  return 0;
}

extern "C" int aigar_reset(aigar_handle *h, uint64_t seed) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const ArenaSel sel{nullptr, nullptr, seed, 0, h->d.A};
  restart_side_buffers(h, sel);
  if (tiles_restart(h)) return -1;
  launch_restart(h->d, h->stream, sel);
  HIPCHK(hipGetLastError());
  return check_device_errors(h);
}

extern "C" int aigar_reset_arenas(aigar_handle *h, const int32_t *arenas, const uint64_t *seeds, int n) {
  if (!h) return fail("null handle");
  const Dev &d = h->d;
  if (d.tiled) return fail("reset_arenas: a tiled handle steps one arena across tiles (reset it with aigar_reset)");
  if (n < 0) return fail("reset_arenas: n = %d is negative", n);
  if (n > d.A) return fail("reset_arenas: n = %d arenas listed, the handle has %d", n, d.A);
  if (n == 0) return 0;
  if (!arenas || !seeds) return fail("reset_arenas: null list");
  std::vector<char> seen(d.A, 0);
  for (int k = 0; k < n; k++) {
    const int a = arenas[k];
    if (a < 0 || a >= d.A) return fail("reset_arenas: arena %d (entry %d) out of range [0, %d)", a, k, d.A);
    if (seen[a]) return fail("reset_arenas: duplicate arena %d (entry %d)", a, k);
    seen[a] = 1;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  const int slot = (int)(h->reset_calls++ % aigar_handle::kResetSlots);
  HIPCHK(hipEventSynchronize(h->ev_reset[slot]));  // (done long ago, unless the caller issues resets back to back)
  char *base = h->h_reset + (size_t)slot * d.A * 2 * sizeof(uint64_t);  // (slots stay 8-byte aligned)
  uint64_t *hs = (uint64_t *)base;
  int *ha = (int *)(base + (size_t)d.A * sizeof(uint64_t));
  memcpy(hs, seeds, sizeof(uint64_t) * n);
  for (int k = 0; k < n; k++) ha[k] = arenas[k];
  HIPCHK(hipMemcpyAsync(h->d_rseed, hs, sizeof(uint64_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_rlist, ha, sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipEventRecord(h->ev_reset[slot], h->stream));
  {
    Mark m(h, "reset_arenas");
    const ArenaSel sel{h->d_rlist, h->d_rseed, 0, 0, n};
    launch_restart(d, h->stream, sel);
    restart_side_buffers(h, sel);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_set_commands(aigar_handle *h, const double *cmd, int on_device) {
  if (!h || !cmd) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const double *src = cmd;
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(h->d_cmd, cmd, sizeof(double) * 4 * h->d.NP, hipMemcpyHostToDevice, h->stream));
    src = h->d_cmd;
  }
  launch_set_commands(h->d, h->stream, src);
  HIPCHK(hipGetLastError());
  if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));  // caller may reuse its buffer
  return 0;
}

extern "C" int aigar_policy_random(aigar_handle *h, double p_split, double p_eject, uint64_t seed) {
  if (!h) return fail("null handle");
  Mark m(h, "policy");
  launch_policy(h->d, h->stream, p_split, p_eject, seed);  // draws keyed by (seed, tick, player)
  HIPCHK(hipGetLastError());
  return 0;
}

// Capture launch(stream) into an executable graph on the handle's private
// capture stream: graphs are then replayed on whatever stream the caller gave
// (torch's default stream is the legacy null stream, which cannot capture).
template <class F>
static hipGraphExec_t capture_graph(aigar_handle *h, F launch) {
  if (!h->cap_stream && hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking) != hipSuccess) {
    h->cap_stream = nullptr;
    return nullptr;
  }
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  bool ok = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
  if (ok) {
    launch(h->cap_stream);
    ok = hipStreamEndCapture(h->cap_stream, &g) == hipSuccess && g;
  }
  if (ok) ok = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
  if (g) (void)hipGraphDestroy(g);
  if (!ok) {
    if (ge) (void)hipGraphExecDestroy(ge);
    (void)hipGetLastError();
    return nullptr;
  }
  return ge;
}
template <class K>
template <class F>
bool KeyedSlot<K>::ensure(aigar_handle *h, const K &k, F issue) {
  if (holds(k)) return true;
  drop(h);
  exec = capture_graph(h, issue);
  memcpy(image, &k, sizeof(K));
  return exec != nullptr;
}

__global__ void k_step_begin(Dev d) {
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < d.A) d.ctl[a].n_ev = 0;
}

static int food_rounds(const aigar_handle *h) { return h->rounds > 0 ? h->rounds : (h->greedy_seen ? 2 : 1); }

// food_rounds() follows the handle's history: when a Greedy policy first runs, the
// graphs captured with the old round count are dropped (recaptured at their next
// call), so a step graph and the tile passes never mix round counts.  (The
// Field.update graph of aigar_step has the round count in its key.)
static void note_greedy(aigar_handle *h) {
  if (h->greedy_seen) return;
  h->greedy_seen = true;
  if (h->rounds > 0) return;  // (the round count is fixed: nothing changes)
  for (GraphSlot *g : h->slots)
    if (g != &h->step) g->drop(h);
  h->run_u_tried = false;
}

extern "C" int aigar_step(aigar_handle *h, int n_ticks) {
  if (!h) return fail("null handle");
  if (n_ticks < 0) return fail("n_ticks < 0");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->d.flags & AIGAR_FLAG_EVENTS)  // the event log restarts every step
    hipLaunchKernelGGL(k_step_begin, dim3((h->d.A + 63) / 64), dim3(64), 0, h->stream, h->d);
  const int rounds = food_rounds(h);
  StepKey k;
  key_clear(k);
  k.rounds = rounds;  // (the population changes the eat phase's rounds)
  // capture one Field.update() (~25 kernel launches) once; replay it per tick
  if (h->use_graph && !h->graph_failed && n_ticks > 0 &&
      !h->step.ensure(h, k, [&](hipStream_t cs) { launch_tick(h->d, cs, rounds, h->scr_k, h->scr_v); }))
    h->graph_failed = true;
  for (int t = 0; t < n_ticks; t++) {
    Mark m(h, "tick");
    if (h->step.exec) HIPCHK(h->step.launch(h));
    else launch_tick(h->d, h->stream, rounds, h->scr_k, h->scr_v);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// One batched env step -- Model.update's takeBotActions + Field.update + every
// bot's getStateRepresentation (model.py:100-112, bot.py:272-299) -- captured
// once as a single hipGraph and replayed n_steps times: no host round trip
// between the policy, the tick's ~25 kernels and the observation.
// policy_done: this step's Greedy moves were picked by the previous step's
// observation (fuse_next there); fuse_next: this step's observation also picks the
// next step's Greedy moves (observe_fuses_greedy) -- one launch fewer per step
static void launch_env_step(aigar_handle *h, hipStream_t s, const aigar_run_params &p, void *out, int dtype,
                            bool policy_done = false, bool fuse_next = false) {
  // the random population's policy runs inside the tick's first kernel (same draws as aigar_policy_random)
#ifdef AIGAR_NO_POLICY_FOLD  // (diagnostics build: the policy as its own launch)
  const RandomPolicy rp{0, 0, 0, 0};
  if (p.policy == AIGAR_POLICY_RANDOM) launch_policy(h->d, s, p.p_split, p.p_eject, p.seed);
#else
  const RandomPolicy rp{p.policy == AIGAR_POLICY_RANDOM, p.p_split, p.p_eject, p.seed};
#endif
  if (p.policy == AIGAR_POLICY_GREEDY && !policy_done) launch_policy_greedy(h->d, s, p.greedy_split ? 1 : 0, nullptr, -1);
  // (a Greedy population splits by choice and many players hold several cells: the eat-phase
  // preparation and the pp activity test walk all of a player's cells at once, tick.hip prep_multi)
  launch_tick(h->d, s, food_rounds(h), h->scr_k, h->scr_v, &rp);
  if (out) launch_observe(h->d, s, out, dtype, 0, nullptr, fuse_next ? (p.greedy_split ? 1 : 0) : -1);  // epoch 0: the device-side epoch
}
// aigar_run's unrolled graph may carry each step's Greedy moves in the step before
static bool run_fuses_greedy(const aigar_handle *h, const aigar_run_params &p, const void *out) {
  return p.policy == AIGAR_POLICY_GREEDY && out && observe_fuses_greedy(h->d) &&
         !getenv("AIGAR_NO_GREEDY_FUSE");
}

extern "C" int aigar_run(aigar_handle *h, int n_steps, const aigar_run_params *p, void *obs_out, int dtype) {
  if (!h || !p) return fail("null argument");
  if (n_steps < 0) return fail("n_steps < 0");
  if (p->policy < AIGAR_POLICY_NONE || p->policy > AIGAR_POLICY_GREEDY) return fail("unknown policy %d", p->policy);
  if (obs_out && dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->d.flags & AIGAR_FLAG_EVENTS)  // the event log restarts every call (all n_steps accumulate)
    hipLaunchKernelGGL(k_step_begin, dim3((h->d.A + 63) / 64), dim3(64), 0, h->stream, h->d);
  if (p->policy == AIGAR_POLICY_GREEDY) note_greedy(h);  // (food_rounds)
  RunKey k;
  key_clear(k);
  key_put(k.p, *p);
  k.out = obs_out;
  k.dtype = obs_out ? dtype : -1;
  if (h->use_graph && n_steps > 0 && !h->run.holds(k)) {
    h->run_u.drop(h);
    h->run_u_tried = false;
    if (!h->run.ensure(h, k, [&](hipStream_t cs) { launch_env_step(h, cs, *p, obs_out, dtype); }))
      return fail("aigar_run: graph capture failed");
  }
  // run_unroll > 1: the same step captured that many times in one graph -- one
  // graph launch, and one inter-graph gap, per run_unroll steps.  Captured at the
  // first call of the key that can use it; if that capture fails, the one-step
  // graph serves alone.
  if (h->run.exec && !h->run_u.exec && !h->run_u_tried && h->run_unroll > 1 && n_steps >= h->run_unroll &&
      !h->profile) {
    h->run_u_tried = true;
    // (the Greedy population: steps 1.. of the graph take the moves their previous
    // step's observation picked -- the first step, and the one-step graph, run the policy)
    const bool fuse = run_fuses_greedy(h, *p, obs_out);
    h->run_u.exec = capture_graph(h, [&](hipStream_t cs) {
      for (int k = 0; k < h->run_unroll; k++)
        launch_env_step(h, cs, *p, obs_out, dtype, fuse && k > 0, fuse && k + 1 < h->run_unroll);
    });
  }
  int t = 0;
  if (h->run_u.exec && !h->profile)
    for (; t + h->run_unroll <= n_steps; t += h->run_unroll) HIPCHK(h->run_u.launch(h));
  for (; t < n_steps; t++) {
    Mark m(h, "run");
    if (h->run.exec) HIPCHK(h->run.launch(h));
    else launch_env_step(h, h->stream, *p, obs_out, dtype);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- C4 tiles
static int need_tiled(aigar_handle *h) {
  if (!h) return fail("null handle");
  if (!h->d.tiled) return fail("not a tiled handle (tile_x * tile_y must be > 1, or AIGAR_TILE_FORCE)");
  return 0;
}
extern "C" int aigar_tile_info(aigar_handle *h, int32_t *info, void **outbox, void **inbox, int64_t *msg_bytes) {
  if (need_tiled(h)) return -1;
  const Dev &d = h->d;
  if (info) {
    const int32_t v[14] = {d.ntiles, d.tile_id, d.own_bx0, d.own_bx1, d.own_by0, d.own_by1,
                           d.loc_bx0, d.loc_bx1, d.loc_by0, d.loc_by1, d.tcap, d.bm_words, d.hcap, d.hrec};
    memcpy(info, v, sizeof v);
  }
  if (outbox) *outbox = d.outbox;
  if (inbox) *inbox = (void *)d.inbox;
  if (msg_bytes) *msg_bytes = (int64_t)h->box_recs * (int64_t)sizeof(TileRec);
  return 0;
}
extern "C" int aigar_tile_msg_bytes(aigar_handle *h, int64_t *bytes) {
  if (need_tiled(h) || !bytes) return bytes ? -1 : fail("null argument");
  if (!h->pass_recs) return fail("tile_msg_bytes: no pass begun");
  *bytes = (int64_t)h->pass_recs * (int64_t)sizeof(TileRec);
  return 0;
}
extern "C" int aigar_tile_set_buffers(aigar_handle *h, void *outbox, void *inbox) {
  if (need_tiled(h)) return -1;
  if (!outbox || !inbox) return fail("tile_set_buffers: null buffer");
  HIPCHK(hipStreamSynchronize(h->stream));
  h->d.outbox = (TileRec *)outbox;
  h->d.inbox = (const TileRec *)inbox;
  return 0;
}
// Greedy bots on tiles: each tile moves the bots it observes, the commands go
// round in their own message (k_tile_cmd_collect / k_tile_cmd_apply, tick.hip)
extern "C" int aigar_tile_policy(aigar_handle *h, int greedy_split) {
  if (need_tiled(h)) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  note_greedy(h);  // (food_rounds)
  {
    Mark m(h, "policy");
    launch_tile_policy(h->d, h->stream, greedy_split ? 1 : 0, h->d_mask, h->box_recs - 1);
  }
  h->pass_recs = h->box_recs;  // (the command message: the whole buffer is exchanged)
  h->cmd_ready = false;
  h->cmd_pending = true;
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aigar_tile_apply_commands(aigar_handle *h) {
  if (need_tiled(h)) return -1;
  // (a flag of its own: pass_recs alone can equal box_recs after an eat pass)
  if (!h->cmd_pending || h->pass_recs != h->box_recs)
    return fail("tile_apply_commands: no aigar_tile_policy before it");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_tile_cmd_apply(h->d, h->stream, h->box_recs);
  HIPCHK(hipGetLastError());
  h->pass_recs = 0;
  h->cmd_pending = false;
  h->cmd_ready = true;
  return 0;
}
extern "C" int aigar_tile_begin(aigar_handle *h, const aigar_run_params *p) {
  if (need_tiled(h) || !p) return p ? -1 : fail("null argument");
  if (p->policy == AIGAR_POLICY_GREEDY && !h->cmd_ready)
    return fail("tile_begin: GREEDY needs this tick's commands (aigar_tile_policy, all-gather, "
                "aigar_tile_apply_commands): no tile holds every pellet a Greedy move reads");
  if (p->policy != AIGAR_POLICY_NONE && p->policy != AIGAR_POLICY_RANDOM && p->policy != AIGAR_POLICY_GREEDY)
    return fail("tile_begin: unknown policy %d", p->policy);
  h->cmd_ready = false;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->d.flags & AIGAR_FLAG_EVENTS)  // the event log holds this tick
    hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(64), 0, h->stream, h->d);
  const RandomPolicy rp{p->policy == AIGAR_POLICY_RANDOM, p->p_split, p->p_eject, p->seed};  // (GREEDY: set already)
  auto issue = [&](hipStream_t s) {
    launch_tick_pre(h->d, s, h->scr_k, h->scr_v, &rp);
    launch_tile_pass(h->d, s, food_rounds(h), h->scr_k, h->scr_v, 1);
  };
  TileKey k;
  key_clear(k);
  key_put(k.p, *p);
  k.box[0] = h->d.outbox;
  k.box[1] = h->d.inbox;
  const bool graphed = h->tile_graph && h->tb.ensure(h, k, issue);
  {
    Mark m(h, "tile_begin");
    if (graphed) HIPCHK(h->tb.launch(h));
    else issue(h->stream);
  }
  h->pass_recs = 1 + h->d.tcap + h->d.hcap * h->d.hrec;  // (+ the observation-history hand-off slots)
  h->cmd_pending = false;
  h->first_pass = 1;
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aigar_tile_apply(aigar_handle *h, int *undone) {
  if (need_tiled(h)) return -1;
  if (!h->pass_recs) return fail("tile_apply: no pass begun");
  HIPCHK(hipSetDevice(h->cfg.device));
  {
    Mark m(h, "tile_apply");
    launch_tile_apply(h->d, h->stream, h->pass_recs, h->first_pass);
  }
  HIPCHK(hipGetLastError());
  if (!undone) return 0;  // device-decided passes: no host round trip (aigar_tile_resume gates itself)
  ArenaCtl c;
  HIPCHK(hipMemcpyAsync(&c, h->d.ctl, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (c.err) return check_device_errors(h);
  *undone = c.n_undone_glob;
  return 0;
}
extern "C" int aigar_tile_resume(aigar_handle *h) {
  if (need_tiled(h)) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  Mark m(h, "tile_resume");
  launch_tile_pass(h->d, h->stream, food_rounds(h), h->scr_k, h->scr_v, 0);
  h->pass_recs = 1 + h->d.tcap + h->d.bm_words / 4;
  h->cmd_pending = false;
  h->first_pass = 0;
  HIPCHK(hipGetLastError());
  return 0;
}
extern "C" int aigar_tile_end(aigar_handle *h, void *obs_out, int dtype) {
  if (need_tiled(h)) return -1;
  if (obs_out && dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->profile || !h->tile_graph) {  // separate launches (the post phases and the observation timed apart)
    {
      Mark m(h, "tile_end");
      launch_tick_post(h->d, h->stream, h->scr_k, h->scr_v);
    }
    if (obs_out) {
      Mark m(h, "observe");
      launch_observe(h->d, h->stream, obs_out, dtype, 0);
    }
    HIPCHK(hipGetLastError());
    return 0;
  }
  auto issue = [&](hipStream_t s) {
    launch_tick_post(h->d, s, h->scr_k, h->scr_v);
    if (obs_out) launch_observe(h->d, s, obs_out, dtype, 0);
  };
  TileKey k;
  key_clear(k);
  k.box[0] = h->d.outbox;
  k.box[1] = h->d.inbox;
  k.out = obs_out;
  k.dtype = obs_out ? dtype : -1;
  if (h->use_graph && h->te.ensure(h, k, issue)) HIPCHK(h->te.launch(h));
  else issue(h->stream);
  HIPCHK(hipGetLastError());
  return 0;
}
// in-process transport: every handle's outbox into every handle's inbox slot
// No host synchronisation: each source's outbox is complete when its stream
// reaches the recorded event (every destination waits for it before copying),
// and every source's later work (the next pass rewrites its outbox) waits for
// all destinations' copies.
extern "C" int aigar_tile_exchange_local(aigar_handle **hs, int n) {
  if (!hs || n < 1) return fail("null argument");
  uint64_t seen = 0;
  for (int i = 0; i < n; i++) {
    if (need_tiled(hs[i])) return -1;
    if (hs[i]->d.ntiles != n || hs[i]->pass_recs != hs[0]->pass_recs || hs[i]->pass_recs == 0)
      return fail("tile_exchange_local: tiles are not at the same pass");
    const uint64_t bit = 1ull << hs[i]->d.tile_id;
    if (seen & bit) return fail("tile_exchange_local: tile %d appears twice", hs[i]->d.tile_id);
    seen |= bit;
    HIPCHK(hipSetDevice(hs[i]->cfg.device));
    if (!hs[i]->ev_x) HIPCHK(hipEventCreateWithFlags(&hs[i]->ev_x, hipEventDisableTiming));
    HIPCHK(hipEventRecord(hs[i]->ev_x, hs[i]->stream));  // outbox written
  }
  const size_t bytes = (size_t)hs[0]->pass_recs * sizeof(TileRec);
  for (int i = 0; i < n; i++) {
    HIPCHK(hipSetDevice(hs[i]->cfg.device));
    for (int k = 0; k < n; k++)
      if (k != i) HIPCHK(hipStreamWaitEvent(hs[i]->stream, hs[k]->ev_x, 0));
  }
  for (int i = 0; i < n; i++) {
    HIPCHK(hipSetDevice(hs[i]->cfg.device));
    for (int k = 0; k < n; k++) {
      const aigar_handle *src = hs[k];
      HIPCHK(hipMemcpyAsync((char *)hs[i]->d.inbox + (size_t)src->d.tile_id * bytes, src->d.outbox, bytes,
                            hipMemcpyDeviceToDevice, hs[i]->stream));
    }
  }
  for (int i = 0; i < n; i++) {  // inbox i filled (re-recorded: the outbox events are waited on already)
    HIPCHK(hipSetDevice(hs[i]->cfg.device));
    HIPCHK(hipEventRecord(hs[i]->ev_x, hs[i]->stream));
  }
  for (int k = 0; k < n; k++) {
    HIPCHK(hipSetDevice(hs[k]->cfg.device));
    for (int i = 0; i < n; i++)
      if (i != k) HIPCHK(hipStreamWaitEvent(hs[k]->stream, hs[i]->ev_x, 0));
  }
  return 0;
}

// ---------------------------------------------------------------- C4 over RCCL
// The exchange is ncclAllGather over the tiles' communicator (xGMI between the
// GPUs of a node).  librccl.so is bound at run time (dlopen of the file the
// caller names -- torch's, so one HIP runtime serves both -- and dlsym of the
// five entry points used); the library itself does not link RCCL.

extern "C" int aigar_rccl_unique_id(const char *path, void *id) {
  if (!id) return fail("null argument");
  if (rccl_load(path)) return -1;
  RcclId u;
  const int r = g_rccl.get_unique_id(&u);
  if (r) return fail("ncclGetUniqueId: %s", g_rccl.error_string(r));
  memcpy(id, &u, sizeof u);
  return 0;
}

extern "C" int aigar_tile_comm_init(aigar_handle *h, const char *path, const void *id, int nranks, int rank) {
  if (need_tiled(h)) return -1;
  if (!id) return fail("null argument");
  if (nranks != h->d.ntiles || rank != h->d.tile_id)
    return fail("tile_comm_init: %d ranks / rank %d for %d tiles / tile %d (one rank per tile, rank = tile id)",
                nranks, rank, h->d.ntiles, h->d.tile_id);
  if (rccl_load(path)) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->rccl_comm) {
    (void)g_rccl.comm_destroy(h->rccl_comm);
    h->rccl_comm = nullptr;
  }
  RcclId u;
  memcpy(&u, id, sizeof u);
  const int r = g_rccl.comm_init_rank(&h->rccl_comm, nranks, u, rank);
  if (r) {
    h->rccl_comm = nullptr;
    return fail("ncclCommInitRank(%d ranks, rank %d): %s", nranks, rank, g_rccl.error_string(r));
  }
  h->rccl_ranks = nranks;
  return 0;
}

// every tile's current-pass message into every tile's inbox (tile k at k * bytes)
static int tile_allgather(aigar_handle *h, hipStream_t s, int recs) {
  if (h->loopback) {  // (aigar_tile_loopback: the other slots hold empty messages)
    const size_t bytes = (size_t)recs * sizeof(TileRec);
    HIPCHK(hipMemcpyAsync((char *)h->d.inbox + (size_t)h->d.tile_id * bytes, h->d.outbox, bytes,
                          hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const int r = g_rccl.all_gather(h->d.outbox, (void *)h->d.inbox, (size_t)recs * sizeof(TileRec), kNcclUint8,
                                  h->rccl_comm, s);
  if (r) {
    h->rccl_bad = true;
    return fail("ncclAllGather: %s", g_rccl.error_string(r));
  }
  return 0;
}

// One tiled step (the rank-side sequence of include/aigar.h's aigar_tile_* calls)
static int issue_tile_step(aigar_handle *h, hipStream_t s, const aigar_run_params &p, int extra, void *obs,
                           int dtype) {
  const RandomPolicy rp{p.policy == AIGAR_POLICY_RANDOM, p.p_split, p.p_eject, p.seed};
  const int first_recs = 1 + h->d.tcap + h->d.hcap * h->d.hrec, later_recs = 1 + h->d.tcap + h->d.bm_words / 4;
  if (p.policy == AIGAR_POLICY_GREEDY) {  // each tile moves the bots it observes; the commands go round first
    Mark m(h, "policy");
    launch_tile_policy(h->d, s, p.greedy_split ? 1 : 0, h->d_mask, h->box_recs - 1);
    if (tile_allgather(h, s, h->box_recs)) return -1;
    launch_tile_cmd_apply(h->d, s, h->box_recs);
  }
  {
    Mark m(h, "tile_begin");
    launch_tick_pre(h->d, s, h->scr_k, h->scr_v, &rp);
    launch_tile_pass(h->d, s, food_rounds(h), h->scr_k, h->scr_v, 1);
  }
  for (int k = 0; k <= extra; k++) {
    {
      Mark m(h, "exchange");
      if (tile_allgather(h, s, k == 0 ? first_recs : later_recs)) return -1;
    }
    {
      Mark m(h, "tile_apply");
      launch_tile_apply(h->d, s, k == 0 ? first_recs : later_recs, k == 0 ? 1 : 0);
    }
    if (k < extra) {
      Mark m(h, "tile_resume");
      launch_tile_pass(h->d, s, food_rounds(h), h->scr_k, h->scr_v, 0);
    }
  }
  {
    Mark m(h, "tile_end");
    launch_tick_post(h->d, s, h->scr_k, h->scr_v);
  }
  if (obs) {
    Mark m(h, "observe");
    launch_observe(h->d, s, obs, dtype, 0);
  }
  return 0;
}

extern "C" int aigar_tile_run(aigar_handle *h, int n_steps, const aigar_run_params *p, int extra_passes,
                              void *obs_out, int dtype) {
  if (need_tiled(h) || !p) return p ? -1 : fail("null argument");
  if (!h->rccl_comm && !h->loopback) return fail("tile_run: no RCCL communicator (aigar_tile_comm_init)");
  if (n_steps < 0 || extra_passes < 0 || extra_passes > 64) return fail("tile_run: bad n_steps / extra_passes");
  if (p->policy < AIGAR_POLICY_NONE || p->policy > AIGAR_POLICY_GREEDY) return fail("tile_run: unknown policy %d", p->policy);
  if (p->policy == AIGAR_POLICY_GREEDY) note_greedy(h);  // (food_rounds)
  if (obs_out && dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (h->d.flags & AIGAR_FLAG_EVENTS)  // the event log restarts every call (all n_steps accumulate)
    hipLaunchKernelGGL(k_step_begin, dim3(1), dim3(64), 0, h->stream, h->d);
  h->pass_recs = 0;  // (the aigar_tile_* call sequence restarts at a tile_begin)
  h->cmd_pending = false;
  RunKey k;
  key_clear(k);
  key_put(k.p, *p);
  k.out = obs_out;
  k.dtype = obs_out ? dtype : -1;
  k.extra = extra_passes;
  if (h->use_graph && !h->profile && !h->tr_failed && n_steps > 0 && !h->tr.holds(k)) {
    h->rccl_bad = false;
    h->tr.ensure(h, k, [&](hipStream_t cs) { (void)issue_tile_step(h, cs, *p, extra_passes, obs_out, dtype); });
    if (h->rccl_bad) h->tr.drop(h);  // an all-gather refused the capture: direct launches from now on
    if (!h->tr.exec) h->tr_failed = true;
  }
  for (int t = 0; t < n_steps; t++) {
    if (h->tr.exec && !h->profile) {
      Mark m(h, "tile_step");
      HIPCHK(h->tr.launch(h));
    } else if (issue_tile_step(h, h->stream, *p, extra_passes, obs_out, dtype)) {
      return -1;
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_tile_run_graphed(aigar_handle *h) { return h && h->tr.exec ? 1 : 0; }

extern "C" int aigar_tile_loopback(aigar_handle *h) {
  if (need_tiled(h)) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  // every slot an empty message (kind TR_HDR, no records, nothing undone, no kills)
  HIPCHK(hipMemsetAsync((void *)h->d.inbox, 0, (size_t)h->box_recs * h->d.ntiles * sizeof(TileRec), h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->loopback = true;
  h->tr.drop(h);
  h->tr_failed = false;
  return 0;
}

// the tile that computed each bot's row at the last observation (-1: dead /
// not observed); every tile computes the same assignment
extern "C" int aigar_tile_observers(aigar_handle *h, int32_t *out) {
  if (need_tiled(h) || !out) return out ? -1 : fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpyAsync(out, h->d.t_obsby, sizeof(int32_t) * h->d.NP, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return check_device_errors(h);
}

// One learner decision for every player (bot.py:166-233 batched, the loop of
// aigar.py:performModelSteps): the action through set_command_point, held for
// skip + 1 ticks with split/eject dropped on the skipped ones, the rewards of
// the window summed, then every bot's observation -- one graph replay.
// Mixed populations (aigar_set_roles): per tick, the NN bots' held action, then
// the Greedy and Random bots' moves (Model.takeBotActions, model.py:113-115; the
// moves are independent of each other), then Field.update; the observation is
// computed for the NN bots only.
// The decision's append (replay.inc): the NN players that had an old state emit
// (old state, action, window reward, new row, dead) into the ring in ascending player
// order, then the new rows are latched -- two launches at the end of the graph.
static void launch_exp_append(aigar_handle *h, hipStream_t s, const double *act, int n_act, const double *reward,
                              const void *obs, const double *extra) {
  const Exp &e = h->exp;
  const int NP = h->d.NP;
  hipLaunchKernelGGL(k_exp_plan, dim3(1), dim3(kExpPlanThreads), 0, s, e, 0, h->d.p_role, (const uint8_t *)nullptr, NP,
                     e.off);
  if (e.dtype == 0)
    hipLaunchKernelGGL(k_exp_rows<uint64_t>, dim3(NP), dim3(256), 0, s, e, e.off, e.old, e.stride, (const char *)obs, act,
                       n_act, reward, (const uint8_t *)nullptr, h->d.p_role, 1, extra);
  else
    hipLaunchKernelGGL(k_exp_rows<uint32_t>, dim3(NP), dim3(256), 0, s, e, e.off, e.old, e.stride, (const char *)obs, act,
                       n_act, reward, (const uint8_t *)nullptr, h->d.p_role, 1, extra);
}
static void launch_exp_latch(aigar_handle *h, hipStream_t s, const void *obs, int dtype, const uint8_t *mask) {
  hipLaunchKernelGGL(k_exp_latch, dim3(h->d.NP), dim3(256), 0, s, h->exp, obs, dtype, mask);
}

static void launch_env_decision(aigar_handle *h, hipStream_t s, const EnvKey &k) {
  for (int t = 0; t <= k.skip; t++) {
    if (t > 0) launch_rewards(h->d, s, k.reward, k.prm, 0, t == 1 ? 1 : 2);  // updateRewards (bot.py:166-168)
    launch_apply_actions(h->d, s, k.act, k.n_act, k.enable_split, t > 0, t == 0);
    if (k.n_greedy) launch_policy_greedy(h->d, s, k.envp.greedy_split, h->d.p_role, AIGAR_ROLE_GREEDY);
    if (k.n_random)
      launch_policy_refrandom(h->d, s, k.envp.random_skip, k.envp.random_split, k.envp.random_eject, k.envp.salt);
    launch_tick(h->d, s, food_rounds(h), h->scr_k, h->scr_v);
  }
  launch_rewards(h->d, s, k.reward, k.prm, 1, k.skip == 0 ? 1 : 2);  // end of move_NN (bot.py:220-230)
  const uint8_t *nn = (k.n_greedy || k.n_random) ? h->d_nnmask : nullptr;
  if (k.pix.side)
    (void)launch_observe_pixel_state(h->d, s, k.obs, k.dtype, k.pix.side, k.pix.flags, k.pix.color_seed, h->d_pix_ovf,
                                     nn, k.pix_hist);
  else launch_observe(h->d, s, k.obs, k.dtype, 0, nn);
  if (k.exp) launch_exp_append(h, s, k.exp_act, k.exp_n_act, k.reward, k.obs, k.exp_extra);
}

// The decision of aigar_env_step / aigar_env_step_q / aigar_env_step_ac: the key's common
// part, then the replay of its graph (k.q: the selection's kernel in front, decide.inc;
// k.mu: the noise's, noise.inc).
static int env_step_keyed(aigar_handle *h, EnvKey &k, int enable_split, int skip,
                          const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype,
                          int n_decisions = 1) {
  if (skip < 0) return fail("env_step: skip < 0");
  if (dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  HIPCHK(hipSetDevice(h->cfg.device));
  k.enable_split = enable_split ? 1 : 0;
  k.skip = skip;
  k.dtype = dtype;
  key_put(k.prm, *p);
  k.reward = reward_out;
  k.obs = obs_out;
  key_put(k.envp, h->envp);
  k.n_greedy = h->n_greedy;
  k.n_random = h->n_random;
  key_put(k.pix, h->pix);
  k.pix_hist = h->d_pix_hist;
  k.exp = h->exp.cap ? h->exp.ctl : nullptr;
  if (!k.q && !k.mu) {  // (the selection stores the index, [NP][1]; the noise its noisy rows)
    k.exp_act = k.act;
    k.exp_n_act = k.n_act;
  }
  if (h->exp.cap && dtype != h->exp.dtype)
    return fail("env_step: dtype %d differs from the replay memory's state_dtype %d (aigar_exp_config)", dtype,
                h->exp.dtype);
  if (k.pix.side && ((uintptr_t)obs_out & 15)) return fail("env_step: the pixel state's obs_out must be 16-byte aligned");
  if (h->d.flags & AIGAR_FLAG_EVENTS)  // the event log holds the window's ticks
    hipLaunchKernelGGL(k_step_begin, dim3((h->d.A + 63) / 64), dim3(64), 0, h->stream, h->d);
  auto launch = [&](hipStream_t cs) {
    if (k.conv.n_conv) {  // the conv layers on the pixel state, the dense layers on their float32 feature rows
      launch_conv(cs, k.conv, k.obs, k.dtype, h->d.NP, h->d.p_alive, h->d.p_role);
      Net dense = k.net;
      dense.x_dtype = 1;
      launch_net(cs, dense, k.conv.act[k.conv.n_conv - 1], h->d.NP, k.net.y, h->d.p_alive, h->d.p_role);
    } else if (k.net.n_layers) {
      launch_net(cs, k.net, k.obs, h->d.NP, k.net.y, h->d.p_alive, h->d.p_role);
    }
    if (k.q) launch_decide(h->d, cs, k.dec, k.q, k.explore, k.u, k.idx_out, k.val_out, k.dec.act);
    if (k.mu)
      launch_noise(h->d, cs, k.noi, k.mu, h->d.NP, 1, k.nstd, k.nu, k.nT, nullptr, k.noisy, nullptr);
    launch_env_decision(h, cs, k);
  };
  if (!h->use_graph) {
    for (int i = 0; i < n_decisions; i++) launch(h->stream);
  } else {
    if (!h->env.ensure(h, k, launch)) return fail("env_step: graph capture failed");
    Mark m(h, "env_step");
    for (int i = 0; i < n_decisions; i++) HIPCHK(h->env.launch(h));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_env_step(aigar_handle *h, const double *act, int n_act, int enable_split, int skip,
                              const aigar_reward_params *p, double *reward_out, void *obs_out, int dtype) {
  if (!h || !act || !p || !reward_out || !obs_out) return fail("null argument");
  if (n_act < 2 || n_act > 4) return fail("env_step: n_act must be 2, 3 or 4");
  EnvKey k;
  key_clear(k);
  k.act = act;
  k.n_act = n_act;
  return env_step_keyed(h, k, enable_split, skip, p, reward_out, obs_out, dtype);
}

// ------------------------------------------------------------ action selection
// A feature's entry points need the feature (on: its "configured?" flag, read once the handle is known)
static int need(aigar_handle *h, bool on, const char *who, const char *what) {
  if (!h) return fail("null handle");
  return on ? 0 : fail("%s: %s", who, what);
}
// Every *_config begins here: nothing that reads the feature's buffers is pending,
// and the decision graph goes.  Its key holds the buffers by pointer, and a freed
// buffer can come back at the same address: the key alone would not notice.
static int begin_reconfig(aigar_handle *h) {
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->env.drop(h);
  return 0;
}
// The train configuration, whichever it is, goes with the network, the memory or the critic it
// was made for (after begin_reconfig: no training step is pending).
static void trainer_free(aigar_handle *h) {
  h->train.drop(h);
  h->trn_mem.release();
  h->trn = Train{};
  h->ctrn = ConvTrain{};
  h->act = ACTrain{};
  h->dpg = DPGTrain{};
  h->spg = SPGTrain{};
}
static void critic_free(aigar_handle *h) {
  if (!h->trn.batch) trainer_free(h);  // (Q-learning trains without the critic: it stays)
  h->crit_q = false;
  h->crit_mem.release();
  h->crit = Net{};
  h->crit_stage = nullptr;
}
static int need_dec(aigar_handle *h, const char *who) {
  return need(h, h && h->dec.n_out, who, "no action selection is configured (aigar_decide_config)");
}

extern "C" int aigar_decide_config(aigar_handle *h, const aigar_decide_params *p, const double *actions) {
  if (!h) return fail("null handle");
  if (p) {
    if (h->d.tiled) return fail("decide_config: a tiled handle has no action selection");
    if (!actions) return fail("decide_config: null action table");
    if (p->n_out < 1 || p->n_out > 1024) return fail("decide_config: n_out = %d is outside 1..1024", p->n_out);
    if (p->strategy != 0 && p->strategy != 1) return fail("decide_config: strategy must be 0 (e-Greedy) or 1 (Boltzmann)");
    if (p->q_dtype != 0 && p->q_dtype != 1) return fail("decide_config: q_dtype must be 0 (float64) or 1 (float32)");
  }
  if (begin_reconfig(h)) return -1;
  h->dec_mem.release();
  h->dec = Decide{};
  if (!p) return 0;
  Decide c{};
  c.n_out = p->n_out;
  c.strategy = p->strategy;
  c.q_dtype = p->q_dtype;
  c.seed = p->seed;
  const size_t NP = (size_t)h->d.NP, nt = (size_t)c.n_out * 4;
  c.table = (double *)h->dec_mem.alloc(nt * sizeof(double), false, h->stream);
  c.act = (double *)h->dec_mem.alloc(NP * 4 * sizeof(double), true, h->stream);
  c.idx = (double *)h->dec_mem.alloc(NP * sizeof(double), false, h->stream);
  if (!c.table || !c.act || !c.idx) {
    h->dec_mem.release();
    return fail("decide_config: out of device memory");
  }
  HIPCHK(hipMemcpyAsync(c.table, actions, nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_fill_d, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, h->stream, c.idx, NP, -1.0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's table is read)
  h->dec = c;
  return 0;
}

extern "C" int aigar_decide(aigar_handle *h, const void *q, const double *explore, const double *u, int32_t *idx_out,
                            double *val_out, double *act_out) {
  if (need_dec(h, "decide")) return -1;
  if (!q || !explore || !idx_out || !val_out) return fail("decide: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_decide(h->d, h->stream, h->dec, q, explore, u, idx_out, val_out, act_out);
  HIPCHK(hipGetLastError());
  return 0;
}

// The decision key's "selection in front" half: q is the caller's values or the network's output
static void key_select(EnvKey &k, const aigar_handle *h, const void *q, const double *explore, const double *u,
                       int32_t *idx_out, double *val_out) {
  k.act = h->dec.act;
  k.n_act = 4;
  k.q = q;
  k.explore = explore;
  k.u = u;
  k.idx_out = idx_out;
  k.val_out = val_out;
  key_put(k.dec, h->dec);
  k.exp_act = h->dec.idx;
  k.exp_n_act = 1;
}

extern "C" int aigar_env_step_q(aigar_handle *h, const void *q, const double *explore, const double *u,
                                int enable_split, int skip, const aigar_reward_params *p, double *reward_out,
                                void *obs_out, int dtype, int32_t *idx_out, double *val_out) {
  if (need_dec(h, "env_step_q")) return -1;
  if (!q || !explore || !p || !reward_out || !obs_out || !idx_out || !val_out) return fail("env_step_q: null argument");
  EnvKey k;
  key_clear(k);
  key_select(k, h, q, explore, u, idx_out, val_out);
  return env_step_keyed(h, k, enable_split, skip, p, reward_out, obs_out, dtype);
}

// ------------------------------------------------------------ exploration noise
static int need_noi(aigar_handle *h, const char *who) {
  return need(h, h && h->noi.n_act, who, "no exploration noise is configured (aigar_noise_config)");
}

extern "C" int aigar_noise_config(aigar_handle *h, const aigar_noise_params *p) {
  if (!h) return fail("null handle");
  if (p) {
    if (h->d.tiled) return fail("noise_config: a tiled handle has no exploration noise");
    if (p->n_act < 2 || p->n_act > 4) return fail("noise_config: n_act = %d is outside 2..4", p->n_act);
    if (p->type != AIGAR_NOISE_GAUSSIAN && p->type != AIGAR_NOISE_ORN_UHL)
      return fail("noise_config: type must be 0 (Gaussian) or 1 (Orn-Uhl)");
    if (p->mu_dtype != 0 && p->mu_dtype != 1) return fail("noise_config: mu_dtype must be 0 (float64) or 1 (float32)");
    if (p->type == AIGAR_NOISE_ORN_UHL &&
        !(std::isfinite(p->theta) && std::isfinite(p->ou_mu) && p->dt >= 0 && std::isfinite(p->dt)))
      return fail("noise_config: Orn-Uhl needs finite theta and ou_mu and a finite dt >= 0 (got %g, %g, %g)", p->theta,
                  p->ou_mu, p->dt);
  }
  if (begin_reconfig(h)) return -1;
  h->noi_mem.release();
  h->noi = Noise{};
  if (!p) return 0;
  Noise c{};
  c.n_act = p->n_act;
  c.type = p->type;
  c.mu_dtype = p->mu_dtype;
  c.store_raw = p->store_raw ? 1 : 0;
  c.theta = p->theta;
  c.ou_mu = p->ou_mu;
  c.dt = p->type == AIGAR_NOISE_ORN_UHL ? p->dt : 0.0;
  c.seed = p->seed;
  const size_t bytes = (size_t)h->d.NP * 4 * sizeof(double);
  c.act = (double *)h->noi_mem.alloc(bytes, true, h->stream);
  c.raw = (double *)h->noi_mem.alloc(bytes, true, h->stream);
  c.ou = (double *)h->noi_mem.alloc(bytes, true, h->stream);
  if (!c.act || !c.raw || !c.ou) {
    h->noi_mem.release();
    return fail("noise_config: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->noi = c;
  return 0;
}

extern "C" int aigar_noise(aigar_handle *h, const void *mu, int rows, const double *std, const double *u, int T,
                           double *prev, double *noisy_out, uint64_t *n_exhausted) {
  if (need_noi(h, "noise")) return -1;
  if (rows < 0) return fail("noise: rows = %d is negative", rows);
  if (rows > (1 << 30)) return fail("noise: rows = %d above 2^30", rows);
  if (rows == 0) return 0;
  if (!mu || !std || !noisy_out) return fail("noise: null argument");
  if (u && (T < 1 || T > kNoiseMaxT)) return fail("noise: T = %d is outside 1..%d", T, kNoiseMaxT);
  if (h->noi.type == AIGAR_NOISE_ORN_UHL && !prev) return fail("noise: an Orn-Uhl config needs the caller's state (prev)");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_noise(h->d, h->stream, h->noi, mu, rows, 0, std, u, u ? T : kNoiseOwnT, prev, noisy_out,
               (unsigned long long *)n_exhausted);
  HIPCHK(hipGetLastError());
  return 0;
}

// The decision key's "noise in front" half: mu is the caller's actions or the network's output
static void key_noise(EnvKey &k, const aigar_handle *h, const void *mu, const double *std, const double *u, int T,
                      double *noisy_out) {
  k.act = h->noi.act;
  k.n_act = h->noi.n_act;
  k.mu = mu;
  k.nstd = std;
  k.nu = u;
  k.nT = u ? T : kNoiseOwnT;
  k.noisy = noisy_out;
  key_put(k.noi, h->noi);
  k.exp_act = h->noi.act;
  k.exp_n_act = h->noi.n_act;
  k.exp_extra = h->noi.store_raw ? h->noi.raw : nullptr;
}

extern "C" int aigar_env_step_ac(aigar_handle *h, const void *mu, const double *std, const double *u, int T,
                                 int enable_split, int skip, const aigar_reward_params *p, double *reward_out,
                                 void *obs_out, int dtype, double *noisy_out) {
  if (need_noi(h, "env_step_ac")) return -1;
  if (!mu || !std || !p || !reward_out || !obs_out) return fail("env_step_ac: null argument");
  if (u && (T < 1 || T > kNoiseMaxT)) return fail("env_step_ac: T = %d is outside 1..%d", T, kNoiseMaxT);
  EnvKey k;
  key_clear(k);
  key_noise(k, h, mu, std, u, T, noisy_out);
  return env_step_keyed(h, k, enable_split, skip, p, reward_out, obs_out, dtype);
}

// ------------------------------------------------------------ acting network
static int pix_channels(const aigar_pixel_params &p);
static void net_free(aigar_handle *h) {
  h->net_mem.release();
  h->net = Net{};
  h->net_stage = nullptr;
  h->conv = Conv{};
  h->conv_stage = nullptr;
}
static int need_net(aigar_handle *h, const char *who) {
  return need(h, h && h->net.n_layers, who, "no acting network is configured (aigar_net_config)");
}
static const char *net_act_name(int a) {
  switch (a) {
    case AIGAR_ACT_LINEAR: return "linear";
    case AIGAR_ACT_RELU: return "relu";
    case AIGAR_ACT_SIGMOID: return "sigmoid";
    case AIGAR_ACT_ELU: return "elu";
    case AIGAR_ACT_TANH: return "tanh";
  }
  return "unknown";
}

// A dense network's shape, as the acting network and the critic take it: every check up to the head's.
static int net_shape_check(const char *who, const aigar_net_params *p) {
  if (p->n_layers < 1 || p->n_layers > kNetMaxLayers)
    return fail("%s: n_layers = %d is outside 1..%d", who, p->n_layers, kNetMaxLayers);
  if (p->n_in < 1 || p->n_in > kNetMaxIn) return fail("%s: n_in = %d is outside 1..%d", who, p->n_in, kNetMaxIn);
  for (int l = 0; l < p->n_layers; l++)
    if (p->units[l] < 1 || p->units[l] > kNetMaxUnits)
      return fail("%s: layer %d has %d units, outside 1..%d", who, l, p->units[l], kNetMaxUnits);
  if (p->x_dtype != 0 && p->x_dtype != 1) return fail("%s: x_dtype must be 0 (float64) or 1 (float32)", who);
  if (p->hidden_act != AIGAR_ACT_RELU && p->hidden_act != AIGAR_ACT_LINEAR)
    return fail("%s: hidden activation %d (%s) is not supported: relu or linear", who, p->hidden_act,
                net_act_name(p->hidden_act));
  return 0;
}

extern "C" int aigar_net_config(aigar_handle *h, const aigar_net_params *p) {
  if (p) {  // (before the handle: a bad set has its own message)
    if (net_shape_check("net_config", p)) return -1;
    if (p->out_act != AIGAR_ACT_LINEAR && p->out_act != AIGAR_ACT_SIGMOID)
      return fail("net_config: output activation %d (%s) is not supported: linear or sigmoid", p->out_act,
                  net_act_name(p->out_act));
  }
  if (!h) return fail("null handle");
  if (p && h->d.tiled) return fail("net_config: a tiled handle has no acting network");
  if (begin_reconfig(h)) return -1;
  trainer_free(h);
  critic_free(h);
  net_free(h);
  if (!p) return 0;
  Net c{};
  c.n_layers = p->n_layers;
  c.x_dtype = p->x_dtype;
  c.hid_act = p->hidden_act;
  c.out_act = p->out_act;
  size_t stage = 0;
  auto alloc = [&](size_t bytes) { return h->net_mem.alloc(bytes, true, h->stream); };
  bool ok = true;
  for (int l = 0; l < c.n_layers && ok; l++) {
    c.in[l] = l ? p->units[l - 1] : p->n_in;
    c.out[l] = p->units[l];
    const size_t ip = net_in_pad(c.in[l]), op = net_out_pad(c.out[l]);
    c.w[l] = (float *)alloc(ip * op * sizeof(float));
    c.b[l] = (float *)alloc(op * sizeof(float));
    ok = c.w[l] && c.b[l];
    stage = std::max(stage, (size_t)c.in[l] * c.out[l] + c.out[l]);
  }
  if (ok) ok = (c.y = (double *)alloc((size_t)h->d.NP * c.out[c.n_layers - 1] * sizeof(double))) != nullptr;
  if (ok) ok = (h->net_stage = (float *)alloc(stage * sizeof(float))) != nullptr;
  if (!ok) {
    net_free(h);
    return fail("net_config: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->net = c;
  return 0;
}

// aigar_net_set_weights, aigar_critic_set_weights: layer `layer` of the dense network c from Keras'
// layout, through c's staging when the caller's arrays are the host's
static int set_dense_weights(aigar_handle *h, const char *who, const Net &c, float *stage, int layer, const float *W,
                             const float *b, int on_device) {
  if (layer < 0 || layer >= c.n_layers) return fail("%s: layer %d is outside 0..%d", who, layer, c.n_layers - 1);
  if (!W || !b) return fail("%s: null argument", who);
  HIPCHK(hipSetDevice(h->cfg.device));
  const int in = c.in[layer], out = c.out[layer];
  const size_t nw = (size_t)in * out;
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(stage, W, nw * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(stage + nw, b, (size_t)out * sizeof(float), hipMemcpyHostToDevice, h->stream));
    W = stage;
    b = stage + nw;
  }
  const int ip = net_in_pad(in), op = net_out_pad(out);
  const size_t n = (size_t)ip * op;
  hipLaunchKernelGGL(k_net_pack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, W, b,
                     c.w[layer], c.b[layer], in, out, ip, op);
  HIPCHK(hipGetLastError());
  if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's arrays are read, the staging is free)
  return 0;
}
extern "C" int aigar_net_set_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device) {
  if (need_net(h, "net_set_weights")) return -1;
  return set_dense_weights(h, "net_set_weights", h->net, h->net_stage, layer, W, b, on_device);
}

extern "C" int aigar_net_forward(aigar_handle *h, const void *x, int x_dtype, int rows, double *out) {
  if (need_net(h, "net_forward")) return -1;
  if (!x || !out) return fail("net_forward: null argument");
  if (x_dtype != 0 && x_dtype != 1) return fail("net_forward: x_dtype must be 0 (float64) or 1 (float32)");
  if (rows < 1 || rows > (1 << 30)) return fail("net_forward: rows = %d is outside 1..2^30", rows);
  HIPCHK(hipSetDevice(h->cfg.device));
  Net c = h->net;
  c.x_dtype = x_dtype;
  if (h->conv.n_conv) {  // in slabs of the activation buffers' rows, one after the other on the stream
    const Conv &cv = h->conv;
    const size_t img = (size_t)cv.side * cv.side * cv.channels * (x_dtype == 0 ? 8 : 4);
    const int n_out = c.out[c.n_layers - 1];
    c.x_dtype = 1;
    for (int r0 = 0; r0 < rows; r0 += cv.cap) {
      const int n = std::min(cv.cap, rows - r0);
      launch_conv(h->stream, cv, (const char *)x + (size_t)r0 * img, x_dtype, n, nullptr, nullptr);
      launch_net(h->stream, c, cv.act[cv.n_conv - 1], n, out + (size_t)r0 * n_out, nullptr, nullptr);
    }
  } else {
    launch_net(h->stream, c, x, rows, out, nullptr, nullptr);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The conv part: the parameter checks (before the handle, each with its own message), the
// dense part through aigar_net_config, then the conv part's own buffers.
extern "C" int aigar_net_config_cnn(aigar_handle *h, const aigar_conv_params *cp, const aigar_net_params *p) {
  if (!cp || !p) return fail("net_config_cnn: null argument");
  if (cp->side < 1 || cp->side > kConvMaxSide)
    return fail("net_config_cnn: side = %d is outside 1..%d", cp->side, kConvMaxSide);
  if (cp->channels < 1 || cp->channels > kConvMaxCh)
    return fail("net_config_cnn: channels = %d is outside 1..%d", cp->channels, kConvMaxCh);
  if (cp->n_conv < 1 || cp->n_conv > kConvMax)
    return fail("net_config_cnn: n_conv = %d is outside 1..%d", cp->n_conv, kConvMax);
  Conv c{};
  c.n_conv = cp->n_conv;
  c.side = cp->side;
  c.channels = cp->channels;
  int in = cp->side;
  for (int l = 0; l < cp->n_conv; l++) {
    if (cp->k[l] < 1 || cp->k[l] > kConvMaxK)
      return fail("net_config_cnn: conv layer %d has kernel k = %d, outside 1..%d", l, cp->k[l], kConvMaxK);
    if (cp->stride[l] < 1 || cp->stride[l] > kConvMaxK)
      return fail("net_config_cnn: conv layer %d has stride = %d, outside 1..%d", l, cp->stride[l], kConvMaxK);
    if (cp->filters[l] < 1 || cp->filters[l] > kConvMaxF)
      return fail("net_config_cnn: conv layer %d has filters = %d, outside 1..%d", l, cp->filters[l], kConvMaxF);
    if (in < cp->k[l])
      return fail("net_config_cnn: conv layer %d has no output: its input side %d is below its kernel %d", l, in,
                  cp->k[l]);
    c.k[l] = cp->k[l];
    c.stride[l] = cp->stride[l];
    c.filters[l] = cp->filters[l];
    c.osz[l] = in = (in - cp->k[l]) / cp->stride[l] + 1;
  }
  const long long flat = (long long)in * in * c.filters[c.n_conv - 1];
  if (flat > kNetMaxIn)
    return fail("net_config_cnn: the flattened length %lld (%d x %d x %d) is above %d", flat, in, in,
                c.filters[c.n_conv - 1], kNetMaxIn);
  c.n_flat = (int)flat;
  if (p->n_in != c.n_flat)
    return fail("net_config_cnn: the dense part's n_in = %d differs from the flattened length %d", p->n_in, c.n_flat);
  if (aigar_net_config(h, p)) return -1;  // (its own checks; drops the graph and any earlier conv part)
  c.cap = std::max(h->d.NP, kConvMinRows);
  size_t stage = 0;
  auto alloc = [&](size_t bytes) { return h->net_mem.alloc(bytes, true, h->stream); };
  bool ok = true;
  for (int l = 0; l < c.n_conv && ok; l++) {
    const size_t K = (size_t)c.k[l] * c.k[l] * (l ? c.filters[l - 1] : c.channels), F = c.filters[l];
    const size_t Fp = net_out_pad((int)F);
    c.w[l] = (float *)alloc(conv_k_pad((int)K) * Fp * sizeof(float));
    c.b[l] = (float *)alloc(Fp * sizeof(float));
    c.act[l] = (float *)alloc((size_t)c.cap * c.osz[l] * c.osz[l] * F * sizeof(float));
    ok = c.w[l] && c.b[l] && c.act[l];
    stage = std::max(stage, K * F + F);
  }
  if (ok) ok = (h->conv_stage = (float *)alloc(stage * sizeof(float))) != nullptr;
  if (!ok) {
    net_free(h);
    return fail("net_config_cnn: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->conv = c;
  return 0;
}

extern "C" int aigar_net_set_conv_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device) {
  if (need_net(h, "net_set_conv_weights")) return -1;
  const Conv &c = h->conv;
  if (!c.n_conv) return fail("net_set_conv_weights: the network has no conv part (aigar_net_config_cnn)");
  if (layer < 0 || layer >= c.n_conv)
    return fail("net_set_conv_weights: layer %d is outside 0..%d", layer, c.n_conv - 1);
  if (!W || !b) return fail("net_set_conv_weights: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int K = c.k[layer] * c.k[layer] * (layer ? c.filters[layer - 1] : c.channels), F = c.filters[layer];
  const size_t nw = (size_t)K * F;
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(h->conv_stage, W, nw * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->conv_stage + nw, b, (size_t)F * sizeof(float), hipMemcpyHostToDevice, h->stream));
    W = h->conv_stage;
    b = h->conv_stage + nw;
  }
  const int Kp = conv_k_pad(K), Fp = net_out_pad(F);
  const size_t n = (size_t)Kp * Fp;
  hipLaunchKernelGGL(k_conv_pack, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, h->stream, W, b,
                     c.w[layer], c.b[layer], K, F, Kp, Fp);
  HIPCHK(hipGetLastError());
  if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's arrays are read, the staging is free)
  return 0;
}

extern "C" int aigar_net_output(aigar_handle *h, double *out) {
  if (need_net(h, "net_output")) return -1;
  if (!out) return fail("net_output: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)h->d.NP * h->net.out[h->net.n_layers - 1] * sizeof(double);
  HIPCHK(hipMemcpyAsync(out, h->net.y, bytes, hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

extern "C" int aigar_env_step_net(aigar_handle *h, int head, const double *explore, const double *u, int T,
                                  int enable_split, int skip, const aigar_reward_params *p, double *reward_out,
                                  void *obs_out, int dtype, int32_t *idx_out, double *val_out, double *noisy_out,
                                  int n_decisions) {
  if (need_net(h, "env_step_net")) return -1;
  if (head != AIGAR_NET_HEAD_Q && head != AIGAR_NET_HEAD_ACTOR)
    return fail("env_step_net: head must be 0 (Q) or 1 (actor)");
  if (!explore || !p || !reward_out || !obs_out) return fail("env_step_net: null argument");
  if (n_decisions < 1) return fail("env_step_net: n_decisions = %d is below 1", n_decisions);
  const Net &c = h->net;
  const int n_out = c.out[c.n_layers - 1];
  if (h->conv.n_conv) {
    if (!h->pix.side)
      return fail("env_step_net: the network's conv part needs a pixel state of side %d and %d channels "
                  "(aigar_pixel_config)", h->conv.side, h->conv.channels);
    if (h->pix.side != h->conv.side || pix_channels(h->pix) != h->conv.channels)
      return fail("env_step_net: the pixel state is %d x %d x %d, the network's conv part takes %d x %d x %d",
                  h->pix.side, h->pix.side, pix_channels(h->pix), h->conv.side, h->conv.side, h->conv.channels);
  } else {
    if (h->pix.side) return fail("env_step_net: the acting network takes no pixel state");
    if (c.in[0] != h->d.L)
      return fail("env_step_net: the network has %d inputs, the state %d values", c.in[0], h->d.L);
  }
  if (dtype != c.x_dtype) return fail("env_step_net: dtype %d differs from the network's x_dtype %d", dtype, c.x_dtype);
  EnvKey k;
  key_clear(k);
  key_put(k.net, c);
  key_put(k.conv, h->conv);
  if (head == AIGAR_NET_HEAD_Q) {
    if (need_dec(h, "env_step_net")) return -1;
    if (h->dec.q_dtype != 0) return fail("env_step_net: the action selection's q_dtype must be 0 (float64)");
    if (h->dec.n_out != n_out)
      return fail("env_step_net: the network has %d outputs, the action selection %d", n_out, h->dec.n_out);
    if (!idx_out || !val_out) return fail("env_step_net: null argument");
    key_select(k, h, c.y, explore, u, idx_out, val_out);
  } else {
    if (need_noi(h, "env_step_net")) return -1;
    if (h->noi.mu_dtype != 0) return fail("env_step_net: the exploration noise's mu_dtype must be 0 (float64)");
    if (h->noi.n_act != n_out)
      return fail("env_step_net: the network has %d outputs, the exploration noise n_act = %d", n_out, h->noi.n_act);
    if (u && (T < 1 || T > kNoiseMaxT)) return fail("env_step_net: T = %d is outside 1..%d", T, kNoiseMaxT);
    key_noise(k, h, c.y, explore, u, T, noisy_out);
  }
  return env_step_keyed(h, k, enable_split, skip, p, reward_out, obs_out, dtype, n_decisions);
}

extern "C" int aigar_warnings(aigar_handle *h, int arena, uint32_t *out) {
  if (!h || !out) return fail("null argument");
  if (arena < 0 || arena >= h->d.A) return fail("arena out of range");
  HIPCHK(hipSetDevice(h->cfg.device));
  ArenaCtl c;
  HIPCHK(hipMemcpyAsync(&c, h->d.ctl + arena, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *out = c.warn;
  return 0;
}

extern "C" int aigar_set_roles(aigar_handle *h, const uint8_t *roles, int on_device) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int NP = h->d.NP;
  std::vector<uint8_t> r(NP, AIGAR_ROLE_NN);
  if (roles) {
    if (on_device) HIPCHK(hipMemcpy(r.data(), roles, NP, hipMemcpyDeviceToHost));
    else memcpy(r.data(), roles, NP);
  }
  std::vector<uint8_t> nn(NP);
  int ng = 0, nr = 0;
  for (int i = 0; i < NP; i++) {
    if (r[i] > AIGAR_ROLE_RANDOM) return fail("set_roles: role %d of player %d is not an AIGAR_ROLE_*", r[i], i);
    ng += r[i] == AIGAR_ROLE_GREEDY;
    nr += r[i] == AIGAR_ROLE_RANDOM;
    nn[i] = r[i] == AIGAR_ROLE_NN;
  }
  HIPCHK(hipMemcpyAsync(h->d.p_role, r.data(), NP, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_nnmask, nn.data(), NP, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->n_greedy = ng;
  h->n_random = nr;
  if (ng) note_greedy(h);  // (food_rounds)
  return 0;
}
extern "C" int aigar_env_config(aigar_handle *h, const aigar_env_params *p) {
  if (!h || !p) return fail("null argument");
  h->envp = *p;
  return 0;
}
extern "C" int aigar_policy_random_bots(aigar_handle *h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_policy_refrandom(h->d, h->stream, h->envp.random_skip, h->envp.random_split, h->envp.random_eject,
                          h->envp.salt);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_obs_len(aigar_handle *h) { return h ? h->d.L : -1; }

extern "C" int aigar_observe(aigar_handle *h, void *out, int dtype, int on_device) {
  return aigar_observe_masked(h, out, dtype, on_device, nullptr, 0);
}
extern "C" int aigar_observe_masked(aigar_handle *h, void *out, int dtype, int on_device, const uint8_t *mask,
                                    int mask_on_device) {
  if (!h || !out) return fail("null argument");
  if (dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  HIPCHK(hipSetDevice(h->cfg.device));
  void *dst = on_device ? out : h->d_obs;
  const uint8_t *m = mask;
  if (mask && !mask_on_device) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->d.NP, hipMemcpyHostToDevice, h->stream));
    m = h->d_mask;
  }
  if (!on_device && mask) {  // rows of masked-out bots are left as the caller's buffer has them
    size_t bytes = (size_t)h->d.NP * h->d.L * (dtype == 0 ? 8 : 4);
    HIPCHK(hipMemcpyAsync(h->d_obs, out, bytes, hipMemcpyHostToDevice, h->stream));
  }
  {
    Mark mk(h, "observe");
    launch_observe(h->d, h->stream, dst, dtype, ++h->obs_calls, m);
    // (with a pixel config the memory's states are pixel states: a grid row is none of them)
    if (h->exp.cap && !h->pix.side) launch_exp_latch(h, h->stream, dst, dtype, m);
  }
  HIPCHK(hipGetLastError());
  if (!on_device) {
    size_t bytes = (size_t)h->d.NP * h->d.L * (dtype == 0 ? 8 : 4);
    HIPCHK(hipMemcpyAsync(out, h->d_obs, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_device_errors(h);
  }
  return 0;
}

extern "C" int aigar_observe_pixels(aigar_handle *h, void *out, int side, uint64_t color_seed, int dtype,
                                    int on_device) {
  if (!h || !out) return fail("null argument");
  if (side < 1 || side > 84) return fail("pixel frame side must be in [1, 84], got %d", side);
  if (dtype < 0 || dtype > 2) return fail("dtype must be 0 (float64 gray), 1 (float32 gray) or 2 (uint8 rgb)");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)h->d.NP * side * side * (dtype == 0 ? 8 : dtype == 1 ? 4 : 3);
  if (!h->d_pix_ovf) {
    h->d_pix_ovf = dalloc<uint8_t>(h, h->d.NP);
    if (!h->d_pix_ovf) return fail("out of device memory");
  }
  void *dst = out;
  if (!on_device) {
    if (bytes > h->pix_bytes) {
      if (h->d_pix) HIPCHK(hipFree(h->d_pix));
      h->d_pix = nullptr;
      h->pix_bytes = 0;
      HIPCHK(hipMalloc(&h->d_pix, bytes));
      h->pix_bytes = bytes;
    }
    dst = h->d_pix;
  }
  {
    Mark m(h, "observe_pixels");
    if (launch_observe_pixels(h->d, h->stream, dst, dtype, side, color_seed, h->d_pix_ovf)) return fail("bad pixel launch");
  }
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(out, h->d_pix, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_device_errors(h);
  }
  return 0;
}

static int pix_channels(const aigar_pixel_params &p) {
  return ((p.flags & AIGAR_PIX_RGB) ? 3 : 1) * ((p.flags & AIGAR_PIX_LAST) ? 2 : 1);
}

extern "C" int aigar_pixel_config(aigar_handle *h, const aigar_pixel_params *p) {
  if (!h) return fail("null handle");
  if (h->exp.cap)
    return fail("pixel_config: a replay memory is set, its rows have the current state's width "
                "(free it first: aigar_exp_config(h, NULL))");
  aigar_pixel_params q{};
  if (p && p->side != 0) q = *p;
  if (q.side) {
    if (h->d.tiled) return fail("pixel_config: a tiled handle has no pixel state");
    if (q.side < 1 || q.side > 84) return fail("pixel_config: side must be in [1, 84], got %d", q.side);
    if (q.flags & ~(AIGAR_PIX_RGB | AIGAR_PIX_LAST)) return fail("pixel_config: unknown flags 0x%x", q.flags);
  }
  if (begin_reconfig(h)) return -1;  // (no reader of the history is pending either)
  if (q.side && !h->d_pix_ovf) {
    h->d_pix_ovf = dalloc<uint8_t>(h, h->d.NP);
    if (!h->d_pix_ovf) return fail("out of device memory");
  }
  const size_t had = pix_hist_bytes(h);
  h->pix = q;
  const size_t want = pix_hist_bytes(h);
  if (want != had) {
    if (h->d_pix_hist) (void)hipFree(h->d_pix_hist);
    h->d_pix_hist = nullptr;
    if (want && hipMalloc((void **)&h->d_pix_hist, want) != hipSuccess) {
      h->pix = aigar_pixel_params{};
      return fail("pixel_config: out of device memory (%zu bytes of frame history)", want);
    }
  }
  if (want) HIPCHK(hipMemsetAsync(h->d_pix_hist, 0, want, h->stream));
  return 0;
}


// ------------------------------------------------------------ replay memory
static int exp_state_len(aigar_handle *h) {
  return h->pix.side ? h->pix.side * h->pix.side * pix_channels(h->pix) : h->d.L;
}
static int need_exp(aigar_handle *h, const char *who) {
  return need(h, h && h->exp.cap, who, "no replay memory is configured (aigar_exp_config)");
}

extern "C" int aigar_exp_config(aigar_handle *h, const aigar_exp_params *p) {
  if (!h) return fail("null handle");
  const bool on = p && p->capacity != 0;
  if (on) {
    if (h->d.tiled) return fail("exp_config: a tiled handle has no replay memory");
    if (p->capacity < h->d.NP)
      return fail("exp_config: capacity %lld is below the handle's %d players (one decision's transitions)",
                  (long long)p->capacity, h->d.NP);
    if (p->capacity > ((int64_t)1 << 30)) return fail("exp_config: capacity %lld above 2^30", (long long)p->capacity);
    if (p->state_dtype != 0 && p->state_dtype != 1) return fail("exp_config: state_dtype must be 0 (float64) or 1 (float32)");
    if (p->flags & ~(AIGAR_EXP_PRIORITIZED | AIGAR_EXP_EXTRA)) return fail("exp_config: unknown flags 0x%x", p->flags);
    if ((p->flags & AIGAR_EXP_PRIORITIZED) && (!(p->alpha >= 0) || !(p->beta > 0)))
      return fail("exp_config: need alpha >= 0 and beta > 0 (got %g, %g)", p->alpha, p->beta);
  }
  if (begin_reconfig(h)) return -1;  // (no reader of the memory is pending either)
  trainer_free(h);
  h->exp_mem.release();
  h->exp = Exp{};
  if (!on) return 0;
  Exp e;
  e.cap = p->capacity;
  e.it_cap = 1;
  while (e.it_cap < e.cap) e.it_cap *= 2;
  e.dtype = p->state_dtype;
  e.esz = e.dtype == 0 ? 8 : 4;
  e.L = exp_state_len(h);
  e.stride = ((size_t)e.L * e.esz + 15) & ~(size_t)15;
  e.prio = (p->flags & AIGAR_EXP_PRIORITIZED) ? 1 : 0;
  e.alpha = p->alpha;
  e.beta = p->beta;
  e.seed = p->seed;
  const size_t cap = (size_t)e.cap, NP = (size_t)h->d.NP;
  bool ok = true;
  size_t total = 0;
  auto get = [&](size_t bytes, bool zero) -> void * {
    if (!ok) return nullptr;
    total += bytes;
    void *q = h->exp_mem.alloc(bytes, zero, h->stream);
    ok = q != nullptr;
    return q;
  };
  // zeroed: the rows and the old states; the trees, the scratch and the fifth field are filled below
  e.s = (char *)get(cap * e.stride, true);
  e.s2 = (char *)get(cap * e.stride, true);
  e.a = (double *)get(cap * 4 * sizeof(double), true);
  e.r = (double *)get(cap * sizeof(double), true);
  e.done = (uint8_t *)get(cap, true);
  if (e.prio) {
    e.vsum = (double *)get(2 * (size_t)e.it_cap * sizeof(double), false);
    e.vmin = (double *)get(2 * (size_t)e.it_cap * sizeof(double), false);
  }
  const bool extra = (p->flags & AIGAR_EXP_EXTRA) != 0;
  if (e.prio || extra) e.last = (int *)get(cap * sizeof(int), false);
  if (extra) {
    e.x = (double *)get(cap * 4 * sizeof(double), false);
    e.xv = (uint8_t *)get(cap, true);
  }
  e.ctl = (ExpCtl *)get(sizeof(ExpCtl), false);
  e.old = (char *)get(NP * e.stride, true);
  e.has_old = (uint8_t *)get(NP, true);
  e.off = (int *)get(NP * sizeof(int), false);
  if (!ok) {
    h->exp_mem.release();
    return fail("exp_config: out of device memory (%zu bytes for %lld transitions of %d values)", total,
                (long long)p->capacity, e.L);
  }
  if (e.last)
    hipLaunchKernelGGL(k_exp_fill_i, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, h->stream, e.last, cap, -1);
  if (e.x) {  // no slot has a fifth field: NaN, invalid
    hipLaunchKernelGGL(k_fill_d, dim3((unsigned)((cap * 4 + 255) / 256)), dim3(256), 0, h->stream, e.x, cap * 4,
                       __builtin_nan(""));
  }
  const size_t ni = e.prio ? 2 * (size_t)e.it_cap : 1;
  hipLaunchKernelGGL(k_exp_init, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, h->stream, e);
  HIPCHK(hipGetLastError());
  h->exp = e;
  return 0;
}

extern "C" int aigar_exp_info(aigar_handle *h, int64_t info[4]) {
  if (need_exp(h, "exp_info")) return -1;
  if (!info) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  ExpCtl c;
  HIPCHK(hipMemcpyAsync(&c, h->exp.ctl, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  info[0] = h->exp.cap;
  info[1] = c.size;
  info[2] = c.next;
  info[3] = c.added;
  return 0;
}

extern "C" int aigar_exp_add(aigar_handle *h, const void *s, const double *a, const double *r, const void *s2,
                             const uint8_t *done, const uint8_t *mask, int n, int on_device) {
  if (need_exp(h, "exp_add")) return -1;
  if (n < 0) return fail("exp_add: n = %d is negative", n);
  if (n == 0) return 0;
  if (!s || !a || !r || !s2 || !done) return fail("exp_add: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const Exp &e = h->exp;
  const size_t row = (size_t)e.L * e.esz, N = (size_t)n;
  if ((size_t)n > h->exp_off_n) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->d_exp_off) (void)hipFree(h->d_exp_off);
    h->d_exp_off = nullptr;
    h->exp_off_n = 0;
    if (hipMalloc((void **)&h->d_exp_off, N * sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      h->d_exp_off = nullptr;
      return fail("exp_add: out of device memory");
    }
    h->exp_off_n = N;
  }
  char *stage = nullptr;
  if (!on_device) {  // one staging block: s | s2 | a | r | done | mask (each part 16-byte aligned)
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_s2 = up(N * row), o_a = o_s2 + up(N * row), o_r = o_a + up(N * 32), o_d = o_r + up(N * 8),
                 o_m = o_d + up(N), bytes = o_m + up(N);
    if (hipMalloc((void **)&stage, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail("exp_add: out of device memory (%zu bytes of staging)", bytes);
    }
    hipError_t er = hipMemcpyAsync(stage, s, N * row, hipMemcpyHostToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(stage + o_s2, s2, N * row, hipMemcpyHostToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(stage + o_a, a, N * 32, hipMemcpyHostToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(stage + o_r, r, N * 8, hipMemcpyHostToDevice, h->stream);
    if (er == hipSuccess) er = hipMemcpyAsync(stage + o_d, done, N, hipMemcpyHostToDevice, h->stream);
    if (er == hipSuccess && mask) er = hipMemcpyAsync(stage + o_m, mask, N, hipMemcpyHostToDevice, h->stream);
    if (er != hipSuccess) {
      (void)hipStreamSynchronize(h->stream);
      (void)hipFree(stage);
      return fail("exp_add: copy failed: %s", hipGetErrorString(er));
    }
    s = stage;
    s2 = stage + o_s2;
    a = (const double *)(stage + o_a);
    r = (const double *)(stage + o_r);
    done = (const uint8_t *)(stage + o_d);
    if (mask) mask = (const uint8_t *)(stage + o_m);
  }
  hipLaunchKernelGGL(k_exp_plan, dim3(1), dim3(kExpPlanThreads), 0, h->stream, e, 1, (const uint8_t *)nullptr, mask, n,
                     h->d_exp_off);
  if (e.dtype == 0)
    hipLaunchKernelGGL(k_exp_rows<uint64_t>, dim3(n), dim3(256), 0, h->stream, e, h->d_exp_off, (const char *)s, row,
                       (const char *)s2, a, 4, r, done, (const uint8_t *)nullptr, 0, (const double *)nullptr);
  else
    hipLaunchKernelGGL(k_exp_rows<uint32_t>, dim3(n), dim3(256), 0, h->stream, e, h->d_exp_off, (const char *)s, row,
                       (const char *)s2, a, 4, r, done, (const uint8_t *)nullptr, 0, (const double *)nullptr);
  hipError_t er = hipGetLastError();
  if (stage) {
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(stage);
  }
  if (er != hipSuccess) return fail("exp_add: launch failed: %s", hipGetErrorString(er));
  return 0;
}

static void launch_exp_fetch(aigar_handle *h, hipStream_t st, const int64_t *idx, int batch, void *s, double *a, double *r,
                             void *s2, uint8_t *done, int count) {
  const Exp &e = h->exp;
  if (e.dtype == 0)
    hipLaunchKernelGGL(k_exp_fetch<uint64_t>, dim3(batch), dim3(256), 0, st, e, idx, (char *)s, a, r, (char *)s2, done, count);
  else
    hipLaunchKernelGGL(k_exp_fetch<uint32_t>, dim3(batch), dim3(256), 0, st, e, idx, (char *)s, a, r, (char *)s2, done, count);
}

extern "C" int aigar_exp_sample(aigar_handle *h, int batch, const double *u, void *s, double *a, double *r, void *s2,
                                uint8_t *done, double *w, int64_t *idx) {
  if (need_exp(h, "exp_sample")) return -1;
  if (batch < 1) return fail("exp_sample: batch = %d", batch);
  if (!w || !idx) return fail("exp_sample: w and idx are needed");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_exp_draw, dim3((batch + 255) / 256), dim3(256), 0, h->stream, h->exp, batch, u, w, idx);
  launch_exp_fetch(h, h->stream, idx, batch, s, a, r, s2, done, 1);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_exp_gather(aigar_handle *h, const int64_t *idx, int batch, void *s, double *a, double *r, void *s2,
                                uint8_t *done) {
  if (need_exp(h, "exp_gather")) return -1;
  if (batch < 0) return fail("exp_gather: batch = %d", batch);
  if (batch == 0) return 0;
  if (!idx) return fail("exp_gather: null idx");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_exp_fetch(h, h->stream, idx, batch, s, a, r, s2, done, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_exp_update_priorities(aigar_handle *h, const int64_t *idx, const double *prio, int n) {
  if (need_exp(h, "exp_update_priorities")) return -1;
  if (n < 0) return fail("exp_update_priorities: n = %d is negative", n);
  if (n == 0 || !h->exp.prio) return 0;  // (ReplayBuffer.update_priorities: pass)
  if (!idx || !prio) return fail("exp_update_priorities: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_exp_update, dim3(1), dim3(kExpPlanThreads), 0, h->stream, h->exp, idx, prio, n);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_exp_extra_get(aigar_handle *h, const int64_t *idx, int batch, double *out, uint8_t *valid) {
  if (need_exp(h, "exp_extra_get")) return -1;
  if (!h->exp.x) return fail("exp_extra_get: the replay memory has no extra field (AIGAR_EXP_EXTRA)");
  if (batch < 0) return fail("exp_extra_get: batch = %d", batch);
  if (batch == 0) return 0;
  if (!idx) return fail("exp_extra_get: null idx");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_exp_extra_get, dim3((unsigned)(((size_t)batch * 4 + 255) / 256)), dim3(256), 0, h->stream, h->exp,
                     idx, batch, out, valid);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_exp_extra_set(aigar_handle *h, const int64_t *idx, const double *rows, int n) {
  if (need_exp(h, "exp_extra_set")) return -1;
  if (!h->exp.x) return fail("exp_extra_set: the replay memory has no extra field (AIGAR_EXP_EXTRA)");
  if (n < 0) return fail("exp_extra_set: n = %d is negative", n);
  if (n == 0) return 0;
  if (!idx || !rows) return fail("exp_extra_set: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipLaunchKernelGGL(k_exp_extra_set, dim3(1), dim3(kExpPlanThreads), 0, h->stream, h->exp, idx, rows, n);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------ the trainers: what the three share
static int need_trn(aigar_handle *h, const char *who) {
  return need(h, h && h->trn.batch, who, "no training is configured (aigar_train_config)");
}
static int need_crit(aigar_handle *h, const char *who) {
  return need(h, h && h->crit.n_layers, who, "no critic is configured (aigar_critic_config)");
}
static int need_act(aigar_handle *h, const char *who) {
  return need(h, h && h->act.batch, who, "no CACLA training is configured (aigar_actrain_config)");
}
static int need_dpg(aigar_handle *h, const char *who) {
  return need(h, h && h->dpg.batch, who, "no DPG training is configured (aigar_dpg_config)");
}
static int need_spg(aigar_handle *h, const char *who) {
  return need(h, h && h->spg.d.batch, who, "no SPG training is configured (aigar_spg_config)");
}

// A *_config's parameter checks (before the handle: a bad set has its own message), in the order
// every trainer reports them: the sizes, its own integers, the learning rates, Adam's constants
// and the discount, its own doubles.  P: aigar_train_params, aigar_actrain_params, aigar_dpg_params,
// aigar_spg_params.
static int check_positive(const char *who, const char *name, double v) {
  return v > 0 && v < __builtin_inf() ? 0 : fail("%s: %s = %g must be positive and finite", who, name, v);
}
static int check_fraction(const char *who, const char *name, double v) {
  return v >= 0 && v < 1 ? 0 : fail("%s: %s = %g is outside [0, 1)", who, name, v);
}
template <class P>
static int check_train_sizes(const char *who, const P *p) {
  if (p->batch < 1 || p->batch > kTrainMaxBatch) return fail("%s: batch = %d is outside 1..%d", who, p->batch, kTrainMaxBatch);
  if (p->min_size < 0) return fail("%s: min_size = %d is negative", who, p->min_size);
  if (p->target_steps < 0) return fail("%s: target_steps = %d is negative", who, p->target_steps);
  return 0;
}
template <class P>
static int check_train_adam(const char *who, const P *p) {
  if (check_fraction(who, "beta1", p->beta1) || check_fraction(who, "beta2", p->beta2) ||
      check_positive(who, "epsilon", p->epsilon))
    return -1;
  if (!(p->discount >= 0 && p->discount <= 1)) return fail("%s: discount = %g is outside [0, 1]", who, p->discount);
  return 0;
}

// ... and its handle checks: these first for every trainer, then its own (head, critic,
// selection) around need_exp, and the widths last.
static int check_train_net(aigar_handle *h, const char *who) {
  if (h->d.tiled) return fail("%s: a tiled handle has no training", who);
  if (need_net(h, who)) return -1;
  if (h->conv.n_conv) return fail("%s: a network with a conv part is not trained on the device", who);
  return 0;
}
static int check_train_widths(aigar_handle *h, const char *who) {
  if (h->net.in[0] == h->exp.L) return 0;
  return fail("%s: the network has %d inputs, the memory's states %d values", who, h->net.in[0], h->exp.L);
}

// What the two Q(s, a) trainers share of both (P: aigar_dpg_params, aigar_spg_params; name: "DPG",
// "SPG"): the sizes before a trainer's own integers, the rates before its own doubles, and the
// handle checks up to need_exp, after which come its own and check_train_widths.
template <class P>
static int check_qsa_sizes(const char *who, const P *p) {
  if (check_train_sizes(who, p)) return -1;
  return p->reserved != 0 ? fail("%s: reserved = %d must be 0", who, p->reserved) : 0;
}
template <class P>
static int check_qsa_rates(const char *who, const P *p) {
  if (check_positive(who, "critic_lr", p->critic_lr) || check_positive(who, "actor_lr", p->actor_lr) ||
      check_train_adam(who, p))
    return -1;
  if (!(p->tau >= 0 && p->tau <= 1)) return fail("%s: tau = %g is outside [0, 1]", who, p->tau);
  if (!(fabs(p->q_increase) < __builtin_inf())) return fail("%s: q_increase = %g must be finite", who, p->q_increase);
  return 0;
}
static int check_qsa_handle(aigar_handle *h, const char *who, const char *name) {
  if (check_train_net(h, who) || need_crit(h, who)) return -1;
  if (!h->crit_q)
    return fail("%s: the critic is V(s) (aigar_critic_config), %s trains Q(s, a) (aigar_qcritic_config)", who, name);
  return need_exp(h, who);
}

// One zeroed buffer of the trainer's block; null, and ok false from then on, when one is refused
static void *train_get(aigar_handle *h, bool &ok, size_t bytes) {
  if (!ok) return nullptr;
  void *q = h->trn_mem.alloc(bytes, true, h->stream);
  ok = q != nullptr;
  return q;
}

// What a trainer's views share: the settings and the staged batch.
template <class P>
static Train train_shared(aigar_handle *h, bool &ok, const P *p) {
  const size_t B = (size_t)p->batch, row = (size_t)h->exp.L * h->exp.esz;
  Train s;
  s.batch = p->batch;
  s.bpad = (p->batch + kNetRows - 1) / kNetRows * kNetRows;
  s.min_size = p->min_size;
  s.target_steps = p->target_steps;
  s.beta1 = p->beta1;
  s.beta2 = p->beta2;
  s.epsilon = p->epsilon;
  s.discount = p->discount;
  s.s = (char *)train_get(h, ok, B * row);
  s.s2 = (char *)train_get(h, ok, B * row);
  s.a = (double *)train_get(h, ok, B * 4 * sizeof(double));
  s.r = (double *)train_get(h, ok, B * sizeof(double));
  s.w = (double *)train_get(h, ok, B * sizeof(double));
  s.u = (double *)train_get(h, ok, B * sizeof(double));
  s.done = (uint8_t *)train_get(h, ok, B);
  s.idx = (int64_t *)train_get(h, ok, B * sizeof(int64_t));
  s.td = (double *)train_get(h, ok, B * sizeof(double));
  s.prio = (double *)train_get(h, ok, B * sizeof(double));
  return s;
}

// One network's view of a trainer: s, and the network's own Adam state, buffers, counters and,
// with `target`, a target that starts as a copy of the network as it is now.
static Train train_view(aigar_handle *h, bool &ok, const Train &s, const Net &c, double lr, bool target) {
  const size_t B = (size_t)s.batch;
  Train v = s;
  v.lr = lr;
  for (int l = 0; l < c.n_layers; l++) {
    const size_t op = net_out_pad(c.out[l]), nw = (size_t)net_in_pad(c.in[l]) * op * sizeof(float);
    if (target) {
      v.tw[l] = (float *)train_get(h, ok, nw);
      v.tb[l] = (float *)train_get(h, ok, op * sizeof(float));
    }
    v.mw[l] = (float *)train_get(h, ok, nw);
    v.mb[l] = (float *)train_get(h, ok, op * sizeof(float));
    v.vw[l] = (float *)train_get(h, ok, nw);
    v.vb[l] = (float *)train_get(h, ok, op * sizeof(float));
    v.tile0[l + 1] = v.tile0[l] + (c.in[l] + 15) / 16 * (int)(op / 16);
    if (ok && target) {
      (void)hipMemcpyAsync(v.tw[l], c.w[l], nw, hipMemcpyDeviceToDevice, h->stream);
      (void)hipMemcpyAsync(v.tb[l], c.b[l], op * sizeof(float), hipMemcpyDeviceToDevice, h->stream);
    }
  }
  const size_t n_out = (size_t)c.out[c.n_layers - 1];
  v.q = (double *)train_get(h, ok, B * n_out * sizeof(double));
  if (target) v.q2 = (double *)train_get(h, ok, B * n_out * sizeof(double));
  v.hsave = (float *)train_get(h, ok, (size_t)std::max(c.n_layers - 1, 1) * v.bpad * kNetMaxUnits * sizeof(float));
  v.delta = (float *)train_get(h, ok, (size_t)c.n_layers * v.bpad * kNetMaxUnits * sizeof(float));
  v.ctl = (TrainCtl *)train_get(h, ok, sizeof(TrainCtl));
  return v;
}

// A Q(s, a) trainer's settings, views and packed-row buffers (dpg.inc; P as check_qsa_sizes').
// actor_pass: DPG's actor half runs through the critic, so it also gets mut and, for ca, a
// TrainCtl of its own; SPG's ca is c.
template <class P>
static DPGTrain qsa_setup(aigar_handle *h, bool &ok, const P *p, bool actor_pass) {
  DPGTrain t;
  t.batch = p->batch;
  t.n_s = h->net.in[0];
  t.n_act = h->net.out[h->net.n_layers - 1];
  t.soft = p->tau > 0 ? 1 : 0;
  t.tau = (float)p->tau;
  t.keep = (float)(1.0 - p->tau);
  t.q_increase = p->q_increase;
  const size_t B = (size_t)p->batch, xrow = (size_t)(t.n_s + t.n_act) * h->exp.esz;
  const Train s = train_shared(h, ok, p);
  t.c = train_view(h, ok, s, h->crit, p->critic_lr, true);
  t.a = train_view(h, ok, s, h->net, p->actor_lr, true);
  t.c.s = (char *)train_get(h, ok, B * xrow);  // (the critic's first layer reads the packed rows)
  t.c.s2 = (char *)train_get(h, ok, B * xrow);
  t.xm = (char *)train_get(h, ok, B * xrow);
  t.xt = (char *)train_get(h, ok, B * xrow);
  if (actor_pass) t.mut = (double *)train_get(h, ok, B * t.n_act * sizeof(double));
  t.qm = (double *)train_get(h, ok, B * sizeof(double));
  t.qt = (double *)train_get(h, ok, B * sizeof(double));
  t.ca = t.c;
  if (actor_pass) t.ca.ctl = (TrainCtl *)train_get(h, ok, sizeof(TrainCtl));
  return t;
}

// The launches that every trainer's step is made of, on stream s.  The mini-batch into a view's
// staging rows (replay.inc):
static void launch_draw_fetch(aigar_handle *h, hipStream_t s, const Train &v, int has_u) {
  const int B = v.batch;
  hipLaunchKernelGGL(k_exp_draw, dim3((B + 255) / 256), dim3(256), 0, s, h->exp, B, has_u ? v.u : (const double *)nullptr, v.w,
                     v.idx);
  launch_exp_fetch(h, s, v.idx, B, v.s, v.a, v.r, v.s2, v.done, 0);
}
// n with the weights of view v's target
static Net target_net(Net n, const Train &v) {
  for (int l = 0; l < n.n_layers; l++) {
    n.w[l] = v.tw[l];
    n.b[l] = v.tb[l];
  }
  return n;
}
// n on the B rows x of its x_dtype, every hidden layer's activations kept (net.inc)
static void launch_net_save(hipStream_t s, const Net &n, int B, const char *x, double *y, float *hsave) {
  const dim3 rows16((unsigned)((B + kNetRows - 1) / kNetRows)), net_block(64 * kNetWaves);
  if (n.x_dtype == 0) hipLaunchKernelGGL(k_net_save<double>, rows16, net_block, 0, s, n, (const double *)x, B, y, hsave);
  else hipLaunchKernelGGL(k_net_save<float>, rows16, net_block, 0, s, n, (const float *)x, B, y, hsave);
}
// [state, action] rows of the memory's dtype (dpg.inc k_sa_pack): `sets` row sets in one launch,
// 2, or 1: the first alone (the blocks B .. 2 B - 1 are the second's)
static void launch_sa_pack(hipStream_t s, const DPGTrain &t, int dtype, int sets, const char *s0, const double *a0, int st0,
                           char *o0, const char *s1, const double *a1, int st1, char *o1) {
  const int B = t.batch;
  if (dtype == 0)
    hipLaunchKernelGGL(k_sa_pack<double>, dim3(sets * B), dim3(64), 0, s, B, t.n_s, t.n_act, (const double *)s0, a0, st0,
                       (double *)o0, (const double *)s1, a1, st1, (double *)o1);
  else
    hipLaunchKernelGGL(k_sa_pack<float>, dim3(sets * B), dim3(64), 0, s, B, t.n_s, t.n_act, (const float *)s0, a0, st0,
                       (float *)o0, (const float *)s1, a1, st1, (float *)o1);
}
// view v's output delta back through n's layers, then every layer's gradient and Adam in place (train.inc)
static void launch_net_update(hipStream_t s, const Net &n, const Train &v) {
  if (n.n_layers > 1)
    hipLaunchKernelGGL(k_net_bwd, dim3((unsigned)(v.bpad / kNetRows)), dim3(64 * kNetWaves), 0, s, n, v);
  if (n.x_dtype == 0) hipLaunchKernelGGL(k_net_grad_adam<double>, dim3(v.tile0[n.n_layers]), dim3(64), 0, s, n, v);
  else hipLaunchKernelGGL(k_net_grad_adam<float>, dim3(v.tile0[n.n_layers]), dim3(64), 0, s, n, v);
}
// The critic half of a Q(s, a) trainer's step, DPG's and SPG's, on the batch in t.a's staging rows
// (dpg.inc).  cr: the critic, ct / at: the critic's and the actor's targets, of the memory's dtype.
static void launch_qsa_critic(aigar_handle *h, hipStream_t s, const DPGTrain &t, const Net &cr, const Net &ct, const Net &at,
                              int prio_evals) {
  const Train &c = t.c, &a = t.a;
  const Exp &e = h->exp;
  const int B = t.batch;
  launch_net(s, at, a.s2, B, a.q2, nullptr, nullptr);
  launch_sa_pack(s, t, e.dtype, 2, a.s, a.a, 4, c.s, a.s2, a.q2, t.n_act, c.s2);
  launch_net_save(s, cr, B, c.s, c.q, c.hsave);
  launch_net(s, ct, c.s2, B, c.q2, nullptr, nullptr);
  hipLaunchKernelGGL(k_td_q, dim3(1), dim3(kTrainMaxBatch), 0, s, c, e, h->d, cr.n_layers, prio_evals);
  launch_net_update(s, cr, c);
  if (e.prio) hipLaunchKernelGGL(k_exp_update, dim3(1), dim3(kExpPlanThreads), 0, s, e, c.idx, c.prio, B);
}

// aigar_*_step after its need_*: n_steps replays of the kind's step graph, each after the copy of
// its draws into the view's u row.
// SPG: zu, the search's uniforms, zu_n doubles a step into zu_row; its launch gets has_u | has_zu << 1.
static int trainer_step(aigar_handle *h, const char *who, int kind, int n_steps, const double *u, const Train &v,
                        void (*launch)(aigar_handle *, hipStream_t, int), const double *zu = nullptr,
                        double *zu_row = nullptr, size_t zu_n = 0) {
  if (n_steps < 1) return fail("%s: n_steps = %d is below 1", who, n_steps);
  HIPCHK(hipSetDevice(h->cfg.device));
  TrainKey k;
  key_clear(k);
  k.kind = kind;
  k.has_u = u ? 1 : 0;
  k.has_zu = zu ? 1 : 0;
  if (kind == kTrainQ && h->ctrn.on) key_put(k.conv, h->conv);
  const int has = k.has_u | k.has_zu << 1;
  const bool graph = h->use_graph;
  if (graph && !h->train.ensure(h, k, [&](hipStream_t cs) { launch(h, cs, has); }))
    return fail("%s: graph capture failed", who);
  Mark m(h, who);
  const size_t B = (size_t)v.batch;
  for (int i = 0; i < n_steps; i++) {
    if (u) HIPCHK(hipMemcpyAsync(v.u, u + (size_t)i * B, B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (zu) HIPCHK(hipMemcpyAsync(zu_row, zu + (size_t)i * zu_n, zu_n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (graph) HIPCHK(h->train.launch(h));
    else launch(h, h->stream, has);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// aigar_*_td: the last drawn step's TD errors and memory indices (stream-ordered copies)
static int trainer_td(aigar_handle *h, const Train &v, double *td, int64_t *idx) {
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t B = (size_t)v.batch;
  if (td) HIPCHK(hipMemcpyAsync(td, v.td, B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  if (idx) HIPCHK(hipMemcpyAsync(idx, v.idx, B * sizeof(int64_t), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

// aigar_*_sync_target: view v's target <- its network c, the padded copies whole
static int target_copy(aigar_handle *h, const Net &c, const Train &v) {
  for (int l = 0; l < c.n_layers; l++) {
    const size_t op = net_out_pad(c.out[l]), nw = (size_t)net_in_pad(c.in[l]) * op * sizeof(float);
    HIPCHK(hipMemcpyAsync(v.tw[l], c.w[l], nw, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(v.tb[l], c.b[l], op * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// aigar_*_reset: view v's Adam state to zero
static int adam_clear(aigar_handle *h, const Net &c, const Train &v) {
  for (int l = 0; l < c.n_layers; l++) {
    const size_t op = net_out_pad(c.out[l]), nw = (size_t)net_in_pad(c.in[l]) * op * sizeof(float);
    HIPCHK(hipMemsetAsync(v.mw[l], 0, nw, h->stream));
    HIPCHK(hipMemsetAsync(v.vw[l], 0, nw, h->stream));
    HIPCHK(hipMemsetAsync(v.mb[l], 0, op * sizeof(float), h->stream));
    HIPCHK(hipMemsetAsync(v.vb[l], 0, op * sizeof(float), h->stream));
  }
  return 0;
}

__global__ void k_train_clear(TrainCtl *ctl, int target) {  // target: the copy was made; else Adam starts over
  if (target) ctl->since = 0;
  else ctl->t = 0;
}

// aigar_*_info: a trainer's control blocks to the host, one synchronisation for all of them
struct CtlRead {
  void *host;
  const void *dev;
  size_t bytes;
};
static int read_ctls(aigar_handle *h, std::initializer_list<CtlRead> blocks) {
  HIPCHK(hipSetDevice(h->cfg.device));
  for (const CtlRead &b : blocks) HIPCHK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// aigar_dpg_* and aigar_spg_* on the trainer's DPGTrain: both targets as copies of their networks ...
static int qsa_sync_target(aigar_handle *h, const DPGTrain &t) {
  HIPCHK(hipSetDevice(h->cfg.device));
  if (target_copy(h, h->crit, t.c) || target_copy(h, h->net, t.a)) return -1;
  hipLaunchKernelGGL(k_train_clear, dim3(1), dim3(1), 0, h->stream, t.c.ctl, 1);
  HIPCHK(hipGetLastError());
  return 0;
}
// ... and a reset's first part: both Adam states to zero (the counters are the trainer's own kernel's)
static int qsa_adam_clear(aigar_handle *h, const DPGTrain &t) {
  HIPCHK(hipSetDevice(h->cfg.device));
  return adam_clear(h, h->crit, t.c) || adam_clear(h, h->net, t.a) ? -1 : 0;
}

// ------------------------------------------------------------ Q-learning trainer
extern "C" int aigar_train_config(aigar_handle *h, const aigar_train_params *p) {
  const char *who = "train_config";
  if (p && (check_train_sizes(who, p) || check_positive(who, "lr", p->lr) || check_train_adam(who, p))) return -1;
  if (!h) return fail("null handle");
  if (p) {
    if (check_train_net(h, who)) return -1;
    if (h->net.out_act != AIGAR_ACT_LINEAR)
      return fail("train_config: the network's head is %s, Q-learning needs a linear head", net_act_name(h->net.out_act));
    if (need_exp(h, who)) return -1;
    if (need_dec(h, who)) return -1;
    if (h->dec.n_out != h->net.out[h->net.n_layers - 1])
      return fail("train_config: the network has %d outputs, the action selection %d", h->net.out[h->net.n_layers - 1],
                  h->dec.n_out);
    if (check_train_widths(h, who)) return -1;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p || (h->trn.batch && !h->ctrn.on)) trainer_free(h);  // (a null p turns off this trainer, not another)
  if (!p) return 0;
  bool ok = true;
  const Train t = train_view(h, ok, train_shared(h, ok, p), h->net, p->lr, true);
  if (!ok) {
    h->trn_mem.release();
    return fail("train_config: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->trn = t;
  return 0;
}

// One training step's launches on stream s (train.inc).
static void launch_train_step(aigar_handle *h, hipStream_t s, int has_u) {
  const Train &t = h->trn;
  const Exp &e = h->exp;
  Net on = h->net;
  on.x_dtype = e.dtype;
  const Net tg = target_net(on, t);
  const int B = t.batch;
  launch_draw_fetch(h, s, t, has_u);
  launch_net_save(s, on, B, t.s, t.q, t.hsave);
  launch_net(s, tg, t.s2, B, t.q2, nullptr, nullptr);
  hipLaunchKernelGGL(k_td, dim3(1), dim3(kTrainMaxBatch), 0, s, t, e, h->d, on.n_layers, on.out[on.n_layers - 1]);
  launch_net_update(s, on, t);
  if (e.prio) hipLaunchKernelGGL(k_exp_update, dim3(1), dim3(kExpPlanThreads), 0, s, e, t.idx, t.prio, B);
  hipLaunchKernelGGL(k_train_tail, dim3(64), dim3(256), 0, s, on, t);
}

// ... of a network with a conv part (convtrain.inc): the same parameters and the same checks of
// them under its own name; trn is the dense part's view, ctrn the conv part's.
static size_t conv_w_bytes(const Conv &c, int l) {
  const int cin = l ? c.filters[l - 1] : c.channels;
  return (size_t)conv_k_pad(c.k[l] * c.k[l] * cin) * net_out_pad(c.filters[l]) * sizeof(float);
}
static size_t conv_b_bytes(const Conv &c, int l) { return (size_t)net_out_pad(c.filters[l]) * sizeof(float); }

extern "C" int aigar_train_config_cnn(aigar_handle *h, const aigar_train_params *p) {
  const char *who = "train_config_cnn";
  if (p && (check_train_sizes(who, p) || check_positive(who, "lr", p->lr) || check_train_adam(who, p))) return -1;
  if (!h) return fail("null handle");
  if (p) {
    if (h->d.tiled) return fail("%s: a tiled handle has no training", who);
    if (need_net(h, who)) return -1;
    if (!h->conv.n_conv)
      return fail("train_config_cnn: the network has no conv part (a dense network is trained by aigar_train_config)");
    if (h->net.out_act != AIGAR_ACT_LINEAR)
      return fail("train_config_cnn: the network's head is %s, Q-learning needs a linear head",
                  net_act_name(h->net.out_act));
    if (need_exp(h, who)) return -1;
    const int img = h->conv.side * h->conv.side * h->conv.channels;
    if (h->exp.L != img)
      return fail("train_config_cnn: the conv part takes %d x %d x %d = %d values, the memory's states %d values",
                  h->conv.side, h->conv.side, h->conv.channels, img, h->exp.L);
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p || h->ctrn.on) trainer_free(h);  // (a null p turns off this trainer, not another)
  if (!p) return 0;
  bool ok = true;
  const Train t = train_view(h, ok, train_shared(h, ok, p), h->net, p->lr, true);
  const Conv &c = h->conv;
  ConvTrain ct{};
  ct.on = 1;
  for (int l = 0; l < c.n_conv; l++) {
    const size_t nw = conv_w_bytes(c, l), nb = conv_b_bytes(c, l);
    const size_t na = (size_t)t.bpad * c.osz[l] * c.osz[l] * c.filters[l] * sizeof(float);
    const int K = c.k[l] * c.k[l] * (l ? c.filters[l - 1] : c.channels);
    ct.tw[l] = (float *)train_get(h, ok, nw);
    ct.tb[l] = (float *)train_get(h, ok, nb);
    ct.mw[l] = (float *)train_get(h, ok, nw);
    ct.mb[l] = (float *)train_get(h, ok, nb);
    ct.vw[l] = (float *)train_get(h, ok, nw);
    ct.vb[l] = (float *)train_get(h, ok, nb);
    ct.act[l] = (float *)train_get(h, ok, na);
    ct.tact[l] = (float *)train_get(h, ok, na);
    ct.delta[l] = (float *)train_get(h, ok, na);
    ct.tile0[l + 1] = ct.tile0[l] + (K + 1 + 15) / 16 * (net_out_pad(c.filters[l]) / 16);
    if (ok) {
      (void)hipMemcpyAsync(ct.tw[l], c.w[l], nw, hipMemcpyDeviceToDevice, h->stream);
      (void)hipMemcpyAsync(ct.tb[l], c.b[l], nb, hipMemcpyDeviceToDevice, h->stream);
    }
  }
  if (!ok) {
    h->trn_mem.release();
    return fail("train_config_cnn: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->trn = t;
  h->ctrn = ct;
  return 0;
}

// c on the trainer's buffers: the online pass's kept activations, or the target's filters and activations
static Conv train_conv(Conv c, const ConvTrain &ct, int bpad, bool target) {
  c.cap = bpad;
  for (int l = 0; l < c.n_conv; l++) {
    c.act[l] = target ? ct.tact[l] : ct.act[l];
    if (target) {
      c.w[l] = ct.tw[l];
      c.b[l] = ct.tb[l];
    }
  }
  return c;
}

// One training step's launches on stream s for a network with a conv part (convtrain.inc).
static void launch_cnn_train_step(aigar_handle *h, hipStream_t s, int has_u) {
  const Train &t = h->trn;
  const ConvTrain &ct = h->ctrn;
  const Exp &e = h->exp;
  const Conv &cv = h->conv;
  const Conv con = train_conv(cv, ct, t.bpad, false), ctg = train_conv(cv, ct, t.bpad, true);
  const int nc = cv.n_conv, B = t.batch;
  Net on = h->net;
  on.x_dtype = 1;  // (the dense part reads the float32 feature rows)
  const Net tg = target_net(on, t);
  Train td = t;  // the dense part's view: its first layer's h is the feature row
  td.s = (char *)ct.act[nc - 1];
  launch_draw_fetch(h, s, t, has_u);
  launch_conv(s, con, t.s, e.dtype, B, nullptr, nullptr);
  launch_net_save(s, on, B, td.s, t.q, t.hsave);
  launch_conv(s, ctg, t.s2, e.dtype, B, nullptr, nullptr);
  launch_net(s, tg, ct.tact[nc - 1], B, t.q2, nullptr, nullptr);
  hipLaunchKernelGGL(k_td, dim3(1), dim3(kTrainMaxBatch), 0, s, t, e, h->d, on.n_layers, on.out[on.n_layers - 1]);
  // every reader of the weights ...
  if (on.n_layers > 1)
    hipLaunchKernelGGL(k_net_bwd, dim3((unsigned)(t.bpad / kNetRows)), dim3(64 * kNetWaves), 0, s, on, t);
  {
    const unsigned tiles = (unsigned)((cv.n_flat + 15) / 16);
    hipLaunchKernelGGL(k_net_bwd_feat, dim3((tiles + kNetWaves - 1) / kNetWaves, (unsigned)(t.bpad / kNetRows)),
                       dim3(64 * kNetWaves), 0, s, on, t, ct.act[nc - 1], ct.delta[nc - 1]);
  }
  for (int l = nc - 1; l >= 1; l--) {
    ConvBwd L;
    L.H = cv.osz[l - 1];
    L.cin = cv.filters[l - 1];
    L.k = cv.k[l];
    L.stride = cv.stride[l];
    L.O = cv.osz[l];
    L.F = cv.filters[l];
    L.K = L.k * L.k * L.F;
    L.Fp = net_out_pad(L.F);
    L.mF = conv_magic(L.F);
    L.mk = conv_magic(L.k);
    L.ms = conv_magic(L.stride);
    L.mH = conv_magic(L.H);
    const size_t M = (size_t)B * L.H * L.H;
    const dim3 grid((unsigned)((M + 16 * kConvWaves - 1) / (16 * kConvWaves))), block(64 * kConvWaves);
#define AIGAR_CONV_BWD(NT) \
  hipLaunchKernelGGL((k_conv_bwd<NT>), grid, block, 0, s, L, t, ct.delta[l], cv.w[l], ct.act[l - 1], ct.delta[l - 1])
    switch ((L.cin + 15) / 16) {
      case 1: AIGAR_CONV_BWD(1); break;
      case 2: AIGAR_CONV_BWD(2); break;
      case 3: AIGAR_CONV_BWD(3); break;
      default: AIGAR_CONV_BWD(4); break;
    }
#undef AIGAR_CONV_BWD
  }
  // ... before every kernel that updates them
  hipLaunchKernelGGL(k_net_grad_adam<float>, dim3(t.tile0[on.n_layers]), dim3(64), 0, s, on, td);
  if (e.dtype == 0) hipLaunchKernelGGL(k_conv_grad_adam<double>, dim3(ct.tile0[nc]), dim3(64), 0, s, cv, ct, t);
  else hipLaunchKernelGGL(k_conv_grad_adam<float>, dim3(ct.tile0[nc]), dim3(64), 0, s, cv, ct, t);
  if (e.prio) hipLaunchKernelGGL(k_exp_update, dim3(1), dim3(kExpPlanThreads), 0, s, e, t.idx, t.prio, B);
  hipLaunchKernelGGL(k_conv_train_tail, dim3(16), dim3(256), 0, s, cv, ct, t);
  hipLaunchKernelGGL(k_train_tail, dim3(64), dim3(256), 0, s, on, t);
}

extern "C" int aigar_train_step(aigar_handle *h, int n_steps, const double *u) {
  if (need_trn(h, "train_step")) return -1;
  return trainer_step(h, "train_step", kTrainQ, n_steps, u, h->trn, h->ctrn.on ? launch_cnn_train_step : launch_train_step);
}

extern "C" int aigar_train_info(aigar_handle *h, int64_t info[4]) {
  if (need_trn(h, "train_info")) return -1;
  if (!info) return fail("train_info: null argument");
  TrainCtl c;
  if (read_ctls(h, {{&c, h->trn.ctl, sizeof c}})) return -1;
  info[0] = c.t;
  info[1] = c.skipped;
  info[2] = c.since;
  info[3] = 0;
  return 0;
}

extern "C" int aigar_train_td(aigar_handle *h, double *td, int64_t *idx) {
  if (need_trn(h, "train_td")) return -1;
  return trainer_td(h, h->trn, td, idx);
}

extern "C" int aigar_train_sync_target(aigar_handle *h) {
  if (need_trn(h, "train_sync_target")) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (target_copy(h, h->net, h->trn)) return -1;
  for (int l = 0; h->ctrn.on && l < h->conv.n_conv; l++) {
    HIPCHK(hipMemcpyAsync(h->ctrn.tw[l], h->conv.w[l], conv_w_bytes(h->conv, l), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ctrn.tb[l], h->conv.b[l], conv_b_bytes(h->conv, l), hipMemcpyDeviceToDevice, h->stream));
  }
  hipLaunchKernelGGL(k_train_clear, dim3(1), dim3(1), 0, h->stream, h->trn.ctl, 1);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_train_reset(aigar_handle *h) {
  if (need_trn(h, "train_reset")) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (adam_clear(h, h->net, h->trn)) return -1;
  for (int l = 0; h->ctrn.on && l < h->conv.n_conv; l++) {
    const size_t nw = conv_w_bytes(h->conv, l), nb = conv_b_bytes(h->conv, l);
    HIPCHK(hipMemsetAsync(h->ctrn.mw[l], 0, nw, h->stream));
    HIPCHK(hipMemsetAsync(h->ctrn.vw[l], 0, nw, h->stream));
    HIPCHK(hipMemsetAsync(h->ctrn.mb[l], 0, nb, h->stream));
    HIPCHK(hipMemsetAsync(h->ctrn.vb[l], 0, nb, h->stream));
  }
  hipLaunchKernelGGL(k_train_clear, dim3(1), dim3(1), 0, h->stream, h->trn.ctl, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------ CACLA: the critic and the trainer
// aigar_critic_config (V(s): q false) and aigar_qcritic_config (Q(s, a): the rows are [state, action])
static int critic_config(aigar_handle *h, const aigar_net_params *p, bool q) {
  const char *who = q ? "qcritic_config" : "critic_config";
  if (p) {  // (before the handle: a bad set has its own message)
    if (net_shape_check(who, p)) return -1;
    if (p->units[p->n_layers - 1] != 1 || p->out_act != AIGAR_ACT_LINEAR)
      return fail("%s: the head has %d units with activation %d (%s), %s is one linear unit", who,
                  p->units[p->n_layers - 1], p->out_act, net_act_name(p->out_act), q ? "Q(s, a)" : "V(s)");
  }
  if (!h) return fail("null handle");
  if (p) {
    if (need_net(h, who)) return -1;
    if (h->conv.n_conv) return fail("%s: the acting network has a conv part, the critic is a dense network", who);
    if (!q && p->n_in != h->net.in[0])
      return fail("%s: n_in = %d differs from the acting network's %d", who, p->n_in, h->net.in[0]);
    if (q) {
      const int n_act = h->net.out[h->net.n_layers - 1];
      if (h->net.out_act != AIGAR_ACT_SIGMOID)
        return fail("%s: the network's head is %s, the DPG actor needs a sigmoid head", who, net_act_name(h->net.out_act));
      if (n_act > 4) return fail("%s: the actor has %d outputs, a stored action has at most 4", who, n_act);
      if (p->n_in != h->net.in[0] + n_act)
        return fail("%s: n_in = %d differs from the acting network's n_in + n_out = %d + %d", who, p->n_in, h->net.in[0],
                    n_act);
    }
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));  // (no training step or forward pass is pending)
  critic_free(h);
  if (!p) return 0;
  Net c{};
  c.n_layers = p->n_layers;
  c.x_dtype = p->x_dtype;
  c.hid_act = p->hidden_act;
  c.out_act = AIGAR_ACT_LINEAR;
  size_t stage = 0;
  bool ok = true;
  for (int l = 0; l < c.n_layers && ok; l++) {
    c.in[l] = l ? p->units[l - 1] : p->n_in;
    c.out[l] = p->units[l];
    const size_t ip = net_in_pad(c.in[l]), op = net_out_pad(c.out[l]);
    c.w[l] = (float *)h->crit_mem.alloc(ip * op * sizeof(float), true, h->stream);
    c.b[l] = (float *)h->crit_mem.alloc(op * sizeof(float), true, h->stream);
    ok = c.w[l] && c.b[l];
    stage = std::max(stage, (size_t)c.in[l] * c.out[l] + c.out[l]);
  }
  if (ok) ok = (h->crit_stage = (float *)h->crit_mem.alloc(stage * sizeof(float), true, h->stream)) != nullptr;
  if (!ok) {
    critic_free(h);
    return fail("%s: out of device memory", who);
  }
  HIPCHK(hipGetLastError());
  h->crit = c;
  h->crit_q = q;
  return 0;
}
extern "C" int aigar_critic_config(aigar_handle *h, const aigar_net_params *p) { return critic_config(h, p, false); }
extern "C" int aigar_qcritic_config(aigar_handle *h, const aigar_net_params *p) { return critic_config(h, p, true); }

extern "C" int aigar_critic_set_weights(aigar_handle *h, int layer, const float *W, const float *b, int on_device) {
  if (need_crit(h, "critic_set_weights")) return -1;
  return set_dense_weights(h, "critic_set_weights", h->crit, h->crit_stage, layer, W, b, on_device);
}

extern "C" int aigar_critic_forward(aigar_handle *h, const void *x, int x_dtype, int rows, double *out) {
  if (need_crit(h, "critic_forward")) return -1;
  if (!x || !out) return fail("critic_forward: null argument");
  if (x_dtype != 0 && x_dtype != 1) return fail("critic_forward: x_dtype must be 0 (float64) or 1 (float32)");
  if (rows < 1 || rows > (1 << 30)) return fail("critic_forward: rows = %d is outside 1..2^30", rows);
  HIPCHK(hipSetDevice(h->cfg.device));
  Net c = h->crit;
  c.x_dtype = x_dtype;
  launch_net(h->stream, c, x, rows, out, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_actrain_config(aigar_handle *h, const aigar_actrain_params *p) {
  const char *who = "actrain_config";
  if (p) {
    if (check_train_sizes(who, p)) return -1;
    if (p->var_epochs < 0 || p->var_epochs > AIGAR_ACTRAIN_MAX_EPOCHS)
      return fail("actrain_config: var_epochs = %d is outside 0..%d", p->var_epochs, AIGAR_ACTRAIN_MAX_EPOCHS);
    if (check_positive(who, "critic_lr", p->critic_lr) || check_positive(who, "actor_lr", p->actor_lr) ||
        check_train_adam(who, p) || check_positive(who, "var_start", p->var_start) ||
        check_fraction(who, "var_beta", p->var_beta))
      return -1;
  }
  if (!h) return fail("null handle");
  if (p) {
    if (check_train_net(h, who)) return -1;
    if (h->net.out_act != AIGAR_ACT_SIGMOID)
      return fail("actrain_config: the network's head is %s, the CACLA actor needs a sigmoid head",
                  net_act_name(h->net.out_act));
    if (h->net.out[h->net.n_layers - 1] > 4)
      return fail("actrain_config: the actor has %d outputs, a stored action has at most 4", h->net.out[h->net.n_layers - 1]);
    if (need_crit(h, who)) return -1;
    if (h->crit_q) return fail("actrain_config: the critic is Q(s, a) (aigar_qcritic_config), CACLA trains V(s)");
    if (need_exp(h, who)) return -1;
    if (check_train_widths(h, who)) return -1;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p || h->act.batch) trainer_free(h);  // (a null p turns off this trainer, not another)
  if (!p) return 0;
  ACTrain t;
  t.batch = p->batch;
  t.var_epochs = p->var_epochs;
  t.var_start = p->var_start;
  t.var_beta = p->var_beta;
  bool ok = true;
  const Train s = train_shared(h, ok, p);
  t.c = train_view(h, ok, s, h->crit, p->critic_lr, true);
  t.a = train_view(h, ok, s, h->net, p->actor_lr, false);
  t.count = (int32_t *)train_get(h, ok, (size_t)p->batch * sizeof(int32_t));
  t.x = (ACtl *)train_get(h, ok, sizeof(ACtl));
  if (!ok) {
    h->trn_mem.release();
    return fail("actrain_config: out of device memory");
  }
  hipLaunchKernelGGL(k_actrain_clear, dim3(1), dim3(1), 0, h->stream, t.c.ctl, t.a.ctl, t.x, t.var_start);
  HIPCHK(hipGetLastError());
  h->act = t;
  return 0;
}

// One CACLA training step's launches on stream s (actrain.inc).
static void launch_actrain_step(aigar_handle *h, hipStream_t s, int has_u) {
  const ACTrain &t = h->act;
  const Train &c = t.c, &a = t.a;
  const Exp &e = h->exp;
  Net cr = h->crit, ac = h->net;
  cr.x_dtype = ac.x_dtype = e.dtype;
  const Net tg = target_net(cr, c);
  const int B = t.batch, n_out = ac.out[ac.n_layers - 1];
  launch_draw_fetch(h, s, c, has_u);
  launch_net_save(s, cr, B, c.s, c.q, c.hsave);
  launch_net(s, tg, c.s2, B, c.q2, nullptr, nullptr);
  hipLaunchKernelGGL(k_td_v, dim3(1), dim3(kTrainMaxBatch), 0, s, t, e, h->d, cr.n_layers);
  launch_net_update(s, cr, c);
  if (e.prio) hipLaunchKernelGGL(k_exp_update, dim3(1), dim3(kExpPlanThreads), 0, s, e, c.idx, c.prio, B);
  for (int ep = 0; ep < std::max(t.var_epochs, 1); ep++) {
    launch_net_save(s, ac, B, a.s, a.q, a.hsave);
    hipLaunchKernelGGL(k_actor_delta, dim3(1), dim3(kTrainMaxBatch), 0, s, t, h->d, ep, ac.n_layers, n_out);
    launch_net_update(s, ac, a);
  }
  hipLaunchKernelGGL(k_train_tail, dim3(64), dim3(256), 0, s, cr, c);
}

extern "C" int aigar_actrain_step(aigar_handle *h, int n_steps, const double *u) {
  if (need_act(h, "actrain_step")) return -1;
  return trainer_step(h, "actrain_step", kTrainCacla, n_steps, u, h->act.c, launch_actrain_step);
}

extern "C" int aigar_actrain_info(aigar_handle *h, int64_t info[8]) {
  if (need_act(h, "actrain_info")) return -1;
  if (!info) return fail("actrain_info: null argument");
  TrainCtl c, a;
  ACtl x;
  if (read_ctls(h, {{&c, h->act.c.ctl, sizeof c}, {&a, h->act.a.ctl, sizeof a}, {&x, h->act.x, sizeof x}})) return -1;
  info[0] = c.t;
  info[1] = c.skipped;
  info[2] = c.since;
  info[3] = a.t;
  info[4] = x.sel;
  info[5] = x.epochs;
  info[6] = x.cut;
  info[7] = x.eskipped;
  return 0;
}

extern "C" int aigar_actrain_td(aigar_handle *h, double *td, int64_t *idx, int32_t *count) {
  if (need_act(h, "actrain_td")) return -1;
  const ACTrain &t = h->act;
  if (trainer_td(h, t.c, td, idx)) return -1;
  if (count) HIPCHK(hipMemcpyAsync(count, t.count, (size_t)t.batch * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

extern "C" int aigar_actrain_var(aigar_handle *h, double *var) {
  if (need_act(h, "actrain_var")) return -1;
  if (!var) return fail("actrain_var: null argument");
  ACtl x;
  if (read_ctls(h, {{&x, h->act.x, sizeof x}})) return -1;
  *var = x.var;
  return 0;
}

extern "C" int aigar_actrain_sync_target(aigar_handle *h) {
  if (need_act(h, "actrain_sync_target")) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  if (target_copy(h, h->crit, h->act.c)) return -1;
  hipLaunchKernelGGL(k_train_clear, dim3(1), dim3(1), 0, h->stream, h->act.c.ctl, 1);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_actrain_reset(aigar_handle *h) {
  if (need_act(h, "actrain_reset")) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  const ACTrain &t = h->act;
  if (adam_clear(h, h->crit, t.c) || adam_clear(h, h->net, t.a)) return -1;
  hipLaunchKernelGGL(k_actrain_clear, dim3(1), dim3(1), 0, h->stream, t.c.ctl, t.a.ctl, t.x, t.var_start);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------ DPG: the Q(s, a) critic's trainer
static_assert(sizeof(DPGTrain) + 2 * sizeof(Net) + sizeof(Dev) <= 4096, "k_dpg_tail's arguments");

extern "C" int aigar_dpg_config(aigar_handle *h, const aigar_dpg_params *p) {
  const char *who = "dpg_config";
  if (p && (check_qsa_sizes(who, p) || check_qsa_rates(who, p))) return -1;
  if (!h) return fail("null handle");
  if (p && (check_qsa_handle(h, who, "DPG") || check_train_widths(h, who))) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p || h->dpg.batch) trainer_free(h);  // (a null p turns off this trainer, not another)
  if (!p) return 0;
  bool ok = true;
  const DPGTrain t = qsa_setup(h, ok, p, true);
  if (!ok) {
    h->trn_mem.release();
    return fail("dpg_config: out of device memory");
  }
  HIPCHK(hipGetLastError());
  h->dpg = t;  // (the blocks are zeroed: every counter starts at 0)
  return 0;
}

// One DPG training step's launches on stream s (dpg.inc).
static void launch_dpg_step(aigar_handle *h, hipStream_t s, int has_u) {
  const DPGTrain &t = h->dpg;
  const Train &c = t.c, &a = t.a, &ca = t.ca;
  Net cr = h->crit, ac = h->net;
  cr.x_dtype = ac.x_dtype = h->exp.dtype;
  const Net ct = target_net(cr, c), at = target_net(ac, a);
  const int B = t.batch;
  launch_draw_fetch(h, s, a, has_u);
  launch_qsa_critic(h, s, t, cr, ct, at, 0);
  // the actor half
  launch_net_save(s, ac, B, a.s, a.q, a.hsave);
  launch_net(s, at, a.s, B, t.mut, nullptr, nullptr);
  launch_sa_pack(s, t, h->exp.dtype, 2, a.s, a.q, t.n_act, t.xm, a.s, t.mut, t.n_act, t.xt);
  launch_net_save(s, cr, B, t.xm, t.qm, ca.hsave);  // (the critic's update is done: its buffers serve the actor pass)
  launch_net(s, ct, t.xt, B, t.qt, nullptr, nullptr);
  hipLaunchKernelGGL(k_dpg_delta, dim3(1), dim3(kTrainMaxBatch), 0, s, t, h->d, cr.n_layers);
  if (cr.n_layers > 1)
    hipLaunchKernelGGL(k_net_bwd, dim3((unsigned)(c.bpad / kNetRows)), dim3(64 * kNetWaves), 0, s, cr, ca);
  hipLaunchKernelGGL(k_net_bwd_in, dim3(1), dim3(64 * (c.bpad / kNetRows)), 0, s, cr, t, h->d, ac.n_layers);
  launch_net_update(s, ac, a);
  hipLaunchKernelGGL(k_dpg_tail, dim3(64), dim3(256), 0, s, cr, ac, t);
}

extern "C" int aigar_dpg_step(aigar_handle *h, int n_steps, const double *u) {
  if (need_dpg(h, "dpg_step")) return -1;
  return trainer_step(h, "dpg_step", kTrainDpg, n_steps, u, h->dpg.a, launch_dpg_step);
}

extern "C" int aigar_dpg_info(aigar_handle *h, int64_t info[8]) {
  if (need_dpg(h, "dpg_info")) return -1;
  if (!info) return fail("dpg_info: null argument");
  TrainCtl c, a;
  if (read_ctls(h, {{&c, h->dpg.c.ctl, sizeof c}, {&a, h->dpg.a.ctl, sizeof a}})) return -1;
  info[0] = c.t;
  info[1] = c.skipped;
  info[2] = c.since;
  info[3] = a.t;
  info[4] = a.skipped;
  info[5] = info[6] = info[7] = 0;
  return 0;
}

extern "C" int aigar_dpg_td(aigar_handle *h, double *td, int64_t *idx) {
  if (need_dpg(h, "dpg_td")) return -1;
  return trainer_td(h, h->dpg.c, td, idx);
}

extern "C" int aigar_dpg_sync_target(aigar_handle *h) {
  if (need_dpg(h, "dpg_sync_target")) return -1;
  return qsa_sync_target(h, h->dpg);
}

extern "C" int aigar_dpg_reset(aigar_handle *h) {
  if (need_dpg(h, "dpg_reset")) return -1;
  const DPGTrain &t = h->dpg;
  if (qsa_adam_clear(h, t)) return -1;
  hipLaunchKernelGGL(k_dpg_clear, dim3(1), dim3(1), 0, h->stream, t.c.ctl, t.a.ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------ SPG: the sampled search on DPG's critic half
static_assert(sizeof(SPGTrain) + sizeof(Net) + sizeof(Dev) <= 4096, "k_spg_search's arguments");
static_assert(sizeof(SPGTrain) + 2 * sizeof(Net) <= 4096, "k_spg_tail's arguments");
static_assert(AIGAR_SPG_MAX_SAMPLES == kSpgMaxSamples, "the header's limit is spg.inc's");
static_assert(sizeof(aigar_spg_params) == 128, "aigar_spg_params is part of the ABI");

extern "C" int aigar_spg_config(aigar_handle *h, const aigar_spg_params *p) {
  const char *who = "spg_config";
  if (p) {
    if (check_qsa_sizes(who, p)) return -1;
    if (p->samples < 0 || p->samples > AIGAR_SPG_MAX_SAMPLES)
      return fail("spg_config: samples = %d is outside 0..%d", p->samples, AIGAR_SPG_MAX_SAMPLES);
    if (p->moving != 0 && p->moving != 1) return fail("spg_config: moving = %d must be 0 or 1", p->moving);
    if (p->replace != 0 && p->replace != 1) return fail("spg_config: replace = %d must be 0 or 1", p->replace);
    if (p->prio_evals != 0 && p->prio_evals != 1) return fail("spg_config: prio_evals = %d must be 0 or 1", p->prio_evals);
    if (p->fused != 0 && p->fused != 1) return fail("spg_config: fused = %d must be 0 or 1", p->fused);
    if (p->pad != 0) return fail("spg_config: pad = %d must be 0", p->pad);
    if (check_qsa_rates(who, p)) return -1;
    if (!(p->noise >= 0 && p->noise < __builtin_inf())) return fail("spg_config: noise = %g must be finite and not negative", p->noise);
    if (!(p->noise_decay > 0 && p->noise_decay <= 1)) return fail("spg_config: noise_decay = %g is outside (0, 1]", p->noise_decay);
  }
  if (!h) return fail("null handle");
  if (p) {
    if (check_qsa_handle(h, who, "SPG")) return -1;
    if (p->replace && !h->exp.x) return fail("spg_config: replace needs a replay memory with the extra field (AIGAR_EXP_EXTRA)");
    if (check_train_widths(h, who)) return -1;
  }
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (p || h->spg.d.batch) trainer_free(h);  // (a null p turns off this trainer, not another)
  if (!p) return 0;
  bool ok = true;
  SPGTrain sp;
  sp.d = qsa_setup(h, ok, p, false);
  sp.K = p->samples;
  sp.moving = p->moving;
  sp.replace = p->replace;
  sp.prio_evals = p->prio_evals;
  sp.fused = p->fused;
  sp.noise0 = p->noise;
  sp.noise_decay = p->noise_decay;
  sp.seed = p->seed;
  const size_t B = (size_t)p->batch;
  sp.ex = (double *)train_get(h, ok, B * 4 * sizeof(double));
  sp.exv = (uint8_t *)train_get(h, ok, B);
  sp.best = (double *)train_get(h, ok, B * 4 * sizeof(double));
  sp.cand = (double *)train_get(h, ok, B * 4 * sizeof(double));
  sp.rows = (double *)train_get(h, ok, B * 4 * sizeof(double));
  sp.beval = (double *)train_get(h, ok, B * sizeof(double));
  sp.qmu = (double *)train_get(h, ok, B * sizeof(double));
  sp.zu = (double *)train_get(h, ok, B * (size_t)std::max(sp.K, 1) * 2 * kNoiseMaxT * 2 * sizeof(double));
  sp.x = (SCtl *)train_get(h, ok, sizeof(SCtl));
  if (!ok) {
    h->trn_mem.release();
    return fail("spg_config: out of device memory");
  }
  hipLaunchKernelGGL(k_spg_clear, dim3(1), dim3(1), 0, h->stream, sp.d.c.ctl, sp.d.a.ctl, sp.x, sp.noise0, 1);
  HIPCHK(hipGetLastError());
  h->spg = sp;  // (the blocks are zeroed: every counter starts at 0)
  return 0;
}

// One SPG training step's launches on stream s (spg.inc), one linear chain: DPG's critic half, then
// the search and the actor's update towards what it found.  has: has_u | has_zu << 1.
static void launch_spg_step(aigar_handle *h, hipStream_t s, int has) {
  const SPGTrain &sp = h->spg;
  const DPGTrain &t = sp.d;
  const Train &c = t.c, &a = t.a;
  const Exp &e = h->exp;
  Net cr = h->crit, ac = h->net;
  cr.x_dtype = ac.x_dtype = e.dtype;
  const int B = t.batch, has_u = has & 1, has_zu = has >> 1 & 1;
  const bool extras = sp.replace && sp.K > 0;
  launch_draw_fetch(h, s, a, has_u);
  if (extras)
    hipLaunchKernelGGL(k_exp_extra_get, dim3((unsigned)(((size_t)B * 4 + 255) / 256)), dim3(256), 0, s, e, a.idx, B, sp.ex,
                       sp.exv);
  launch_qsa_critic(h, s, t, cr, target_net(cr, c), target_net(ac, a), sp.prio_evals);
  // the search
  launch_net_save(s, ac, B, a.s, a.q, a.hsave);
  if (sp.fused) {  // the whole search in one launch, 16 rows a block
    const dim3 grid((unsigned)(c.bpad / kNetRows)), block(64 * kNetWaves);
    const int nt0 = (net_out_pad(cr.out[0]) / 16 + kNetWaves - 1) / kNetWaves;
#define AIGAR_SPG_SEARCH(T, NT) hipLaunchKernelGGL((k_spg_search<T, NT>), grid, block, 0, s, cr, sp, h->d, has_zu)
    if (e.dtype == 0) {
      if (nt0 == 1) AIGAR_SPG_SEARCH(double, 1);
      else if (nt0 == 2) AIGAR_SPG_SEARCH(double, 2);
      else if (nt0 == 3) AIGAR_SPG_SEARCH(double, 3);
      else AIGAR_SPG_SEARCH(double, 4);
    } else {
      if (nt0 == 1) AIGAR_SPG_SEARCH(float, 1);
      else if (nt0 == 2) AIGAR_SPG_SEARCH(float, 2);
      else if (nt0 == 3) AIGAR_SPG_SEARCH(float, 3);
      else AIGAR_SPG_SEARCH(float, 4);
    }
#undef AIGAR_SPG_SEARCH
  } else {
    launch_sa_pack(s, t, e.dtype, extras ? 2 : 1, a.s, a.q, t.n_act, t.xm, a.s, sp.ex, 4, t.xt);
    launch_net(s, cr, t.xm, B, sp.qmu, nullptr, nullptr);
    if (extras) launch_net(s, cr, t.xt, B, t.qt, nullptr, nullptr);
    hipLaunchKernelGGL(k_spg_pick, dim3(1), dim3(kTrainMaxBatch), 0, s, sp, 1);
    for (int x = 0; x < sp.K; x++) {
      if (e.dtype == 0) hipLaunchKernelGGL(k_spg_cand<double>, dim3(B), dim3(64), 0, s, sp, h->d, x, has_zu);
      else hipLaunchKernelGGL(k_spg_cand<float>, dim3(B), dim3(64), 0, s, sp, h->d, x, has_zu);
      launch_net(s, cr, t.xm, B, t.qm, nullptr, nullptr);
      hipLaunchKernelGGL(k_spg_pick, dim3(1), dim3(kTrainMaxBatch), 0, s, sp, 0);
    }
  }
  // the actor half
  hipLaunchKernelGGL(k_spg_delta, dim3(1), dim3(kTrainMaxBatch), 0, s, sp, h->d, ac.n_layers, t.n_act);
  launch_net_update(s, ac, a);
  if (sp.replace) hipLaunchKernelGGL(k_spg_writeback, dim3(1), dim3(kExpPlanThreads), 0, s, sp, e);
  hipLaunchKernelGGL(k_spg_tail, dim3(64), dim3(256), 0, s, cr, ac, sp);
}

extern "C" int aigar_spg_step(aigar_handle *h, int n_steps, const double *u, const double *zu) {
  if (need_spg(h, "spg_step")) return -1;
  const SPGTrain &sp = h->spg;
  if (sp.K == 0) zu = nullptr;  // (no sample is drawn)
  return trainer_step(h, "spg_step", kTrainSpg, n_steps, u, sp.d.a, launch_spg_step, zu, sp.zu,
                      (size_t)sp.d.batch * sp.K * 2 * kNoiseMaxT * 2);
}

extern "C" int aigar_spg_info(aigar_handle *h, int64_t info[8]) {
  if (need_spg(h, "spg_info")) return -1;
  if (!info) return fail("spg_info: null argument");
  TrainCtl c, a;
  SCtl x;
  if (read_ctls(h, {{&c, h->spg.d.c.ctl, sizeof c}, {&a, h->spg.d.a.ctl, sizeof a}, {&x, h->spg.x, sizeof x}})) return -1;
  info[0] = c.t;
  info[1] = c.skipped;
  info[2] = c.since;
  info[3] = a.t;
  info[4] = a.skipped;
  info[5] = x.aempty;
  info[6] = x.sel;
  info[7] = 0;
  return 0;
}

extern "C" int aigar_spg_td(aigar_handle *h, double *td, int64_t *idx) {
  if (need_spg(h, "spg_td")) return -1;
  return trainer_td(h, h->spg.d.c, td, idx);
}

extern "C" int aigar_spg_noise(aigar_handle *h, double **dev) {
  if (need_spg(h, "spg_noise")) return -1;
  if (!dev) return fail("spg_noise: null argument");
  *dev = &h->spg.x->noise;
  return 0;
}

extern "C" int aigar_spg_sync_target(aigar_handle *h) {
  if (need_spg(h, "spg_sync_target")) return -1;
  return qsa_sync_target(h, h->spg.d);
}

extern "C" int aigar_spg_reset(aigar_handle *h) {
  if (need_spg(h, "spg_reset")) return -1;
  const SPGTrain &sp = h->spg;
  if (qsa_adam_clear(h, sp.d)) return -1;
  hipLaunchKernelGGL(k_spg_clear, dim3(1), dim3(1), 0, h->stream, sp.d.c.ctl, sp.d.a.ctl, sp.x, sp.noise0, 0);
  HIPCHK(hipGetLastError());
  return 0;
}

// The configured Q(s, a) trainer's DPGTrain, DPG's or SPG's, or null
static const DPGTrain *qsa_train(const aigar_handle *h) {
  return h->dpg.batch ? &h->dpg : h->spg.d.batch ? &h->spg.d : nullptr;
}
// The configured trainer's view of the acting network, or (crit) of the critic.
static const Train &trainer_view(const aigar_handle *h, bool crit) {
  if (const DPGTrain *t = qsa_train(h)) return crit ? t->c : t->a;
  if (h->act.batch) return crit ? h->act.c : h->act.a;
  return h->trn;
}

// which: 0 online, 1 target, 2 Adam's m, 3 Adam's v (the last three need a train configuration)
// 4 the critic (needs only a critic), 5 its target, 6 / 7 its Adam state (an actrain configuration,
// under which 2 / 3 are the actor's Adam state and 1 is refused; or a DPG configuration, under
// which 1 is the actor's target too).  *np: the network whose shape it has.
static int net_which(aigar_handle *h, const char *who, int which, int layer, const Net **np, const float **wp,
                     const float **bp) {
  if (need_net(h, who)) return -1;
  if (which < 0 || which > 7) return fail("%s: which = %d is outside 0..7", who, which);
  const bool crit = which >= 4;
  if (crit && !h->crit.n_layers) return fail("%s: no critic is configured (aigar_critic_config)", who);
  const Net &c = crit ? h->crit : h->net;
  if (layer < 0 || layer >= c.n_layers) return fail("%s: layer %d is outside 0..%d", who, layer, c.n_layers - 1);
  const bool dpg = qsa_train(h) != nullptr;  // (an SPG configuration serves the codes as DPG's does)
  if (which == 1 && h->act.batch) return fail("%s: which = 1: CACLA keeps no actor target", who);
  if (which > 4 && !dpg && need_act(h, who)) return -1;
  if (which >= 1 && which <= 3 && !dpg && !h->act.batch && need_trn(h, who)) return -1;
  const Train &t = trainer_view(h, crit);
  const int k = which & 3;
  *np = &c;
  *wp = k == 0 ? c.w[layer] : k == 1 ? t.tw[layer] : k == 2 ? t.mw[layer] : t.vw[layer];
  *bp = k == 0 ? c.b[layer] : k == 1 ? t.tb[layer] : k == 2 ? t.mb[layer] : t.vb[layer];
  return 0;
}

extern "C" int aigar_net_get_weights(aigar_handle *h, int which, int layer, float *W, float *b, int on_device) {
  const float *wp, *bp;
  const Net *np;
  if (net_which(h, "net_get_weights", which, layer, &np, &wp, &bp)) return -1;
  if (!W || !b) return fail("net_get_weights: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int in = np->in[layer], out = np->out[layer];
  const size_t nw = (size_t)in * out;
  float *stage = which >= 4 ? h->crit_stage : h->net_stage;
  float *dW = on_device ? W : stage, *db = on_device ? b : stage + nw;
  hipLaunchKernelGGL(k_net_unpack, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 4096)), dim3(256), 0, h->stream, wp, bp,
                     dW, db, in, out, net_out_pad(out));
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(W, dW, nw * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(b, db, (size_t)out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// The conv part's read-back: which 0 online, 1 target, 2 Adam's m, 3 Adam's v (the last three need
// aigar_train_config_cnn); W [k][k][cin][F], b [F] in Keras' layout.
static int conv_which(aigar_handle *h, const char *who, int which, int layer, const float **wp, const float **bp) {
  if (need_net(h, who)) return -1;
  const Conv &c = h->conv;
  if (!c.n_conv) return fail("%s: the network has no conv part (aigar_net_config_cnn)", who);
  if (which < 0 || which > 3) return fail("%s: which = %d is outside 0..3", who, which);
  if (layer < 0 || layer >= c.n_conv) return fail("%s: layer %d is outside 0..%d", who, layer, c.n_conv - 1);
  if (which && !h->ctrn.on) return fail("%s: no CNN training is configured (aigar_train_config_cnn)", who);
  const ConvTrain &t = h->ctrn;
  *wp = which == 0 ? c.w[layer] : which == 1 ? t.tw[layer] : which == 2 ? t.mw[layer] : t.vw[layer];
  *bp = which == 0 ? c.b[layer] : which == 1 ? t.tb[layer] : which == 2 ? t.mb[layer] : t.vb[layer];
  return 0;
}

extern "C" int aigar_net_get_conv_weights(aigar_handle *h, int which, int layer, float *W, float *b, int on_device) {
  const float *wp, *bp;
  if (conv_which(h, "net_get_conv_weights", which, layer, &wp, &bp)) return -1;
  if (!W || !b) return fail("net_get_conv_weights: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  const Conv &c = h->conv;
  const int K = c.k[layer] * c.k[layer] * (layer ? c.filters[layer - 1] : c.channels), F = c.filters[layer];
  const size_t nw = (size_t)K * F;
  float *dW = on_device ? W : h->conv_stage, *db = on_device ? b : h->conv_stage + nw;
  hipLaunchKernelGGL(k_conv_unpack, dim3((unsigned)std::min<size_t>((nw + 255) / 256, 4096)), dim3(256), 0, h->stream, wp, bp,
                     dW, db, K, F, net_out_pad(F));
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(W, dW, nw * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(b, db, (size_t)F * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int aigar_net_pad_check(aigar_handle *h, int which, int64_t *count) {
  const float *wp, *bp;
  const Net *np;
  if (net_which(h, "net_pad_check", which, 0, &np, &wp, &bp)) return -1;
  if (!count) return fail("net_pad_check: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  unsigned long long *dc = nullptr, n = 0;
  HIPCHK(hipMalloc((void **)&dc, sizeof n));
  hipError_t er = hipMemsetAsync(dc, 0, sizeof n, h->stream);
  for (int l = 0; l < np->n_layers && er == hipSuccess; l++) {
    (void)net_which(h, "net_pad_check", which, l, &np, &wp, &bp);
    const int in = np->in[l], out = np->out[l], ip = net_in_pad(in), op = net_out_pad(out);
    hipLaunchKernelGGL(k_net_pad_count, dim3((unsigned)std::min<size_t>(((size_t)ip * op + 255) / 256, 4096)), dim3(256), 0,
                       h->stream, wp, bp, in, out, ip, op, dc);
    er = hipGetLastError();
  }
  // the conv part's copies of the acting network: the same code's (1 .. 3: under aigar_train_config_cnn)
  for (int l = 0; which < 4 && (which == 0 || h->ctrn.on) && l < h->conv.n_conv && er == hipSuccess; l++) {
    const float *cw, *cb;
    (void)conv_which(h, "net_pad_check", which, l, &cw, &cb);
    const Conv &c = h->conv;
    const int K = c.k[l] * c.k[l] * (l ? c.filters[l - 1] : c.channels), F = c.filters[l], Kp = conv_k_pad(K), Fp = net_out_pad(F);
    hipLaunchKernelGGL(k_net_pad_count, dim3((unsigned)std::min<size_t>(((size_t)Kp * Fp + 255) / 256, 4096)), dim3(256), 0,
                       h->stream, cw, cb, K, F, Kp, Fp, dc);
    er = hipGetLastError();
  }
  if (er == hipSuccess) er = hipMemcpyAsync(&n, dc, sizeof n, hipMemcpyDeviceToHost, h->stream);
  if (er == hipSuccess) er = hipStreamSynchronize(h->stream);
  (void)hipFree(dc);
  if (er != hipSuccess) return fail("net_pad_check: %s", hipGetErrorString(er));
  *count = (int64_t)n;
  return 0;
}

extern "C" int aigar_pixel_state_len(aigar_handle *h) {
  return h ? h->pix.side * h->pix.side * (h->pix.side ? pix_channels(h->pix) : 0) : -1;
}

extern "C" int aigar_observe_pixel_state(aigar_handle *h, void *out, int dtype, int on_device, const uint8_t *mask,
                                         int mask_on_device) {
  if (!h || !out) return fail("null argument");
  if (!h->pix.side) return fail("observe_pixel_state: no pixel state is configured (aigar_pixel_config)");
  if (dtype != 0 && dtype != 1) return fail("dtype must be 0 (float64) or 1 (float32)");
  if (on_device && ((uintptr_t)out & 15)) return fail("observe_pixel_state: a device out must be 16-byte aligned");
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t bytes = (size_t)h->d.NP * aigar_pixel_state_len(h) * (dtype == 0 ? 8 : 4);
  void *dst = out;
  if (!on_device) {
    if (bytes > h->pix_bytes) {
      if (h->d_pix) HIPCHK(hipFree(h->d_pix));
      h->d_pix = nullptr;
      h->pix_bytes = 0;
      HIPCHK(hipMalloc(&h->d_pix, bytes));
      h->pix_bytes = bytes;
    }
    dst = h->d_pix;
  }
  const uint8_t *m = mask;
  if (mask && !mask_on_device) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->d.NP, hipMemcpyHostToDevice, h->stream));
    m = h->d_mask;
  }
  if (!on_device && mask)  // rows of masked-out bots are left as the caller's buffer has them
    HIPCHK(hipMemcpyAsync(h->d_pix, out, bytes, hipMemcpyHostToDevice, h->stream));
  {
    Mark mk(h, "observe_pixel_state");
    if (launch_observe_pixel_state(h->d, h->stream, dst, dtype, h->pix.side, h->pix.flags, h->pix.color_seed,
                                   h->d_pix_ovf, m, h->d_pix_hist))
      return fail("bad pixel state launch");
    if (h->exp.cap) launch_exp_latch(h, h->stream, dst, dtype, m);
  }
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(out, h->d_pix, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return check_device_errors(h);
  }
  if (mask && !mask_on_device) HIPCHK(hipStreamSynchronize(h->stream));  // caller may reuse its mask
  return 0;
}

__global__ void k_set_actions(Dev d, const double *cur, const double *prev) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)d.NP * 4) return;
  if (cur) d.o_act_cur[i] = cur[i];
  if (prev) d.o_act_prev[i] = prev[i];
}

extern "C" int aigar_set_actions(aigar_handle *h, const double *cur, const double *prev, int on_device) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  size_t n = (size_t)h->d.NP * 4;
  if (on_device) {
    hipLaunchKernelGGL(k_set_actions, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d, cur, prev);
  } else {
    if (cur) HIPCHK(hipMemcpyAsync(h->d.o_act_cur, cur, n * 8, hipMemcpyHostToDevice, h->stream));
    if (prev) HIPCHK(hipMemcpyAsync(h->d.o_act_prev, prev, n * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// Bot.reset (bot.py:125-164) for the masked players: an NN bot's last /
// second-last self and enemy grids restart at zero and fovSize / lastFovSize at
// 0 (the collector calls model.resetBots() every FRAME_SKIP_RATE + 2 updates,
// aigar.py:845-852).  C4: every tile's copy is then current (all zero).
__global__ void k_reset_bots(Dev d, const uint8_t *mask) {
  const int GG = d.G * d.G;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= (size_t)d.NP * GG) return;
  const int gp = (int)(i / GG);
  if (mask && !mask[gp]) return;
  d.o_self_lf[i] = d.o_self_slf[i] = d.o_en_lf[i] = d.o_en_slf[i] = 0.0;
  if (i % GG == 0) {
    d.o_lastfov[gp] = 0.0;
    if (d.tiled) d.t_holder[gp] = -1;
  }
}

extern "C" int aigar_reset_bots(aigar_handle *h, const uint8_t *mask, int on_device) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const uint8_t *m = mask;
  if (mask && !on_device) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->d.NP, hipMemcpyHostToDevice, h->stream));
    m = h->d_mask;
  }
  const size_t n = (size_t)h->d.NP * h->d.G * h->d.G;
  hipLaunchKernelGGL(k_reset_bots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d, m);
  if (h->d_pix_hist) {
    const size_t LL = (size_t)h->pix.side * h->pix.side, np = LL * h->d.NP;
    hipLaunchKernelGGL(k_pix_hist_clear_bots, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, h->stream,
                       h->d_pix_hist, LL, np, m);
  }
  if (h->exp.cap)  // Bot.reset: oldState = None (bot.py:186)
    hipLaunchKernelGGL(k_exp_clear_bots, dim3((h->d.NP + 255) / 256), dim3(256), 0, h->stream, h->exp.has_old, h->d.NP, m);
  if (h->noi.n_act)  // the Orn-Uhl state restarts with the bot (actorCritic.py:1121-1123)
    hipLaunchKernelGGL(k_noise_clear_bots, dim3((h->d.NP + 255) / 256), dim3(256), 0, h->stream, h->noi.ou, h->d.NP,
                       h->noi.n_act, m);
  HIPCHK(hipGetLastError());
  if (mask && !on_device) HIPCHK(hipStreamSynchronize(h->stream));  // caller may reuse its buffer
  return 0;
}

extern "C" int aigar_player_stats(aigar_handle *h, double *out, int on_device) {
  if (!h || !out) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_player_stats(h->d, h->stream, on_device ? out : h->d_stats);
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(out, h->d_stats, sizeof(double) * 5 * h->d.NP, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

// ---- AIGAR_FLAG_SCORE: the bots' mass history (k_score_sample, the first launch of every tick)
static int need_score(aigar_handle *h, const char *who) {
  if (!h) return fail("null handle");
  if (!h->d.sc) return fail("%s: the handle keeps no score (create it with AIGAR_FLAG_SCORE in aigar_config.flags)", who);
  return 0;
}
extern "C" int aigar_score(aigar_handle *h, double *out, int on_device) {
  if (need_score(h, "aigar_score")) return -1;
  if (!out) return fail("aigar_score: null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_score_read(h->d, h->stream, on_device ? out : h->d_score);
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(out, h->d_score, sizeof(double) * 4 * h->d.NP, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}
extern "C" int aigar_score_reset(aigar_handle *h, const uint8_t *mask, int on_device) {
  if (need_score(h, "aigar_score_reset")) return -1;
  HIPCHK(hipSetDevice(h->cfg.device));
  const uint8_t *m = mask;
  if (mask && !on_device) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->d.NP, hipMemcpyHostToDevice, h->stream));
    m = h->d_mask;
  }
  launch_score_reset(h->d, h->stream, m);
  HIPCHK(hipGetLastError());
  if (mask && !on_device) HIPCHK(hipStreamSynchronize(h->stream));  // caller may reuse its buffer
  return 0;
}
extern "C" int aigar_score_trace(aigar_handle *h, double *buf, int64_t cap) {
  if (need_score(h, "aigar_score_trace")) return -1;
  if (buf && cap < 0) return fail("aigar_score_trace: cap = %lld is negative", (long long)cap);
  HIPCHK(hipSetDevice(h->cfg.device));
  launch_score_trace(h->d, h->stream, buf, cap);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int aigar_set_stream(aigar_handle *h, void *s) {
  if (!h) return fail("null handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  h->stream = (hipStream_t)s;
  h->own_stream = false;
  return 0;
}

extern "C" int aigar_sync(aigar_handle *h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  return check_device_errors(h);
}

// diagnostics: the first list row (the slot of every player's first cell) and
// the cell counts, [NP] bytes and [NP] ints (tools/first_slot.py)
extern "C" int aigar_debug_first_slots(aigar_handle *h, uint8_t *slot0, int *ncells) {
  if (!h || !slot0 || !ncells) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(slot0, h->d.p_list, h->d.NP, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ncells, h->d.p_ncells, sizeof(int) * h->d.NP, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int aigar_profile(aigar_handle *h, int enable) {
  if (!h) return fail("null handle");
  HIPCHK(hipStreamSynchronize(h->stream));
  for (auto &m : h->marks) {
    h->event_pool.push_back(m.second.first);
    h->event_pool.push_back(m.second.second);
  }
  h->marks.clear();
  h->profile = enable != 0;
  return 0;
}
// total HIP-event time (ms) and launch count of a timer since aigar_profile(h, 1):
// "tick" (one Field.update), "observe" (k_observe), "policy" (k_policy_random)
extern "C" int aigar_kernel_time(aigar_handle *h, const char *name, double *ms, int *launches) {
  if (!h || !name || !ms || !launches) return fail("null argument");
  HIPCHK(hipStreamSynchronize(h->stream));
  double tot = 0;
  int n = 0;
  for (auto &m : h->marks) {
    if (m.first != name) continue;
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, m.second.first, m.second.second));
    tot += t;
    n++;
  }
  *ms = tot;
  *launches = n;
  return 0;
}

// ---------------------------------------------------------------- snapshots
template <class T>
static int d2h(aigar_handle *h, std::vector<T> &v, const T *src, size_t n) {
  v.resize(n);
  if (n) HIPCHK(hipMemcpyAsync(v.data(), src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return 0;
}
template <class T>
static int h2d(aigar_handle *h, T *dst, const std::vector<T> &v) {
  if (!v.empty()) HIPCHK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return 0;
}

extern "C" int aigar_get_state(aigar_handle *h, int arena, aigar_state *st) {
  if (!h || !st) return fail("null argument");
  Dev &d = h->d;
  if (arena < 0 || arena >= d.A) return fail("arena %d out of range", arena);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (check_device_errors(h)) return -1;
  ArenaCtl c;
  HIPCHK(hipMemcpy(&c, d.ctl + arena, sizeof c, hipMemcpyDeviceToHost));
  const int B = d.B, NP = d.NP;
  const size_t p0 = (size_t)arena * B;
  std::vector<int> alive, resp, ncells, split, eject, dead;
  std::vector<double> cmdx, cmdy;
  if (d2h(h, alive, d.p_alive + p0, B) || d2h(h, resp, d.p_respawn + p0, B) || d2h(h, ncells, d.p_ncells + p0, B) ||
      d2h(h, split, d.p_split + p0, B) || d2h(h, eject, d.p_eject + p0, B) || d2h(h, cmdx, d.p_cmdx + p0, B) ||
      d2h(h, cmdy, d.p_cmdy + p0, B) || d2h(h, dead, d.dead + p0, c.n_dead))
    return -1;
  // cells: 16 slot rows of this arena's players
  std::vector<uint8_t> lst((size_t)kMaxCells * B);
  std::vector<double> cf[9];
  std::vector<int> csvc((size_t)kMaxCells * B);
  std::vector<uint32_t> cfl((size_t)kMaxCells * B);
  std::vector<int64_t> cseq((size_t)kMaxCells * B);
  double *cfs[9] = {d.c_x, d.c_y, d.c_m, d.c_r, d.c_vx, d.c_vy, d.c_svx, d.c_svy, d.c_mt};
  for (int f = 0; f < 9; f++) cf[f].resize((size_t)kMaxCells * B);
  for (int s = 0; s < kMaxCells; s++) {
    size_t o = (size_t)s * NP + p0, ho = (size_t)s * B;
    HIPCHK(hipMemcpyAsync(lst.data() + ho, d.p_list + o, B, hipMemcpyDeviceToHost, h->stream));
    for (int f = 0; f < 9; f++)
      HIPCHK(hipMemcpyAsync(cf[f].data() + ho, cfs[f] + o, 8 * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(csvc.data() + ho, d.c_svc + o, 4 * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cfl.data() + ho, d.c_flags + o, 4 * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cseq.data() + ho, d.c_seq + o, 8 * B, hipMemcpyDeviceToHost, h->stream));
  }
  const size_t po = (size_t)arena * d.PS, bo = (size_t)arena * d.Ecap, vo = (size_t)arena * d.Vcap;
  std::vector<double> px, py, pm, bf[8], vf[8];
  std::vector<int64_t> ps, bseq, bej, vseq;
  std::vector<int> bsvc, vsvc, pcol, bcol;
  std::vector<uint32_t> bfl, vfl;
  int n_pel = 0;
  {  // the row store: each row's live records [entry 0, entry cols) of its current home,
     // packed on the device (k_pel_gather) so only the live records are copied
    std::vector<int> pst;
    std::vector<PelRec> store;
    std::vector<int> scol;
    if (d2h(h, pst, d.pstart + (size_t)arena * d.PH1, d.PH1)) return -1;
    HIPCHK(hipStreamSynchronize(h->stream));
    long tot = 0;
    for (int r = 0; r < d.cols; r++) tot += pst[(size_t)r * (d.cols + 1) + d.cols] - pst[(size_t)r * (d.cols + 1)];
    if (tot > d.Pcap) return fail("get_state: %ld live pellet records exceed the capacity %d", tot, d.Pcap);
    launch_pel_gather(d, h->stream, arena);
    HIPCHK(hipGetLastError());
    if (d2h(h, store, d.pn + (size_t)arena * d.Pcap, (int)tot) || d2h(h, scol, d.pn_col + (size_t)arena * d.Pcap, (int)tot))
      return -1;
    HIPCHK(hipStreamSynchronize(h->stream));  // (unpacked below)
    for (long i = 0; i < tot; i++) {
      px.push_back(store[i].x); py.push_back(store[i].y); pm.push_back(store[i].m); ps.push_back(store[i].seq);
      pcol.push_back(scol[i]);
    }
    n_pel = (int)px.size();
  }
  double *bfs[8] = {d.b_x, d.b_y, d.b_m, d.b_r, d.b_vx, d.b_vy, d.b_svx, d.b_svy};
  double *vfs[8] = {d.v_x, d.v_y, d.v_m, d.v_r, d.v_vx, d.v_vy, d.v_svx, d.v_svy};
  for (int f = 0; f < 8; f++)
    if (d2h(h, bf[f], bfs[f] + bo, c.n_blob) || d2h(h, vf[f], vfs[f] + vo, c.n_vir)) return -1;
  if (d2h(h, bsvc, d.b_svc + bo, c.n_blob) || d2h(h, bseq, d.b_seq + bo, c.n_blob) ||
      d2h(h, bej, d.b_ej + bo, c.n_blob) || d2h(h, bfl, d.b_flags + bo, c.n_blob) || d2h(h, bcol, d.b_col + bo, c.n_blob) ||
      d2h(h, vsvc, d.v_svc + vo, c.n_vir) || d2h(h, vseq, d.v_seq + vo, c.n_vir) ||
      d2h(h, vfl, d.v_flags + vo, c.n_vir))
    return -1;
  HIPCHK(hipStreamSynchronize(h->stream));

  int nc = 0;
  for (int p = 0; p < B; p++) nc += ncells[p];
  std::vector<int> bl, vl;
  for (int i = 0; i < c.n_blob; i++)
    if (bfl[i] & F_ALIVE) bl.push_back(i);
  for (int i = 0; i < c.n_vir; i++)
    if (vfl[i] & F_ALIVE) vl.push_back(i);
  std::sort(bl.begin(), bl.end(), [&](int x, int y) { return bseq[x] < bseq[y]; });
  std::sort(vl.begin(), vl.end(), [&](int x, int y) { return vseq[x] < vseq[y]; });
  std::vector<int> pord;
  for (int i = 0; i < n_pel; i++) {
    const int bx = std::min(d.cols - 1, std::max(0, (int)(px[i] / kBucket)));
    const int by = std::min(d.cols - 1, std::max(0, (int)(py[i] / kBucket)));
    if (bx >= d.own_bx0 && bx < d.own_bx1 && by >= d.own_by0 && by < d.own_by1) pord.push_back(i);  // (tiles: owned)
  }
  std::sort(pord.begin(), pord.end(), [&](int x, int y) { return ps[x] < ps[y]; });
  int caps[5] = {st->n_cells, st->n_pellets, st->n_blobs, st->n_viruses, st->n_dead};
  st->n_players = B;
  st->field_size = d.size;
  st->virus_enabled = d.virus_enabled;
  st->rng_mode = AIGAR_RNG_PHILOX;
  st->seq_next = c.seq_next;
  st->tick = c.tick;
  st->max_pellets = d.max_pellets;
  st->max_viruses = d.max_viruses;
  st->philox_key[0] = c.key0;
  st->philox_key[1] = c.key1;
  st->ctr_pellet = c.ctr_pellet;
  st->ctr_virus = c.ctr_virus;
  memset(st->mt_key, 0, sizeof st->mt_key);
  st->mt_pos = 0;
  st->n_cells = nc;
  st->n_pellets = (int)pord.size();
  st->n_blobs = (int)bl.size();
  st->n_viruses = (int)vl.size();
  st->n_dead = c.n_dead;
  if (!st->cells_f) return 0;
  if (caps[0] < nc || caps[1] < (int)pord.size() || caps[2] < (int)bl.size() || caps[3] < (int)vl.size() || caps[4] < c.n_dead)
    return fail("get_state: caller arrays too small");
  for (int p = 0; p < B; p++) {
    st->players_f[2 * p] = cmdx[p];
    st->players_f[2 * p + 1] = cmdy[p];
    int64_t *q = st->players_i + 5 * p;
    q[0] = alive[p]; q[1] = resp[p]; q[2] = split[p]; q[3] = eject[p]; q[4] = ncells[p];
  }
  int k = 0;
  for (int p = 0; p < B; p++)
    for (int j = 0; j < ncells[p]; j++, k++) {
      size_t hi = (size_t)lst[(size_t)j * B + p] * B + p;
      for (int f = 0; f < 9; f++) st->cells_f[9 * k + f] = cf[f][hi];
      int64_t *q = st->cells_i + 4 * k;
      q[0] = p; q[1] = csvc[hi]; q[2] = cseq[hi]; q[3] = (cfl[hi] & F_INHASH) ? 1 : 0;
    }
  for (size_t i = 0; i < pord.size(); i++) {
    int j = pord[i];
    double *f = st->pellets_f + 4 * i;
    f[0] = px[j]; f[1] = py[j]; f[2] = pm[j]; f[3] = pm[j] > 0 ? std::sqrt(pm[j] / 3.141592653589793) : 0.0;
    st->pellets_seq[i] = ps[j];
    if (st->pellets_col) st->pellets_col[i] = pcol[j];
  }
  for (size_t i = 0; i < bl.size(); i++) {
    int j = bl[i];
    for (int f = 0; f < 8; f++) st->blobs_f[8 * i + f] = bf[f][j];
    st->blobs_i[3 * i] = bsvc[j]; st->blobs_i[3 * i + 1] = bseq[j]; st->blobs_i[3 * i + 2] = bej[j];
    if (st->blobs_col) st->blobs_col[i] = bcol[j];
  }
  for (size_t i = 0; i < vl.size(); i++) {
    int j = vl[i];
    for (int f = 0; f < 8; f++) st->viruses_f[8 * i + f] = vf[f][j];
    st->viruses_i[3 * i] = vsvc[j]; st->viruses_i[3 * i + 1] = vseq[j];
    st->viruses_i[3 * i + 2] = (vfl[j] & F_INHASH) ? 1 : 0;
  }
  for (int i = 0; i < c.n_dead; i++) st->dead[i] = dead[i];
  return 0;
}

// counting sort of items by centre bucket (host side, used by load_state)
static void host_grid(int cols, const std::vector<double> &x, const std::vector<double> &y, std::vector<int> &start,
                      std::vector<int> &order, int shift = 0) {
  const int cc = (cols + (1 << shift) - 1) >> shift;
  int H = cc * cc;
  start.assign(H + 1, 0);
  std::vector<int> b(x.size());
  for (size_t i = 0; i < x.size(); i++) {
    auto cb = [&](double v) {
      int q = (int)(v / 20);
      if (v < 0) q = 0;
      return (q < cols ? q : cols - 1) >> shift;
    };
    b[i] = cb(y[i]) * cc + cb(x[i]);
    start[b[i] + 1]++;
  }
  for (int i = 0; i < H; i++) start[i + 1] += start[i];
  std::vector<int> cur(start.begin(), start.end() - 1);
  order.assign(x.size(), 0);
  for (size_t i = 0; i < x.size(); i++) order[cur[b[i]]++] = (int)i;
}

extern "C" int aigar_load_state(aigar_handle *h, int arena, const aigar_state *st) {
  if (!h || !st) return fail("null argument");
  Dev &d = h->d;
  if (arena < 0 || arena >= d.A) return fail("arena %d out of range", arena);
  if (st->n_players != d.B) return fail("load_state: n_players %d != bots_per_arena %d", st->n_players, d.B);
  if (st->field_size != d.size) return fail("load_state: field_size %d != %d", st->field_size, d.size);
  if (!!st->virus_enabled != !!d.virus_enabled) return fail("load_state: virus_enabled mismatch");
  if (st->n_pellets > d.Pcap || st->n_blobs > d.Ecap || st->n_viruses > d.Vcap)
    return fail("load_state: snapshot exceeds capacities (pellets %d/%d blobs %d/%d viruses %d/%d)", st->n_pellets,
                d.Pcap, st->n_blobs, d.Ecap, st->n_viruses, d.Vcap);
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int B = d.B, NP = d.NP;
  const size_t p0 = (size_t)arena * B;
  std::vector<int> alive(B), resp(B), ncells(B, 0), split(B), eject(B), dead(st->n_dead);
  std::vector<double> cmdx(B), cmdy(B);
  for (int p = 0; p < B; p++) {
    cmdx[p] = st->players_f[2 * p];
    cmdy[p] = st->players_f[2 * p + 1];
    const int64_t *q = st->players_i + 5 * p;
    alive[p] = (int)q[0]; resp[p] = (int)q[1]; split[p] = (int)q[2]; eject[p] = (int)q[3];
  }
  const size_t CB = (size_t)kMaxCells * B;
  std::vector<uint8_t> lst(CB, 0);
  std::vector<double> cf[9];
  for (int f = 0; f < 9; f++) cf[f].assign(CB, 0.0);
  std::vector<int> csvc(CB, 0);
  std::vector<uint32_t> cfl(CB, 0);
  std::vector<int64_t> cseq(CB, 0);
  std::vector<double> gx, gy;
  std::vector<int> gid;
  double rmax_c = 0;
  for (int k = 0; k < st->n_cells; k++) {
    const int64_t *q = st->cells_i + 4 * k;
    int p = (int)q[0];
    if (p < 0 || p >= B) return fail("load_state: cell owner %d out of range", p);
    int j = ncells[p]++;
    if (j >= kMaxCells) return fail("load_state: player %d has more than 16 cells", p);
    lst[(size_t)j * B + p] = (uint8_t)j;  // slot j == list position j
    size_t hi = (size_t)j * B + p;
    for (int f = 0; f < 9; f++) cf[f][hi] = st->cells_f[9 * k + f];
    csvc[hi] = (int)q[1];
    cseq[hi] = q[2];
    cfl[hi] = F_ALIVE | (q[3] ? F_INHASH : 0);
    gx.push_back(cf[0][hi]);
    gy.push_back(cf[1][hi]);
    gid.push_back((int)((size_t)j * NP + p0 + p));
    rmax_c = std::max(rmax_c, cf[3][hi]);
  }
  for (int i = 0; i < st->n_dead; i++) dead[i] = (int)st->dead[i];
  if (h2d(h, d.p_alive + p0, alive) || h2d(h, d.p_respawn + p0, resp) || h2d(h, d.p_ncells + p0, ncells) ||
      h2d(h, d.p_split + p0, split) || h2d(h, d.p_eject + p0, eject) || h2d(h, d.p_cmdx + p0, cmdx) ||
      h2d(h, d.p_cmdy + p0, cmdy) || h2d(h, d.dead + p0, dead))
    return -1;
  double *cfs[9] = {d.c_x, d.c_y, d.c_m, d.c_r, d.c_vx, d.c_vy, d.c_svx, d.c_svy, d.c_mt};
  for (int s = 0; s < kMaxCells; s++) {
    size_t o = (size_t)s * NP + p0, ho = (size_t)s * B;
    HIPCHK(hipMemcpyAsync(d.p_list + o, lst.data() + ho, B, hipMemcpyHostToDevice, h->stream));
    for (int f = 0; f < 9; f++)
      HIPCHK(hipMemcpyAsync(cfs[f] + o, cf[f].data() + ho, 8 * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d.c_svc + o, csvc.data() + ho, 4 * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d.c_flags + o, cfl.data() + ho, 4 * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(d.c_seq + o, cseq.data() + ho, 8 * B, hipMemcpyHostToDevice, h->stream));
  }
  // cell grid (for observations before the next tick)
  std::vector<int> start, order;
  host_grid(d.cols, gx, gy, start, order, d.cshift_c);
  std::vector<int> items(order.size());
  for (size_t i = 0; i < order.size(); i++) items[i] = gid[order[i]];
  const size_t H1 = (size_t)d.H + 1;
  HIPCHK(hipMemcpyAsync(d.cstart + arena * H1, start.data(), 4 * start.size(), hipMemcpyHostToDevice, h->stream));
  if (!items.empty())
    HIPCHK(hipMemcpyAsync(d.citems + (size_t)arena * CB, items.data(), 4 * items.size(), hipMemcpyHostToDevice,
                          h->stream));
  // pellets -> P0 sorted by bucket
  // (tiles: only the pellets in the held range)
  std::vector<double> px, py, pm;
  std::vector<int64_t> ps;
  std::vector<int> pc;
  for (int i = 0; i < st->n_pellets; i++) {
    const double x = st->pellets_f[4 * i], y = st->pellets_f[4 * i + 1];
    const int bx = std::min(d.cols - 1, std::max(0, (int)(x / kBucket)));
    const int by = std::min(d.cols - 1, std::max(0, (int)(y / kBucket)));
    if (bx < d.loc_bx0 || bx >= d.loc_bx1 || by < d.loc_by0 || by >= d.loc_by1) continue;
    px.push_back(x);
    py.push_back(y);
    pm.push_back(st->pellets_f[4 * i + 2]);
    ps.push_back(st->pellets_seq[i]);
    pc.push_back(st->pellets_col ? (int)st->pellets_col[i] : -1);
  }
  host_grid(d.cols, px, py, start, order);
  {  // the row store, every row in home 0 (aigar_dev.h)
    const int C = d.cols;
    std::vector<PelRec> sr(d.PS);
    std::vector<int> sc(d.PS, -1), pst(d.PH1, 0);
    for (int r = 0; r < C; r++) {
      const int b0 = start[(size_t)r * C], n = start[(size_t)(r + 1) * C] - b0, base = r * d.PR;
      if (n > d.PR) return fail("load_state: %d pellets in bucket row %d, more than its %d slots", n, r, d.PR);
      for (int bx = 0; bx <= C; bx++) pst[(size_t)r * (C + 1) + bx] = base + (start[(size_t)r * C + bx] - b0);
      for (int k = 0; k < n; k++) {
        const int i = order[b0 + k];
        sr[base + k] = PelRec{px[i], py[i], pm[i], ps[i]};
        sc[base + k] = pc[i];
      }
    }
    const size_t po = (size_t)arena * d.PS;
    if (h2d(h, d.pel + po, sr) || h2d(h, d.pel_col + po, sc) || h2d(h, d.pstart + (size_t)arena * d.PH1, pst))
      return -1;
    HIPCHK(hipStreamSynchronize(h->stream));  // (the host records go out of scope)
  }
  // blobs and viruses in list order; blob grid for completeness, virus grid for observations
  const size_t bo = (size_t)arena * d.Ecap, vo = (size_t)arena * d.Vcap;
  double *bfs[8] = {d.b_x, d.b_y, d.b_m, d.b_r, d.b_vx, d.b_vy, d.b_svx, d.b_svy};
  double *vfs[8] = {d.v_x, d.v_y, d.v_m, d.v_r, d.v_vx, d.v_vy, d.v_svx, d.v_svy};
  for (int f = 0; f < 8; f++) {
    std::vector<double> bv(st->n_blobs), vv(st->n_viruses);
    for (int i = 0; i < st->n_blobs; i++) bv[i] = st->blobs_f[8 * i + f];
    for (int i = 0; i < st->n_viruses; i++) vv[i] = st->viruses_f[8 * i + f];
    if (h2d(h, bfs[f] + bo, bv) || h2d(h, vfs[f] + vo, vv)) return -1;
  }
  std::vector<int> bsvc(st->n_blobs), vsvc(st->n_viruses), bcol(st->n_blobs);
  std::vector<int64_t> bseq(st->n_blobs), bej(st->n_blobs), vseq(st->n_viruses);
  std::vector<uint32_t> bfl(d.Ecap, 0), vfl(d.Vcap, 0);
  std::vector<double> vgx, vgy;
  double rmax_v = 0;
  for (int i = 0; i < st->n_blobs; i++) {
    bsvc[i] = (int)st->blobs_i[3 * i]; bseq[i] = st->blobs_i[3 * i + 1]; bej[i] = st->blobs_i[3 * i + 2];
    bcol[i] = st->blobs_col ? (int)st->blobs_col[i] : -1;
    bfl[i] = F_ALIVE;
  }
  std::vector<int> vg_ids;
  for (int i = 0; i < st->n_viruses; i++) {
    vsvc[i] = (int)st->viruses_i[3 * i]; vseq[i] = st->viruses_i[3 * i + 1];
    vfl[i] = F_ALIVE | (st->viruses_i[3 * i + 2] ? F_INHASH : 0);
    vgx.push_back(st->viruses_f[8 * i]);
    vgy.push_back(st->viruses_f[8 * i + 1]);
    rmax_v = std::max(rmax_v, st->viruses_f[8 * i + 3]);
  }
  if (h2d(h, d.b_svc + bo, bsvc) || h2d(h, d.b_seq + bo, bseq) || h2d(h, d.b_ej + bo, bej) || h2d(h, d.b_col + bo, bcol) ||
      h2d(h, d.b_flags + bo, bfl) || h2d(h, d.v_svc + vo, vsvc) || h2d(h, d.v_seq + vo, vseq) ||
      h2d(h, d.v_flags + vo, vfl))
    return -1;
  host_grid(d.cols, vgx, vgy, start, order, d.cshift);
  HIPCHK(hipMemcpyAsync(d.vstart + arena * H1, start.data(), 4 * start.size(), hipMemcpyHostToDevice, h->stream));
  if (!order.empty()) HIPCHK(hipMemcpyAsync(d.vitems + vo, order.data(), 4 * order.size(), hipMemcpyHostToDevice, h->stream));
  // control block
  ArenaCtl c;
  memset(&c, 0, sizeof c);
  c.seq_next = st->seq_next;
  c.tick = st->tick;
  c.key0 = st->philox_key[0];
  c.key1 = st->philox_key[1];
  c.ctr_pellet = st->ctr_pellet;
  c.ctr_virus = st->ctr_virus;
  c.n_pel = (int)px.size();
  c.n_pel_glob = st->n_pellets;
  c.n_blob = st->n_blobs;
  c.n_vir = st->n_viruses;
  c.n_dead = st->n_dead;
  c.rmax_cell = std::max(rmax_c, std::sqrt(10.0 / 3.141592653589793));
  c.rmax_virus = std::max(rmax_v, std::sqrt(100.0 / 3.141592653589793));
  c.food_round = 1;  // reservation epochs restart: clear this arena's keys
  HIPCHK(hipMemsetAsync(d.pel_owner + (size_t)arena * d.PD, 0, 8 * (size_t)d.PD, h->stream));
  HIPCHK(hipMemsetAsync(d.b_owner + (size_t)arena * d.Ecap, 0, 8 * (size_t)d.Ecap, h->stream));
  // look-back epochs restart too: clear this arena's tile states
  HIPCHK(hipMemsetAsync(d.pl_state + (size_t)arena * d.pl_tiles, 0, 8 * (size_t)d.pl_tiles, h->stream));
  HIPCHK(hipMemsetAsync(d.pel_dead + (size_t)arena * d.PD, 0, (size_t)d.PD, h->stream));
  HIPCHK(hipMemsetAsync(d.cgcnt + (size_t)arena * 2 * 4100, 0, sizeof(int) * 2 * 4100, h->stream));
  for (int sl = 0; sl < 2; sl++)
    HIPCHK(hipMemsetAsync(d.scan_state + ((size_t)sl * d.A + arena) * d.scan_tiles, 0, 8 * (size_t)d.scan_tiles,
                          h->stream));
  HIPCHK(hipMemcpyAsync(d.ctl + arena, &c, sizeof c, hipMemcpyHostToDevice, h->stream));
  // the arena's bots restart (NN bot reset, bot.py:151-158); the commands are the snapshot's
  const ArenaSel sel{nullptr, nullptr, 0, arena, 1};
  launch_restart_bots(d, h->stream, sel);
  restart_side_buffers(h, sel);
  if (tiles_restart(h)) return -1;
  launch_player_fov(d, h->stream, sel);  // FOV cache of the loaded players
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int aigar_policy_greedy(aigar_handle *h, int greedy_split, const uint8_t *mask, int on_device) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->cfg.device));
  const uint8_t *m = mask;
  if (mask && !on_device) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->d.NP, hipMemcpyHostToDevice, h->stream));
    m = h->d_mask;
  }
  note_greedy(h);  // (food_rounds)
  {
    Mark mk(h, "policy");
    launch_policy_greedy(h->d, h->stream, greedy_split ? 1 : 0, m, -1);
  }
  HIPCHK(hipGetLastError());
  if (mask && !on_device) HIPCHK(hipStreamSynchronize(h->stream));  // (host mask buffer reused next call)
  return 0;
}

extern "C" int aigar_set_split_likelihood(aigar_handle *h, int arena, const int32_t *lh) {
  if (!h) return fail("null handle");
  if (arena < 0 || arena >= h->d.A) return fail("arena out of range");
  HIPCHK(hipSetDevice(h->cfg.device));
  int *dst = h->d.p_split_lh + (size_t)arena * h->d.B;
  if (!lh) {
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(int) * h->d.B, h->stream));
  } else {
    HIPCHK(hipMemcpyAsync(dst, lh, sizeof(int) * h->d.B, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int aigar_apply_actions(aigar_handle *h, const double *act, int n_act, int enable_split, int skipping,
                                   int record, int on_device) {
  if (!h || !act) return fail("null argument");
  if (n_act < 2 || n_act > 4) return fail("apply_actions: n_act must be 2, 3 or 4");
  HIPCHK(hipSetDevice(h->cfg.device));
  const double *src = act;
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(h->d_cmd, act, sizeof(double) * n_act * h->d.NP, hipMemcpyHostToDevice, h->stream));
    src = h->d_cmd;
  }
  launch_apply_actions(h->d, h->stream, src, n_act, enable_split, skipping, record);
  HIPCHK(hipGetLastError());
  if (!on_device) HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int aigar_rewards(aigar_handle *h, double *out, const aigar_reward_params *p, int update_last,
                             int on_device) {
  if (!h || !out || !p) return fail("null argument");
  HIPCHK(hipSetDevice(h->cfg.device));
  double *dst = on_device ? out : h->d_stats;
  launch_rewards(h->d, h->stream, dst, *p, update_last, 0);
  HIPCHK(hipGetLastError());
  if (!on_device) {
    HIPCHK(hipMemcpyAsync(out, h->d_stats, sizeof(double) * h->d.NP, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int aigar_counters(aigar_handle *h, int arena, int64_t *out, int n) {
  if (!h) return fail("null handle");
  if (arena < 0 || arena >= h->d.A) return fail("arena out of range");
  if (!out || n < 0 || n > 8) return fail("counters: need 0 <= n <= 8 and an output array");
  HIPCHK(hipSetDevice(h->cfg.device));
  ArenaCtl c;
  HIPCHK(hipMemcpyAsync(&c, h->d.ctl + arena, sizeof c, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int k = 0; k < n; k++) out[k] = c.stat[k];
  return 0;
}

extern "C" int aigar_get_events(aigar_handle *h, int arena, int64_t *out, int cap, int *n) {
  if (!h || !n) return fail("null argument");
  Dev &d = h->d;
  if (arena < 0 || arena >= d.A) return fail("arena %d out of range", arena);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (check_device_errors(h)) return -1;
  ArenaCtl c;
  HIPCHK(hipMemcpy(&c, d.ctl + arena, sizeof c, hipMemcpyDeviceToHost));
  int ne = std::min(c.n_ev, d.EVcap);
  *n = ne;
  if (!out) return 0;
  if (cap < ne) return fail("get_events: cap %d < %d events", cap, ne);
  std::vector<int64_t> ev((size_t)ne * 5);
  if (ne) HIPCHK(hipMemcpy(ev.data(), d.ev + (size_t)arena * d.EVcap * 5, ev.size() * 8, hipMemcpyDeviceToHost));
  std::vector<int> ord(ne);
  for (int i = 0; i < ne; i++) ord[i] = i;
  std::sort(ord.begin(), ord.end(), [&](int x, int y) {
    if (ev[5 * x] != ev[5 * y]) return ev[5 * x] < ev[5 * y];
    return (uint64_t)ev[5 * x + 1] < (uint64_t)ev[5 * y + 1];
  });
  for (int i = 0; i < ne; i++) {
    const int64_t *e = &ev[5 * (size_t)ord[i]];
    out[4 * i] = e[0] >> 8;
    out[4 * i + 1] = e[2];
    out[4 * i + 2] = e[3];
    out[4 * i + 3] = e[4];
  }
  return 0;
}

// the raw event rows (sort keys kept) -- tiles merge their logs by key
extern "C" int aigar_get_events_raw(aigar_handle *h, int arena, int64_t *out, int cap, int *n) {
  if (!h || !n) return fail("null argument");
  Dev &d = h->d;
  if (arena < 0 || arena >= d.A) return fail("arena %d out of range", arena);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (check_device_errors(h)) return -1;
  ArenaCtl c;
  HIPCHK(hipMemcpy(&c, d.ctl + arena, sizeof c, hipMemcpyDeviceToHost));
  const int ne = std::min(c.n_ev, d.EVcap);
  *n = ne;
  if (!out) return 0;
  if (cap < ne) return fail("get_events_raw: cap %d < %d events", cap, ne);
  if (ne) HIPCHK(hipMemcpy(out, d.ev + (size_t)arena * d.EVcap * 5, (size_t)ne * 5 * 8, hipMemcpyDeviceToHost));
  return 0;
}

__global__ void k_selftest_pow(const double *x, const double *y, double *out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = aigar_math::pow_glibc(x[i], y[i]);
}

extern "C" int aigar_selftest_pow(const double *x, const double *y, double *out, int n) {
  if (!x || !y || !out || n < 0) return fail("null argument");
  double *dx = nullptr, *dy = nullptr, *dz = nullptr;
  size_t b = sizeof(double) * (size_t)(n > 0 ? n : 1);
  HIPCHK(hipMalloc(&dx, b));
  HIPCHK(hipMalloc(&dy, b));
  HIPCHK(hipMalloc(&dz, b));
  HIPCHK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy, y, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_pow, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dy, dz, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dz, sizeof(double) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dz);
  return 0;
}

__global__ void k_selftest_log(const double *x, double *out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = aigar_math::log_glibc(x[i]);
}

extern "C" int aigar_selftest_log(const double *x, double *out, int n) {
  if (!x || !out || n < 0) return fail("null argument");
  double *dx = nullptr, *dz = nullptr;
  size_t b = sizeof(double) * (size_t)(n > 0 ? n : 1);
  HIPCHK(hipMalloc(&dx, b));
  HIPCHK(hipMalloc(&dz, b));
  HIPCHK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_log, dim3((n + 255) / 256), dim3(256), 0, 0, dx, dz, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dz, sizeof(double) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dz);
  return 0;
}

// out[0, n): atan2(y, x); out[n, 2n): sin(x); out[2n, 3n): cos(x) -- the stepper's trig
// entry points (aigar_glibc_trig.h), one thread per element
__global__ void k_selftest_trig(const double *y, const double *x, double *out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = aigar_math::trig_atan2(y[i], x[i]);
  double s, c;
  aigar_math::trig_sincos(x[i], s, c);
  out[n + i] = s;
  out[2 * (size_t)n + i] = c;
}

extern "C" int aigar_selftest_trig(const double *y, const double *x, double *out, int n) {
  if (!x || !y || !out || n < 0) return fail("null argument");
  double *dx = nullptr, *dy = nullptr, *dz = nullptr;
  const size_t b = sizeof(double) * (size_t)(n > 0 ? n : 1);
  HIPCHK(hipMalloc(&dx, b));
  HIPCHK(hipMalloc(&dy, b));
  HIPCHK(hipMalloc(&dz, 3 * b));
  HIPCHK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy, y, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_trig, dim3((n + 255) / 256), dim3(256), 0, 0, dy, dx, dz, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dz, 3 * sizeof(double) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dz);
  return 0;
}

// The per-entity helpers of aigar_sem.h and the exact integer helpers of aigar_math.h, one
// thread per element, the header functions themselves (tests/test_gpu_sem.py).  in is
// [in_cols][n], out [out_cols][n], 8-byte words: values are doubles, integers come back as
// exact doubles, the Philox op's 64-bit words travel as bit patterns.
namespace {
struct SemOp {
  int in_cols, out_cols;
};
constexpr SemOp kSemOps[AIGAR_SEM_N_OPS] = {
    {2, 1},   // MOD_POS
    {2, 1},   // TRUNC_DIV_POS
    {2, 1},   // PY_MOD
    {1, 1},   // ROUND3
    {17, 2},  // SUM
    {1, 2},   // RADIUS
    {2, 3},   // BUCKET
    {4, 4},   // FOOTPRINT
    {6, 4},   // MOVE
    {7, 2},   // MOMENTUM
    {2, 1},   // MERGE_TIME
    {8, 6},   // PHILOX
    {2, 6},   // TRIG_FORMS
};
}  // namespace

__global__ void k_selftest_sem(int op, const double *in, double *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t N = (size_t)n;
#define SEM_IN(c) in[(size_t)(c) * N + i]
#define SEM_OUT(c) out[(size_t)(c) * N + i]
  switch (op) {
    case AIGAR_SEM_MOD_POS: {
      const double a = SEM_IN(0), b = SEM_IN(1);
      SEM_OUT(0) = aigar_math::mod_pos(a, b, 1.0 / b);
    } break;
    case AIGAR_SEM_TRUNC_DIV_POS: {
      const double x = SEM_IN(0), b = SEM_IN(1);
      SEM_OUT(0) = (double)aigar_math::trunc_div_pos(x, b, 1.0 / b);
    } break;
    case AIGAR_SEM_PY_MOD:
      SEM_OUT(0) = py_mod(SEM_IN(0), SEM_IN(1));
      break;
    case AIGAR_SEM_ROUND3:
      SEM_OUT(0) = py_round3(SEM_IN(0));
      break;
    case AIGAR_SEM_SUM: {
      double t[kMaxCells];
#pragma unroll
      for (int k = 0; k < kMaxCells; k++) t[k] = SEM_IN(k);
      int cnt = (int)SEM_IN(kMaxCells);
      cnt = cnt < 0 ? 0 : (cnt > kMaxCells ? kMaxCells : cnt);  // (the array's length)
      SEM_OUT(0) = np_sum(t, cnt);
      NpAcc acc;
#pragma unroll
      for (int k = 0; k < kMaxCells; k++)  // (k a constant, as at add's call sites)
        if (k < cnt) acc.add(k, cnt, t[k]);
      SEM_OUT(1) = acc.sum(cnt);
    } break;
    case AIGAR_SEM_RADIUS:
      SEM_OUT(0) = radius_of(SEM_IN(0));
      SEM_OUT(1) = pellet_radius(SEM_IN(0));
      break;
    case AIGAR_SEM_BUCKET: {
      const double c = SEM_IN(0);
      const int cols = (int)SEM_IN(1);
      SEM_OUT(0) = (double)bucket_floor_s(c);
      SEM_OUT(1) = c >= 0 ? (double)bucket_floor(c) : -1.0;  // (bucket_floor: c >= 0 only)
      SEM_OUT(2) = c >= 0 ? (double)center_bucket_coord(c, cols) : -1.0;
    } break;
    case AIGAR_SEM_FOOTPRINT: {
      const Rect r = footprint(SEM_IN(0), SEM_IN(1), SEM_IN(2), (int)SEM_IN(3));
      SEM_OUT(0) = (double)r.x0;
      SEM_OUT(1) = (double)r.x1;
      SEM_OUT(2) = (double)r.y0;
      SEM_OUT(3) = (double)r.y1;
    } break;
    case AIGAR_SEM_MOVE: {
      double vx, vy, c, s;
      set_move_direction(SEM_IN(0), SEM_IN(1), SEM_IN(2), SEM_IN(3), SEM_IN(4), SEM_IN(5), vx, vy, c, s);
      SEM_OUT(0) = vx;
      SEM_OUT(1) = vy;
      SEM_OUT(2) = c;
      SEM_OUT(3) = s;
    } break;
    case AIGAR_SEM_MOMENTUM: {
      double svx, svy;
      int svc;
      add_momentum(SEM_IN(0), SEM_IN(1), SEM_IN(2), SEM_IN(3), SEM_IN(4), SEM_IN(5), SEM_IN(6), svx, svy, svc);
      SEM_OUT(0) = svx;
      SEM_OUT(1) = svy;
    } break;
    case AIGAR_SEM_MERGE_TIME:
      SEM_OUT(0) = merge_time_for(SEM_IN(0), SEM_IN(1));
      break;
    case AIGAR_SEM_PHILOX: {
      uint64_t w[4];
      philox(aigar_math::as_u64(SEM_IN(0)), aigar_math::as_u64(SEM_IN(1)), aigar_math::as_u64(SEM_IN(2)),
             aigar_math::as_u64(SEM_IN(3)), aigar_math::as_u64(SEM_IN(4)), aigar_math::as_u64(SEM_IN(5)), w);
#pragma unroll
      for (int k = 0; k < 4; k++) SEM_OUT(k) = aigar_math::as_double(w[k]);
      SEM_OUT(4) = u01(w[0]);
      SEM_OUT(5) = (double)ph_randint(w[0], SEM_IN(6), SEM_IN(7));
    } break;
    case AIGAR_SEM_TRIG_FORMS: {
      const double y = SEM_IN(0), x = SEM_IN(1);
      SEM_OUT(0) = aigar_math::atan2_glibc(y, x);
      SEM_OUT(1) = aigar_math::atan2_glibc_flat(y, x);
      SEM_OUT(2) = aigar_math::sin_glibc(x);
      SEM_OUT(3) = aigar_math::cos_glibc(x);
      double s, c;
      aigar_math::sincos_glibc(x, s, c);
      SEM_OUT(4) = s;
      SEM_OUT(5) = c;
    } break;
    default:
      break;
  }
#undef SEM_IN
#undef SEM_OUT
}

extern "C" int aigar_selftest_sem(int op, const double *in, int in_cols, double *out, int out_cols, int n) {
  if (op < 0 || op >= AIGAR_SEM_N_OPS) return fail("selftest_sem: op %d is none of 0..%d", op, AIGAR_SEM_N_OPS - 1);
  if (in_cols != kSemOps[op].in_cols) return fail("selftest_sem: in_cols %d, op %d takes %d", in_cols, op, kSemOps[op].in_cols);
  if (out_cols != kSemOps[op].out_cols)
    return fail("selftest_sem: out_cols %d, op %d gives %d", out_cols, op, kSemOps[op].out_cols);
  if (!in) return fail("selftest_sem: in is null");
  if (!out) return fail("selftest_sem: out is null");
  if (n < 0) return fail("selftest_sem: n %d is negative", n);
  if (n == 0) return 0;
  double *di = nullptr, *dout = nullptr;
  const size_t bi = sizeof(double) * (size_t)in_cols * n, bo = sizeof(double) * (size_t)out_cols * n;
  HIPCHK(hipMalloc(&di, bi));
  HIPCHK(hipMalloc(&dout, bo));
  HIPCHK(hipMemcpy(di, in, bi, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dout, 0, bo));
  hipLaunchKernelGGL(k_selftest_sem, dim3((n + 255) / 256), dim3(256), 0, 0, op, di, dout, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost));
  (void)hipFree(di);
  (void)hipFree(dout);
  return 0;
}
