// replay.inc -- the learners' experience replay memory on the device (include/aigar.h
// aigar_exp_*; DESIGN.md §4g).  Included by api.hip: the memory's device layout and
// its kernels; the entry points are in api.hip.
//
// The reference's ReplayBuffer / PrioritizedReplayBuffer (replay_buffer.py) over
// SumSegmentTree / MinSegmentTree (common/segment_tree.py), as a ring of rows plus
// two implicit binary trees of 2 * it_cap doubles.  Every tree node is a pure
// function of its two children, so rebuilding the touched ancestors level by level
// once the leaves are final gives the bits of the reference's one-at-a-time
// __setitem__ (no order among atomics is relied on: the only atomic is a max).
//
// Kernels (wave64, gfx950):
//   k_exp_plan    one workgroup: scan the emitters into slot offsets (ascending row
//                 order = ReplayBuffer.add once per transition), advance the ring,
//                 write the new leaves and rebuild their ancestors
//   k_exp_rows    one workgroup per row: old state / new state / scalars into the
//                 slot, then the latch (new state -> old state); plain row copies
//   k_exp_latch   the observe calls' latch
//   k_exp_draw    one thread per draw: u -> index and importance weight
//   k_exp_fetch   one workgroup per sampled row: the rows out
//   k_exp_update  one workgroup: priorities -> leaves (last occurrence wins), ancestors
//   k_exp_extra_get / k_exp_extra_set  the fifth field of given slots out / in (last occurrence wins)

struct ExpCtl {  // device-resident state of the ring
  int64_t size, next, added, calls;
  double max_prio;
  // the running add (k_exp_plan -> k_exp_rows): first slot, emitters, rows to skip
  // (an add of more than capacity rows keeps the last capacity of them)
  int64_t base, n_emit, n_skip;
};

struct Exp {
  int64_t cap = 0, it_cap = 0;
  int dtype = 0, esz = 8, L = 0, prio = 0;
  size_t stride = 0;  // bytes of a ring row (16-byte padded)
  double alpha = 0, beta = 0;
  uint64_t seed = 0;
  char *s = nullptr, *s2 = nullptr;  // [cap][stride]
  double *a = nullptr, *r = nullptr;  // [cap][4], [cap]
  uint8_t *done = nullptr;            // [cap]
  double *vsum = nullptr, *vmin = nullptr;  // [2 * it_cap]
  int *last = nullptr;                // [cap] scratch of k_exp_update / k_exp_extra_set, -1 between calls
  double *x = nullptr;                // [cap][4] the tuple's fifth field (AIGAR_EXP_EXTRA; null: none)
  uint8_t *xv = nullptr;              // [cap] ... and whether the slot has one (0: the reference's None, x is NaN)
  ExpCtl *ctl = nullptr;
  char *old = nullptr;        // [NP][stride] every player's old state (Bot.oldState)
  uint8_t *has_old = nullptr;  // [NP]
  int *off = nullptr;          // [NP] slot offsets of the decision's emitters (-1: none)
};

constexpr int kExpPlanThreads = 1024;
constexpr uint64_t kExpStream = 0x657870ull;  // Philox site word of the memory's own draws

template <class T>
__device__ __forceinline__ bool exp_row_is_nan(const void *row) {
  const T v = *(const T *)row;
  return v != v;
}
__device__ __forceinline__ bool exp_dead_row(const void *row, int esz) {
  return esz == 8 ? exp_row_is_nan<double>(row) : exp_row_is_nan<float>(row);
}

// Block-wide exclusive scan of one int per thread (kExpPlanThreads threads); returns
// the thread's offset, *total the sum.  Hillis-Steele in LDS: 10 rounds, once a call.
__device__ int exp_block_scan(int v, int *lds, int *total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < kExpPlanThreads; d <<= 1) {
    const int add = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  *total = lds[kExpPlanThreads - 1];
  const int incl = lds[t];
  __syncthreads();
  return incl - v;
}

// The ancestors of the leaves [lo, lo + cnt) (cnt >= 1, no wrap), level by level.
__device__ void exp_rebuild_range(const Exp &e, int64_t lo, int64_t cnt) {
  int64_t a = e.it_cap + lo, b = e.it_cap + lo + cnt - 1;
  while (a > 1) {
    a >>= 1;
    b >>= 1;
    __syncthreads();  // the level below is written (and visible: one workgroup)
    for (int64_t k = a + threadIdx.x; k <= b; k += blockDim.x) {
      const double s0 = e.vsum[2 * k], s1 = e.vsum[2 * k + 1];
      e.vsum[k] = s0 + s1;
      const double m0 = e.vmin[2 * k], m1 = e.vmin[2 * k + 1];
      e.vmin[k] = (m1 < m0) ? m1 : m0;  // builtin min(m0, m1)
    }
  }
  __syncthreads();
}

// mode 0: the decision's emitters -- NN players with an old state; mode 1: the rows
// of a caller's add with mask[i] != 0 (null: all).  off[i] = the row's rank among
// the emitters (-1: none).  Then ReplayBuffer.add's bookkeeping for all of them at
// once and, prioritized, PrioritizedReplayBuffer.add's leaves max_priority ** alpha.
__global__ void __launch_bounds__(kExpPlanThreads) k_exp_plan(Exp e, int mode, const uint8_t *role, const uint8_t *mask,
                                                               int n, int *off) {
  __shared__ int lds[kExpPlanThreads];
  const int t = threadIdx.x;
  const int per = (n + kExpPlanThreads - 1) / kExpPlanThreads;
  const int i0 = min(n, t * per), i1 = min(n, i0 + per);
  int c = 0;
  for (int i = i0; i < i1; i++) c += mode == 0 ? (role[i] == AIGAR_ROLE_NN && e.has_old[i]) : (!mask || mask[i]);
  int total;
  int o = exp_block_scan(c, lds, &total);
  for (int i = i0; i < i1; i++) {
    const bool em = mode == 0 ? (role[i] == AIGAR_ROLE_NN && e.has_old[i]) : (!mask || mask[i]);
    off[i] = em ? o++ : -1;
  }
  ExpCtl *ctl = e.ctl;
  const int64_t base = ctl->next, size = ctl->size, added = ctl->added;
  const double leaf = e.prio ? aigar_math::pow_glibc(ctl->max_prio, e.alpha) : 0.0;
  __syncthreads();  // (every thread has read the ring state)
  const int64_t kept = total < e.cap ? total : e.cap, skip = total - kept;
  if (t == 0) {
    ctl->base = base;
    ctl->n_emit = total;
    ctl->n_skip = skip;
    ctl->next = (base + total) % e.cap;
    ctl->size = size + total < e.cap ? size + total : e.cap;
    ctl->added = added + total;
  }
  if (!e.prio || kept == 0) return;
  const int64_t first = (base + skip) % e.cap;
  for (int64_t k = t; k < kept; k += kExpPlanThreads) {
    const int64_t slot = (first + k) % e.cap;
    e.vsum[e.it_cap + slot] = leaf;
    e.vmin[e.it_cap + slot] = leaf;
  }
  const int64_t c0 = first + kept <= e.cap ? kept : e.cap - first;  // the part before the ring's end
  exp_rebuild_range(e, first, c0);
  if (kept > c0) exp_rebuild_range(e, 0, kept - c0);
}

template <class W>
__device__ __forceinline__ void exp_copy_row(void *dst, const void *src, int L) {
  W *d = (W *)dst;
  const W *s = (const W *)src;
  for (int j = threadIdx.x; j < L; j += blockDim.x) d[j] = s[j];
}

// One workgroup per row i.  latch = 1 (the decision): s rows are the old states
// ([n][stride]), s2 the observation buffer ([n][L]), done = the new row is NaN, and
// afterwards the new row becomes the old state of every NN player (none if dead).
// latch = 0 (aigar_exp_add): caller rows [n][L], caller done.  States move as their
// bit patterns (NaN payloads included), in units of the element: the caller's rows
// are aligned to no more than that.  xtra: [n][n_act] the slot's fifth field (null: none,
// the slot's extra is NaN and invalid); only a memory with the extra field keeps it.
template <class W>
__global__ void __launch_bounds__(256) k_exp_rows(Exp e, const int *off, const char *s, size_t s_stride, const char *s2,
                                                  const double *act, int n_act, const double *rew, const uint8_t *done,
                                                  const uint8_t *role, int latch, const double *xtra) {
  const int i = blockIdx.x;
  const ExpCtl *ctl = e.ctl;
  const int o = off[i];
  const char *srow = s + (size_t)i * s_stride, *nrow = s2 + (size_t)i * e.L * sizeof(W);
  const bool dead = latch ? exp_dead_row(nrow, sizeof(W)) : false;
  if (o >= 0 && o >= ctl->n_skip) {
    const int64_t slot = (ctl->base + o) % e.cap;
    exp_copy_row<W>(e.s + slot * e.stride, srow, e.L);
    exp_copy_row<W>(e.s2 + slot * e.stride, nrow, e.L);
    if (threadIdx.x < 4) e.a[slot * 4 + threadIdx.x] = (int)threadIdx.x < n_act ? act[(size_t)i * n_act + threadIdx.x] : 0.0;
    if (threadIdx.x == 4) e.r[slot] = rew[i];
    if (threadIdx.x == 5) e.done[slot] = latch ? (dead ? 1 : 0) : (done[i] ? 1 : 0);
    if (e.x) {
      const int t = (int)threadIdx.x - 8;
      if (t >= 0 && t < 4) e.x[slot * 4 + t] = xtra ? (t < n_act ? xtra[(size_t)i * n_act + t] : 0.0) : __builtin_nan("");
      if (t == 4) e.xv[slot] = xtra ? 1 : 0;
    }
  }
  if (!latch || role[i] != AIGAR_ROLE_NN) return;
  // (each thread reads old[j] above before it writes old[j] here: same thread, same j)
  if (!dead) exp_copy_row<W>(e.old + (size_t)i * e.stride, nrow, e.L);
  if (threadIdx.x == 0) e.has_old[i] = dead ? 0 : 1;
}

// The observe calls' latch: the rows an observation call wrote (mask[i] != 0, null:
// all) become those players' old states; a NaN row (a dead player) clears it.  The
// call's dtype may differ from the memory's: the values are then converted.
__global__ void __launch_bounds__(256) k_exp_latch(Exp e, const void *obs, int dtype, const uint8_t *mask) {
  const int i = blockIdx.x;
  if (mask && !mask[i]) return;
  const int L = e.L;
  char *dst = e.old + (size_t)i * e.stride;
  bool dead;
  if (dtype == 0) {
    const double *row = (const double *)obs + (size_t)i * L;
    dead = row[0] != row[0];
    if (!dead) {
      if (e.dtype == 0) exp_copy_row<uint64_t>(dst, row, L);
      else for (int j = threadIdx.x; j < L; j += blockDim.x) ((float *)dst)[j] = (float)row[j];
    }
  } else {
    const float *row = (const float *)obs + (size_t)i * L;
    dead = row[0] != row[0];
    if (!dead) {
      if (e.dtype == 1) exp_copy_row<uint32_t>(dst, row, L);
      else for (int j = threadIdx.x; j < L; j += blockDim.x) ((double *)dst)[j] = (double)row[j];
    }
  }
  if (threadIdx.x == 0) e.has_old[i] = dead ? 0 : 1;
}

__global__ void k_exp_clear_arenas(uint8_t *has_old, int B, ArenaSel sel) {
  for (int i = threadIdx.x; i < B; i += blockDim.x) has_old[(size_t)sel.arena(blockIdx.x) * B + i] = 0;
}
__global__ void k_exp_clear_bots(uint8_t *has_old, int n, const uint8_t *mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) has_old[i] = 0;
}
__global__ void k_exp_fill_i(int *p, size_t n, int v) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void k_exp_init(Exp e) {  // a cleared memory: empty trees, max_priority 1.0
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e.prio && i < 2 * (size_t)e.it_cap) {
    e.vsum[i] = 0.0;                // SumSegmentTree's neutral element
    e.vmin[i] = __builtin_inf();    // MinSegmentTree's
  }
  if (i == 0) {
    ExpCtl c{};
    c.max_prio = 1.0;
    *e.ctl = c;
  }
}

// SumSegmentTree.sum(0, end + 1) as _reduce_helper associates it for a prefix range
// (segment_tree.py:36-49): the recursion splits only to the right, giving
// v[left] + (v[left'] + (... + v[last])).  The last node is found by the descent;
// walking back up, every right child met adds its left sibling in front.
__device__ double exp_prefix_sum(const Exp &e, int64_t end) {
  int64_t node = 1, ns = 0, ne = e.it_cap - 1;
  while (ne != end) {
    const int64_t mid = (ns + ne) >> 1;
    if (end <= mid) {
      node = 2 * node;
      ne = mid;
    } else {
      node = 2 * node + 1;
      ns = mid + 1;
    }
  }
  double acc = e.vsum[node];
  for (; node > 1; node >>= 1)
    if (node & 1) acc = e.vsum[node - 1] + acc;
  return acc;
}

// One draw per thread.  Uniform: idx = floor(u * size), w = 1.  Prioritized:
// _sample_proportional + the weights of PrioritizedReplayBuffer.sample
// (replay_buffer.py:114-171) with its quirks: the mass spans the leaves [0, size - 2].
__global__ void __launch_bounds__(256) k_exp_draw(Exp e, int batch, const double *u_in, double *w, int64_t *idx) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= batch) return;
  const ExpCtl *ctl = e.ctl;
  const int64_t size = ctl->size;
  if (size == 0 || (e.prio && size < 2)) {  // nothing to draw from (the reference recurses forever)
    idx[k] = -1;
    w[k] = __builtin_nan("");
    return;
  }
  double u;
  if (u_in) {
    u = u_in[k];
  } else {
    uint64_t o[4];
    aigar::philox((uint64_t)k, (uint64_t)ctl->calls, 0, kExpStream, e.seed, 0x4147415245585021ull, o);
    u = aigar::u01(o[0]);
  }
  if (!e.prio) {
    int64_t i = (int64_t)(u * (double)size);
    idx[k] = i < size ? i : size - 1;  // (u < 1 keeps i < size; a caller's u >= 1 is clamped)
    w[k] = 1.0;
    return;
  }
  double mass = u * exp_prefix_sum(e, size - 2);
  int64_t node = 1;
  while (node < e.it_cap) {  // find_prefixsum_idx (segment_tree.py:124-131)
    const double left = e.vsum[2 * node];
    if (left > mass) {
      node = 2 * node;
    } else {
      mass -= left;
      node = 2 * node + 1;
    }
  }
  const int64_t i = node - e.it_cap;
  idx[k] = i;
  const double total = e.vsum[1], n = (double)size, nb = -e.beta;
  const double p_min = e.vmin[1] / total;
  const double max_weight = aigar_math::pow_glibc(p_min * n, nb);
  const double p_sample = e.vsum[e.it_cap + i] / total;
  w[k] = aigar_math::pow_glibc(p_sample * n, nb) / max_weight;
}

// One workgroup per row: the transition idx[k] into row k of the caller's buffers;
// an index outside [0, size) leaves row k as it is.  count: this was a sample call.
template <class W>
__global__ void __launch_bounds__(256) k_exp_fetch(Exp e, const int64_t *idx, char *s, double *a, double *r, char *s2,
                                                   uint8_t *done, int count) {
  const int k = blockIdx.x;
  ExpCtl *ctl = e.ctl;
  const int64_t i = idx[k];
  if (i >= 0 && i < ctl->size) {
    const size_t row = (size_t)e.L * sizeof(W);
    if (s) exp_copy_row<W>(s + k * row, e.s + i * e.stride, e.L);
    if (s2) exp_copy_row<W>(s2 + k * row, e.s2 + i * e.stride, e.L);
    if (a && threadIdx.x < 4) a[(size_t)k * 4 + threadIdx.x] = e.a[i * 4 + threadIdx.x];
    if (r && threadIdx.x == 4) r[k] = e.r[i];
    if (done && threadIdx.x == 5) done[k] = e.done[i];
  }
  if (count && k == 0 && threadIdx.x == 6) ctl->calls += 1;  // (this call's draws are made: k_exp_draw ran before)
}

// PrioritizedReplayBuffer.update_priorities (replay_buffer.py:173-195) for n entries
// in one workgroup.  An entry with prio <= 0 (or NaN) or an index outside [0, size) is
// skipped.  max_priority takes every entry that is not skipped; the leaf takes the last
// entry of its index (the largest position: an atomic max, whose result no order
// among the atomics changes); then the ancestors, level by level.
__global__ void __launch_bounds__(kExpPlanThreads) k_exp_update(Exp e, const int64_t *idx, const double *prio, int n) {
  __shared__ double red[kExpPlanThreads];
  const int t = threadIdx.x;
  const int64_t size = e.ctl->size;
  double m = 0.0;
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    const double p = prio[j];
    if (!(p > 0.0) || i < 0 || i >= size) continue;
    m = p > m ? p : m;
    atomicMax(&e.last[i], j);
  }
  red[t] = m;
  __syncthreads();
  for (int d = kExpPlanThreads / 2; d > 0; d >>= 1) {
    if (t < d) red[t] = red[t + d] > red[t] ? red[t + d] : red[t];
    __syncthreads();
  }
  if (t == 0 && red[0] > e.ctl->max_prio) e.ctl->max_prio = red[0];
  // (the barriers above also order the atomics before the reads below)
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    const double p = prio[j];
    if (!(p > 0.0) || i < 0 || i >= size) continue;
    if (e.last[i] != j) continue;
    const double leaf = aigar_math::pow_glibc(p, e.alpha);
    e.vsum[e.it_cap + i] = leaf;
    e.vmin[e.it_cap + i] = leaf;
  }
  for (int64_t width = e.it_cap >> 1, lvl = 1; width >= 1; width >>= 1, lvl++) {
    __syncthreads();  // the level below is written
    for (int j = t; j < n; j += kExpPlanThreads) {
      const int64_t i = idx[j];
      const double p = prio[j];
      if (!(p > 0.0) || i < 0 || i >= size) continue;
      if (e.last[i] != j) continue;  // (one entry per touched leaf walks up; shared ancestors get equal values)
      const int64_t k = (e.it_cap + i) >> lvl;
      const double s0 = e.vsum[2 * k], s1 = e.vsum[2 * k + 1];
      e.vsum[k] = s0 + s1;
      const double m0 = e.vmin[2 * k], m1 = e.vmin[2 * k + 1];
      e.vmin[k] = (m1 < m0) ? m1 : m0;
    }
  }
  __syncthreads();
  for (int j = t; j < n; j += kExpPlanThreads) {  // the scratch is -1 again for the next call
    const int64_t i = idx[j];
    if (i >= 0 && i < size) e.last[i] = -1;
  }
}

// The fifth field of the slots idx[k] into row k of out / valid (each may be null); an
// index outside [0, size) leaves row k as it is.  One thread per (k, value).
__global__ void __launch_bounds__(256) k_exp_extra_get(Exp e, const int64_t *idx, int batch, double *out, uint8_t *valid) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x, k = g >> 2, t = g & 3;
  if (k >= batch) return;
  const int64_t i = idx[k];
  if (i < 0 || i >= e.ctl->size) return;
  if (out) out[(size_t)k * 4 + t] = e.x[i * 4 + t];
  if (valid && t == 0) valid[k] = e.xv[i];
}

// ReplayBuffer.update_dones (replay_buffer.py:197-209) for n entries in one workgroup: slot
// idx[j] gets rows[j] and becomes valid.  An index outside [0, size) is skipped; of several
// entries with one index the last wins (the largest position: an atomic max, whose result
// no order among the atomics changes), as in k_exp_update.
__global__ void __launch_bounds__(kExpPlanThreads) k_exp_extra_set(Exp e, const int64_t *idx, const double *rows, int n) {
  const int t = threadIdx.x;
  const int64_t size = e.ctl->size;
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    if (i >= 0 && i < size) atomicMax(&e.last[i], j);
  }
  __syncthreads();
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    if (i < 0 || i >= size || e.last[i] != j) continue;
    for (int v = 0; v < 4; v++) e.x[i * 4 + v] = rows[(size_t)j * 4 + v];
    e.xv[i] = 1;
  }
  __syncthreads();
  for (int j = t; j < n; j += kExpPlanThreads) {  // the scratch is -1 again for the next call
    const int64_t i = idx[j];
    if (i >= 0 && i < size) e.last[i] = -1;
  }
}
