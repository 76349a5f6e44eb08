// spg.inc -- the SPG (Sampled Policy Gradient) learner's training step on the device
// (include/aigar.h aigar_spg*; DESIGN.md §4o).  Included by api.hip after dpg.inc: the trainer's
// device state and its control kernels; the entry points are in api.hip.
//
// The reference's trainer (actorCritic.py ActorCritic.learn for OCACLA_ENABLED 730-733:
// train_critic_DPG(get_evals=True) 986-1029, train_actor_OCACLA 860-919).  tests/spg_model.py is
// the specification in plain Python.  One step is one captured graph, a linear chain:
//   k_exp_draw, k_exp_fetch, k_exp_extra_get (replay.inc) the mini-batch and, with replace, the
//                  drawn slots' fifth field
// the critic half: DPG's (dpg.inc; api.hip launch_qsa_critic), k_td_q with this trainer's prio_evals
// the search, with the critic as just updated and the actor as it is
//   k_net_save     mu = the actor on s, its hidden activations kept
//   k_sa_pack      the rows [s, mu] and [s, extra]
//   k_net          qmu = Q([s, mu]); with replace and K > 0 also qe = Q([s, extra])
//   k_spg_pick     one workgroup, a row a thread: best starts as the stored action with the value
//                  from before the critic's update, then the extra and mu are compared
//   K rounds of
//     k_spg_cand   a row a workgroup: the Gaussian pair(s) around the row's base, the clip, the
//                  packed row [s, cand]
//     k_net        Q([s, cand])
//     k_spg_pick   the comparison
// the actor half
//   k_spg_delta    one workgroup: the selection, count, the actor's output delta towards best, the
//                  half's decision, the actor's lr_t, the rows of the write-back
//   k_net_bwd, k_net_grad_adam  (train.inc) on the actor's view
//   k_spg_writeback  (replace) k_exp_extra_set's last-wins scheme on the drawn slots
// and k_spg_tail: dpg.inc's dpg_tail (both targets' update, the critic's counters) with this
// trainer's booking of the actor half, the noise's decay and the ordinal.
//
// The Gaussian pair is spg_gauss_pair, a copy of k_noise's arithmetic (see there).  Every loop is bounded by a
// compile-time constant (AIGAR_SPG_MAX_SAMPLES rounds, 16 attempts a pair); all stores are plain
// vector stores; the only atomics are the warn bit's or and the write-back's max.

constexpr int kSpgMaxSamples = 8;

struct SCtl {  // device-resident state of the search
  double noise;            // the search noise's std (aigar_spg_noise: the caller may write it)
  int64_t ord;             // steps run since the configuration or the last reset (the own draws' counter)
  int64_t aempty;          // actor halves without a selected row (total)
  int32_t sel, half;       // the last applied step: rows selected; this step: 0 applied, 1 empty, 2 not finite
};

struct SPGTrain {  // aigar_spg_config (d.batch 0: off)
  DPGTrain d;  // the batch, the views and DPG's buffers: d.xm the rows [s, candidate], d.qm their values,
               // d.xt the rows [s, extra], d.qt their values; d.c.q stays Q(s, a) from before the update
  int K = 0, moving = 0, replace = 0, prio_evals = 0, fused = 0;  // fused: the search is k_spg_search's
  double noise0 = 0, noise_decay = 0;
  uint64_t seed = 0;
  double *ex = nullptr;    // [batch][4] the drawn slots' extras
  uint8_t *exv = nullptr;  // [batch] ... and whether they are valid
  double *best = nullptr, *cand = nullptr, *rows = nullptr;  // [batch][4] each; rows: the write-back
  double *beval = nullptr, *qmu = nullptr;                   // [batch]
  double *zu = nullptr;    // [batch][K][2][16][2] the caller's uniforms of the running step
  SCtl *x = nullptr;
};

// Row r's first comparisons, float64 `>` (a NaN never wins): best starts as the stored action with
// Q(s, a) from before the critic's update; with K > 0 the valid extra (replace) and then mu are
// compared.  qe, qm: Q([s, extra]) and Q([s, mu]) of the row.  Both search paths call it.
__device__ __forceinline__ double spg_first_pick(const SPGTrain &t, int r, double qe, double qm, double (&b)[4]) {
  const Train &a = t.d.a;
  const int n_act = t.d.n_act;
  double be = t.d.c.q[r];
  for (int j = 0; j < 4; j++) b[j] = j < n_act ? a.a[(size_t)r * 4 + j] : 0.0;
  if (t.K > 0) {
    if (t.replace && t.exv[r] && qe > be) {
      for (int j = 0; j < n_act; j++) b[j] = t.ex[(size_t)r * 4 + j];
      be = qe;
    }
    if (qm > be) {
      for (int j = 0; j < n_act; j++) b[j] = a.q[(size_t)r * n_act + j];
      be = qm;
    }
  }
  return be;
}

// The comparisons of a row, a row a thread, float64 `>` (a NaN never wins).  first: best starts as
// the stored action with Q(s, a) from before the critic's update; with K > 0 the valid extra
// (replace) and then mu are compared.  Otherwise: the round's candidate.
__global__ void __launch_bounds__(kTrainMaxBatch) k_spg_pick(SPGTrain t, int first) {
  const int r = threadIdx.x;
  if (r >= t.d.batch) return;
  double *best = t.best + (size_t)r * 4;
  if (!first) {
    const double ev = t.d.qm[r];
    if (ev > t.beval[r]) {
      for (int j = 0; j < 4; j++) best[j] = t.cand[(size_t)r * 4 + j];
      t.beval[r] = ev;
    }
    return;
  }
  double b[4];
  const double be = spg_first_pick(t, r, (t.K > 0 && t.replace) ? t.d.qt[r] : 0.0, t.qmu[r], b);
  for (int j = 0; j < 4; j++) best[j] = b[j];
  t.beval[r] = be;
}

// numpy's legacy Gaussian pair (the polar method of legacy_gauss): the first of the attempts with
// 0 < r2 < 1; false: every attempt was rejected and z = (0, 0).  ur: the pair's nT <= kNoiseMaxT
// attempts [nT][2], or null: kNoiseOwnT own attempts, two a Philox block, block b at the counter
// (c0, c1 | b << 16, c2, c3) under the key (k0, k1).  The arithmetic of k_noise's (noise.inc), kept
// in step with it by hand: lifting it out of k_noise into a function both call moved k_noise's
// registers (DESIGN.md §4o), so k_noise stays as it is.
__device__ __forceinline__ bool spg_gauss_pair(const double *ur, int nT, uint64_t c0, uint64_t c1, uint64_t c2,
                                                 uint64_t c3, uint64_t k0, uint64_t k1, double (&z)[2]) {
  double x1 = 0., x2 = 0., r2 = 0.;
  bool ok = false;
  if (ur) {
    for (int t = 0; t < nT; t++) {
      if (ok) break;
      const double y1 = 2.0 * ur[2 * t] - 1.0, y2 = 2.0 * ur[2 * t + 1] - 1.0;
      const double r = y1 * y1 + y2 * y2;
      if (r < 1.0 && r != 0.0) {
        x1 = y1;
        x2 = y2;
        r2 = r;
        ok = true;
      }
    }
  } else {
    for (int b = 0; b < kNoiseOwnT / 2; b++) {  // one Philox block is two attempts
      if (ok) break;
      uint64_t o[4];
      philox(c0, c1 | (uint64_t)b << 16, c2, c3, k0, k1, o);
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const double y1 = 2.0 * u01(o[2 * h]) - 1.0, y2 = 2.0 * u01(o[2 * h + 1]) - 1.0;
        const double r = y1 * y1 + y2 * y2;
        if (!ok && r < 1.0 && r != 0.0) {
          x1 = y1;
          x2 = y2;
          r2 = r;
          ok = true;
        }
      }
    }
  }
  z[0] = z[1] = 0.;
  if (ok) {
    const double f = sqrt(-2.0 * aigar_math::log_glibc(r2) / r2);
    z[0] = f * x2;  // numpy returns f * x2 first and keeps f * x1 for the next call
    z[1] = f * x1;
  }
  return ok;
}

// One pair of round x's candidate of `row`: the Gaussian pair (the caller's attempts ur, or
// Philox under arena 0's key at (row, ST_SPG | pair << 8 | b << 16 | x << 24, ord, seed)) around the
// base values m[0..1], clipped as numpy.clip(a, 0, 1), into v[0..nv - 1]; returns the warn bits.
__device__ __forceinline__ uint32_t spg_cand_pair(const Dev &d, const SPGTrain &t, const double *ur, uint64_t row, int pair,
                                                  int x, int nv, const double *m, double *v) {
  uint32_t warn = 0;
  double s = t.x->noise;
  if (!(s >= 0.0 && s < __builtin_inf())) {  // outside the contract: no noise and a warn bit
    s = 0.0;
    warn |= WARN_NOISE_NONFINITE;
  }
  double z[2];
  if (!spg_gauss_pair(ur, kNoiseMaxT, row, ST_SPG | (uint64_t)pair << 8 | (uint64_t)x << 24, (uint64_t)t.x->ord, t.seed,
                        d.ctl[0].key0, d.ctl[0].key1, z))
    warn |= WARN_NOISE_EXHAUSTED;
  for (int j = 0; j < nv; j++) {
    double b = m[j];
    if (!(fabs(b) < __builtin_inf())) {  // outside the contract: taken as 0 and a warn bit
      b = 0.0;
      warn |= WARN_NOISE_NONFINITE;
    }
    double c = b + s * z[j];
    c = c < 0.0 ? 0.0 : c;  // only a < 0 becomes 0.0, so a -0.0 stays -0.0
    v[j] = c > 1.0 ? 1.0 : c;
  }
  return warn;
}

// Round x's candidate of every row, a row a workgroup: lanes 0 and 1 draw the pairs around the
// row's base (best under moving, else mu), clip as numpy.clip(a, 0, 1) and leave the values in
// LDS; then the workgroup packs the row [s, cand] of the states' dtype T.
template <class T>
__global__ void __launch_bounds__(64) k_spg_cand(SPGTrain t, Dev d, int x, int has_zu) {
  __shared__ double cs[4];
  const int r = blockIdx.x, tid = threadIdx.x, n_act = t.d.n_act, n_s = t.d.n_s;
  const Train &a = t.d.a;
  const bool live = !t.d.c.ctl->skip;  // (a skipped step's warn bits are not raised)
  if (tid < 2) {
    const int pair = tid, i0 = 2 * pair;
    uint32_t warn = 0;
    if (i0 < n_act) {
      const int nv = n_act - i0 < 2 ? n_act - i0 : 2;
      const double *ur = has_zu ? t.zu + ((((size_t)r * t.K + x) * 2 + pair) * kNoiseMaxT) * 2 : nullptr;
      double m[2] = {0., 0.}, v[2];
      for (int j = 0; j < nv; j++) m[j] = t.moving ? t.best[(size_t)r * 4 + i0 + j] : a.q[(size_t)r * n_act + i0 + j];
      warn = spg_cand_pair(d, t, ur, (uint64_t)r, pair, x, nv, m, v);
      for (int j = 0; j < nv; j++) {
        cs[i0 + j] = v[j];
        t.cand[(size_t)r * 4 + i0 + j] = v[j];
      }
    }
    for (int i = i0; i < i0 + 2; i++)
      if (i >= n_act) t.cand[(size_t)r * 4 + i] = 0.0;
    if (warn && live) atomicOr(&d.ctl[0].warn, warn);
  }
  __syncthreads();
  const T *s = (const T *)a.s + (size_t)r * n_s;
  T *o = (T *)t.d.xm + (size_t)r * (n_s + n_act);
  for (int i = tid; i < n_s + n_act; i += 64) o[i] = i < n_s ? s[i] : (T)cs[i - n_s];
}

// ---- fused = 1: the whole search of 16 rows in one block (k_net's lane map, net_wload / net_chunk)
//
// Of the critic's first layer, the whole 64-k chunks that lie entirely below n_s are the same for
// every candidate of a row: they run once, their accumulators are kept (acc0), and every candidate
// -- mu, the extra, each sample -- restores them and finishes the chain with the remaining chunks
// (the state's tail, the candidate's n_act values, the -0.0f padding): the same MFMAs in the same
// ascending order as k_net's, so one accumulator per tile still runs through all of k.  The further
// layers run from LDS as net_layer's; the head's value of a row lands in LDS, lanes 0..15 compare
// (k_spg_pick's rules) and lanes 0..31 draw the next candidate (k_spg_cand's) from the row's best.
// Bounded by 2 + kSpgMaxSamples candidates and 16 attempts a pair; no cross-block dependence.

struct SpgLds {
  float xs[kNetRows][kNetXStride];
  float hid[2][kNetRows][kNetHStride];
  double cs[kNetRows][4];    // the running candidate of every row
  double best[kNetRows][4];  // ... and its best so far
  double q[kNetRows], be[kNetRows], qmu[kNetRows], qe[kNetRows];
};

// the epilogue of net_layer: bias, activation, the next layer's tile in LDS or the head's value
template <int NT>
__device__ __forceinline__ void spg_finish(const Net &c, int l, const net_f4 (&acc)[NT], SpgLds &m, int dst) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int n = c.out[l], op = net_out_pad(n), nt = op >> 4;
  const bool last = l == c.n_layers - 1;
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const int t = w + kNetWaves * i;
    if (t < nt) {
      const int j = 16 * t + r16;
      const float bj = c.b[l][j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 4 * g + r;
        const float yv = acc[i][r] + bj;  // one float32 add
        if (!last) {
          const float hv = c.hid_act == AIGAR_ACT_RELU ? (yv > 0.f ? yv : 0.0f) : yv;
          m.hid[dst][row][j] = j < n ? hv : -0.0f;
        } else if (j == 0) {
          m.q[row] = (double)yv;  // (the critic's head is one linear unit)
        }
      }
    }
  }
  if (!last) {
    const int extra = net_in_pad(n) - op;
    for (int i = tid; i < kNetRows * extra; i += 64 * kNetWaves) m.hid[dst][i / extra][op + i % extra] = -0.0f;
  }
  __syncthreads();
}

// layer l >= 1 from the hidden tile src (net_layer's chain without its prefetch)
template <int NT>
__device__ __forceinline__ void spg_layer(const Net &c, int l, SpgLds &m, int &src) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int op = net_out_pad(c.out[l]), nt = op >> 4, nc = net_in_pad(c.in[l]) / kNetKC;
  int col[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) col[i] = 16 * min(w + kNetWaves * i, nt - 1) + r16;
  net_f4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc[i] = net_f4{0.f, 0.f, 0.f, 0.f};
  float bc[kNetKC / 4][NT];
  for (int ch = 0; ch < nc; ch++) {
    net_wload<NT>(bc, c.w[l], op, ch * kNetKC, g, col);
    net_chunk<NT>(acc, &m.hid[src][r16][ch * kNetKC + g], bc);
  }
  spg_finish<NT>(c, l, acc, m, src ^ 1);
  src ^= 1;
}

// T: the states' dtype; NT: the first layer's tiles of a wave at the most
template <class T, int NT>
__global__ void __launch_bounds__(64 * kNetWaves) k_spg_search(Net cr, SPGTrain t, Dev d, int has_zu) {
  __shared__ SpgLds m;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int row0 = (int)blockIdx.x * kNetRows, B = t.d.batch, n_s = t.d.n_s, n_act = t.d.n_act, K0 = n_s + n_act;
  const Train &a = t.d.a;
  const T *S = (const T *)a.s;
  const int op = net_out_pad(cr.out[0]), nt = op >> 4, nc = net_in_pad(K0) / kNetKC;
  const int np = n_s / kNetKC;  // the whole chunks below n_s (np < nc: the actions lie behind them)
  const bool live = !t.d.c.ctl->skip, extras = t.replace && t.K > 0;
  int col[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) col[i] = 16 * min(w + kNetWaves * i, nt - 1) + r16;
  float bc[kNetKC / 4][NT];
  // chunk ch of the rows [s, cs] into xs: column `lane` of rows w, w + 4, w + 8, w + 12
  auto stage = [&](int ch) {
    const int k = ch * kNetKC + lane;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = w + 4 * i;
      float v = -0.0f;
      if (row0 + row < B && k < K0) v = k < n_s ? (float)S[(size_t)(row0 + row) * n_s + k] : (float)(T)m.cs[row][k - n_s];
      m.xs[row][lane] = v;
    }
    __syncthreads();
  };
  net_f4 acc0[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc0[i] = net_f4{0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < np; ch++) {
    stage(ch);
    net_wload<NT>(bc, cr.w[0], op, ch * kNetKC, g, col);
    net_chunk<NT>(acc0, &m.xs[r16][g], bc);
    __syncthreads();
  }
  // Q([s, cs]) of the 16 rows into m.q
  auto evaluate = [&]() {
    net_f4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; i++) acc[i] = acc0[i];
    for (int ch = np; ch < nc; ch++) {
      stage(ch);
      net_wload<NT>(bc, cr.w[0], op, ch * kNetKC, g, col);
      net_chunk<NT>(acc, &m.xs[r16][g], bc);
      __syncthreads();
    }
    spg_finish<NT>(cr, 0, acc, m, 0);
    int src = 0;
    for (int l = 1; l < cr.n_layers; l++) {
      switch ((net_out_pad(cr.out[l]) / 16 + kNetWaves - 1) / kNetWaves) {
        case 1: spg_layer<1>(cr, l, m, src); break;
        case 2: spg_layer<2>(cr, l, m, src); break;
        case 3: spg_layer<3>(cr, l, m, src); break;
        default: spg_layer<4>(cr, l, m, src); break;
      }
    }
  };
  const int row = tid >> 2, j4 = tid & 3;  // (tid < 64: value j4 of row `row`)
  const bool mine = tid < 4 * kNetRows && row0 + row < B;
  // mu
  if (tid < 4 * kNetRows) m.cs[row][j4] = (mine && j4 < n_act) ? a.q[(size_t)(row0 + row) * n_act + j4] : 0.0;
  __syncthreads();
  evaluate();
  if (tid < kNetRows) m.qmu[tid] = m.q[tid];
  // the extra
  if (extras) {
    __syncthreads();
    if (tid < 4 * kNetRows) m.cs[row][j4] = (mine && j4 < n_act) ? t.ex[(size_t)(row0 + row) * 4 + j4] : 0.0;
    __syncthreads();
    evaluate();
    if (tid < kNetRows) m.qe[tid] = m.q[tid];
  }
  __syncthreads();
  // the first comparisons
  if (tid < kNetRows && row0 + tid < B) {
    double b[4];
    const double be = spg_first_pick(t, row0 + tid, extras ? m.qe[tid] : 0.0, m.qmu[tid], b);
    for (int j = 0; j < 4; j++) m.best[tid][j] = b[j];
    m.be[tid] = be;
  }
  __syncthreads();
  for (int x = 0; x < t.K; x++) {  // (K <= kSpgMaxSamples)
    if (tid < 2 * kNetRows) {
      const int rw = tid >> 1, pair = tid & 1, i0 = 2 * pair, r = row0 + rw;
      double v[2] = {0., 0.};
      if (r < B && i0 < n_act) {
        const int nv = n_act - i0 < 2 ? n_act - i0 : 2;
        const double *ur = has_zu ? t.zu + ((((size_t)r * t.K + x) * 2 + pair) * kNoiseMaxT) * 2 : nullptr;
        double b[2] = {0., 0.};
        for (int j = 0; j < nv; j++) b[j] = t.moving ? m.best[rw][i0 + j] : a.q[(size_t)r * n_act + i0 + j];
        const uint32_t warn = spg_cand_pair(d, t, ur, (uint64_t)r, pair, x, nv, b, v);
        if (warn && live) atomicOr(&d.ctl[0].warn, warn);
      }
      m.cs[rw][i0] = v[0];
      m.cs[rw][i0 + 1] = v[1];
    }
    __syncthreads();
    evaluate();
    if (tid < kNetRows && row0 + tid < B && m.q[tid] > m.be[tid]) {
      for (int j = 0; j < 4; j++) m.best[tid][j] = j < n_act ? m.cs[tid][j] : 0.0;
      m.be[tid] = m.q[tid];
    }
    __syncthreads();
  }
  if (tid < kNetRows && row0 + tid < B) {
    const int r = row0 + tid;
    for (int j = 0; j < 4; j++) t.best[(size_t)r * 4 + j] = m.best[tid][j];
    t.beval[r] = m.be[tid];
    t.qmu[r] = m.qmu[tid];
  }
}

// The selection (best_eval > qmu), count, the actor's output delta towards best on the selected
// rows (k_actor_delta's rule: +0.0f on the others), the half's decision, the actor's lr_t, and the
// rows of the write-back: best padded with zeros for a selected row, the stored action otherwise.
__global__ void __launch_bounds__(kTrainMaxBatch) k_spg_delta(SPGTrain t, Dev d, int n_layers, int n_out) {
  const Train &a = t.d.a;
  const int r = threadIdx.x, B = t.d.batch;
  const bool live = !t.d.c.ctl->skip;  // (uniform: written by k_td_q)
  const bool sel = live && r < B && t.beval[r] > t.qmu[r];
  const int count = __syncthreads_count(sel ? 1 : 0);
  bool bad = false;
  if (live && r < B) {
    float *row = a.delta + ((size_t)(n_layers - 1) * a.bpad + r) * kNetMaxUnits;
    const int op = net_out_pad(n_out);
    for (int j = 0; j < op; j++) {
      float v = j < n_out ? 0.0f : -0.0f;
      if (sel && j < n_out) {
        const double mu = a.q[(size_t)r * n_out + j], act = t.best[(size_t)r * 4 + j];
        v = (float)(((2.0 * (mu - act)) / (double)(n_out * count)) * (mu * (1.0 - mu)));
        bad = bad || !(fabsf(v) < __builtin_inff());
      }
      row[j] = v;
    }
    for (int j = 0; j < 4; j++)
      t.rows[(size_t)r * 4 + j] = sel ? (j < n_out ? t.best[(size_t)r * 4 + j] : 0.0) : a.a[(size_t)r * 4 + j];
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (r == 0) {
    const bool apply = live && count > 0 && !any_bad;
    a.ctl->skip = apply ? 0 : 1;
    a.ctl->lr_t = adam_lr_t(a, a.ctl->t + 1);
    if (live) {
      t.x->sel = count;
      t.x->half = count == 0 ? 1 : any_bad ? 2 : 0;
      if (any_bad) atomicOr(&d.ctl[0].warn, (uint32_t)WARN_TRAIN_NONFINITE);
    }
  }
}

// k_exp_extra_set on the step's own rows (one workgroup; the last entry of a repeated index
// wins), unless the step is skipped.
__global__ void __launch_bounds__(kExpPlanThreads) k_spg_writeback(SPGTrain s, Exp e) {
  if (s.d.c.ctl->skip) return;  // (uniform)
  const int t = threadIdx.x, n = s.d.batch;
  const int64_t *idx = s.d.a.idx;
  const int64_t size = e.ctl->size;
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    if (i >= 0 && i < size) atomicMax(&e.last[i], j);
  }
  __syncthreads();
  for (int j = t; j < n; j += kExpPlanThreads) {
    const int64_t i = idx[j];
    if (i < 0 || i >= size || e.last[i] != j) continue;
    for (int v = 0; v < 4; v++) e.x[i * 4 + v] = s.rows[(size_t)j * 4 + v];
    e.xv[i] = 1;
  }
  __syncthreads();
  for (int j = t; j < n; j += kExpPlanThreads) {  // the scratch is -1 again for the next call
    const int64_t i = idx[j];
    if (i >= 0 && i < size) e.last[i] = -1;
  }
}

// The step's end: dpg_tail with the actor half's three outcomes and noise <- noise * noise_decay
// after an applied step, then the steps' ordinal.
__global__ void __launch_bounds__(256) k_spg_tail(Net cr, Net ac, SPGTrain s) {
  TrainCtl *ac_ctl = s.d.a.ctl;
  SCtl *x = s.x;
  dpg_tail(cr, ac, s.d, [&] {
    if (x->half == 0) ac_ctl->t += 1;
    else if (x->half == 1) x->aempty += 1;
    else ac_ctl->skipped += 1;
    x->noise = x->noise * s.noise_decay;
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) x->ord += 1;
}

// aigar_spg_config (all: the noise and the totals start over) and aigar_spg_reset: both step
// counters and the ordinal to zero
__global__ void k_spg_clear(TrainCtl *c, TrainCtl *a, SCtl *x, double noise, int all) {
  c->t = 0;
  a->t = 0;
  x->ord = 0;
  if (all) {
    x->noise = noise;
    x->aempty = 0;
    x->sel = 0;
    x->half = 0;
  }
}
