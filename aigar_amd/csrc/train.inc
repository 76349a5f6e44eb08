// train.inc -- the Q-learning network's training step on the device (include/aigar.h
// aigar_train*; DESIGN.md §4l).  Included by api.hip: the trainer's device state and its
// kernels; the entry points are in api.hip.
//
// The reference's trainer (qLearning.py:116-193 QLearn.train, network.py:378-392
// trainOnBatch; Keras 2.2.4 Adam on loss='mse' with the prioritized memory's importance
// weights as sample_weight, a hard target copy every TARGET_NETWORK_STEPS).
// tests/train_model.py is the specification in plain Python.  One step is one captured
// graph:
//   k_exp_draw, k_exp_fetch   (replay.inc) the mini-batch into the handle's staging rows
//   k_net_save                (net.inc) the online pass; every hidden layer's activations kept
//   k_net                     the target pass, on a Net whose weights are the target's
//   k_td          one workgroup: targets, TD errors, priorities, the output delta, and the
//                 step's skip decision, a flag that every later kernel of the step reads first
//   k_net_bwd     16 batch rows a workgroup: delta back through the layers, tiles through LDS
//   k_net_grad_adam  one wave per 16 x 16 tile of a layer's kernel: dW, db and Adam in place,
//                 in the padded layout that k_net reads
//   k_exp_update  (replay.inc, prioritized memory) the priorities; a skipped step's are all 0
//   k_train_tail  the counters and, when due, the target copy
//
// Both products run on v_mfma_f32_16x16x4_f32 as k_net's do: the f32-input MFMA is exact,
// and every output carries ONE accumulator through its whole chain in ascending order, so
// the result is the model's fmaf chain.
//   e[r][k]   = sum_j delta_l[r][j] W_l[k][j]   A = delta_l (row r, k-step j), B = W_l^T
//   dW[k][j]  = sum_r h_{l-1}[r][k] delta_l[r][j]   A = h^T (row k, k-step r), B = delta_l
// Padding as in net.inc: a padded step multiplies -0.0f with +0.0f, and acc + (-0.0f) == acc
// for every acc.  Padded units of a delta or an activation row are -0.0f (against the
// kernels' +0.0f padding); batch rows beyond the batch enter as h = -0.0f, delta = +0.0f.
// Adam touches only the real entries, so the padded entries of the packed copies stay 0.0f.

struct TrainCtl {  // device-resident counters and the running step's decisions
  int64_t t, skipped, since;  // steps applied, steps skipped, steps since the last target copy
  int32_t skip, due;          // this step: skipped / followed by the target copy
  double lr_t;                // this step's lr * sqrt(1 - beta2^t) / (1 - beta1^t)
};

struct Train {  // aigar_train_config (batch 0: off)
  int batch = 0, bpad = 0, min_size = 0, target_steps = 0;
  double lr = 0, beta1 = 0, beta2 = 0, epsilon = 0, discount = 0;
  float *tw[kNetMaxLayers] = {}, *tb[kNetMaxLayers] = {};  // the target network, packed as Net's
  float *mw[kNetMaxLayers] = {}, *mb[kNetMaxLayers] = {};  // Adam's m
  float *vw[kNetMaxLayers] = {}, *vb[kNetMaxLayers] = {};  // ... and v, in the same layout
  int tile0[kNetMaxLayers + 1] = {};  // first gradient tile of every layer
  char *s = nullptr, *s2 = nullptr;   // the drawn rows, [batch][L] of the memory's dtype
  double *a = nullptr, *r = nullptr, *w = nullptr, *u = nullptr;  // [batch][4], [batch], [batch], [batch]
  uint8_t *done = nullptr;
  int64_t *idx = nullptr;
  double *q = nullptr, *q2 = nullptr;     // [batch][n_out] online on s, target on s2
  double *td = nullptr, *prio = nullptr;  // [batch]
  float *hsave = nullptr;                 // [n_layers - 1][bpad][kNetMaxUnits] hidden activations
  float *delta = nullptr;                 // [n_layers][bpad][kNetMaxUnits]
  TrainCtl *ctl = nullptr;
};

constexpr int kTrainMaxBatch = 256;  // k_td is one workgroup, a row a thread

// ---- what the three learners' TD kernels share (k_td here, k_td_v in actrain.inc, k_td_q in
// dpg.inc), so that a replay priority and a skipped step mean the same under each of them

// a view's lr * sqrt(1 - beta2^tn) / (1 - beta1^tn) for its step number tn
__device__ __forceinline__ double adam_lr_t(const Train &v, int64_t tn) {
  return v.lr * sqrt(1.0 - aigar_math::pow_glibc(v.beta2, (double)tn)) / (1.0 - aigar_math::pow_glibc(v.beta1, (double)tn));
}

// The memory holds fewer than max(batch, min_size) transitions (a prioritized one fewer than 2):
// no step.
__device__ __forceinline__ bool train_small(const Train &t, const Exp &e) {
  const int64_t size = e.ctl->size;
  const int64_t need = t.batch > t.min_size ? t.batch : t.min_size;
  return size < need || (e.prio && size < 2);
}

// Row r's priority and the value of its output delta's one entry, d(w mse)/dq over the
// n_out * batch entries of the output.
__device__ __forceinline__ float td_prio_grad(const Train &t, int r, bool skip, double td, int n_out) {
  t.prio[r] = skip ? 0.0 : fabs(td) + 1e-4;  // (k_exp_update passes over an entry that is not > 0)
  return skip ? 0.0f : (float)(((2.0 * t.w[r]) * (-td)) / (double)(n_out * t.batch));
}

// Thread 0's decisions of a step: the flags that every later kernel of the step reads first, the
// view's lr_t, the memory's draw count and the warn bit.
__device__ __forceinline__ void td_decide(const Train &t, const Exp &e, const Dev &d, bool small, bool any_bad) {
  TrainCtl *ctl = t.ctl;
  const bool skip = small || any_bad;
  const int64_t tn = ctl->t + 1;
  ctl->skip = skip ? 1 : 0;
  ctl->due = (!skip && t.target_steps > 0 && tn % t.target_steps == 0) ? 1 : 0;
  ctl->lr_t = adam_lr_t(t, tn);
  if (!small) e.ctl->calls += 1;  // (the memory's own draws of this step are used)
  if (any_bad) atomicOr(&d.ctl[0].warn, (uint32_t)WARN_TRAIN_NONFINITE);
}

// A scalar critic's row r (V(s), Q(s, a): q and q2 are [batch]): its TD error (float64), kept
// in c.td; bad: it is not finite.
__device__ __forceinline__ double td_scalar(const Train &c, int r, bool &bad) {
  double tg = c.r[r];
  if (!c.done[r]) tg = tg + c.discount * c.q2[r];
  const double td = tg - c.q[r];
  bad = !(fabs(td) < __builtin_inf());
  c.td[r] = td;
  return td;
}

// ... and the output delta row of a one-unit head: g, then the padded units
__device__ __forceinline__ void delta_scalar(const Train &v, int n_layers, int r, float g) {
  float *row = v.delta + ((size_t)(n_layers - 1) * v.bpad + r) * kNetMaxUnits;
  for (int j = 0; j < 16; j++) row[j] = j == 0 ? g : -0.0f;
}

// Targets, TD errors (float64, qLearning.py:116-129), priorities, the output delta and the
// step's decisions.  The step is skipped when the memory is too small, and, with the warn bit,
// when a TD error is not finite or a stored action index is outside the head.
__global__ void __launch_bounds__(kTrainMaxBatch) k_td(Train t, Exp e, Dev d, int n_layers, int n_out) {
  const int r = threadIdx.x, B = t.batch;
  const bool small = train_small(t, e);
  int a = 0;
  double td = 0.0;
  bool bad = false;
  if (r < B && !small) {
    const double av = t.a[(size_t)r * 4];
    double tg = t.r[r];
    if (!t.done[r]) {
      const double *row = t.q2 + (size_t)r * n_out;
      double m = row[0];
      for (int j = 1; j < n_out; j++) {
        const double v = row[j];
        if (v != v || v > m) m = v;  // (a NaN stays: no value is greater than it)
      }
      tg = tg + t.discount * m;
    }
    if (av >= 0.0 && av < (double)n_out) {
      a = (int)av;
      td = tg - t.q[(size_t)r * n_out + a];
      bad = !(fabs(td) < __builtin_inf());
    } else {
      td = __builtin_nan("");
      bad = true;
    }
    t.td[r] = td;
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (r < B) {
    const float g = td_prio_grad(t, r, small || any_bad, td, n_out);
    float *row = t.delta + ((size_t)(n_layers - 1) * t.bpad + r) * kNetMaxUnits;
    const int op = net_out_pad(n_out);
    for (int j = 0; j < op; j++) row[j] = j == a ? g : (j < n_out ? 0.0f : -0.0f);
  }
  if (r == 0) td_decide(t, e, d, small, any_bad);
}

// delta_l -> delta_{l - 1} for l = n_layers - 1 ... 1, 16 batch rows a workgroup, four waves.
// The 16-unit tiles of layer l - 1 are dealt to the waves; delta_l is the A operand from LDS,
// W_l^T the B operand from the packed kernel (row k, four consecutive j a lane group).
__global__ void __launch_bounds__(64 * kNetWaves) k_net_bwd(Net c, Train t) {
  __shared__ float dl[2][kNetRows][kNetHStride];
  if (t.ctl->skip) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * kNetRows, B = t.batch, L = c.n_layers;
  {
    const int op = net_out_pad(c.out[L - 1]);
    const float *src = t.delta + ((size_t)(L - 1) * t.bpad + row0) * kNetMaxUnits;
    for (int i = tid; i < kNetRows * op; i += 64 * kNetWaves) {
      const int row = i / op, j = i % op;
      dl[0][row][j] = row0 + row < B ? src[(size_t)row * kNetMaxUnits + j] : 0.0f;
    }
  }
  __syncthreads();
  int cur = 0;
  for (int l = L - 1; l >= 1; l--) {
    const int op = net_out_pad(c.out[l]), K = c.in[l], nt = net_out_pad(K) >> 4;
    const float *W = c.w[l];
    const float *hp = t.hsave + ((size_t)(l - 1) * t.bpad + row0) * kNetMaxUnits;
    float *dg = t.delta + ((size_t)(l - 1) * t.bpad + row0) * kNetMaxUnits;
    for (int tile = w; tile < nt; tile += kNetWaves) {  // (uniform in a wave)
      const float *wr = W + (size_t)(16 * tile + r16) * op + g;  // (row < in_pad: the packed copy has it)
      const float *ar = &dl[cur][r16][g];
      net_f4 acc = net_f4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < op; j += 16) {
        float bv[4], av[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
          bv[s] = wr[j + 4 * s];
          av[s] = ar[j + 4 * s];
        }
#pragma unroll
        for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
      }
      // D: e[row 4 g + reg][unit 16 tile + r16]
      const int k = 16 * tile + r16;
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int row = 4 * g + reg;
        float v = acc[reg];
        if (c.hid_act == AIGAR_ACT_RELU) v = hp[(size_t)row * kNetMaxUnits + k] > 0.f ? v : 0.0f;
        if (k >= K) v = -0.0f;  // (a padded unit is the next chain's padded step)
        dl[cur ^ 1][row][k] = v;
        if (row0 + row < B) dg[(size_t)row * kNetMaxUnits + k] = v;
      }
    }
    cur ^= 1;
    __syncthreads();
  }
}

// Keras 2.2.4 Adam (amsgrad off) on one parameter: m, v float32, the arithmetic float64 on
// the widened values, every operation rounding on its own (-ffp-contract=off).
__device__ __forceinline__ void train_adam(const Train &t, double lr_t, float g, float *p, float *m, float *v) {
  const double g64 = (double)g;
  const float mn = (float)(t.beta1 * (double)*m + (1.0 - t.beta1) * g64);
  const float vn = (float)(t.beta2 * (double)*v + (1.0 - t.beta2) * (g64 * g64));
  *m = mn;
  *v = vn;
  *p = (float)((double)*p - lr_t * (double)mn / (sqrt((double)vn) + t.epsilon));
}

// One wave per 16 x 16 tile (k0, j0) of a layer's kernel, all layers in one launch: the chain
// over the batch rows in ascending order, then Adam on the tile in place.  The tiles of the
// first 16 k also take the bias: a plain float32 sum over ascending rows.  T: the states' dtype
// (the first layer's h is the drawn state, rounded once).
template <class T>
__global__ void __launch_bounds__(64) k_net_grad_adam(Net c, Train t) {
  if (t.ctl->skip) return;
  const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4, B = t.batch;
  int l = 0;
  while (l + 1 < c.n_layers && (int)blockIdx.x >= t.tile0[l + 1]) l++;
  const int n = c.out[l], op = net_out_pad(n), K = c.in[l], tj = op >> 4;
  const int tile = (int)blockIdx.x - t.tile0[l], k0 = 16 * (tile / tj), j0 = 16 * (tile % tj);
  const float *dp = t.delta + (size_t)l * t.bpad * kNetMaxUnits + j0 + r16;
  const float *hp = l ? t.hsave + (size_t)(l - 1) * t.bpad * kNetMaxUnits + k0 + r16 : nullptr;
  const T *xp = (const T *)t.s + k0 + r16;
  const bool kin = k0 + r16 < K;
  net_f4 acc = net_f4{0.f, 0.f, 0.f, 0.f};
  for (int r0 = 0; r0 < B; r0 += 16) {
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int r = r0 + 4 * s + g;
      const bool in = r < B;
      if (l) av[s] = in ? hp[(size_t)r * kNetMaxUnits] : -0.0f;
      else av[s] = (in && kin) ? (float)xp[(size_t)r * K] : -0.0f;
      bv[s] = in ? dp[(size_t)r * kNetMaxUnits] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  const double lr_t = t.ctl->lr_t;
  // D: dW[k0 + 4 g + reg][j0 + r16]
  const int j = j0 + r16;
#pragma unroll
  for (int reg = 0; reg < 4; reg++) {
    const int k = k0 + 4 * g + reg;
    if (k < K && j < n) {
      const size_t i = (size_t)k * op + j;
      train_adam(t, lr_t, acc[reg], c.w[l] + i, t.mw[l] + i, t.vw[l] + i);
    }
  }
  if (k0 == 0 && g == 0 && j < n) {
    float db = 0.0f;
    for (int r = 0; r < B; r++) db = db + dp[(size_t)r * kNetMaxUnits];
    train_adam(t, lr_t, db, c.b[l] + j, t.mb[l] + j, t.vb[l] + j);
  }
}

// The step's end: the counters and, when due, target <- online (the padded copies whole).
__global__ void __launch_bounds__(256) k_train_tail(Net c, Train t) {
  TrainCtl *ctl = t.ctl;
  const int skip = ctl->skip, due = ctl->due;  // (written by k_td; this kernel leaves them)
  if (due) {
    for (int l = 0; l < c.n_layers; l++) {
      const size_t op = net_out_pad(c.out[l]), nw = (size_t)net_in_pad(c.in[l]) * op;
      for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
        t.tw[l][i] = c.w[l][i];
        if (i < op) t.tb[l][i] = c.b[l][i];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (skip) {
      ctl->skipped += 1;
    } else {
      ctl->t += 1;
      ctl->since = due ? 0 : ctl->since + 1;
    }
  }
}

// the padded copy -> W [in][out], b [out] (Keras' layout)
__global__ void k_net_unpack(const float *wp, const float *bp, float *W, float *b, int in, int out, int out_pad) {
  const size_t n = (size_t)in * out;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t k = i / out, j = i % out;
    W[i] = wp[k * out_pad + j];
    if (k == 0) b[j] = bp[j];
  }
}

// the padded entries of a packed copy whose bit pattern is not +0.0f's, counted
__global__ void k_net_pad_count(const float *wp, const float *bp, int in, int out, int in_pad, int out_pad,
                                unsigned long long *count) {
  const size_t n = (size_t)in_pad * out_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / out_pad), j = (int)(i % out_pad);
    int bad = 0;
    if ((k >= in || j >= out) && __float_as_uint(wp[i]) != 0u) bad++;
    if (k == 0 && j >= out && __float_as_uint(bp[j]) != 0u) bad++;
    if (bad) atomicAdd(count, (unsigned long long)bad);
  }
}
