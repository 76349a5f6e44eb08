// dpg.inc -- the DPG learner's training step on the device (include/aigar.h aigar_dpg*,
// aigar_qcritic_config; DESIGN.md §4n), and what the SPG learner's (spg.inc) shares with it: the
// state of a Q(s, a) trainer (DPGTrain), the critic half's kernels and the tail's body.  Included
// by api.hip after actrain.inc; the entry points are in api.hip.
//
// The reference's trainer (actorCritic.py ActorCritic.learn for ALGORITHM == "DPG":
// train_critic_DPG 986-1029, train_actor_DPG 751-789 on createCombinedActorCritic 581-598,
// softlyUpdateTargetModel 366-373).  tests/dpg_model.py is the specification in plain Python.
// The critic Q(s, a) takes rows [s, a] of n_s + n_act values.  One step is one captured graph:
//   k_exp_draw, k_exp_fetch   (replay.inc) the mini-batch into the staging rows
// the critic half (api.hip launch_qsa_critic: DPG's and SPG's)
//   k_net          mu2 = the actor's target on s2
//   k_sa_pack      the rows [s, a] and [s2, mu2]
//   k_net_save     q = Q([s, a]) with the critic, its hidden activations kept
//   k_net          q2 = Q([s2, mu2]) with the critic's target
//   k_td_q         one workgroup: targets, TD errors, priorities (SPG's prio_evals: |Q(s, a)| in the
//                  TD error's place), the critic's output delta, the step's skip decision (k_td_v's
//                  without the selection)
//   k_net_bwd, k_net_grad_adam  (train.inc) on the critic's view
//   k_exp_update   (replay.inc, prioritized memory)
// the actor half, with the critic as just updated and both targets as before this step
//   k_net_save     mu = the actor on s, its hidden activations kept
//   k_net          mu- = the actor's target on s
//   k_sa_pack      the rows [s, mu] and [s, mu-]
//   k_net_save     qmu = Q([s, mu]) with the critic, its hidden activations kept
//   k_net          qt = Q([s, mu-]) with the critic's target
//   k_dpg_delta    one workgroup: the combined model's output delta, the half's skip decision,
//                  the actor's lr_t
//   k_net_bwd      on the critic's view for the actor pass: delta_0, no gradient is formed
//   k_net_bwd_in   dQ/da = delta_0 W_0^T on the action rows of W_0, times mu (1 - mu): the
//                  actor's output delta
//   k_net_bwd, k_net_grad_adam  on the actor's view
// and k_dpg_tail: dpg_tail (the soft update or the due hard copy of both targets, the critic's
// counters; k_spg_tail calls it too) with the actor half's counter.
//
// The forward, backward and gradient kernels are net.inc's and train.inc's, unchanged: each
// network has a Train of its own; `ca` is the critic's with a TrainCtl whose skip is the actor
// half's (SPG has no pass through the critic: its ca is c, and mut stays null).

struct DPGTrain {  // aigar_dpg_config, and SPGTrain's d (api.hip qsa_setup; batch 0: off)
  int batch = 0, n_s = 0, n_act = 0, soft = 0;  // soft: tau > 0 (else the hard copy)
  float tau = 0, keep = 0;                      // float32(tau), float32(1.0 - tau)
  double q_increase = 0;
  Train c, a, ca;  // the critic's, the actor's, the critic's for the actor pass (c's buffers, its own ctl)
  // c.s / c.s2: the packed rows [s, a] / [s2, mu2]; a.s / a.s2: the drawn states;
  // c.q = Q(s, a), c.q2 = Q'(s2, mu2), a.q = mu(s), a.q2 = mu'(s2); a.ctl->t is t_a
  char *xm = nullptr, *xt = nullptr;      // the packed rows [s, mu] / [s, mu-]
  double *mut = nullptr;                  // [batch][n_act] mu-(s)
  double *qm = nullptr, *qt = nullptr;    // [batch] Q([s, mu]), Q'([s, mu-])
};

// Two row sets in one launch, a row a workgroup: out[r] = [state row r (n_s values of T), the
// first n_act values of the float64 action row r cast to T].  A NaN state row stays one.
template <class T>
__global__ void __launch_bounds__(64) k_sa_pack(int B, int n_s, int n_act, const T *s0, const double *a0, int stride0,
                                                T *o0, const T *s1, const double *a1, int stride1, T *o1) {
  const int set = (int)blockIdx.x / B, r = (int)blockIdx.x % B, n = n_s + n_act;
  const T *s = (set ? s1 : s0) + (size_t)r * n_s;
  const double *a = (set ? a1 : a0) + (size_t)r * (set ? stride1 : stride0);
  T *o = (set ? o1 : o0) + (size_t)r * n;
  for (int i = threadIdx.x; i < n; i += 64) o[i] = i < n_s ? s[i] : (T)a[i - n_s];
}

// k_td_v without the selection: targets, TD errors (float64), priorities, the critic's delta and
// the step's decisions, every piece train.inc's.  With prio_evals (SPG) the priority of an applied
// step's row is |Q(s, a)| + 1e-4: the reference hands get_evals' Q(s, a) to the memory in the TD
// error's place (aigar.py:1081).  DPG passes 0.
__global__ void __launch_bounds__(kTrainMaxBatch) k_td_q(Train c, Exp e, Dev d, int n_layers, int prio_evals) {
  const int r = threadIdx.x, B = c.batch;
  const bool small = train_small(c, e);
  double td = 0.0;
  bool bad = false;
  if (r < B && !small) td = td_scalar(c, r, bad);
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (r < B) {
    delta_scalar(c, n_layers, r, td_prio_grad(c, r, small || any_bad, td, 1));
    if (prio_evals && !small && !any_bad) c.prio[r] = fabs(c.q[r]) + 1e-4;
  }
  if (r == 0) td_decide(c, e, d, small, any_bad);
}

// The combined model's output delta (mse of Q([s, mu]) against Q'([s, mu-]) + q_increase, every
// row, no importance weights) into the last delta row of the critic's view for the actor pass, and
// the actor half's decisions: it is skipped with the step, or when a delta is not finite.
__global__ void __launch_bounds__(kTrainMaxBatch) k_dpg_delta(DPGTrain t, Dev d, int n_layers) {
  const Train &c = t.c, &a = t.a;
  const int r = threadIdx.x, B = t.batch;
  const bool live = !c.ctl->skip;  // (uniform: written by k_td_q)
  float g = 0.0f;
  bool bad = false;
  if (live && r < B) {
    const double tgt = t.qt[r] + t.q_increase;
    g = (float)((2.0 * (t.qm[r] - tgt)) / (double)(1 * B));
    bad = !(fabsf(g) < __builtin_inff());
    delta_scalar(t.ca, n_layers, r, g);
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (r == 0) {
    const int skip = (live && !any_bad) ? 0 : 1;
    t.ca.ctl->skip = skip;
    a.ctl->skip = skip;  // (k_net_bwd_in may still raise it)
    a.ctl->lr_t = adam_lr_t(a, a.ctl->t + 1);
    if (any_bad) atomicOr(&d.ctl[0].warn, (uint32_t)WARN_TRAIN_NONFINITE);
  }
}

// ea[r][k] = sum_j delta_0[r][j] W_0[n_s + k][j]: the critic's error carried through its first
// layer onto the action columns of its input, one workgroup, one wave per 16 batch rows, on
// v_mfma_f32_16x16x4_f32 as k_net_bwd's product.  A = delta_0 (row r16, k-step j), B = W_0^T on
// the input rows n_s .. n_s + n_act - 1 (column r16 < n_act; the other columns supply +0.0f and
// are dropped).  ONE accumulator runs through all of j in ascending order; a padded step is
// -0.0f (delta) times +0.0f (weight).  D: ea[row 4 g + reg][action r16].  The lanes of a real
// (r, k) form the actor's output delta float32((double)ea (mu (1 - mu))); the block's vote on a
// non-finite one skips the actor's update.
__global__ void __launch_bounds__(64 * (kTrainMaxBatch / 16)) k_net_bwd_in(Net cr, DPGTrain t, Dev d, int actor_layers) {
  const Train &ca = t.ca, &a = t.a;
  if (ca.ctl->skip) return;  // (uniform)
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4, row0 = 16 * ((int)threadIdx.x >> 6);
  const int B = t.batch, n_act = t.n_act, op = net_out_pad(cr.out[0]);
  const bool col = r16 < n_act, arow = row0 + r16 < B;
  const float *wr = cr.w[0] + (size_t)(t.n_s + (col ? r16 : 0)) * op + g;  // (row n_s + k < in_0)
  const float *ar = ca.delta + (size_t)(row0 + r16) * kNetMaxUnits + g;     // (row < bpad)
  net_f4 acc = net_f4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < op; j += 16) {
    float bv[4], av[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      bv[s] = col ? wr[j + 4 * s] : 0.0f;
      av[s] = arow ? ar[j + 4 * s] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  bool bad = false;
  float *dl = a.delta + ((size_t)(actor_layers - 1) * a.bpad + row0) * kNetMaxUnits + r16;
#pragma unroll
  for (int reg = 0; reg < 4; reg++) {
    const int row = 4 * g + reg;
    if (row0 + row < B) {
      float v = -0.0f;  // (a padded unit)
      if (col) {
        const double mu = a.q[(size_t)(row0 + row) * n_act + r16];
        v = (float)((double)acc[reg] * (mu * (1.0 - mu)));
        bad = bad || !(fabsf(v) < __builtin_inff());
      }
      dl[(size_t)row * kNetMaxUnits] = v;
    }
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (threadIdx.x == 0 && any_bad) {
    a.ctl->skip = 1;
    atomicOr(&d.ctl[0].warn, (uint32_t)WARN_TRAIN_NONFINITE);
  }
}

// theta- = float32(float32(theta- keep) + float32(theta tau)) over a padded copy (+0 stays +0)
__device__ __forceinline__ void dpg_target(const Net &n, const Train &v, bool soft, float tau, float keep) {
  for (int l = 0; l < n.n_layers; l++) {
    const size_t op = net_out_pad(n.out[l]), nw = (size_t)net_in_pad(n.in[l]) * op;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
      if (soft) {
        v.tw[l][i] = __fadd_rn(__fmul_rn(v.tw[l][i], keep), __fmul_rn(n.w[l][i], tau));
        if (i < op) v.tb[l][i] = __fadd_rn(__fmul_rn(v.tb[l][i], keep), __fmul_rn(n.b[l][i], tau));
      } else {
        v.tw[l][i] = n.w[l][i];
        if (i < op) v.tb[l][i] = n.b[l][i];
      }
    }
  }
}

// The end of a Q(s, a) trainer's step, DPG's and SPG's: both targets' soft update (tau > 0, after
// every applied step) or their hard copy when due, then in one thread the critic's counters and,
// after an applied step, actor_half(): the trainer's own booking of its actor half's outcome.
template <class F>
__device__ __forceinline__ void dpg_tail(const Net &cr, const Net &ac, const DPGTrain &t, F actor_half) {
  TrainCtl *cc = t.c.ctl;
  const int skip = cc->skip, due = cc->due;  // (the tail kernels leave them)
  const bool soft = t.soft != 0;
  if (!skip && (soft || due)) {
    dpg_target(cr, t.c, soft, t.tau, t.keep);
    dpg_target(ac, t.a, soft, t.tau, t.keep);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (skip) {
      cc->skipped += 1;
    } else {
      cc->t += 1;
      cc->since = (!soft && due) ? 0 : cc->since + 1;
      actor_half();
    }
  }
}

// The step's end: dpg_tail, the actor half's counter from its skip decision.
__global__ void __launch_bounds__(256) k_dpg_tail(Net cr, Net ac, DPGTrain t) {
  TrainCtl *ac_ctl = t.a.ctl;
  const int askip = ac_ctl->skip;  // (this kernel leaves it)
  dpg_tail(cr, ac, t, [&] {
    if (askip) ac_ctl->skipped += 1;
    else ac_ctl->t += 1;
  });
}

// aigar_dpg_reset: both step counters to zero
__global__ void k_dpg_clear(TrainCtl *c, TrainCtl *a) {
  c->t = 0;
  a->t = 0;
}
