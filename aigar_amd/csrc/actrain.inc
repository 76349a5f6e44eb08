// actrain.inc -- the CACLA learner's training step on the device (include/aigar.h
// aigar_actrain*, aigar_critic*; DESIGN.md §4m).  Included by api.hip after train.inc: the
// trainer's device state and its two control kernels; the entry points are in api.hip.
//
// The reference's trainer (actorCritic.py ActorCritic.learn for ALGORITHM == "CACLA":
// train_critic 1032-1065, train_actor_batch 791-858, the critic's hard target copy 745-746;
// CACLA_VAR_ENABLED picks the number of actor epochs of a row from its TD error).
// tests/cacla_model.py is the specification in plain Python.  One step is one captured graph:
//   k_exp_draw, k_exp_fetch   (replay.inc) the mini-batch into the staging rows
//   k_net_save                (net.inc) V(s) with the critic, its hidden activations kept
//   k_net                     V(s2) with the critic's target
//   k_td_v        one workgroup: targets, TD errors, priorities, the critic's output delta, the
//                 step's skip decision, the running variance and every row's epoch count
//   k_net_bwd, k_net_grad_adam  (train.inc) on the critic's view
//   k_exp_update  (replay.inc, prioritized memory)
// then max(var_epochs, 1) times the actor epoch
//   k_net_save                mu(s) with the actor as it is NOW
//   k_actor_delta one workgroup: n_e, the actor's output delta on the rows that take part,
//                 the epoch's skip decision, the actor's lr_t and step counter
//   k_net_bwd, k_net_grad_adam  on the actor's view
// and k_train_tail (train.inc) on the critic's view: the counters and the target copy.
//
// The backward and gradient kernels are train.inc's, unchanged: each network has a Train
// of its own (m, v, hsave, delta, TrainCtl) that shares the staged batch.

struct ACtl {  // device-resident state of the selection and the actor's epochs
  double var;                 // CACLA-Var's running variance of the TD error
  int64_t cut, eskipped;      // rows cut down to var_epochs, actor epochs skipped (totals)
  int32_t sel, epochs, stop;  // the last step: rows selected, epochs; this step: an epoch was skipped
};

struct ACTrain {  // aigar_actrain_config (batch 0: off)
  int batch = 0, var_epochs = 0;
  double var_start = 0, var_beta = 0;
  Train c, a;  // the critic's and the actor's view (c.q = V(s), c.q2 = V(s2), a.q = mu(s); a.ctl->t is t_a)
  int32_t *count = nullptr;  // [batch] actor epochs of every row of the last step
  ACtl *x = nullptr;
};

// Targets, TD errors (float64), priorities, the critic's delta and the step's decisions as
// k_td's, then the selection.  The variance's recurrence is the one serial part: one lane runs it
// over ascending r and leaves every row's value in LDS.
__global__ void __launch_bounds__(kTrainMaxBatch) k_td_v(ACTrain t, Exp e, Dev d, int n_layers) {
  __shared__ double tds[kTrainMaxBatch], vars[kTrainMaxBatch];
  __shared__ int emax;
  const Train &c = t.c;
  const int r = threadIdx.x, B = t.batch, E = t.var_epochs;
  const bool small = train_small(c, e);
  ACtl *x = t.x;
  double td = 0.0;
  bool bad = false;
  if (r < B && !small) td = td_scalar(c, r, bad);
  tds[r] = td;
  if (r == 0) emax = 0;
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  const bool skip = small || any_bad;
  if (r < B) delta_scalar(c, n_layers, r, td_prio_grad(c, r, skip, td, 1));
  if (r == 0) {
    td_decide(c, e, d, small, any_bad);
    x->stop = 0;
    if (!skip && E > 0) {
      double var = x->var;
      const double keep = 1.0 - t.var_beta;
      for (int i = 0; i < B; i++) {
        const double v = tds[i];
        var = keep * var + t.var_beta * (v * v);
        vars[i] = var;
      }
      x->var = var;
    }
  }
  __syncthreads();
  int n = 0, cut = 0;
  if (r < B && !skip && td > 0.0) {
    if (E == 0) {
      n = 1;
    } else {
      const double cr = ceil(td / sqrt(vars[r]));
      const bool in = cr >= 1.0 && cr <= (double)E;  // (false for a NaN or an infinity)
      n = in ? (int)cr : E;
      cut = in ? 0 : 1;
    }
  }
  if (r < B) t.count[r] = n;
  if (n) atomicMax(&emax, n);
  const int sel = __syncthreads_count(n > 0);
  const int ncut = __syncthreads_count(cut);
  if (r == 0) {
    x->sel = sel;
    x->epochs = emax;
    x->cut += ncut;
  }
}

// Epoch e of the step's actor update: the rows with count > e take part, the others enter with a
// +0.0f delta.  The epoch is skipped when the step was, when e is not below the step's epochs,
// when an earlier epoch of the step was skipped, or when a delta is not finite.
__global__ void __launch_bounds__(kTrainMaxBatch) k_actor_delta(ACTrain t, Dev d, int e, int n_layers, int n_out) {
  const Train &a = t.a;
  const int r = threadIdx.x, B = t.batch;
  ACtl *x = t.x;
  const bool live = !t.c.ctl->skip && e < x->epochs;  // (uniform: both were written by k_td_v)
  const bool run = live && !x->stop;
  const bool part = run && r < B && t.count[r] > e;
  const int n_e = __syncthreads_count(part ? 1 : 0);  // (a ballot and a popcount a wave, summed)
  bool bad = false;
  if (run && r < B) {
    float *row = a.delta + ((size_t)(n_layers - 1) * a.bpad + r) * kNetMaxUnits;
    const int op = net_out_pad(n_out);
    for (int j = 0; j < op; j++) {
      float v = j < n_out ? 0.0f : -0.0f;
      if (part && j < n_out) {
        const double mu = a.q[(size_t)r * n_out + j], act = a.a[(size_t)r * 4 + j];
        v = (float)(((2.0 * (mu - act)) / (double)(n_out * n_e)) * (mu * (1.0 - mu)));
        bad = bad || !(fabsf(v) < __builtin_inff());
      }
      row[j] = v;
    }
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (r == 0) {
    const bool apply = run && !any_bad;
    TrainCtl *ctl = a.ctl;
    ctl->skip = apply ? 0 : 1;
    if (apply) {
      const int64_t tn = ctl->t + 1;
      ctl->lr_t = adam_lr_t(a, tn);
      ctl->t = tn;
    } else if (live) {
      x->eskipped += 1;
      x->stop = 1;
      if (any_bad) atomicOr(&d.ctl[0].warn, (uint32_t)WARN_TRAIN_NONFINITE);
    }
  }
}

// aigar_actrain_reset: both step counters to zero, the variance to its start
__global__ void k_actrain_clear(TrainCtl *c, TrainCtl *a, ACtl *x, double var_start) {
  c->t = 0;
  a->t = 0;
  x->var = var_start;
}
