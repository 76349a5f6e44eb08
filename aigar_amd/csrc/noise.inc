// noise.inc -- the actor-critic learners' exploration noise on the device (include/aigar.h
// aigar_noise*; DESIGN.md §4i).  Included by api.hip: the noise's device state and its
// kernel; the entry points are in api.hip.
//
// The reference's ActorCritic.applyNoise (actorCritic.py:922-936) for every live NN
// player at once: numpy's legacy Gaussian (the polar method of RandomState.normal, with
// glibc's log) added to the actor's output, or the Ornstein-Uhlenbeck recurrence, then
// numpy.clip(a, 0, 1).  All arithmetic is float64 in the reference's operation order
// (compiled with -ffp-contract=off; the only fused multiply-adds are log_glibc's).
// tests/noise_model.py is the specification in plain Python.
//
// k_noise (wave64, gfx950): one lane per (row, pair of values); a pair is one accepted
// attempt of the polar method, so a row of 2 values uses one lane and a row of 3 or 4
// two.  The rejection loop is bounded by T <= 16 attempts and only searches: the one
// log_glibc call, the division and the square root come after it, so the loop body is a
// handful of multiplies and no lane waits in it for another lane's logarithm.  The log
// table is read from constant memory like the pow tables; all stores are plain vector
// stores; the only atomics are the warn bit's or and the exhaustion counter's add.

struct Noise {  // aigar_noise_config (n_act 0: off); plain, no padding: part of the decision graph's key
  int n_act, type, mu_dtype, store_raw;
  double theta, ou_mu, dt;
  uint64_t seed;
  double *act;  // [NP][n_act] the noisy actions (the decision graph's actions)
  double *raw;  // [NP][n_act] the actor's own outputs of the rows that decided (CACLA's fifth field)
  double *ou;   // [NP][n_act] the Orn-Uhl state of every player
};

constexpr int kNoiseMaxT = 16;   // attempts per pair at the most
constexpr int kNoiseOwnT = 16;   // ... with own draws
constexpr int kNoiseThreads = 256;

template <class T>
__device__ __forceinline__ double noise_mu(const void *mu, size_t i) {
  return (double)((const T *)mu)[i];
}

// mu [rows][n_act]; std: one device double; u: [rows][2][T][2] draws or null (own Philox);
// env != 0 (the decision): rows == NP, only live NN players decide, the state is c.ou and
// the rows go to c.act / c.raw (and noisy_out, NaN where nobody decides); env == 0 (the
// call): every row is perturbed into noisy_out, the state is the caller's prev.
template <class T>
__global__ void __launch_bounds__(kNoiseThreads) k_noise(Dev d, Noise c, const void *mu, int rows, int env,
                                                         const double *std, const double *u, int nT, double *prev,
                                                         double *noisy_out, unsigned long long *n_exhausted) {
  const size_t gid = (size_t)blockIdx.x * kNoiseThreads + threadIdx.x;
  const size_t row = gid >> 1;
  const int pair = (int)(gid & 1), n = c.n_act, i0 = 2 * pair;
  if (row >= (size_t)rows || i0 >= n) return;
  const int nv = n - i0 < 2 ? n - i0 : 2;  // values of this pair
  if (env && (!d.p_alive[row] || d.p_role[row] != AIGAR_ROLE_NN)) {  // (bot.py:223-226)
    if (noisy_out)
      for (int j = 0; j < nv; j++) noisy_out[row * n + i0 + j] = __builtin_nan("");
    return;
  }
  const int a = (int)((row / (size_t)d.B) % (size_t)d.A);
  uint32_t warn = 0;
  double s = std[0];
  if (!(s >= 0.0 && s < __builtin_inf())) {  // outside the contract: no noise and a warn bit
    s = 0.0;
    warn |= WARN_NOISE_NONFINITE;
  }
  // the polar method (numpy legacy_gauss): the first attempt with 0 < r2 < 1
  double x1 = 0., x2 = 0., r2 = 0.;
  bool ok = false;
  if (u) {
    const double *ur = u + (row * 2 + pair) * (size_t)nT * 2;
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
    const uint64_t tick = (uint64_t)d.ctl[a].tick, k0 = d.ctl[a].key0, k1 = d.ctl[a].key1;
    for (int b = 0; b < kNoiseOwnT / 2; b++) {  // one Philox block is two attempts
      if (ok) break;
      uint64_t o[4];
      philox((uint64_t)row, ST_NOISE | (uint64_t)pair << 8 | (uint64_t)b << 16, tick, c.seed, k0, k1, o);
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
  double z[2] = {0., 0.};
  if (ok) {
    const double f = sqrt(-2.0 * aigar_math::log_glibc(r2) / r2);
    z[0] = f * x2;  // numpy returns f * x2 first and keeps f * x1 for the next call
    z[1] = f * x1;
  } else {
    warn |= WARN_NOISE_EXHAUSTED;
    if (n_exhausted) atomicAdd(n_exhausted, 1ull);
  }
  double *state = c.type == AIGAR_NOISE_ORN_UHL ? (env ? c.ou : prev) : nullptr;
  const double sd = s * sqrt(c.dt);
#pragma unroll
  for (int j = 0; j < 2; j++) {
    if (j >= nv) break;
    const size_t i = row * n + i0 + j;
    double m = noise_mu<T>(mu, i);
    if (!(fabs(m) < __builtin_inf())) {  // outside the contract: taken as 0 and a warn bit
      m = 0.0;
      warn |= WARN_NOISE_NONFINITE;
    }
    double v;
    if (state) {  // actorCritic.py:930-935, in Python's association
      const double p = state[i];
      double nz = p + c.theta * (c.ou_mu - p) * c.dt + sd * z[j];
      if (!(fabs(nz) < __builtin_inf())) {  // outside the contract (a huge std, a non-finite prev): restart at 0
        nz = 0.0;
        warn |= WARN_NOISE_NONFINITE;
      }
      state[i] = nz;
      v = m + nz;
    } else {
      v = m + s * z[j];
    }
    v = v < 0.0 ? 0.0 : v;  // numpy.clip(a, 0, 1): only a < 0 becomes 0.0, so a -0.0 stays -0.0
    v = v > 1.0 ? 1.0 : v;
    if (env) {
      c.act[i] = v;
      c.raw[i] = m;
    }
    if (noisy_out) noisy_out[i] = v;
  }
  if (warn) atomicOr(&d.ctl[a].warn, warn);
}

static void launch_noise(const Dev &d, hipStream_t s, const Noise &c, const void *mu, int rows, int env,
                         const double *std, const double *u, int nT, double *prev, double *noisy_out,
                         unsigned long long *n_exhausted) {
  const dim3 grid((unsigned)(((size_t)rows * 2 + kNoiseThreads - 1) / kNoiseThreads)), block(kNoiseThreads);
  if (c.mu_dtype == 0)
    hipLaunchKernelGGL(k_noise<double>, grid, block, 0, s, d, c, mu, rows, env, std, u, nT, prev, noisy_out, n_exhausted);
  else
    hipLaunchKernelGGL(k_noise<float>, grid, block, 0, s, d, c, mu, rows, env, std, u, nT, prev, noisy_out, n_exhausted);
}

// the Orn-Uhl state restarts at zero wherever the bots' history does (actorCritic.py:1121-1123)
__global__ void k_noise_clear_arenas(double *ou, int per, ArenaSel sel) {
  for (int i = threadIdx.x; i < per; i += blockDim.x) ou[(size_t)sel.arena(blockIdx.x) * per + i] = 0.0;
}
__global__ void k_noise_clear_bots(double *ou, int n, int n_act, const uint8_t *mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i]))
    for (int j = 0; j < n_act; j++) ou[(size_t)i * n_act + j] = 0.0;
}
