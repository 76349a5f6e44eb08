// decide.inc -- the Q-learning bots' action selection on the device (include/aigar.h
// aigar_decide*; DESIGN.md §4h).  Included by api.hip: the selection's device state and
// its kernel; the entry points are in api.hip.
//
// The reference's QLearn.decideMove (qLearning.py:208-243) for every live NN player at
// once: the e-Greedy coin, the Boltzmann draw (boltzmannDist + numpy.random.choice,
// qLearning.py:8-13, 223-226) or numpy.argmax, then the row of the discrete action table
// (network.py:26-65).  All arithmetic is float64 in the reference's operation order
// (compiled with -ffp-contract=off; the only fused multiply-adds are pow_glibc's).
//
// k_decide (wave64, gfx950): one wave per player, four players per block, lanes over
// the actions.  The maximum and numpy.argmax's first index are wave reductions; the
// n_out pow_glibc calls of the Boltzmann weights run side by side; numpy.sum's pairwise
// association is kept (eight strided accumulators per block of <= 128, blocks split at
// n / 2 rounded down to 8); the cumsum is a serial chain by one lane, as any other
// association rounds differently; searchsorted and the first-equal search are wave-wide
// again.  d / p and the cdf live in the wave's LDS slice (2 * n_out doubles); the greedy
// paths (no explore, temperature 0) touch no LDS.  Every branch is per wave: an
// exploring, a dead and a greedy player may share a block.

#include "aigar_wave.h"

struct Decide {  // aigar_decide_config (n_out 0: off); plain, no padding: part of the decision graph's key
  int n_out, strategy, q_dtype, pad;
  uint64_t seed;
  double *table;  // [n_out][4] the discrete actions
  double *act;    // [NP][4] the chosen rows (the decision graph's actions)
  double *idx;    // [NP] the chosen index as a double (the replay memory's action source)
};

constexpr int kDecWaves = 4;  // players per block

// numpy's pairwise sum (loops_utils.h) of a[0 .. n) in LDS, by the whole wave; every lane
// returns the same value.  A block of 8 <= n <= 128: lanes j, j + 8, ... each run
// accumulator j % 8 (redundantly in the wave's eight groups), the xor butterfly over the
// low three lane bits is ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) in every lane
// (a + b == b + a), then the remainder in sequence.
__device__ __forceinline__ double dec_sum_block(const double *a, int n, int lane) {
  if (n < 8) {
    double r = 0.;
    for (int i = 0; i < n; i++) r += a[i];
    return r;
  }
  const int j = lane & 7, full = n - (n % 8);
  double r = a[j];
  for (int i = 8; i < full; i += 8) r += a[i + j];
  r = r + __shfl_xor(r, 1);
  r = r + __shfl_xor(r, 2);
  r = r + __shfl_xor(r, 4);
  for (int i = full; i < n; i++) r += a[i];
  return r;
}
// the split above 128 elements: depth D covers n <= 1024 with D = 4 (a half is at most
// n / 2 + 7: 1024 -> 519 -> 266 -> 140 -> 77), unrolled at compile time -- no call stack
template <int D>
__device__ __forceinline__ double dec_sum(const double *a, int n, int lane) {
  if (n <= 128) return dec_sum_block(a, n, lane);
  if constexpr (D > 0) {
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double left = dec_sum<D - 1>(a, n2, lane);
    return left + dec_sum<D - 1>(a + n2, n - n2, lane);
  } else {
    return __builtin_nan("");  // (unreachable for n <= 1024)
  }
}

template <class T>
__device__ __forceinline__ double dec_q(const void *q, size_t i) {
  return (double)((const T *)q)[i];
}

// idx_out [NP], val_out [NP]; act (null: none) [NP][4] gets the chosen table rows of the
// deciding players, c.idx the index as a double.  u: [NP][3] draws or null (own Philox).
template <class T>
__global__ void __launch_bounds__(64 * kDecWaves) k_decide(Dev d, Decide c, const void *q, const double *explore,
                                                           const double *u, int32_t *idx_out, double *val_out,
                                                           double *act) {
  extern __shared__ double dec_lds[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int gp = blockIdx.x * kDecWaves + w;
  if (gp >= d.NP) return;
  const int n = c.n_out;
  // only live NN players decide (bot.py:223-226)
  if (!d.p_alive[gp] || d.p_role[gp] != AIGAR_ROLE_NN) {
    if (lane == 0) {
      idx_out[gp] = -1;
      val_out[gp] = __builtin_nan("");
      c.idx[gp] = -1.0;
    }
    return;
  }
  const size_t row = (size_t)gp * n;
  // numpy.argmax: the first index of the maximum; a NaN or an infinity in the row
  bool bad = false;
  double m = -__builtin_inf();
  int mi = 0x7fffffff;
  for (int i = lane; i < n; i += 64) {
    const double v = dec_q<T>(q, row + i);
    bad |= !(fabs(v) < __builtin_inf());
    if (mi == 0x7fffffff || v > m) {
      m = v;
      mi = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double om = __shfl_xor(m, off);
    const int oi = __shfl_xor(mi, off);
    if (oi != 0x7fffffff && (mi == 0x7fffffff || om > m || (om == m && oi < mi))) {
      m = om;
      mi = oi;
    }
  }
  int idx = mi;
  double val = m;
  const int a = gp / d.B;
  if (__any(bad)) {  // outside the contract: index 0 and a warn bit, nothing else
    idx = 0;
    val = dec_q<T>(q, row);
    if (lane == 0) atomicOr(&d.ctl[a].warn, (uint32_t)WARN_Q_NONFINITE);
  } else {
    double u0, u1, u2;
    if (u) {
      u0 = u[(size_t)gp * 3];
      u1 = u[(size_t)gp * 3 + 1];
      u2 = u[(size_t)gp * 3 + 2];
    } else {
      uint64_t o[4];
      philox((uint64_t)gp, ST_DECIDE, (uint64_t)d.ctl[a].tick, c.seed, d.ctl[a].key0, d.ctl[a].key1, o);
      u0 = u01(o[0]);
      u1 = u01(o[1]);
      u2 = u01(o[2]);
    }
    const double epsilon = explore[0], temperature = explore[1];
    if (c.strategy == 0) {
      if (u0 < epsilon) {  // decideExploration (qLearning.py:208-215); the draw-to-index map is the device's own
        const double x = u1 * (double)n;
        idx = x >= 0 ? (x < (double)n ? (int)x : n - 1) : 0;
        val = __builtin_nan("");
      }
    } else if (temperature != 0) {
      double *dl = dec_lds + (size_t)w * 2 * n, *cl = dl + n;
      // boltzmannDist (qLearning.py:8-13): math.e ** ((value - maxVal) / temp)
      for (int i = lane; i < n; i += 64)
        dl[i] = aigar_math::pow_glibc(2.718281828459045, (dec_q<T>(q, row + i) - m) / temperature);
      wave_fence();
      const double s = dec_sum<4>(dl, n, lane);
      wave_fence();  // (every lane has read its d before they become p)
      for (int i = lane; i < n; i += 64) dl[i] = dl[i] / s;
      wave_fence();
      // numpy.random.choice(p=p): cdf = p.cumsum(); cdf /= cdf[-1]; searchsorted(u, side='right')
      double acc = 0.;
      if (lane == 0)
        for (int i = 0; i < n; i++) {
          acc += dl[i];
          cl[i] = acc;
        }
      wave_fence();
      const double total = __shfl(acc, 0);
      int cnt = 0;
      for (int i = lane; i < n; i += 64) cnt += (cl[i] / total <= u2) ? 1 : 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
      const int k = cnt < n - 1 ? cnt : n - 1;
      // numpy.argmax(q_Values == action_value): equal probabilities fold onto the first
      const double pk = dl[k];
      int j = 0x7fffffff;
      for (int i = lane; i < n; i += 64)
        if (dl[i] == pk) {
          j = i;
          break;
        }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) j = min(j, __shfl_xor(j, off));
      idx = j < n ? j : k;  // (j >= n: p_k is a NaN, outside the contract)
      val = pk;
    }
  }
  if (lane < 4) {
    const double t = c.table[(size_t)idx * 4 + lane];
    if (act) act[(size_t)gp * 4 + lane] = t;
  }
  if (lane == 0) {
    idx_out[gp] = idx;
    val_out[gp] = val;
    c.idx[gp] = (double)idx;
  }
}

static void launch_decide(const Dev &d, hipStream_t s, const Decide &c, const void *q, const double *explore,
                          const double *u, int32_t *idx_out, double *val_out, double *act) {
  const dim3 grid((d.NP + kDecWaves - 1) / kDecWaves), block(64 * kDecWaves);
  const size_t lds = c.strategy == 1 ? sizeof(double) * 2 * kDecWaves * (size_t)c.n_out : 0;
  if (c.q_dtype == 0) hipLaunchKernelGGL(k_decide<double>, grid, block, lds, s, d, c, q, explore, u, idx_out, val_out, act);
  else hipLaunchKernelGGL(k_decide<float>, grid, block, lds, s, d, c, q, explore, u, idx_out, val_out, act);
}
