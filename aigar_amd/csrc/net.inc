// net.inc -- the learners' acting network on the device (include/aigar.h aigar_net*;
// DESIGN.md §4j).  Included by api.hip: the network's device state and its kernels; the
// entry points are in api.hip.
//
// The reference's acting networks are small MLPs (network.py:207-241, actorCritic.py:219-330:
// Q_LAYERS / CACLA_ACTOR_LAYERS = (100, 100), relu, a linear Q head or a sigmoid actor
// head).  tests/net_model.py is the specification in plain Python: per layer and unit ONE
// float32 fmaf chain over k = 0, 1, ..., in - 1 from +0.0f, then one float32 add of the
// bias; the sigmoid head in float64 through pow_glibc.
//
// k_net (wave64, gfx950): one launch for the whole network.  A block of four waves takes
// 16 rows through all layers; the 16-unit tiles of a layer are dealt to the waves (tile t
// to wave t % 4), so a wave carries at most four accumulators, which are also the
// independent MFMAs that cover v_mfma_f32_16x16x4_f32's dependent latency.  The product is
// D[row][unit] = X[row][k] W[k][unit] with X the A operand: D comes out with the unit on the
// lane, the next layer needs the unit as its k, so the hidden tile goes through LDS
// (16 x 256 floats, two of them in turn) and never to memory.  The first layer's rows are
// read in chunks of 64 k, coalesced, converted fp64 -> fp32 once and staged in LDS (double
// buffered, one barrier per chunk); the weights are read from the handle's padded copy, a
// chunk ahead into registers, in straight-line code (a block is one wave per SIMD, so every
// load that waits for its own use is a full memory latency on the chain).
// Every output tile carries ONE accumulator through the whole of k in ascending order: the
// exact f32-input MFMA then gives the model's fmaf chain.
//
// Padding.  k is padded with x = -0.0f against w = +0.0f, so a padded step adds the product
// -0.0f: acc + (-0) == acc for EVERY acc, -0.0f included.  (A chain from +0.0f cannot reach
// -0.0f by exact cancellation, which rounds to +0; it can by underflow,
// fmaf(-0x1p-100f, 0x1p-100f, +0.0f) == -0.0f, so padding with +0 products would not be an
// identity.)  Padded units and rows beyond the input are computed and dropped; a row that
// is not evaluated enters as -0.0f, so no NaN of it meets the matrix core.

constexpr int kNetMaxLayers = 5;    // AIGAR_NET_MAX_LAYERS
constexpr int kNetMaxUnits = 256;   // AIGAR_NET_MAX_UNITS
constexpr int kNetMaxIn = 16384;    // AIGAR_NET_MAX_IN
constexpr int kNetRows = 16;        // rows of a block's tile
constexpr int kNetWaves = 4;        // waves of a block; a layer's unit tiles are dealt to them
constexpr int kNetTiles = kNetMaxUnits / 16 / kNetWaves;  // accumulators of a wave at the most
constexpr int kNetKC = 64;          // the first layer's k chunk
constexpr int kNetXStride = kNetKC + 4;       // (stride % 64 == 4: lane (row, k) reads bank 4 row + k)
constexpr int kNetHStride = kNetMaxUnits + 4;

struct Net {  // aigar_net_config (n_layers 0: off); plain, no padding: part of the decision graph's key
  int n_layers, x_dtype, hid_act, out_act;
  int in[kNetMaxLayers], out[kNetMaxLayers];
  float *w[kNetMaxLayers];  // [in_pad][out_pad] zero-padded kernels
  float *b[kNetMaxLayers];  // [out_pad]
  double *y;                // [NP][out of the last layer] the decision's output
};
static_assert(sizeof(Net) == 14 * sizeof(int) + 11 * sizeof(void *), "Net has padding");

__host__ __device__ inline int net_in_pad(int in) { return (in + kNetKC - 1) / kNetKC * kNetKC; }
__host__ __device__ inline int net_out_pad(int out) { return (out + 15) & ~15; }

typedef float net_f4 __attribute__((ext_vector_type(4)));

// the output activation, in float64 (the project's own definition of the sigmoid)
__device__ __forceinline__ double net_head(float y, int act) {
  const double v = (double)y;
  if (act != AIGAR_ACT_SIGMOID) return v;
  double t = -fabs(v);
  if (!(t >= -750.0)) t = -750.0;
  const double z = aigar_math::pow_glibc(2.718281828459045, t);
  return v >= 0.0 ? 1.0 / (1.0 + z) : z / (1.0 + z);
}

// One chunk of 64 k for the wave's NT tiles: the weights of rows kc .. kc + 63 into registers.
// Tile i of wave w is unit tile w + 4 i; a wave with fewer tiles than NT repeats its last
// valid one (a valid address, the product is dropped), so the code has no branch in it.
template <int NT>
__device__ __forceinline__ void net_wload(float (&b)[kNetKC / 4][NT], const float *W, int op, int kc, int g,
                                          const int (&col)[NT]) {
#pragma unroll
  for (int s = 0; s < kNetKC / 4; s++) {
    const float *wr = W + (size_t)(kc + 4 * s + g) * op;
#pragma unroll
    for (int i = 0; i < NT; i++) b[s][i] = wr[col[i]];
  }
}
// ... and its 16 k-steps: a[4 s] is A[row lane % 16][kc + 4 s + lane / 16] in LDS
template <int NT>
__device__ __forceinline__ void net_chunk(net_f4 (&acc)[NT], const float *a, const float (&b)[kNetKC / 4][NT]) {
#pragma unroll
  for (int s = 0; s < kNetKC / 4; s++) {
    const float av = a[4 * s];
#pragma unroll
    for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[s][i], acc[i], 0, 0, 0);
  }
}

// Layer l for a block whose waves carry up to NT tiles each.  The next chunk's weights (and,
// in the first layer, the next chunk's states) are in flight while the matrix core works on
// this one; the last iteration re-loads its own chunk, so nothing in the loop is conditional.
// SAVE (the trainer's online pass, train.inc): every hidden layer's activations also go to
// hsave [n_layers - 1][16 gridDim.x][kNetMaxUnits], padded units as -0.0f.
template <class T, int NT, bool SAVE>
__device__ __forceinline__ void net_layer(const Net &c, int l, const T *x, size_t row0, const bool (&lrow)[4],
                                          float (*xs)[kNetRows][kNetXStride], float (*hid)[kNetRows][kNetHStride],
                                          const int *rowflag, int &src, double *y, float *hsave) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lk = lane;
  const int r16 = lane & 15, g = lane >> 4;
  const int n = c.out[l], op = net_out_pad(n), nt = op >> 4, K = c.in[l];
  const float *W = c.w[l];
  const int nc = net_in_pad(K) / kNetKC;
  int col[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) col[i] = 16 * min(w + kNetWaves * i, nt - 1) + r16;
  net_f4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc[i] = net_f4{0.f, 0.f, 0.f, 0.f};
  float bc[kNetKC / 4][NT], bn[kNetKC / 4][NT];
  net_wload<NT>(bc, W, op, 0, g, col);
  if (l == 0) {
    auto load = [&](int kc, float *v) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int k = kc + lk;
        v[i] = (lrow[i] && k < K) ? (float)x[(row0 + (size_t)(w + 4 * i)) * (size_t)K + k] : -0.0f;
      }
    };
    float v[4];
    load(0, v);
#pragma unroll
    for (int i = 0; i < 4; i++) xs[0][w + 4 * i][lk] = v[i];
    __syncthreads();
    for (int ch = 0; ch < nc; ch++) {
      const int buf = ch & 1, kn = min(ch + 1, nc - 1) * kNetKC;
      load(kn, v);
      net_wload<NT>(bn, W, op, kn, g, col);
      net_chunk<NT>(acc, &xs[buf][r16][g], bc);
#pragma unroll
      for (int i = 0; i < 4; i++) xs[buf ^ 1][w + 4 * i][lk] = v[i];  // (last read in chunk ch - 1, before its barrier)
#pragma unroll
      for (int s = 0; s < kNetKC / 4; s++)
#pragma unroll
        for (int i = 0; i < NT; i++) bc[s][i] = bn[s][i];
      __syncthreads();
    }
  } else {
    for (int ch = 0; ch < nc; ch++) {
      net_wload<NT>(bn, W, op, min(ch + 1, nc - 1) * kNetKC, g, col);
      net_chunk<NT>(acc, &hid[src][r16][ch * kNetKC + g], bc);
#pragma unroll
      for (int s = 0; s < kNetKC / 4; s++)
#pragma unroll
        for (int i = 0; i < NT; i++) bc[s][i] = bn[s][i];
    }
  }
  // D: unit 16 t + lane % 16 of rows 4 (lane / 16) + reg
  const bool last = l == c.n_layers - 1;
  const int dst = l == 0 ? 0 : src ^ 1;
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
          hid[dst][row][j] = j < n ? hv : -0.0f;  // (a padded unit is the next layer's padded k)
        } else if (j < n && rowflag[row]) {
          y[(row0 + row) * (size_t)n + j] = rowflag[row] == 2 ? __builtin_nan("") : net_head(yv, c.out_act);
        }
      }
    }
  }
  if (!last) {  // the next layer's k padding beyond the unit tiles, up to its whole chunks
    const int extra = net_in_pad(n) - op;
    for (int i = tid; i < kNetRows * extra; i += 64 * kNetWaves) hid[dst][i / extra][op + i % extra] = -0.0f;
  }
  src = dst;
  __syncthreads();
  if constexpr (SAVE) {
    if (!last) {  // the finished tile, from LDS: row tid / 16, units tid % 16, + 16, ...
      float *hs = hsave + (((size_t)l * gridDim.x) * kNetRows + row0 + (tid >> 4)) * kNetMaxUnits;
      for (int j = tid & 15; j < op; j += 16) hs[j] = hid[dst][tid >> 4][j];
    }
  }
}

// x [rows][in_0] of T; y [rows][n_out] float64.  alive / role (null: the call alone): only
// live NN players' rows are evaluated and stored.  A row whose first value is a NaN is
// not evaluated: its output row is NaN.
template <class T, bool SAVE>
__device__ __forceinline__ void net_body(const Net &c, const T *x, int rows, double *y, const int *alive,
                                         const uint8_t *role, float *hsave) {
  __shared__ float xs[2][kNetRows][kNetXStride];
  __shared__ float hid[2][kNetRows][kNetHStride];
  __shared__ int rowflag[kNetRows];  // 0: not stored, 1: evaluated, 2: a NaN row
  const int tid = threadIdx.x, w = tid >> 6;
  const size_t row0 = (size_t)blockIdx.x * kNetRows;
  const int K0 = c.in[0];
  // this thread's part of a chunk of states: column tid % 64 of rows w, w + 4, w + 8, w + 12
  bool lrow[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t row = row0 + (size_t)(w + 4 * i);
    bool ok = row < (size_t)rows;
    if (ok && alive) ok = alive[row] && role[row] == AIGAR_ROLE_NN;
    const bool nan = ok && x[row * (size_t)K0] != x[row * (size_t)K0];
    lrow[i] = ok && !nan;
    if ((tid & 63) == 0) rowflag[w + 4 * i] = !ok ? 0 : (nan ? 2 : 1);
  }
  int src = 0;  // the hidden tile that the next layer reads
  for (int l = 0; l < c.n_layers; l++) {
    switch ((net_out_pad(c.out[l]) / 16 + kNetWaves - 1) / kNetWaves) {  // tiles of a wave at the most
      case 1: net_layer<T, 1, SAVE>(c, l, x, row0, lrow, xs, hid, rowflag, src, y, hsave); break;
      case 2: net_layer<T, 2, SAVE>(c, l, x, row0, lrow, xs, hid, rowflag, src, y, hsave); break;
      case 3: net_layer<T, 3, SAVE>(c, l, x, row0, lrow, xs, hid, rowflag, src, y, hsave); break;
      default: net_layer<T, 4, SAVE>(c, l, x, row0, lrow, xs, hid, rowflag, src, y, hsave); break;
    }
  }
}
template <class T>
__global__ void __launch_bounds__(64 * kNetWaves) k_net(Net c, const T *x, int rows, double *y, const int *alive,
                                                        const uint8_t *role) {
  net_body<T, false>(c, x, rows, y, alive, role, nullptr);
}
// ... and the trainer's online pass: all rows, the hidden activations kept
template <class T>
__global__ void __launch_bounds__(64 * kNetWaves) k_net_save(Net c, const T *x, int rows, double *y, float *hsave) {
  net_body<T, true>(c, x, rows, y, nullptr, nullptr, hsave);
}

static void launch_net(hipStream_t s, const Net &c, const void *x, int rows, double *y, const int *alive,
                       const uint8_t *role) {
  const dim3 grid((unsigned)(((size_t)rows + kNetRows - 1) / kNetRows)), block(64 * kNetWaves);
  if (c.x_dtype == 0) hipLaunchKernelGGL(k_net<double>, grid, block, 0, s, c, (const double *)x, rows, y, alive, role);
  else hipLaunchKernelGGL(k_net<float>, grid, block, 0, s, c, (const float *)x, rows, y, alive, role);
}

// W [in][out], b [out] (Keras' layout) -> the padded copy; every padded entry is written
__global__ void k_net_pack(const float *W, const float *b, float *wp, float *bp, int in, int out, int in_pad,
                           int out_pad) {
  const size_t n = (size_t)in_pad * out_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / out_pad), j = (int)(i % out_pad);
    wp[i] = (k < in && j < out) ? W[(size_t)k * out + j] : 0.0f;
    if (k == 0) bp[j] = j < out ? b[j] : 0.0f;
  }
}
