// conv.inc -- the convolutional front end of the CNN learners' acting network (include/aigar.h
// aigar_net_config_cnn; DESIGN.md §4k).  Included by api.hip after net.inc: the conv part's
// device state and its kernels; the entry points are in api.hip.
//
// The reference's CNN over the pixel state (network.py:154-183, actorCritic.py:122-136): up to
// three Conv2D layers (kernel, stride, filters), square kernels, valid padding, relu,
// channels_last, then Flatten and the dense layers k_net evaluates.  tests/conv_model.py is the
// specification in plain Python: one output (oy, ox, f) is ONE float32 fmaf chain from +0.0f
// over the flattened index (ky k + kx) Cin + c in ascending order, then one float32 add of the
// bias, then relu; the last layer's output flattened in (y, x, f) order is k_net's input row.
//
// k_conv (wave64, gfx950): one launch per conv layer, an implicit GEMM on
// v_mfma_f32_16x16x4_f32.  M is (sample, output position), N the filters in 16-wide tiles, K
// is k k Cin in the model's order.  A wave owns 16 rows of M and ALL of the layer's filter
// tiles (at most four accumulators: the independent MFMAs that cover the dependent latency),
// so every gathered A value is read once per wave; nothing is shared between waves, so there
// is no LDS and no barrier.  A[row][k] is gathered from the image or the previous activation:
// the (kx, c) part of a patch row is contiguous in a channels-last image, so with
// ky = k / (k Cin) (a multiply-high by a constant the host prepares) the address is
// patch + ky * side * Cin + k % (k Cin).  B is read from the handle's packed, zero-padded copy
// [K padded][F padded to 16], 16 consecutive floats per k.  Both are requested a chunk of 32 k
// ahead into registers, in straight-line code; the last iteration re-loads its own chunk.
// An activation [sample][oy][ox][f] IS the row-major [M][F] product, and the last one is the
// feature row in the model's flatten order.
// Every output tile carries ONE accumulator through the whole of K in ascending order.
//
// Padding as in net.inc: K is padded with x = -0.0f against w = +0.0f; padded filters and M
// rows past the end are computed and dropped; a sample that is not evaluated (dead or not an
// NN player in the decision, or its first image value a NaN) enters as -0.0f, so none of its
// NaNs meets the matrix core.  For a NaN sample the feature row's first value is written as
// NaN: k_net's own NaN-row rule then gives the NaN output row.

constexpr int kConvMax = 3;         // conv layers at the most
constexpr int kConvMaxSide = 128;
constexpr int kConvMaxCh = 8;       // channels of the image
constexpr int kConvMaxK = 8;        // kernel side and stride
constexpr int kConvMaxF = 64;       // filters of a layer
constexpr int kConvKC = 32;         // the k chunk (8 MFMA steps)
constexpr int kConvWaves = 4;       // waves of a block, 16 rows of M each
constexpr int kConvMinRows = 64;    // samples the activation buffers hold at least

struct Conv {  // aigar_net_config_cnn (n_conv 0: off); plain, no padding: part of the decision graph's key
  int n_conv, side, channels, n_flat;
  int k[kConvMax], stride[kConvMax], filters[kConvMax], osz[kConvMax];
  int cap, pad;            // samples the activation buffers hold
  float *w[kConvMax];      // [K padded][F padded] zero-padded filters
  float *b[kConvMax];      // [F padded]
  float *act[kConvMax];    // [cap][osz][osz][F] the layer's output; the last one is the feature row
};
static_assert(sizeof(Conv) == 18 * sizeof(int) + 9 * sizeof(void *), "Conv has padding");

__host__ __device__ inline int conv_k_pad(int K) { return (K + kConvKC - 1) / kConvKC * kConvKC; }

struct ConvLayer {  // one launch's geometry
  int in_side, cin, k, stride, osz, F, K;
  unsigned magic;  // floor(2^32 / (k cin)) + 1: __umulhi(i, magic) == i / (k cin) for i < 2^32 / (k cin)
};

// 0: not stored (not a live NN player), 1: evaluated, 2: a NaN sample
__device__ __forceinline__ int conv_sample_flag(const void *img, int img_dtype, size_t img_len, size_t s,
                                                const int *alive, const uint8_t *role) {
  if (alive && !(alive[s] && role[s] == AIGAR_ROLE_NN)) return 0;
  bool nan;
  if (img_dtype == 0) {
    const double v = ((const double *)img)[s * img_len];
    nan = v != v;
  } else {
    const float v = ((const float *)img)[s * img_len];
    nan = v != v;
  }
  return nan ? 2 : 1;
}

// in [S][in_side][in_side][cin] of T -> out [S][osz][osz][F] float32 (relu).  img: the samples'
// images (their first value decides whether a sample is evaluated), img_len values each.
template <class T, int NT>
__global__ void __launch_bounds__(64 * kConvWaves) k_conv(ConvLayer L, const T *in, const float *Wp, const float *bp,
                                                          float *out, int S, const void *img, int img_dtype, int img_len,
                                                          int last, const int *alive, const uint8_t *role) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int P = L.osz * L.osz;
  const size_t M = (size_t)S * P;
  const size_t m0 = ((size_t)blockIdx.x * kConvWaves + w) * 16;
  if (m0 >= M) return;  // (the whole wave; the kernel has no barrier)
  // this lane's row of A: sample s, output position (oy, ox)
  const size_t m = m0 + r16;
  int code = 0;  // the row's flag | 4 where it is its sample's first position
  size_t s = 0;
  int pos = 0;
  if (m < M) {
    s = m / P;
    pos = (int)(m - s * P);
    code = conv_sample_flag(img, img_dtype, (size_t)img_len, s, alive, role);
    if (pos == 0) code |= 4;
  }
  const bool ev = (code & 3) == 1;
  const int oy = pos / L.osz, ox = pos - oy * L.osz;
  const int rowlen = L.in_side * L.cin, d = L.k * L.cin;
  const T *patch = in + (s * L.in_side + (size_t)(oy * L.stride)) * rowlen + (size_t)(ox * L.stride) * L.cin;
  const int Fp = NT * 16;
  const int nc = conv_k_pad(L.K) / kConvKC;

  auto aload = [&](int kc, float(&a)[kConvKC / 4]) {
#pragma unroll
    for (int t = 0; t < kConvKC / 4; t++) {
      const int k = kc + 4 * t + g;
      const int ky = (int)__umulhi((unsigned)k, L.magic);
      a[t] = (ev && k < L.K) ? (float)patch[ky * rowlen + (k - ky * d)] : -0.0f;
    }
  };
  auto bload = [&](int kc, float(&b)[kConvKC / 4][NT]) {
#pragma unroll
    for (int t = 0; t < kConvKC / 4; t++) {
      const float *wr = Wp + (size_t)(kc + 4 * t + g) * Fp + r16;
#pragma unroll
      for (int i = 0; i < NT; i++) b[t][i] = wr[16 * i];
    }
  };

  net_f4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; i++) acc[i] = net_f4{0.f, 0.f, 0.f, 0.f};
  float ac[kConvKC / 4], an[kConvKC / 4], bc[kConvKC / 4][NT], bn[kConvKC / 4][NT];
  aload(0, ac);
  bload(0, bc);
  for (int ch = 0; ch < nc; ch++) {
    const int kn = min(ch + 1, nc - 1) * kConvKC;
    aload(kn, an);
    bload(kn, bn);
#pragma unroll
    for (int t = 0; t < kConvKC / 4; t++)
#pragma unroll
      for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[t], bc[t][i], acc[i], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < kConvKC / 4; t++) {
      ac[t] = an[t];
#pragma unroll
      for (int i = 0; i < NT; i++) bc[t][i] = bn[t][i];
    }
  }
  // D: filter 16 i + lane % 16 of rows 4 (lane / 16) + r
  int cd[4];
#pragma unroll
  for (int r = 0; r < 4; r++) cd[r] = __shfl(code, 4 * g + r);
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const int j = 16 * i + r16;
    if (j < L.F) {
      const float bj = bp[j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        if (cd[r] & 3) {  // (0: past the end of M, or a row that is not stored)
          const float yv = acc[i][r] + bj;  // one float32 add
          float hv = yv > 0.f ? yv : 0.0f;
          if (last && cd[r] == (2 | 4) && j == 0) hv = __builtin_nanf("");
          out[(m0 + 4 * g + r) * (size_t)L.F + j] = hv;
        }
      }
    }
  }
}

// The conv layers of c on S <= c.cap samples x [S][side][side][channels] (x_dtype 0: float64,
// 1: float32): one launch per layer; c.act[n_conv - 1] then holds the feature rows.
static void launch_conv(hipStream_t s, const Conv &c, const void *x, int x_dtype, int S, const int *alive,
                        const uint8_t *role) {
  const int img_len = c.side * c.side * c.channels;
  for (int l = 0; l < c.n_conv; l++) {
    ConvLayer L;
    L.in_side = l ? c.osz[l - 1] : c.side;
    L.cin = l ? c.filters[l - 1] : c.channels;
    L.k = c.k[l];
    L.stride = c.stride[l];
    L.osz = c.osz[l];
    L.F = c.filters[l];
    L.K = L.k * L.k * L.cin;
    L.magic = (unsigned)((1ull << 32) / (unsigned)(L.k * L.cin) + 1);  // (k cin == 1: K == 1, and 0 / 1 == umulhi(0, 1))
    const size_t M = (size_t)S * L.osz * L.osz;
    const dim3 grid((unsigned)((M + 16 * kConvWaves - 1) / (16 * kConvWaves))), block(64 * kConvWaves);
    const int last = l == c.n_conv - 1;
#define AIGAR_CONV_GO(T, NT, inp)                                                                                    \
  hipLaunchKernelGGL((k_conv<T, NT>), grid, block, 0, s, L, (const T *)(inp), c.w[l], c.b[l], c.act[l], S, x, x_dtype, \
                     img_len, last, alive, role)
#define AIGAR_CONV_NT(T, inp)                 \
  switch ((L.F + 15) / 16) {                  \
    case 1: AIGAR_CONV_GO(T, 1, inp); break;  \
    case 2: AIGAR_CONV_GO(T, 2, inp); break;  \
    case 3: AIGAR_CONV_GO(T, 3, inp); break;  \
    default: AIGAR_CONV_GO(T, 4, inp); break; \
  }
    if (l) {
      AIGAR_CONV_NT(float, c.act[l - 1])
    } else if (x_dtype == 0) {
      AIGAR_CONV_NT(double, x)
    } else {
      AIGAR_CONV_NT(float, x)
    }
#undef AIGAR_CONV_NT
#undef AIGAR_CONV_GO
  }
}

// W [k][k][cin][F] = [K][F], b [F] (Keras' layout) -> the padded copy; every padded entry is written
__global__ void k_conv_pack(const float *W, const float *b, float *wp, float *bp, int K, int F, int K_pad, int F_pad) {
  const size_t n = (size_t)K_pad * F_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / F_pad), j = (int)(i % F_pad);
    wp[i] = (k < K && j < F) ? W[(size_t)k * F + j] : 0.0f;
    if (k == 0) bp[j] = j < F ? b[j] : 0.0f;
  }
}
