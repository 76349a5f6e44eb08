// convtrain.inc -- the Q-learning training step of an acting network with a conv part (include/aigar.h
// aigar_train_config_cnn; DESIGN.md §4p).  Included by api.hip after train.inc: the conv part's
// trainer state and its kernels; the entry points are in api.hip.
//
// tests/cnn_train_model.py is the specification in plain Python, on tests/conv_model.py and
// tests/train_model.py.  The step is train.inc's with the conv layers around the dense part:
//   k_exp_draw, k_exp_fetch   the mini-batch: s and s2 are images of the memory's dtype
//   k_conv x n_conv           (conv.inc) the online pass on s into the trainer's kept activations
//   k_net_save<float>         the dense part on the feature rows
//   k_conv x n_conv, k_net    the target pass on s2 (a Conv and a Net whose weights are the target's)
//   k_td, k_net_bwd           (train.inc) down to delta_1, the first dense layer's output delta
//   k_net_bwd_feat            delta_1 through the first dense layer onto the feature row, gated
//   k_conv_bwd                delta_l -> delta_{l - 1}, one launch for layer 3 and one for layer 2
//   k_net_grad_adam<float>    the dense layers' gradients and Adam (its first layer's h is the feature row)
//   k_conv_grad_adam          every conv layer's dW, db and Adam in place on the packed filters
//   k_exp_update, k_conv_train_tail, k_train_tail
// Every kernel that reads weights comes before every kernel that updates them.
//
// All three products run on v_mfma_f32_16x16x4_f32, one accumulator through the whole chain in
// ascending order (train.inc):
//   e[r][i]            = sum_j delta_1[r][j] W0[i][j]            A = delta_1, B = W0^T
//   e[(r, iy, ix)][c]  = sum_(ky, kx, f) x W_l[ky][kx][c][f]      A = delta_l gathered, B = W_l
//   dW[(ky, kx, c)][f] = sum_m h[m, (ky, kx, c)] delta_l[m][f]    A = the patches transposed, B = delta_l
// Padding: a padded step is -0.0f on the data side against +0.0f on the weight side.  The input
// error's steps at taps whose window position does not exist are part of the contract, x = -0.0f
// against the real weight.  In the filter gradient the rows m past the end enter as h = -0.0f,
// delta = +0.0f.  The bias gradient rides the same chain as one more row of A, all ones:
// fmaf(1.0f, delta, acc) is the float32 sum.

struct ConvTrain {  // aigar_train_config_cnn (on 0: off)
  int on, pad;
  float *tw[kConvMax], *tb[kConvMax];  // the target's filters, packed as Conv's
  float *mw[kConvMax], *mb[kConvMax];  // Adam's m
  float *vw[kConvMax], *vb[kConvMax];  // ... and v, in the same layout
  float *act[kConvMax];                // [bpad][osz][osz][F] the online pass's kept outputs
  float *tact[kConvMax];               // ... and the target pass's
  float *delta[kConvMax];              // [bpad][osz][osz][F]
  int tile0[kConvMax + 1];             // first gradient tile of every layer
};

// floor(2^32 / d) + 1: __umulhi(i, magic) == i / d for i < 2^32 / d  (d == 1: i == 0 only; see cdiv)
static inline unsigned conv_magic(int d) { return (unsigned)((1ull << 32) / (unsigned)d + 1); }
__device__ __forceinline__ int cdiv(int i, int d, unsigned magic) { return d == 1 ? i : (int)__umulhi((unsigned)i, magic); }

// delta_1 [bpad][kNetMaxUnits] (the first dense layer's output delta, padded units -0.0f) ->
// dlast [B][n_flat]: e where feat > 0, else +0.0f.  A wave per 16 x 16 tile (16 batch rows, 16
// feature columns); W0 is the packed kernel [in_pad][op], row i, four consecutive j a lane group.
__global__ void __launch_bounds__(64 * kNetWaves) k_net_bwd_feat(Net c, Train t, const float *feat, float *dlast) {
  if (t.ctl->skip) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int n_flat = c.in[0], op = net_out_pad(c.out[0]), B = t.batch;
  const int tile = (int)blockIdx.x * kNetWaves + w, row0 = (int)blockIdx.y * kNetRows;
  if (16 * tile >= n_flat) return;  // (the whole wave; no barrier)
  const float *wr = c.w[0] + (size_t)(16 * tile + r16) * op + g;  // (row < in_pad: the packed copy has it)
  const float *ar = t.delta + (size_t)(row0 + r16) * kNetMaxUnits + g;  // (row < bpad)
  const bool rin = row0 + r16 < B;
  net_f4 acc = net_f4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < op; j += 16) {
    float bv[4], av[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      bv[s] = wr[j + 4 * s];
      av[s] = rin ? ar[j + 4 * s] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  // D: e[row 4 g + reg][feature 16 tile + r16]
  const int i = 16 * tile + r16;
  if (i < n_flat) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int row = row0 + 4 * g + reg;
      if (row < B) {
        const size_t o = (size_t)row * n_flat + i;
        dlast[o] = feat[o] > 0.f ? acc[reg] : 0.0f;
      }
    }
  }
}

struct ConvBwd {  // one k_conv_bwd launch's geometry: layer l's delta back onto its input
  int H, cin, k, stride, O, F, K;  // input side and channels; kernel, stride, output side, filters; K = k k F
  int Fp;                          // the packed filter's row length
  unsigned mF, mk, ms, mH;         // conv_magic of F, k, stride, H
};

// din [B][H][H][cin] = (sum over the taps) where a_in > 0, else +0.0f.  A wave owns 16 rows of
// M = (r, iy, ix) and all NT tiles of the input channels.  A is gathered from dout [B][O][O][F]
// with the validity test; B is read from the forward packed copy [(ky, kx, c)][Fp], stride Fp
// between lanes.  Both are requested a chunk ahead, in straight-line code.
template <int NT>
__global__ void __launch_bounds__(64 * kConvWaves) k_conv_bwd(ConvBwd L, Train t, const float *dout, const float *Wp,
                                                              const float *a_in, float *din) {
  if (t.ctl->skip) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const int P = L.H * L.H;
  const int M = t.batch * P;
  const int m0 = ((int)blockIdx.x * kConvWaves + w) * 16;
  if (m0 >= M) return;  // (the whole wave; no barrier)
  const int m = m0 + r16;
  const bool min_ = m < M;
  const int r = min_ ? m / P : 0, pos = min_ ? m - r * P : 0;
  const int iy = cdiv(pos, L.H, L.mH), ix = pos - iy * L.H;
  const float *drow = dout + (size_t)r * L.O * L.O * L.F;
  const int nc = conv_k_pad(L.K) / kConvKC;

  auto aload = [&](int kc, float(&a)[kConvKC / 4]) {
#pragma unroll
    for (int s = 0; s < kConvKC / 4; s++) {
      const int kk = kc + 4 * s + g;
      const int tap = cdiv(kk, L.F, L.mF), f = kk - tap * L.F;
      const int ky = cdiv(tap, L.k, L.mk), kx = tap - ky * L.k;
      const int dy = iy - ky, dx = ix - kx;
      const int qy = dy >= 0 ? cdiv(dy, L.stride, L.ms) : 0, qx = dx >= 0 ? cdiv(dx, L.stride, L.ms) : 0;
      const bool ok = min_ && kk < L.K && dy >= 0 && dx >= 0 && qy * L.stride == dy && qx * L.stride == dx && qy < L.O &&
                      qx < L.O;
      a[s] = ok ? drow[((size_t)qy * L.O + qx) * L.F + f] : -0.0f;
    }
  };
  auto bload = [&](int kc, float(&b)[kConvKC / 4][NT]) {
#pragma unroll
    for (int s = 0; s < kConvKC / 4; s++) {
      const int kk = kc + 4 * s + g;
      const int tap = cdiv(kk, L.F, L.mF), f = kk - tap * L.F;
      const float *wr = Wp + ((size_t)tap * L.cin + r16) * L.Fp + f;
#pragma unroll
      for (int i = 0; i < NT; i++) b[s][i] = (kk < L.K && 16 * i + r16 < L.cin) ? wr[(size_t)16 * i * L.Fp] : 0.0f;
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
    for (int s = 0; s < kConvKC / 4; s++)
#pragma unroll
      for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[s], bc[s][i], acc[i], 0, 0, 0);
#pragma unroll
    for (int s = 0; s < kConvKC / 4; s++) {
      ac[s] = an[s];
#pragma unroll
      for (int i = 0; i < NT; i++) bc[s][i] = bn[s][i];
    }
  }
  // D: channel 16 i + r16 of rows 4 g + reg
#pragma unroll
  for (int i = 0; i < NT; i++) {
    const int c = 16 * i + r16;
    if (c < L.cin) {
#pragma unroll
      for (int reg = 0; reg < 4; reg++) {
        const int mm = m0 + 4 * g + reg;
        if (mm < M) {
          const size_t o = (size_t)mm * L.cin + c;
          din[o] = a_in[o] > 0.f ? acc[i][reg] : 0.0f;
        }
      }
    }
  }
}

// One wave per 16 x 16 tile (k0, j0) of a conv layer's [K + 1][F] (row K: the bias), all layers
// in one launch: the chain over ascending m = (r, oy, ox), then Adam on the tile in place, in the
// packed layout k_conv reads.  T: the states' dtype (the first layer's h is the drawn image,
// rounded once).
template <class T>
__global__ void __launch_bounds__(64) k_conv_grad_adam(Conv c, ConvTrain ct, Train t) {
  if (t.ctl->skip) return;
  const int lane = threadIdx.x, r16 = lane & 15, g = lane >> 4;
  int l = 0;
  while (l + 1 < c.n_conv && (int)blockIdx.x >= ct.tile0[l + 1]) l++;
  const int H = l ? c.osz[l - 1] : c.side, cin = l ? c.filters[l - 1] : c.channels;
  const int k = c.k[l], st = c.stride[l], O = c.osz[l], F = c.filters[l], Fp = net_out_pad(F), K = k * k * cin;
  const int tj = Fp >> 4, tile = (int)blockIdx.x - ct.tile0[l], k0 = 16 * (tile / tj), j0 = 16 * (tile % tj);
  const int P = O * O, M = t.batch * P;
  // this lane's row of A: (ky, kx, ch) of row k0 + r16, or the ones row, or a padded row
  const int kr = k0 + r16;
  const int tap = kr / cin, ch = kr - tap * cin, ky = tap / k, kx = tap - ky * k;
  const size_t koff = ((size_t)ky * H + kx) * cin + ch;
  const size_t img = (size_t)H * H * cin;
  const float *hp = l ? ct.act[l - 1] : nullptr;
  const T *xp = (const T *)t.s;
  const float *dp = ct.delta[l];
  const int j = j0 + r16;
  net_f4 acc = net_f4{0.f, 0.f, 0.f, 0.f};
  for (int mb = 0; mb < M; mb += 16) {
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int m = mb + 4 * s + g;
      const bool in = m < M;
      const int r = in ? m / P : 0, pos = in ? m - r * P : 0, oy = pos / O, ox = pos - oy * O;
      const size_t o = (size_t)r * img + ((size_t)oy * st * H + (size_t)ox * st) * cin + koff;
      float a = -0.0f;
      if (in && kr < K) a = l ? hp[o] : (float)xp[o];
      else if (in && kr == K) a = 1.0f;
      av[s] = a;
      bv[s] = (in && j < F) ? dp[(size_t)m * F + j] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
  }
  const double lr_t = t.ctl->lr_t;
  // D: dW[k0 + 4 g + reg][j0 + r16]
  if (j < F) {
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
      const int kk = k0 + 4 * g + reg;
      if (kk < K) {
        const size_t i = (size_t)kk * Fp + j;
        train_adam(t, lr_t, acc[reg], c.w[l] + i, ct.mw[l] + i, ct.vw[l] + i);
      } else if (kk == K) {
        train_adam(t, lr_t, acc[reg], c.b[l] + j, ct.mb[l] + j, ct.vb[l] + j);
      }
    }
  }
}

// When the target copy is due: target <- online for the conv filters (the padded copies whole).
// Before k_train_tail, which leaves ctl->due as k_td wrote it.
__global__ void __launch_bounds__(256) k_conv_train_tail(Conv c, ConvTrain ct, Train t) {
  if (!t.ctl->due) return;
  for (int l = 0; l < c.n_conv; l++) {
    const int cin = l ? c.filters[l - 1] : c.channels;
    const size_t Fp = net_out_pad(c.filters[l]), nw = (size_t)conv_k_pad(c.k[l] * c.k[l] * cin) * Fp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (size_t)gridDim.x * blockDim.x) {
      ct.tw[l][i] = c.w[l][i];
      if (i < Fp) ct.tb[l][i] = c.b[l][i];
    }
  }
}

// the packed filter -> W [K][F], b [F] (Keras' layout [k][k][cin][F])
__global__ void k_conv_unpack(const float *wp, const float *bp, float *W, float *b, int K, int F, int F_pad) {
  const size_t n = (size_t)K * F;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t k = i / F, j = i % F;
    W[i] = wp[k * F_pad + j];
    if (k == 0) b[j] = bp[j];
  }
}
