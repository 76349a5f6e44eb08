// pixels.inc -- the pixel observation kernel, included by obs.hip inside
// namespace aigar (it shares the observation's FOV walk, wave_fov_walk).
// Description at the include site.

constexpr int PIX_OCAP = 1024;  // drawn objects per frame (second pass, for the frames the first overflows)
constexpr int PIX_OCAP_FAST = 256;  // first pass: small LDS footprint, high occupancy
// the bitonic sort pads the object list to a power of two inside the arrays
static_assert((PIX_OCAP & (PIX_OCAP - 1)) == 0 && (PIX_OCAP_FAST & (PIX_OCAP_FAST - 1)) == 0, "pow2 caps");
constexpr int PIX_LMAX = 84;    // frame side (CNN_INPUT_DIM_1/2/3: 42 / 84 / 42)
constexpr int PIX_RMAX = 255;   // drawn radius (half-width table)

__device__ __forceinline__ uint64_t pix_mix(uint64_t v) {
  v += 0x9E3779B97F4A7C15ull;
  v = (v ^ (v >> 30)) * 0xBF58476D1CE4E5B9ull;
  v = (v ^ (v >> 27)) * 0x94D049BB133111EBull;
  return v ^ (v >> 31);
}
// aigar_amd/model.py player_color / pellet_color (the facade's colours)
__device__ uint32_t pix_player_rgb(int index, uint64_t seed) {
  for (uint64_t k = 0;; k++) {
    const uint64_t h = pix_mix((seed << 32) ^ ((uint64_t)index << 8) ^ k);
    const uint32_t r = h & 255, g = (h >> 8) & 255, b = (h >> 16) & 255;
    if (r + g + b <= 600) return (r << 16) | (g << 8) | b;
  }
}
__device__ __forceinline__ uint32_t pix_pellet_rgb(int64_t seq, uint64_t seed) {
  const uint64_t h = pix_mix((seed << 40) ^ (uint64_t)seq ^ 0x5E11E7ull);
  return ((uint32_t)(50 + h % 150) << 16) | ((uint32_t)(50 + (h >> 16) % 150) << 8) | (uint32_t)(50 + (h >> 32) % 150);
}

// pixelColorWeight on a packed pixel: alpha = (255 w) >> 8, d + ((s - d) alpha >> 8)
__device__ __forceinline__ void pix_blend(uint32_t *fr, int L, int x, int y, uint32_t c, int w) {
  if ((unsigned)x >= (unsigned)L || (unsigned)y >= (unsigned)L) return;
  const int alpha = (255 * w) >> 8;
  uint32_t &p = fr[y * L + x];
  uint32_t o = 0;
#pragma unroll
  for (int sh = 16; sh >= 0; sh -= 8) {
    const int dv = (p >> sh) & 255, sv = (c >> sh) & 255;
    o |= (uint32_t)(alpha == 255 ? sv : dv + (((sv - dv) * alpha) >> 8)) << sh;
  }
  p = o;
}
__device__ __forceinline__ void pix_put(uint32_t *fr, int L, int x, int y, uint32_t c) {
  if ((unsigned)x < (unsigned)L && (unsigned)y < (unsigned)L) fr[y * L + x] = c;
}

// span half-widths of filledCircleColor / filledEllipseColor(rad, rad) as a
// union per row offset: hw[dy] = widest span drawn on rows y +- dy (-1: none)
__device__ void pix_spans(int16_t *hw, int rad, bool circle) {
  for (int i = 0; i <= rad; i++) hw[i] = -1;
  auto span = [&](int row, int half) {
    row = row < 0 ? -row : row;
    if (half > hw[row]) hw[row] = (int16_t)half;
  };
  if (rad == 0) {  // a point (filledCircle's rad 0 case; filledEllipse's rx == 0 vline)
    hw[0] = 0;
    return;
  }
  if (circle) {
    int cx = 0, cy = rad, ocx = -1, ocy = -1, df = 1 - rad, d_e = 3, d_se = -2 * rad + 5;
    do {
      if (ocy != cy) {
        span(cy, cx);
        ocy = cy;
      }
      if (ocx != cx) {
        if (cx != cy) span(cx, cy);
        ocx = cx;
      }
      if (df < 0) {
        df += d_e;
        d_e += 2;
        d_se += 2;
      } else {
        df += d_se;
        d_e += 2;
        d_se += 4;
        cy--;
      }
      cx++;
    } while (cx <= cy);
  } else {  // rx == ry: the second branch of filledEllipseColor
    int oh = 0xFFFF, oi = 0xFFFF, ix = 0, iy = rad * 64, h, i;
    do {
      h = (ix + 32) >> 6;
      i = (iy + 32) >> 6;
      if (oi != i && oh != i) {
        span(i, h);  // j = h * rx / ry
        oi = i;
      }
      if (oh != h && oi != h && i != h) {
        span(h, i);  // k = i * rx / ry
        oh = h;
      }
      ix = ix + iy / rad;
      iy = iy - ix / rad;
    } while (i > h);
  }
}

// aaellipseColor(xc, yc, rad, rad) rim, sequential (lane 0)
__device__ void pix_aa_rim(uint32_t *fr, int L, int xc, int yc, int rad, uint32_t c) {
  const int a2 = rad * rad, b2 = a2, ds = 2 * a2, dt = 2 * b2, xc2 = 2 * xc, yc2 = 2 * yc;
  const double sab = sqrt((double)(a2 + b2));
  const int od = (int)rint(sab * 0.01) + 1;
  const int dxt = (int)rint((double)a2 / sab) + od, dyt = (int)rint((double)b2 / sab) + od;
  int t = 0, s = -2 * a2 * rad, d = 0, x = xc, y = yc - rad, xs, ys;
  pix_put(fr, L, x, y, c);
  pix_put(fr, L, xc2 - x, y, c);
  pix_put(fr, L, x, yc2 - y, c);
  pix_put(fr, L, xc2 - x, yc2 - y, c);
  for (int i = 1; i <= dxt; i++) {
    x--;
    d += t - b2;
    if (d >= 0) {
      ys = y - 1;
    } else if ((d - s - a2) > 0) {
      if ((2 * d - s - a2) >= 0) {
        ys = y + 1;
      } else {
        ys = y;
        y++;
        d -= s + a2;
        s += ds;
      }
    } else {
      y++;
      ys = y + 1;
      d -= s + a2;
      s += ds;
    }
    t -= dt;
    float cp = s != 0 ? (float)abs(d) / (float)abs(s) : 1.0f;
    cp = cp > 1.0f ? 1.0f : cp;
    const int w = (uint8_t)(cp * 255), iw = 255 - w, xx = xc2 - x;
    pix_blend(fr, L, x, y, c, iw);
    pix_blend(fr, L, xx, y, c, iw);
    pix_blend(fr, L, x, ys, c, w);
    pix_blend(fr, L, xx, ys, c, w);
    pix_blend(fr, L, x, yc2 - y, c, iw);
    pix_blend(fr, L, xx, yc2 - y, c, iw);
    pix_blend(fr, L, x, yc2 - ys, c, w);
    pix_blend(fr, L, xx, yc2 - ys, c, w);
  }
  for (int i = 1; i <= dyt; i++) {
    y++;
    d -= s + a2;
    if (d <= 0) {
      xs = x + 1;
    } else if ((d + t - b2) < 0) {
      if ((2 * d + t - b2) <= 0) {
        xs = x - 1;
      } else {
        xs = x;
        x--;
        d += t - b2;
        t -= dt;
      }
    } else {
      x--;
      xs = x - 1;
      d += t - b2;
      t -= dt;
    }
    s += ds;
    float cp = t != 0 ? (float)abs(d) / (float)abs(t) : 1.0f;
    cp = cp > 1.0f ? 1.0f : cp;
    const int w = (uint8_t)(cp * 255), iw = 255 - w, xx = xc2 - x, yy = yc2 - y, xx2 = xc2 - xs;
    pix_blend(fr, L, x, y, c, iw);
    pix_blend(fr, L, xx, y, c, iw);
    pix_blend(fr, L, x, yy, c, iw);
    pix_blend(fr, L, xx, yy, c, iw);
    pix_blend(fr, L, xs, y, c, w);
    pix_blend(fr, L, xx2, y, c, w);
    pix_blend(fr, L, xs, yy, c, w);
    pix_blend(fr, L, xx2, yy, c, w);
  }
}

// The learner's pixel state (bot.py:276-282: (rgb_values - 255) / 100) of one packed pixel,
// C = 1 (grayscale: the fp64 weighted average, then the expression in fp64) or 3 (RGB:
// the reference subtracts from a uint8 array, which wraps: ((b + 1) & 255) / 100).
// T: the output type, rounded once from the fp64 value.
template <class T>
struct PixSt {
  T c0, c1, c2;  // (grayscale: c0 alone)
};
template <class T, bool RGB>
__device__ __forceinline__ PixSt<T> pix_state(uint32_t p) {
  PixSt<T> v;
  if (RGB) {
    v.c0 = (T)((double)(((p >> 16) + 1) & 255) / 100.0);
    v.c1 = (T)((double)(((p >> 8) + 1) & 255) / 100.0);
    v.c2 = (T)((double)((p + 1) & 255) / 100.0);
  } else {
    const double R = (p >> 16) & 255, G = (p >> 8) & 255, B = p & 255;
    const double g = ((R * 0.298 + G * 0.587) + B * 0.114) / ((0.298 + 0.587) + 0.114);
    v.c0 = v.c1 = v.c2 = (T)((g - 255.0) / 100.0);
  }
  return v;
}
// one pixel's channels [current C | previous C when LAST], contiguous at o: the widest
// store the row layout keeps aligned (a row starts on a 16-byte boundary, a pixel's 2 or
// 6 elements on a pair boundary; 3 elements leave only the element's own alignment)
template <class T, bool RGB, bool LAST>
__device__ __forceinline__ void pix_store(T *o, const PixSt<T> &a, const PixSt<T> &b) {
  typedef T T2 __attribute__((ext_vector_type(2)));
  auto pair = [&](int k, T x, T y) {
    T2 w;
    w.x = x;
    w.y = y;
    *(T2 *)(o + k) = w;
  };
  if (RGB && LAST) {
    pair(0, a.c0, a.c1);
    pair(2, a.c2, b.c0);
    pair(4, b.c1, b.c2);
  } else if (RGB) {
    o[0] = a.c0;
    o[1] = a.c1;
    o[2] = a.c2;
  } else if (LAST) {
    pair(0, a.c0, b.c0);
  } else {
    o[0] = a.c0;
  }
}

// ST 0 (k_observe_pixels), out: DT 0 float64 / 1 float32 grayscale [player][x][y]; 2 uint8
// RGB [player][x][y][3].
// ST = PIX_ST | flags (k_observe_pixel_state), out: DT 0 float64 / 1 float32 pixel state
// [player][x][y][CT], CT = C (1, or 3 with PIX_ST_RGB) current channels, then with
// PIX_ST_LAST the C channels of this bot's previous pixel state.  mask (may be null): a
// player whose byte is 0 is not touched, in either pass.  hist [player][x][y]: the previous
// frame as ~0x00RRGGBB (so cleared memory is the white frame, whose state is zero); it is
// read and rewritten by the lane that writes the pixel, only where a row is written, so a
// frame the first pass leaves to the second advances once.  A dead player's row is all
// NaN and its history stays.
// OCAP < PIX_OCAP: first pass, every player; a frame with more objects sets ovf[player]
// and is left to the OCAP == PIX_OCAP pass, which draws only those players.
constexpr int PIX_ST = 1, PIX_ST_RGB = 2, PIX_ST_LAST = 4;
template <int DT, int OCAP, int ST>
__device__ __forceinline__ void observe_pixels_body(const Dev &d, void *out, int L, uint64_t cseed, uint8_t *ovf,
                                                    const uint8_t *mask, uint32_t *hist) {
  constexpr int C = (ST & PIX_ST_RGB) ? 3 : 1, CT = (ST & PIX_ST_LAST) ? 2 * C : C;
  // per drawn object: the sort key (mass; after the sort, the frame position), the order
  // key kind << 56 | seq (after the sort: kind << 56 | drawn radius << 32 | colour), slot
  __shared__ union {
    double m[OCAP];
    int2 pos[OCAP];
  } o_u;
  double *o_m = o_u.m;
  int2 *o_pos = o_u.pos;
  __shared__ uint64_t o_ord[OCAP];  // kind: 0 pellet, 1 blob, 2 virus, 3 cell
  __shared__ uint32_t o_g[OCAP];
  extern __shared__ uint32_t fr[];  // the frame, L * L packed 0x00RRGGBB (dynamic: sized per launch)
  __shared__ int16_t hw[PIX_RMAX + 1];
  __shared__ int16_t hw_small[4][4];  // filledEllipse half-widths for rad 0..3
  __shared__ int n_obj, bad;
  const int gp = blockIdx.x, lane = threadIdx.x, NP = d.NP, a = gp / d.B, LL = L * L;
  const size_t obase = (size_t)gp * LL;
  if (ST && mask && !mask[gp]) return;  // (both passes: its flag may be an earlier call's)
  if (OCAP == PIX_OCAP && !ovf[gp]) return;  // drawn by the first pass
  if (!d.p_alive[gp]) {  // getStateRepresentation: None for dead players
    if (lane == 0) ovf[gp] = 0;
    if (ST) {
      for (size_t i = lane; i < (size_t)LL * CT; i += 64) {
        if (DT == 0) ((double *)out)[obase * CT + i] = __builtin_nan("");
        else ((float *)out)[obase * CT + i] = __builtin_nanf("");
      }
      return;
    }
    for (int i = lane; i < LL; i += 64) {
      if (DT == 0) ((double *)out)[obase + i] = __builtin_nan("");
      else if (DT == 1) ((float *)out)[obase + i] = __builtin_nanf("");
      else for (int k = 0; k < 3; k++) ((uint8_t *)out)[3 * (obase + i) + k] = 0;
    }
    return;
  }
  const ArenaCtl &ctl = d.ctl[a];
  const double fx = d.p_fx[gp], fy = d.p_fy[gp], fs = d.p_fs[gp];
  const double scale = (double)L / fs;  // screenDims / fovSize
  const Rect Q = footprint(fx, fy, fs / 2, d.size);
  if (lane == 0) n_obj = bad = 0;
  if (lane < 4) {  // (written in place: a private array would live in scratch)
    for (int i = 0; i < 4; i++) hw_small[lane][i] = -1;
    pix_spans(hw_small[lane], lane, false);
  }
  for (int i = lane; i < LL; i += 64) fr[i] = 0xFFFFFFu;  // screen.fill(WHITE)
  __syncthreads();
  // an object whose drawing (rim included: within +1, +2 kept) misses the frame changes no pixel
  auto touches = [&](double x, double y, double r) {
    const int64_t px = (int64_t)(((x - fx) + fs / 2) * scale), py = (int64_t)(((y - fy) + fs / 2) * scale);
    const int64_t rad = (int64_t)(r * scale) + 2;
    return px + rad >= 0 && px - rad < L && py + rad >= 0 && py - rad < L;
  };
  auto append = [&](bool keep, double m, uint64_t ord, uint32_t g) {
    const unsigned long long bal = __ballot(keep);
    const int base = n_obj;
    const int slot = base + __popcll(bal & ((1ull << lane) - 1));
    if (keep && slot < OCAP) {
      o_m[slot] = m;
      o_ord[slot] = ord;
      o_g[slot] = g;
    }
    __syncthreads();
    if (lane == 0) n_obj = base + __popcll(bal);
    __syncthreads();
  };
  // pellets, player cells (own included: getPlayerCellsInFov), viruses
  wave_fov_walk(d, a, Q, fx, fy, fs, ctl.rmax_cell, ctl.rmax_virus, true, d.virus_enabled, [] {},
                [&](bool valid, int kd, size_t g) {
    bool ok = false;
    double m = 0;
    uint64_t ord = 0;
    if (valid) {
      const PelRec *PR = d.pel;
      const double *X = kd == 0 ? &PR->x : (kd == 1 ? d.c_x : d.v_x);
      const double *Y = kd == 0 ? &PR->y : (kd == 1 ? d.c_y : d.v_y);
      const double *M = kd == 0 ? &PR->m : (kd == 1 ? d.c_m : d.v_m);
      const int64_t *S = kd == 0 ? &PR->seq : (kd == 1 ? d.c_seq : d.v_seq);
      const uint32_t fl = kd == 0 ? (F_ALIVE | F_INHASH) : (kd == 1 ? d.c_flags[g] : d.v_flags[g]);
      const size_t gr = kd == 0 ? g * kPelStride : g;
      const double x = X[gr], y = Y[gr];
      m = M[gr];
      const double r = kd == 0 ? pellet_radius(m) : (kd == 1 ? d.c_r[g] : d.v_r[g]);
      ok = (fl & (F_ALIVE | F_INHASH)) == (F_ALIVE | F_INHASH) && in_fov(x, y, r, fx, fy, fs) &&
           touches(x, y, r);  // (isInFov implies the hash query's footprint test: aigar_sem.h)
      ord = ((uint64_t)(kd == 0 ? 0 : (kd == 1 ? 3 : 2)) << 56) | (uint64_t)S[gr];
    }
    append(ok, m, ord, (uint32_t)g);
  });
  // blobs (getBlobsInFov): the arena's blob slots
  const int nb = ctl.n_blob;
  for (int i0 = 0; i0 < nb; i0 += 64) {
    const int i = i0 + lane;
    bool ok = false;
    double m = 0;
    uint64_t ord = 0;
    const size_t g = (size_t)a * d.Ecap + i;
    if (i < nb && (d.b_flags[g] & F_ALIVE)) {
      const double x = d.b_x[g], y = d.b_y[g], r = d.b_r[g];
      m = d.b_m[g];
      ok = in_fov(x, y, r, fx, fy, fs) && touches(x, y, r);
      ord = (1ull << 56) | (uint64_t)d.b_seq[g];
    }
    append(ok, m, ord, (uint32_t)g);
  }
  const int n = n_obj;
  if (n > OCAP) {
    if (lane == 0) {
      if (OCAP < PIX_OCAP) ovf[gp] = 1;
      else atomicOr(&d.ctl[a].err, (uint32_t)ERR_PIX_CAP);
    }
    return;
  }
  if (OCAP < PIX_OCAP && lane == 0) ovf[gp] = 0;
  // bitonic sort by (mass, ord): list.sort(key=mass), stable over the kind lists
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + lane; i < np2; i += 64) {
    o_m[i] = __builtin_inf();
    o_ord[i] = ~0ull;
    o_g[i] = 0;
  }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < np2 / 2; t += 64) {
        const int i = 2 * j * (t / j) + (t % j), l = i + j;
        const bool up = (i & k) == 0;
        const bool gt = o_m[i] > o_m[l] || (o_m[i] == o_m[l] && o_ord[i] > o_ord[l]);
        if (gt == up) {
          const double tm = o_m[i];
          o_m[i] = o_m[l];
          o_m[l] = tm;
          const uint64_t to = o_ord[i];
          o_ord[i] = o_ord[l];
          o_ord[l] = to;
          const uint32_t tg = o_g[i];
          o_g[i] = o_g[l];
          o_g[l] = tg;
        }
      }
      __syncthreads();
    }
  // drawSingleCell (rgbGenerator.py:36-53), in sorted order.  First, lane-parallel, each
  // object's frame position, drawn radius and colour, packed over the (consumed) sort keys.
  for (int k = lane; k < n; k += 64) {
    const int kind = (int)(o_ord[k] >> 56);
    const size_t g = o_g[k];
    double x, y, r;
    uint32_t col;
    if (kind == 0) {
      x = d.pel[g].x;
      y = d.pel[g].y;
      r = pellet_radius(o_m[k]);
      // a pellet made from a blob keeps the blob's colour (addPellet(blob), field.py:110)
      const int pc = d.pel_col[g];
      col = pc >= 0 ? pix_player_rgb(pc, cseed) : pix_pellet_rgb(d.pel[g].seq, cseed);
    } else if (kind == 1) {  // an ejected blob: its player's colour (field.py:141, cell.py:219)
      x = d.b_x[g];
      y = d.b_y[g];
      r = d.b_r[g];
      const int bc = d.b_col[g];
      col = bc >= 0 ? pix_player_rgb(bc, cseed) : pix_pellet_rgb(d.b_seq[g], cseed);
    } else if (kind == 2) {
      x = d.v_x[g];
      y = d.v_y[g];
      r = d.v_r[g];
      col = 0x00FF00u;  // field.py:274
    } else {
      x = d.c_x[g];
      y = d.c_y[g];
      r = d.c_r[g];
      col = pix_player_rgb((int)(g % NP) - a * d.B, cseed);
    }
    const double rs = r * scale;
    const int rad = rs > PIX_RMAX ? PIX_RMAX + 1 : (int)rs;
    if (rad > PIX_RMAX) bad = 1;
    o_pos[k] = make_int2((int)(int64_t)(((x - fx) + fs / 2) * scale), (int)(int64_t)(((y - fy) + fs / 2) * scale));
    o_ord[k] = ((uint64_t)kind << 56) | ((uint64_t)rad << 32) | col;
  }
  __syncthreads();
  if (bad) {  // (uniform: every lane returns)
    if (lane == 0) atomicOr(&d.ctl[a].err, (uint32_t)ERR_PIX_CAP);
    return;
  }
  auto rad_of = [&](int k) { return (int)((o_ord[k] >> 32) & 0xFFFFFF); };
  bool tagged = false;  // some pixel carries a batch tag in its top byte
  for (int k = 0; k < n;) {
    const int rad = rad_of(k);
    if (rad < 4) {
      // a run of small objects (pygame.draw.circle: opaque filledEllipse spans): drawn all
      // at once, one object per lane; atomicMax of (run index + 1) << 24 | colour keeps the
      // last-drawn object's colour at every pixel, exactly as drawing them one by one
      int e = k + 1;
      while (e < n && e - k < 255 && rad_of(e) < 4) e++;
      if (tagged) {
        for (int i = lane; i < LL; i += 64) fr[i] &= 0xFFFFFFu;
        __syncthreads();
      }
      for (int j = k + lane; j < e; j += 64) {
        const int rj = rad_of(j), cx = o_pos[j].x, cy = o_pos[j].y;
        const uint32_t tag = ((uint32_t)(j - k + 1) << 24) | (uint32_t)(o_ord[j] & 0xFFFFFFu);
        for (int dy = -rj; dy <= rj; dy++) {
          const int yy = cy + dy, hh = hw_small[rj][dy < 0 ? -dy : dy];
          if ((unsigned)yy >= (unsigned)L) continue;
          for (int dx = -hh; dx <= hh; dx++) {
            const int xx = cx + dx;
            if ((unsigned)xx < (unsigned)L) atomicMax(&fr[yy * L + xx], tag);
          }
        }
      }
      __syncthreads();
      tagged = true;
      k = e;
      continue;
    }
    const int kind = (int)(o_ord[k] >> 56);
    const uint32_t col = (uint32_t)(o_ord[k] & 0xFFFFFFu);
    const int px = o_pos[k].x, py = o_pos[k].y;
    if (lane == 0) pix_spans(hw, rad, true);
    __syncthreads();
    const int y0 = max(py - rad, 0), y1 = min(py + rad, L - 1);
    const int x0 = max(px - rad, 0), x1 = min(px + rad, L - 1);
    const int W = x1 - x0 + 1, Hh = y1 - y0 + 1;
    if (W > 0 && Hh > 0)
      for (int t = lane; t < W * Hh; t += 64) {
        const int yy = y0 + t / W, xx = x0 + t % W;
        const int dy = yy > py ? yy - py : py - yy, dx = xx > px ? xx - px : px - xx;
        if (dx <= hw[dy]) fr[yy * L + xx] = col;  // (clears a batch tag too)
      }
    __syncthreads();
    if (lane == 0) {  // viruses: black rim
      // (the state kernels inline the rim: as a call it costs them a stack frame next to
      // their scalar spills; k_observe_pixels keeps the compiler's choice, and its code)
      if (ST) [[clang::always_inline]] pix_aa_rim(fr, L, px, py, rad, kind == 2 ? 0u : col);
      else pix_aa_rim(fr, L, px, py, rad, kind == 2 ? 0u : col);
    }
    __syncthreads();
    k++;
  }
  // surfarray order [x][y]; grayscale = numpy.average(rgb, weights): left-to-right sum
  for (int i = lane; i < LL; i += 64) {
    const int xx = i / L, yy = i - xx * L;
    const uint32_t p = fr[yy * L + xx];
    if (ST) {
      uint32_t q = 0xFFFFFFu;
      if (ST & PIX_ST_LAST) {
        uint32_t *hp = hist + obase + i;
        q = ~*hp & 0xFFFFFFu;
        *hp = ~p & 0xFFFFFFu;
      }
      if (DT == 0)
        pix_store<double, C == 3, CT != C>((double *)out + (obase + i) * CT, pix_state<double, C == 3>(p),
                                           pix_state<double, C == 3>(q));
      else
        pix_store<float, C == 3, CT != C>((float *)out + (obase + i) * CT, pix_state<float, C == 3>(p),
                                          pix_state<float, C == 3>(q));
      continue;
    }
    const double R = (p >> 16) & 255, G = (p >> 8) & 255, B = p & 255;
    if (DT == 2) {
      uint8_t *o = (uint8_t *)out + 3 * (obase + i);
      o[0] = (uint8_t)R;
      o[1] = (uint8_t)G;
      o[2] = (uint8_t)B;
    } else {
      const double v = ((R * 0.298 + G * 0.587) + B * 0.114) / ((0.298 + 0.587) + 0.114);
      if (DT == 0) ((double *)out)[obase + i] = v;
      else ((float *)out)[obase + i] = (float)v;
    }
  }
}
template <int DT, int OCAP>
__global__ void __launch_bounds__(64) k_observe_pixels(Dev d, void *out, int L, uint64_t cseed, uint8_t *ovf) {
  observe_pixels_body<DT, OCAP, 0>(d, out, L, cseed, ovf, nullptr, nullptr);
}
template <int DT, int OCAP, int ST>
__global__ void __launch_bounds__(64) k_observe_pixel_state(Dev d, void *out, int L, uint64_t cseed, uint8_t *ovf,
                                                            const uint8_t *mask, uint32_t *hist) {
  observe_pixels_body<DT, OCAP, ST>(d, out, L, cseed, ovf, mask, hist);
}
int launch_observe_pixels(const Dev &d, hipStream_t s, void *out, int dtype, int side, uint64_t seed, uint8_t *ovf) {
  if (side < 1 || side > PIX_LMAX || dtype < 0 || dtype > 2) return -1;
  const size_t lds = (size_t)side * side * 4;
#define PIX_LAUNCH(DT)                                                                                 \
  do {                                                                                                 \
    hipLaunchKernelGGL((k_observe_pixels<DT, PIX_OCAP_FAST>), dim3(d.NP), dim3(64), lds, s, d, out, side, seed, \
                       ovf);                                                                           \
    hipLaunchKernelGGL((k_observe_pixels<DT, PIX_OCAP>), dim3(d.NP), dim3(64), lds, s, d, out, side, seed, ovf); \
  } while (0)
  if (dtype == 0) PIX_LAUNCH(0);
  else if (dtype == 1) PIX_LAUNCH(1);
  else PIX_LAUNCH(2);
#undef PIX_LAUNCH
  return 0;
}
// flags: AIGAR_PIX_RGB | AIGAR_PIX_LAST (hist: [NP][side * side] words when LAST, else unused)
int launch_observe_pixel_state(const Dev &d, hipStream_t s, void *out, int dtype, int side, int flags, uint64_t seed,
                               uint8_t *ovf, const uint8_t *mask, uint32_t *hist) {
  if (side < 1 || side > PIX_LMAX || dtype < 0 || dtype > 1 || (flags & ~(AIGAR_PIX_RGB | AIGAR_PIX_LAST))) return -1;
  if ((flags & AIGAR_PIX_LAST) && !hist) return -1;
  const size_t lds = (size_t)side * side * 4;
#define PIX_LAUNCH(DT, ST)                                                                                       \
  do {                                                                                                           \
    hipLaunchKernelGGL((k_observe_pixel_state<DT, PIX_OCAP_FAST, ST>), dim3(d.NP), dim3(64), lds, s, d, out, side, \
                       seed, ovf, mask, hist);                                                                   \
    hipLaunchKernelGGL((k_observe_pixel_state<DT, PIX_OCAP, ST>), dim3(d.NP), dim3(64), lds, s, d, out, side, seed, \
                       ovf, mask, hist);                                                                         \
  } while (0)
#define PIX_FLAGS(DT)                                                   \
  do {                                                                  \
    switch (flags) {                                                    \
      case 0: PIX_LAUNCH(DT, PIX_ST); break;                            \
      case AIGAR_PIX_RGB: PIX_LAUNCH(DT, PIX_ST | PIX_ST_RGB); break;   \
      case AIGAR_PIX_LAST: PIX_LAUNCH(DT, PIX_ST | PIX_ST_LAST); break; \
      default: PIX_LAUNCH(DT, PIX_ST | PIX_ST_RGB | PIX_ST_LAST);       \
    }                                                                   \
  } while (0)
  if (dtype == 0) PIX_FLAGS(0);
  else PIX_FLAGS(1);
#undef PIX_FLAGS
#undef PIX_LAUNCH
  return 0;
}
