// conv_in.hip -- the first layer, conv3x3 3->64 straight from the NCHW fp32
// image (07:78 enc1.0, 14:122 enc1, VGG16 features.0) (gfx950, NHWC out).
//
//  * fwd / wgrad / dgrad, thread-per-pixel kernels
//  * wgrad with the activation backward fused (MFMA) and the finalizes
//  * im2col of the 3x3 patches, and the MFMA forward on the packed weights
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// first layer: thread = (pixel, 4 output channels); channel groups fastest
template <typename T>
__global__ void conv_in_fwd_kernel(int n, int h, int w, int cin, int cout,
                                   const float *__restrict__ x, const float *__restrict__ wt,
                                   const float *__restrict__ b, int act, const float *alpha,
                                   T *__restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float sw[];   // [cin*9][cout] + bias
  const int kk = cin * 9;
  for (int i = threadIdx.x; i < kk * cout; i += blockDim.x) {
    const int co = i % cout, j = i / cout;     // j = ci*9 + t
    sw[i] = wt[(long long)co * kk + j];
  }
  for (int i = threadIdx.x; i < cout; i += blockDim.x) sw[kk * cout + i] = b ? b[i] : 0.f;
  __syncthreads();
  const int G = cout / 4;
  const long long P = (long long)n * h * w;
  const float al = alpha ? alpha[0] : 0.f;
  for (long long id = blockIdx.x * (long long)blockDim.x + threadIdx.x; id < P * G;
       id += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(id % G);
    const long long p = id / G;
    const int ww = (int)(p % w);
    const long long nh = p / w;
    const int hh = (int)(nh % h);
    const int nn = (int)(nh / h);
    f32x4 acc = *reinterpret_cast<const f32x4 *>(sw + kk * cout + g * 4);
    for (int ci = 0; ci < cin; ++ci) {
      const float *xp = x + ((long long)nn * cin + ci) * h * w;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int y2 = hh + t / 3 - 1, x2 = ww + t % 3 - 1;
        if (y2 < 0 || y2 >= h || x2 < 0 || x2 >= w) continue;
        const float v = xp[(long long)y2 * w + x2];
        acc += v * *reinterpret_cast<const f32x4 *>(sw + (ci * 9 + t) * cout + g * 4);
      }
    }
    if (act == 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = fmaxf(acc[k], 0.f);
    } else if (act == 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = acc[k] > 0.f ? acc[k] : al * acc[k];
    }
    store4<T>(y + p * cout + g * 4, acc);
  }
}

// wgrad of the first layer: dW[co][j] (j = ci*9+t, padded to 32 with j=kk the
// bias "ones" column).  One workgroup = a pixel range; stage 64 pixels of dy
// [64][cout] and of the im2col patch [64][32] in LDS as fp32.
template <typename T>
__global__ void conv_in_wgrad_kernel(int n, int h, int w, int cin, int cout,
                                     const float *__restrict__ x, const T *__restrict__ dy,
                                     float *__restrict__ part, long long px_per_block) {
  __shared__ __attribute__((aligned(16))) float sdy[64][65];
  __shared__ __attribute__((aligned(16))) float spt[64][32];
  const int kk = cin * 9;
  const long long P = (long long)n * h * w;
  const long long pb = blockIdx.x * px_per_block;
  const long long pe = min(P, pb + px_per_block);
  // thread -> (co, jgroup of 8): cout*4 threads active (cout <= 64)
  const int co = threadIdx.x & 63, jg = threadIdx.x >> 6;
  // per-stage fp32 sums folded into fp64 accumulators: the bias column is a
  // sum of signed gradients with heavy cancellation (pairwise-like accuracy)
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long long p0 = pb; p0 < pe; p0 += 64) {
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += blockDim.x) {
      const int r = i >> 6, c = i & 63;
      const long long p = p0 + r;
      sdy[r][c] = (p < pe && c < cout) ? Elt<T>::load(dy, p * cout + c) : 0.f;
    }
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) {
      const int r = i >> 5, j = i & 31;
      const long long p = p0 + r;
      float v = 0.f;
      if (p < pe) {
        if (j < kk) {
          const int ci = j / 9, t = j % 9;
          const int ww = (int)(p % w);
          const long long nh = p / w;
          const int hh = (int)(nh % h);
          const int nn = (int)(nh / h);
          const int y2 = hh + t / 3 - 1, x2 = ww + t % 3 - 1;
          if (y2 >= 0 && y2 < h && x2 >= 0 && x2 < w)
            v = x[(((long long)nn * cin + ci) * h + y2) * w + x2];
        } else if (j == kk) {
          v = 1.f;
        }
      }
      spt[r][j] = v;
    }
    __syncthreads();
    if (co < cout) {
      float st[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int r = 0; r < 64; ++r) {
        const float d = sdy[r][co];
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(&spt[r][jg * 8]);
        const f32x4 a1 = *reinterpret_cast<const f32x4 *>(&spt[r][jg * 8 + 4]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { st[k] += d * a0[k]; st[4 + k] += d * a1[k]; }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += st[k];
    }
  }
  if (co < cout) {
#pragma unroll
    for (int k = 0; k < 8; ++k) part[((long long)blockIdx.x * cout + co) * 32 + jg * 8 + k] = (float)acc[k];
  }
}

// First-conv weight + bias grad fused with the backward of its activation
// (14:122-123: Conv2d(3, 64) -> PReLU; 07:78: -> ReLU), straight from the
// NCHW fp32 image: no im2col matrix and no materialised pre-activation grad.
//   gp[p][co] = t > 0 ? g : alpha g  (ReLU: 0),   dalpha = sum_{t<=0} g t
//   dW[co][n] = sum_p gp[p][co] patch[p][n],  n = ci*9 + ky*3 + kx (< 27),
//   column 27 of patch = 1  ->  db[co] = sum_p gp[p][co]
// bf16 MFMA 16x16x32 over 64-pixel steps: A = gp^T from an LDS transpose
// (channel rows of 64 pixels), B = the 32 patch rows of the same pixels,
// staged per step in LDS from the image (zero padded).  Per block:
// a fixed pixel range -> one [64][32] partial slab (+ a dalpha row), reduced
// by rr_colreduce + conv_in_wgrad_act_finalize in fixed order.
//
// REC: the pre-activation t is not read but recomputed per step from the
// staged patch and the packed first-layer weights (`t` then points at the
// kpad-32 pack the forward used, [64][32] bf16): conv_in_mfma_kernel's own
// MFMA -- A = the pack's rows (wave wv: channels 16 wv .. +15), B = 16 pixels
// x 32 patch entries with the ones column at k = 27, zero accumulator --
// rounded to bf16 as the forward stored it, so gp, the dalpha sum and gT are
// formed from the same bits in the same order.  The patch is staged a second
// time pixel-major (pX) for that B fragment; t goes through gT's own words
// (channel rows, the (lc, lpp) thread reads exactly the words it then
// overwrites with gp).
constexpr int CIA_NPX = 64;
constexpr int CIA_ROW = CIA_NPX + 8;                  // bf16 per LDS row (144 B)
constexpr int CIA_XROW = 32 + 8;                      // bf16 per pixel-major patch row (80 B)
template <bool REC>
__global__ __launch_bounds__(256, REC ? 4 : 1) void conv_in_wgrad_act_kernel(
    int n, int h, int w, const float *__restrict__ x, const bf16_t *__restrict__ g,
    const bf16_t *__restrict__ t, int act, const float *__restrict__ alpha,
    float *__restrict__ part, long long ppb) {
  // gT: gp^T, 64 channel rows of the step's 64 pixels; pT: the 32 patch rows
  // (27 image taps, a ones row, 4 zero rows) of the same pixels, bf16
  __shared__ __attribute__((aligned(16))) u16 gT[64 * CIA_ROW];
  __shared__ __attribute__((aligned(16))) u16 pT[32 * CIA_ROW];
  __shared__ __attribute__((aligned(16))) u16 pX[REC ? CIA_NPX * CIA_XROW : 8];
  __shared__ float red[256];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long P = (long long)n * h * w, hw = (long long)h * w;
  const long long p0 = blockIdx.x * ppb, p1 = min(P, p0 + ppb);
  const float al = act == 2 ? alpha[0] : 0.f;
  float sa = 0.f;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int lc = tid & 7, lpp = tid >> 3;             // gp load: 8-channel chunk, pixel pair
  const int bn = lane & 15, bk = lane >> 4;           // fragment col / k-block
  const int sj = tid & 63, sg = tid >> 6;             // patch staging: pixel, row group
  // registers of one step's operands, loaded a step ahead of their use
  uint4 rg[2], rt[2] = {};
  float rp[8];
  auto load_step = [&](long long q0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long long p = q0 + 2 * lpp + j;
      const bool ok = p < p1;
      const long long e = (ok ? p : p0) * 64 + lc * 8;
      rg[j] = *reinterpret_cast<const uint4 *>(g + e);
      if constexpr (!REC) rt[j] = *reinterpret_cast<const uint4 *>(t + e);
      if (!ok) rg[j] = uint4{0u, 0u, 0u, 0u};
    }
    const long long p = q0 + sj;
    const bool live = p < p1;
    int img = 0, y = 0, xx0 = 0;
    if (live) {
      img = (int)(p / hw);
      const int rem = (int)(p - img * hw);
      y = rem / w;
      xx0 = rem - y * w;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = sg + 4 * u;
      float val = 0.f;
      if (r < 27) {
        const int ci = r / 9, ky = (r % 9) / 3, kx = r % 3;
        const int yy = y + ky - 1, xx = xx0 + kx - 1;
        const bool ok = live && yy >= 0 && yy < h && xx >= 0 && xx < w;
        const float vv = x[ok ? (((long long)img * 3 + ci) * h + yy) * w + xx : 0];
        val = ok ? vv : 0.f;
      } else if (r == 27) {
        val = live ? 1.f : 0.f;
      }
      rp[u] = val;
    }
  };
  auto bf = [](uint32_t word, int hi) { return __uint_as_float(hi ? (word & 0xffff0000u) : (word << 16)); };
  // REC: the wave's weight fragment, rows co = 16 wv + bn, k = 8 bk .. +7
  bf16x8 fw = {};
  if constexpr (REC) fw = *reinterpret_cast<const bf16x8 *>(t + (wv * 16 + bn) * 32 + bk * 8);
  if (p0 < p1) load_step(p0);
  for (long long q0 = p0; q0 < p1; q0 += CIA_NPX) {
    if constexpr (REC) {
      // ---- the patch, both layouts; t = W patch for the wave's 16 channels
      // ---- x 64 pixels -> gT[co][px]; read back in the (lc, lpp) mapping
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const u16 pv = f32_to_bf16(rp[u]);
        pT[(sg + 4 * u) * CIA_ROW + sj] = pv;
        pX[sj * CIA_XROW + sg + 4 * u] = pv;
      }
      __syncthreads();
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const bf16x8 fp = *reinterpret_cast<const bf16x8 *>(&pX[(nb * 16 + bn) * CIA_XROW + bk * 8]);
        const f32x4 tv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fp, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) gT[(wv * 16 + 4 * bk + i) * CIA_ROW + nb * 16 + bn] = f32_to_bf16(tv[i]);
      }
      __syncthreads();
    }
    // ---- gp for pixels q0 + 2 lpp, +1, channels 8 lc .. +7 -> gT[co][px] ----
    u16 v[2][8];
    uint32_t tpair[8];                                  // REC: t of (px 2 lpp, +1) per channel
    if constexpr (REC) {
#pragma unroll
      for (int k = 0; k < 8; ++k)
        tpair[k] = *reinterpret_cast<const uint32_t *>(&gT[(lc * 8 + k) * CIA_ROW + 2 * lpp]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t gw[4] = {rg[j].x, rg[j].y, rg[j].z, rg[j].w};
      const uint32_t tw[4] = {rt[j].x, rt[j].y, rt[j].z, rt[j].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float gg = bf(gw[k >> 1], k & 1);
        const float tt = REC ? bf(tpair[k], j) : bf(tw[k >> 1], k & 1);
        const float gp = tt > 0.f ? gg : al * gg;
        sa += tt > 0.f ? 0.f : gg * tt;
        v[j][k] = f32_to_bf16(gp);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)
      *reinterpret_cast<uint32_t *>(&gT[(lc * 8 + k) * CIA_ROW + 2 * lpp]) =
          (uint32_t)v[0][k] | ((uint32_t)v[1][k] << 16);
    if constexpr (!REC) {
#pragma unroll
      for (int u = 0; u < 8; ++u) pT[(sg + 4 * u) * CIA_ROW + sj] = f32_to_bf16(rp[u]);
    }
    __syncthreads();
    if (q0 + CIA_NPX < p1) load_step(q0 + CIA_NPX);     // next step's operands in flight
    // ---- MFMA: wave wv owns channels 16 wv .. +15, both 32-pixel k-steps ----
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int px = ks * 32 + bk * 8;
      const bf16x8 fa = *reinterpret_cast<const bf16x8 *>(&gT[(wv * 16 + bn) * CIA_ROW + px]);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const bf16x8 fb = *reinterpret_cast<const bf16x8 *>(&pT[(nb * 16 + bn) * CIA_ROW + px]);
        acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // ---- partial slab [64][32] + dalpha row [32] ----
  float *pw = part + (long long)blockIdx.x * (64 * 32 + 32);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) pw[(wv * 16 + 4 * bk + i) * 32 + nb * 16 + bn] = acc[nb][i];
  red[tid] = sa;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid < 32) pw[64 * 32 + tid] = tid == 0 ? red[0] : 0.f;
}

__global__ void conv_in_wgrad_act_finalize(int chunks, const double *__restrict__ part, float *dw,
                                           float *db, float *dalpha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over 64 * 32 + 1
  const int cols = 64 * 32 + 32;
  if (i > 64 * 32) return;
  double sv[1] = {0};
  rr_fixed_sum<1>(part + i, cols, chunks, sv);
  const double s = sv[0];
  if (i == 64 * 32) {
    if (dalpha) dalpha[0] = (float)s;
    return;
  }
  const int co = i / 32, j = i % 32;
  if (j < 27) dw[co * 27 + j] = (float)s;
  else if (j == 27 && db) db[co] = (float)s;
}

__global__ void conv_in_wgrad_finalize(int cout, int kk, int blocks, const double *__restrict__ part,
                                       float *dw, float *db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over cout*32
  if (i >= cout * 32) return;
  const int co = i / 32, j = i % 32;
  if (j > kk) return;
  double sv[1] = {0};
  rr_fixed_sum<1>(part + i, (long long)cout * 32, blocks, sv);
  const double s = sv[0];
  if (j < kk) dw[(long long)co * kk + j] = (float)s;
  else if (db) db[co] = (float)s;
}

// dgrad of the first layer into the NCHW fp32 image grad: thread = pixel
template <typename T>
__global__ void conv_in_dgrad_kernel(int n, int h, int w, int cin, int cout,
                                     const T *__restrict__ dy, const float *__restrict__ wt,
                                     float *__restrict__ dx, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [t][ci][cout]
  const int kk = cin * 9;
  for (int i = threadIdx.x; i < kk * cout; i += blockDim.x) {
    const int co = i % cout, j = i / cout;   // j = t*cin + ci
    const int t = j / cin, ci = j % cin;
    sw[i] = wt[((long long)co * cin + ci) * 9 + t];
  }
  __syncthreads();
  const long long P = (long long)n * h * w;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P;
       p += (long long)gridDim.x * blockDim.x) {
    const int ww = (int)(p % w);
    const long long nh = p / w;
    const int hh = (int)(nh % h);
    const int nn = (int)(nh / h);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < 9; ++t) {
      // output pixel o with o + (ky-1, kx-1) = this pixel
      const int ky = t / 3, kx = t % 3;
      const int y2 = hh - ky + 1, x2 = ww - kx + 1;
      if (y2 < 0 || y2 >= h || x2 < 0 || x2 >= w) continue;
      const T *dp = dy + (((long long)nn * h + y2) * w + x2) * cout;
      for (int c = 0; c < cout; c += 4) {
        const f32x4 d = load4<T>(dp + c);
        for (int ci = 0; ci < cin && ci < 4; ++ci) {
          const f32x4 wv = *reinterpret_cast<const f32x4 *>(sw + (t * cin + ci) * cout + c);
          acc[ci] += d[0] * wv[0] + d[1] * wv[1] + d[2] * wv[2] + d[3] * wv[3];
        }
      }
    }
    for (int ci = 0; ci < cin && ci < 4; ++ci) {
      const long long o = (((long long)nn * cin + ci) * h + hh) * w + ww;
      dx[o] = accumulate ? dx[o] + acc[ci] : acc[ci];
    }
  }
}

// ---------------------------------------------------------------------------
// im2col of the first 3x3 conv straight from the NCHW fp32 image:
// col[p][j] = x[n][ci][h+ky-1][w+kx-1] for j = ci*9 + ky*3 + kx < 9*cin,
// col[p][9*cin] = 1 (the bias column: its wgrad column is the bias grad),
// 0 up to kpad.  The first conv then runs as a K = kpad implicit GEMM.
template <typename T>
__global__ void im2col3_kernel(int n, int h, int w, int cin, int kpad, const float *__restrict__ x,
                               T *__restrict__ col) {
  const int G = kpad / 4;
  const long long total = (long long)n * h * w * G;
  const int kk = cin * 9;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const long long p = i / G;
    const int ww = (int)(p % w);
    const long long nh = p / w;
    const int hh = (int)(nh % h);
    const int nn = (int)(nh / h);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = g * 4 + e;
      float val = 0.f;
      if (j < kk) {
        const int ci = j / 9, t = j - (j / 9) * 9;
        const int y2 = hh + t / 3 - 1, x2 = ww + t % 3 - 1;
        if (y2 >= 0 && y2 < h && x2 >= 0 && x2 < w)
          val = x[(((long long)nn * cin + ci) * h + y2) * w + x2];
      } else if (j == kk) {
        val = 1.f;
      }
      v[e] = val;
    }
    store4<T>(col + p * kpad + g * 4, v);
  }
}

// First 3x3 conv (cin 3 -> cout 64), bf16, fused im2col + MFMA.  K = 27
// taps + the bias column (k = 27, value 1) padded to 32 = ONE
// v_mfma_f32_16x16x32_bf16 per 16x16 tile.  The B fragment (lane: pixel
// l & 15, k = 8 (l >> 4) .. +7) is gathered straight from the NCHW fp32 image
// (L1/L2-hot: each value is read by 9 taps x neighbouring pixels) and rounded
// to bf16 exactly as rr_im2col3 does; the A fragments (packed weights
// [64][32] bf16, rr_pack_conv_in with kpad 32) stay in registers.  A wave
// owns 64 consecutive pixels x 64 channels; epilogue staged through LDS so
// every store is a 1 KiB run (8 pixels x 128 B): y_pre = conv + bias,
// y_act = relu / prelu(alpha) of it (either may be null).
__global__ __launch_bounds__(256) void conv_in_mfma_kernel(int n, int h, int w,
                                                           const float *__restrict__ x,
                                                           const bf16_t *__restrict__ wp, int act,
                                                           const float *__restrict__ alpha,
                                                           bf16_t *__restrict__ y_pre,
                                                           bf16_t *__restrict__ y_act) {
  constexpr int SR = 68;                       // fp32 staging row (floats), padded
  __shared__ __attribute__((aligned(16))) float stg[4][32 * SR];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long hw = (long long)h * w;
  const long long P = (long long)n * hw;
  const long long p0 = ((long long)blockIdx.x * 4 + wv) * 64;
  if (p0 >= P) return;                         // whole wave out of range (no block barrier used)
  const int fr = lane & 15, q = lane >> 4;
  // weights: A[mi] = rows co = 16 mi + fr, k = 8q .. 8q+7
  bf16x8 fa[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
    fa[mi] = *reinterpret_cast<const bf16x8 *>(wp + (mi * 16 + fr) * 32 + q * 8);
  // this lane's 8 k's: (plane, dy, dx) of the tap; k == 27 is the bias column
  const int hwi = h * w;
  int kofs[8], kdy[8], kdx[8];
  bool ktap[8], kone[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = q * 8 + j;
    const int ci = k / 9, t = k - (k / 9) * 9;
    kdy[j] = t / 3 - 1;
    kdx[j] = t % 3 - 1;
    kofs[j] = ci * hwi + kdy[j] * w + kdx[j];
    ktap[j] = k < 27;
    kone[j] = k == 27;
  }
  const int Pi = (int)P;
  // raw buffer over the whole image batch (host: 12 P < 2^32 bytes)
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(x), 0, (int)(3 * P * 4), 0x00020000);
  const int pw0 = (int)p0;
  f32x4 acc[4][4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    // branch-free gather: every lane loads (a clamped, in-bounds address when
    // the tap is padding) and selects; 32-bit index math (host: 3P < 2^31)
    const int p = pw0 + ni * 16 + fr;
    const bool live = p < Pi;
    const int pc = live ? p : 0;
    const int nn = pc / hwi, rem = pc - (pc / hwi) * hwi;
    const int yy = rem / w, xx = rem - (rem / w) * w;
    const int base = nn * 3 * hwi + rem;
    bf16x8 fb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int y2 = yy + kdy[j], x2 = xx + kdx[j];
      const bool ok = ktap[j] && live && (unsigned)y2 < (unsigned)h && (unsigned)x2 < (unsigned)w;
      // padding taps: offset past num_records -> the range check returns 0
      const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
          xr, ok ? (base + kofs[j]) * 4 : 0xffffffff, 0, 0));
      fb[j] = (__bf16)(v + (kone[j] ? 1.f : 0.f));    // v_cvt_pk_bf16_f32: RNE
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi], fb, f32x4{0.f, 0.f, 0.f, 0.f},
                                                           0, 0, 0);
  }
  // epilogue in two halves of 32 pixels (ni 0-1, then 2-3): a 32-row fp32
  // staging tile per wave (35 KB per workgroup instead of 70) lets 4
  // workgroups share a CU instead of 2.  Stage: pixel ni*16 + fr, channels
  // 16 mi + 4 q .. +3
  float *sw = stg[wv];
  // negative-side slope: 1 (none), 0 (ReLU), alpha (PReLU)
  const float slope = act == 2 ? alpha[0] : (act == 1 ? 0.f : 1.f);
  const int rows = (int)min(64LL, P - p0);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // first half read back
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 2; ++nj)
        *reinterpret_cast<f32x4 *>(sw + (nj * 16 + fr) * SR + mi * 16 + q * 4) = acc[mi][half * 2 + nj];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's LDS writes landed
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rl = i * 8 + (lane >> 3), c8 = (lane & 7) * 8;
      const int r = half * 32 + rl;
      if (r < rows) {
        const long long p = p0 + r;
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(sw + rl * SR + c8);
        const f32x4 v1 = *reinterpret_cast<const f32x4 *>(sw + rl * SR + c8 + 4);
        if (y_pre) store8<bf16_t>(y_pre + p * 64 + c8, v0, v1);
        if (y_act) {
          f32x4 a0, a1;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            a0[k] = v0[k] > 0.f ? v0[k] : slope * v0[k];
            a1[k] = v1[k] > 0.f ? v1[k] : slope * v1[k];
          }
          store8<bf16_t>(y_act + p * 64 + c8, a0, a1);
        }
      }
    }
  }
}

}  // namespace

extern "C" int rr_im2col3(int dtype, int n, int h, int w, int cin, int kpad, const float *x,
                          void *col, rr_stream stream) {
  if (!x || !col || cin <= 0 || kpad % 4 || kpad < 9 * cin + 1) return RR_EINVAL;
  const long long total = (long long)n * h * w * (kpad / 4);
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(im2col3_kernel<T>, g, b, 0, st, n, h, w, cin, kpad, x, (T *)col);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_conv_in_fwd(int dtype, int n, int h, int w, int cin, int cout, const float *x,
                              const float *wt, const float *b, int act, const float *alpha,
                              void *y, rr_stream stream) {
  if (!x || !wt || !y || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin > 4 || cout % 4 ||
      cout > 128 || (act == 2 && !alpha))
    return RR_EINVAL;
  const long long work = (long long)n * h * w * (cout / 4);
  const size_t shm = ((size_t)cin * 9 * cout + cout) * sizeof(float);
  dim3 g(rr_grid_cap((work + 255) / 256, 8192)), bl(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv_in_fwd_kernel<T>, g, bl, shm, st, n, h, w, cin, cout, x, wt, b, act,
                       alpha, (T *)y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

int rr_colreduce_misc(const float *in, int rows, int cols, double *out, hipStream_t st);   // misc.hip
static int conv_in_wgrad_blocks(int n, int h, int w) {
  const long long P = (long long)n * h * w;
  long long b = (P + 2047) / 2048;
  if (b > 1024) b = 1024;
  return (int)(b < 1 ? 1 : b);
}

extern "C" size_t rr_conv_in_wgrad_workspace(int n, int h, int w, int cin, int cout) {
  (void)cin;
  const int blocks = conv_in_wgrad_blocks(n, h, w);
  return (size_t)blocks * cout * 32 * sizeof(float) + rr_colreduce_bytes(blocks, cout * 32);
}

extern "C" int rr_conv_in_wgrad(int dtype, int n, int h, int w, int cin, int cout, const float *x,
                                const void *dy, float *dw, float *db, void *ws, size_t ws_bytes,
                                rr_stream stream) {
  if (!x || !dy || !dw || cin * 9 >= 32 || cout > 64 || cout <= 0) return RR_EINVAL;
  const int blocks = conv_in_wgrad_blocks(n, h, w);
  const size_t pbytes = (size_t)blocks * cout * 32 * sizeof(float);
  if (!ws || ws_bytes < pbytes + rr_colreduce_bytes(blocks, cout * 32)) return RR_EWORKSPACE;
  const long long P = (long long)n * h * w;
  long long ppb = (P + blocks - 1) / blocks;
  hipStream_t st = (hipStream_t)stream;
  const int rc = rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv_in_wgrad_kernel<T>, dim3(blocks), dim3(256), 0, st, n, h, w, cin, cout,
                       x, (const T *)dy, (float *)ws, ppb);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc != RR_OK) return rc;
  double *red = (double *)((char *)ws + pbytes);
  const int chunks = rr_colreduce_misc((const float *)ws, blocks, cout * 32, red, st);
  if (chunks < 0) return RR_ELAUNCH;
  hipLaunchKernelGGL(conv_in_wgrad_finalize, dim3((cout * 32 + 255) / 256), dim3(256), 0, st, cout,
                     cin * 9, chunks, (const double *)red, dw, db);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

static int conv_in_act_blocks(long long P) {
  long long b = (P + 511) / 512;
  if (b > 2048) b = 2048;
  return (int)(b < 1 ? 1 : b);
}

extern "C" size_t rr_conv_in_wgrad_act_workspace(int n, int h, int w) {
  const int blocks = conv_in_act_blocks((long long)n * h * w);
  return (size_t)blocks * (64 * 32 + 32) * sizeof(float) + rr_colreduce_bytes(blocks, 64 * 32 + 32);
}

// rec: t_pre is the forward's kpad-32 weight pack, the pre-activation recomputed
static int conv_in_wgrad_act(bool rec, int n, int h, int w, const float *x, const void *dy,
                             const void *t_pre, int act, const float *alpha, float *dw, float *db,
                             float *dalpha, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!x || !dy || !t_pre || !dw || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (act < 1 || act > 2 || (act == 2 && !alpha)) return RR_EINVAL;
  const long long P = (long long)n * h * w;
  const int blocks = conv_in_act_blocks(P);
  const size_t pbytes = (size_t)blocks * (64 * 32 + 32) * sizeof(float);
  if (!ws || ws_bytes < pbytes + rr_colreduce_bytes(blocks, 64 * 32 + 32)) return RR_EWORKSPACE;
  long long ppb = (P + blocks - 1) / blocks;
  ppb = (ppb + CIA_NPX - 1) / CIA_NPX * CIA_NPX;            // whole 64-pixel steps (8-aligned)
  hipStream_t st = (hipStream_t)stream;
  if (rec)
    hipLaunchKernelGGL(conv_in_wgrad_act_kernel<true>, dim3(blocks), dim3(256), 0, st, n, h, w, x,
                       (const bf16_t *)dy, (const bf16_t *)t_pre, act, alpha, (float *)ws, ppb);
  else
    hipLaunchKernelGGL(conv_in_wgrad_act_kernel<false>, dim3(blocks), dim3(256), 0, st, n, h, w, x,
                       (const bf16_t *)dy, (const bf16_t *)t_pre, act, alpha, (float *)ws, ppb);
  RR_CHECK_LAUNCH();
  double *red = (double *)((char *)ws + pbytes);
  const int chunks = rr_colreduce_misc((const float *)ws, blocks, 64 * 32 + 32, red, st);
  if (chunks < 0) return RR_ELAUNCH;
  hipLaunchKernelGGL(conv_in_wgrad_act_finalize, dim3((64 * 32 + 1 + 255) / 256), dim3(256), 0, st,
                     chunks, (const double *)red, dw, db, act == 2 ? dalpha : nullptr);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_conv_in_wgrad_act(int n, int h, int w, const float *x, const void *dy,
                                    const void *t_pre, int act, const float *alpha, float *dw,
                                    float *db, float *dalpha, void *ws, size_t ws_bytes,
                                    rr_stream stream) {
  return conv_in_wgrad_act(false, n, h, w, x, dy, t_pre, act, alpha, dw, db, dalpha, ws, ws_bytes, stream);
}

extern "C" int rr_conv_in_wgrad_act_rec(int n, int h, int w, const float *x, const void *dy,
                                        const void *wpack32, int act, const float *alpha, float *dw,
                                        float *db, float *dalpha, void *ws, size_t ws_bytes,
                                        rr_stream stream) {
  return conv_in_wgrad_act(true, n, h, w, x, dy, wpack32, act, alpha, dw, db, dalpha, ws, ws_bytes, stream);
}

extern "C" int rr_conv_in_dgrad(int dtype, int n, int h, int w, int cin, int cout, const void *dy,
                                const float *wt, float *dx, int accumulate, rr_stream stream) {
  if (!dy || !wt || !dx || cin > 4 || cout % 4) return RR_EINVAL;
  const long long P = (long long)n * h * w;
  const size_t shm = (size_t)cin * 9 * cout * sizeof(float);
  dim3 g(rr_grid_cap((P + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv_in_dgrad_kernel<T>, g, b, shm, st, n, h, w, cin, cout, (const T *)dy, wt,
                       dx, accumulate);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_conv_in_mfma(int n, int h, int w, const float *x, const void *wpack32, int act,
                               const float *alpha, void *y_pre, void *y_act, rr_stream stream) {
  if (!x || !wpack32 || (!y_pre && !y_act) || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (act < 0 || act > 2 || (act == 2 && !alpha) || (y_act == nullptr && act != 0)) return RR_EINVAL;
  const long long P = (long long)n * h * w;
  if (12 * P >= 0x7fffffffLL) return RR_EUNSUPPORTED;         // 32-bit buffer byte offsets
  const long long blocks = (P + 255) / 256;
  hipLaunchKernelGGL(conv_in_mfma_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     n, h, w, x, (const bf16_t *)wpack32, act, alpha, (bf16_t *)y_pre,
                     (bf16_t *)y_act);
  RR_CHECK_LAUNCH();
  return RR_OK;
}
