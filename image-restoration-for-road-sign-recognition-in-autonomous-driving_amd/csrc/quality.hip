// quality.hip -- the metric leg of the 08 loop (08:118-125),
// on device: the clean image through cv2.resize, then PSNR and SSIM against
// the restored one.
//   * rr_cv_resize_linear_u8: cv2.resize(img, (ow, oh)) INTER_LINEAR
//     (08:118-119) -- OpenCV's own fixed-point bilinear (resize.cpp
//     resizeGeneric_ + HResizeLinear / VResizeLinear), not Pillow's: 11-bit
//     weights from float source coordinates, an exact int32 horizontal pass,
//     the vertical pass as the x86 SIMD body computes it
//     (VResizeLinearVec_32s8u) with the scalar 22-bit rounding on the row
//     tail; bit-equal to oracle/imgproc_cpu.cv_resize_linear (parity vs cv2
//     itself unpinned: cv2 is not installed).
//   * rr_cv_resize_ragged_u8: the same for n images of unequal size in one
//     buffer, one launch, the scale taken per image on the device.
//   * rr_eval_ragged_u8: PSNR and SSIM (08:123-125) of those resized clean
//     images against a dense restored batch in two launches; the resized clean
//     image lives in LDS tiles only.
//   * rr_ssim_u8: skimage structural_similarity(a, b, data_range=255,
//     channel_axis=2) (08:125) of two dense batches: 7x7 uniform window,
//     sample covariance (49/48), K1 = .01, K2 = .03, mean of S over the
//     interior (3-pixel border cropped), mean over channels, fp64.
// The cvr_* functions state the resize's per-pixel arithmetic once for the
// three kernels that use it: those share this file.  The fp64 S makes the
// SSIM kernels VALU-bound; the resizes are byte traffic.
#include "imgproc.h"

namespace {

// ------------------------------------------------------------------ SSIM ----
constexpr int SS_T = 256;

// one workgroup per (image, channel): thread = output column, sliding 7-row
// window of exact integer 7x7 sums (x, y, x^2, y^2, xy); S in fp64; fixed-order
// reduction -> per-(image, channel) mean of S over the cropped interior
__global__ __launch_bounds__(SS_T) void ssim_kernel(int h, int w, int C, const uint8_t *__restrict__ a,
                                                    const uint8_t *__restrict__ b,
                                                    double *__restrict__ chan_mean) {
  const int img = blockIdx.x / C, ch = blockIdx.x % C;
  const uint8_t *pa = a + (long long)img * h * w * C + ch;
  const uint8_t *pb = b + (long long)img * h * w * C + ch;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double cov_norm = 49.0 / 48.0;
  double acc = 0.0;
  for (int cx = 3 + threadIdx.x; cx < w - 3; cx += SS_T) {
    auto hsum = [&](int y, int &sx, int &sy, int &sxx, int &syy, int &sxy) {
      sx = sy = sxx = syy = sxy = 0;
      const long long base = ((long long)y * w + cx - 3) * C;
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        const int x = pa[base + d * C], y2 = pb[base + d * C];
        sx += x; sy += y2; sxx += x * x; syy += y2 * y2; sxy += x * y2;
      }
    };
    int vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;
    for (int y = 0; y < h; ++y) {
      int sx, sy, sxx, syy, sxy;
      hsum(y, sx, sy, sxx, syy, sxy);
      vx += sx; vy += sy; vxx += sxx; vyy += syy; vxy += sxy;
      if (y >= 7) {
        hsum(y - 7, sx, sy, sxx, syy, sxy);
        vx -= sx; vy -= sy; vxx -= sxx; vyy -= syy; vxy -= sxy;
      }
      if (y >= 6) {
        const double ux = vx / 49.0, uy = vy / 49.0;
        const double uxx = vxx / 49.0, uyy = vyy / 49.0, uxy = vxy / 49.0;
        const double sxv = cov_norm * (uxx - ux * ux);
        const double syv = cov_norm * (uyy - uy * uy);
        const double sxyv = cov_norm * (uxy - ux * uy);
        const double A1 = 2 * ux * uy + C1, A2 = 2 * sxyv + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = sxv + syv + C2;
        acc += (A1 * A2) / (B1 * B2);
      }
    }
  }
  __shared__ double red[SS_T];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = SS_T / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) chan_mean[blockIdx.x] = red[0] / ((double)(h - 6) * (w - 6));
}

// ---------------------------------------------------------- cv resize ----
// resize.cpp's coefficient of output coordinate d: float source position
// (d + 0.5) * scale - 0.5 evaluated in double then rounded to float (no FMA:
// contraction would change the rounding), its floor and fraction
__device__ __forceinline__ void cvr_coord(int d, double scale, int *i, float *f) {
#pragma clang fp contract(off)
  const double v = ((double)d + 0.5) * scale - 0.5;
  const float fv = (float)v;
  const float fl = floorf(fv);
  *i = (int)fl;
  *f = fv - fl;
}

__device__ __forceinline__ int cvr_round(float v) { return __float2int_rn(v); }   // cvRound

// The per-pixel arithmetic, shared by the dense kernel, the ragged kernel and
// the fused evaluation (one statement of it, so the three agree bit for bit):
// the two source columns and 11-bit weights of output column x (index clamped
// and fraction zeroed at the borders), the two source rows and weights of
// output row y (rows clamped when fetched, weights kept), and the blend.
struct CvrX { int sx, sx1, a0, a1; };
struct CvrY { int r0, r1, b0, b1; };

__device__ __forceinline__ CvrX cvr_xcoef(int x, int w, double scale) {
#pragma clang fp contract(off)
  int sx;
  float fx;
  cvr_coord(x, scale, &sx, &fx);
  if (sx < 0) { sx = 0; fx = 0.f; }
  if (sx >= w - 1) { sx = w - 1; fx = 0.f; }
  CvrX k;
  k.a0 = cvr_round((1.f - fx) * 2048.f);
  k.a1 = cvr_round(fx * 2048.f);
  k.sx = sx;
  k.sx1 = sx + 1 < w ? sx + 1 : w - 1;
  return k;
}

__device__ __forceinline__ CvrY cvr_ycoef(int y, int h, double scale) {
#pragma clang fp contract(off)
  int sy;
  float fy;
  cvr_coord(y, scale, &sy, &fy);
  CvrY k;
  k.b0 = cvr_round((1.f - fy) * 2048.f);
  k.b1 = cvr_round(fy * 2048.f);
  k.r0 = sy < 0 ? 0 : (sy > h - 1 ? h - 1 : sy);
  k.r1 = sy + 1 < 0 ? 0 : (sy + 1 > h - 1 ? h - 1 : sy + 1);
  return k;
}

// output pixel x of a row, from source rows p0 (ky.r0) and p1 (ky.r1);
// vec_end = first row element (x * C + ch) of the scalar tail
template <int C>
__device__ __forceinline__ void cvr_blend(const uint8_t *__restrict__ p0, const uint8_t *__restrict__ p1,
                                          const CvrX &kx, const CvrY &ky, int x, int vec_end,
                                          uint8_t (&o)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int s0 = (int)p0[kx.sx * C + c] * kx.a0 + (int)p0[kx.sx1 * C + c] * kx.a1;
    const int s1 = (int)p1[kx.sx * C + c] * kx.a0 + (int)p1[kx.sx1 * C + c] * kx.a1;
    int v;
    if (x * C + c < vec_end) {
      // v_mul_hi on the int16-packed S >> 4, then v_rshr_pack_u<2>
      v = ((((s0 >> 4) * ky.b0) >> 16) + (((s1 >> 4) * ky.b1) >> 16) + 2) >> 2;
    } else {
      v = (int)(((long long)s0 * ky.b0 + (long long)s1 * ky.b1 + (1LL << 21)) >> 22);
    }
    o[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// VResizeLinearVec_32s8u: x <= width - lanes in full vectors, then
// x < width - lanes / 2 in half vectors; the rest scalar (host)
static int cvr_vec_end(int ow, int c, int simd_lanes) {
  const int width = ow * c;
  int ve = (width / simd_lanes) * simd_lanes;
  while (ve < width - simd_lanes / 2) ve += simd_lanes / 2;
  return ve;
}

// one thread per output pixel, C channels
template <int C>
__global__ void cv_resize_linear_kernel(int n, int h, int w, int oh, int ow, double sx_scale,
                                        double sy_scale, int vec_end,
                                        const uint8_t *__restrict__ in, uint8_t *__restrict__ out) {
  const long long total = (long long)n * oh * ow;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(q % ow);
    const long long r = q / ow;
    const int y = (int)(r % oh);
    const int im = (int)(r / oh);
    const CvrX kx = cvr_xcoef(x, w, sx_scale);
    const CvrY ky = cvr_ycoef(y, h, sy_scale);
    const uint8_t *p0 = in + ((long long)im * h + ky.r0) * w * C;
    const uint8_t *p1 = in + ((long long)im * h + ky.r1) * w * C;
    uint8_t o[C];
    cvr_blend<C>(p0, p1, kx, ky, x, vec_end, o);
    uint8_t *dst = out + q * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = o[c];
  }
}

// ------------------------------------------------------ ragged cv resize ----
// cv2.resize of every image of a ragged buffer to oh x ow in one launch
// (rr_cv_resize_ragged_u8): one workgroup per (image, CVG_T * CVG_PER output
// pixels), so the table record is uniform over the workgroup; the scale is
// that image's own, by the dense entry point's expression; an image already
// oh x ow is copied (cv::resize); a record that fails rg_valid reads nothing
// and its output is zeros.
constexpr int CVG_T = 256, CVG_PER = 4;

template <int C>
__global__ __launch_bounds__(CVG_T) void cv_resize_ragged_kernel(int max_h, int max_w, int oh, int ow,
                                                                 int chunks, int vec_end, long long in_bytes,
                                                                 const uint8_t *__restrict__ in,
                                                                 const rr_ragged_image *__restrict__ tab,
                                                                 uint8_t *__restrict__ out) {
#pragma clang fp contract(off)
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const rr_ragged_image r = tab[img];
  const bool ok = rg_valid(r, C, max_h, max_w, in_bytes);          // uniform
  const bool same = r.h == oh && r.w == ow;
  const int w = ok ? r.w : 1, h = ok ? r.h : 1;
  // hal::resize: scale = 1 / inv_scale, inv_scale = dst / src (double)
  const double sxs = 1.0 / ((double)ow / (double)w), sys = 1.0 / ((double)oh / (double)h);
  const long long npix = (long long)oh * ow;
  const uint8_t *src = in + (ok ? r.offset : 0);
  uint8_t *dst = out + (long long)img * npix * C;
  for (int k = 0; k < CVG_PER; ++k) {
    const long long q = ((long long)chunk * CVG_PER + k) * CVG_T + threadIdx.x;
    if (q >= npix) break;
    uint8_t o[C];
    if (!ok) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = 0;
    } else if (same) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = src[q * C + c];
    } else {
      const int y = (int)(q / ow), x = (int)(q - (long long)y * ow);
      const CvrX kx = cvr_xcoef(x, w, sxs);
      const CvrY ky = cvr_ycoef(y, h, sys);
      cvr_blend<C>(src + (long long)ky.r0 * w * C, src + (long long)ky.r1 * w * C, kx, ky, x, vec_end, o);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) dst[q * C + c] = o[c];
  }
}

// ------------------------------------------------------ fused evaluation ----
// PSNR and SSIM of cv2.resize(clean_i, (ow, oh)) against restored_i for a
// ragged batch of clean images (rr_eval_ragged_u8; 08:118-125) in two
// launches, the resized clean image never in HBM.
//   1. ev_tile_kernel: one workgroup per (image, EV_T x EV_T block of output
//      pixels).  It fills two LDS tiles with the block and the 6 rows / columns
//      below / right of it (clipped at the image edge): the resized clean
//      pixels, each by cvr_blend from its 2 x 2 source pixels, and the restored
//      pixels.  Ownership: a PIXEL belongs to the block that contains it (the
//      squared error), a 7 x 7 WINDOW to the block that contains its top-left
//      pixel (SSIM), so every pixel and every window that fits the image is
//      counted by exactly one workgroup.  The window sums of x, y, x^2, y^2,
//      xy are exact integers (horizontal 7-sums into LDS, then vertical); S
//      is written as ssim_kernel writes it, in fp64, but it is NOT the same
//      arithmetic: this kernel is compiled with fp contraction off, and
//      ssim_kernel is not, so there uxx - ux * ux, 2 * ux * uy + C1 and their
//      kin become fused multiply-adds and S can differ in its last bits
//      (open items); the block's S is summed per channel
//      in a fixed order (thread-serial, a fixed butterfly over the wave, the
//      four waves in index order).  One partial record per workgroup, no
//      atomics.
//   2. ev_final_kernel: one thread per image (lane 0 of a wave whose lanes
//      fetch the records) adds its blocks' records in block order and closes with psnr_kernel's and ssim_chan_mean_kernel's
//      expressions.  A record that fails rg_valid: NaN, NaN, nothing read.
constexpr int EV_T = 32, EV_H = EV_T + 6, EV_THREADS = 256;

struct EvPartial {
  unsigned long long sse;            // sum (a - b)^2 over the block's own pixels and channels
  double s[4];                       // sum of S over the block's own windows, per channel
};

struct EvArgs {
  int n, max_h, max_w, oh, ow, tiles_y, tiles_x, vec_end;
  long long in_bytes;
  const uint8_t *clean;
  const rr_ragged_image *tab;
  const uint8_t *restored;
  EvPartial *part;
};

template <int C>
__global__ __launch_bounds__(EV_THREADS) void ev_tile_kernel(EvArgs a) {
#pragma clang fp contract(off)
  // a staged pixel is one dword whatever C is: channel ch in byte ch
  __shared__ uint32_t ta[EV_H * EV_H], tb[EV_H * EV_H];
  __shared__ uint4 hs[EV_H * EV_T];          // horizontal 7-sums: sx | sy << 16, sxx, syy, sxy
  __shared__ CvrX kxs[EV_H];
  __shared__ CvrY kys[EV_H];
  __shared__ double wsum[4][EV_THREADS / 64];
  __shared__ unsigned int wsse[EV_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int tiles = a.tiles_y * a.tiles_x;
  const int img = blockIdx.x / tiles, tl = blockIdx.x - img * tiles;
  const int y0 = (tl / a.tiles_x) * EV_T, x0 = (tl % a.tiles_x) * EV_T;
  const rr_ragged_image r = a.tab[img];
  if (!rg_valid(r, C, a.max_h, a.max_w, a.in_bytes)) return;       // uniform, before any barrier
  // staged rows / columns, own pixels, own windows (all >= 0; th, tw, bh, bw >= 1)
  const int th = a.oh - y0 < EV_H ? a.oh - y0 : EV_H, tw = a.ow - x0 < EV_H ? a.ow - x0 : EV_H;
  const int bh = th < EV_T ? th : EV_T, bw = tw < EV_T ? tw : EV_T;
  const int nwy = th - 6 < 0 ? 0 : (th - 6 < EV_T ? th - 6 : EV_T);
  const int nwx = tw - 6 < 0 ? 0 : (tw - 6 < EV_T ? tw - 6 : EV_T);
  const bool same = r.h == a.oh && r.w == a.ow;
  const uint8_t *src = a.clean + r.offset;
  if (!same) {
    // hal::resize: scale = 1 / inv_scale, inv_scale = dst / src (double)
    if (t < tw) kxs[t] = cvr_xcoef(x0 + t, r.w, 1.0 / ((double)a.ow / (double)r.w));
    else if (t >= 64 && t - 64 < th) kys[t - 64] = cvr_ycoef(y0 + t - 64, r.h, 1.0 / ((double)a.oh / (double)r.h));
    __syncthreads();
  }
  const uint8_t *rst = a.restored + (long long)img * a.oh * a.ow * C;
  for (int i = t; i < th * tw; i += EV_THREADS) {
    const int ly = i / tw, lx = i - ly * tw;
    const int y = y0 + ly, x = x0 + lx;
    uint8_t o[C];
    if (same) {
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = src[((long long)y * r.w + x) * C + c];
    } else {
      const CvrY ky = kys[ly];
      cvr_blend<C>(src + (long long)ky.r0 * r.w * C, src + (long long)ky.r1 * r.w * C, kxs[lx], ky, x,
                   a.vec_end, o);
    }
    const uint8_t *pb = rst + ((long long)y * a.ow + x) * C;
    uint32_t va = 0, vb = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      va |= (uint32_t)o[c] << (8 * c);
      vb |= (uint32_t)pb[c] << (8 * c);
    }
    ta[ly * EV_H + lx] = va;
    tb[ly * EV_H + lx] = vb;
  }
  __syncthreads();
  // squared error over the block's own pixels: exact, <= 32 * 32 * 4 * 255^2 < 2^32
  unsigned int se = 0;
  for (int i = t; i < bh * bw; i += EV_THREADS) {
    const int ly = i / bw, lx = i - ly * bw;
    const uint32_t va = ta[ly * EV_H + lx], vb = tb[ly * EV_H + lx];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int d = (int)((va >> (8 * c)) & 255u) - (int)((vb >> (8 * c)) & 255u);
      se += (unsigned int)(d * d);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  if (lane == 0) wsse[wv] = se;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double cov_norm = 49.0 / 48.0;
  for (int c = 0; c < C; ++c) {
    // horizontal 7-sums of every staged row at the block's window columns
    for (int i = t; i < th * nwx; i += EV_THREADS) {
      const int ly = i / nwx, wx = i - ly * nwx;
      int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        const int x = (int)((ta[ly * EV_H + wx + d] >> (8 * c)) & 255u);
        const int y = (int)((tb[ly * EV_H + wx + d] >> (8 * c)) & 255u);
        sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
      }
      hs[ly * EV_T + wx] = make_uint4((uint32_t)sx | ((uint32_t)sy << 16), (uint32_t)sxx, (uint32_t)syy,
                                      (uint32_t)sxy);
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = t; i < nwy * nwx; i += EV_THREADS) {
      const int wy = i / nwx, wx = i - wy * nwx;
      int vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        const uint4 q = hs[(wy + d) * EV_T + wx];
        vx += (int)(q.x & 0xFFFFu); vy += (int)(q.x >> 16);
        vxx += (int)q.y; vyy += (int)q.z; vxy += (int)q.w;
      }
      const double ux = vx / 49.0, uy = vy / 49.0;
      const double uxx = vxx / 49.0, uyy = vyy / 49.0, uxy = vxy / 49.0;
      const double sxv = cov_norm * (uxx - ux * ux);
      const double syv = cov_norm * (uyy - uy * uy);
      const double sxyv = cov_norm * (uxy - ux * uy);
      const double A1 = 2 * ux * uy + C1, A2 = 2 * sxyv + C2;
      const double B1 = ux * ux + uy * uy + C1, B2 = sxv + syv + C2;
      acc += (A1 * A2) / (B1 * B2);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) wsum[c][wv] = acc;
    __syncthreads();                                         // hs is rewritten by the next channel
  }
  if (t == 0) {
    EvPartial p;
    p.sse = 0;
    for (int u = 0; u < EV_THREADS / 64; ++u) p.sse += wsse[u];
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      if (c < C)
        for (int u = 0; u < EV_THREADS / 64; ++u) s += wsum[c][u];
      p.s[c] = s;
    }
    a.part[blockIdx.x] = p;
  }
}

// one wave per image: the lanes fetch 64 records at a time into LDS (one
// dependent global load per record made the adding thread the longer of the
// two kernels), lane 0 alone adds them, in block order
__global__ __launch_bounds__(64) void ev_final_kernel(EvArgs a, int c, double *__restrict__ psnr,
                                                      double *__restrict__ ssim) {
  __shared__ EvPartial sp[64];
  const int i = blockIdx.x, t = threadIdx.x;
  if (!rg_valid(a.tab[i], c, a.max_h, a.max_w, a.in_bytes)) {      // uniform, before any barrier
    if (t == 0) psnr[i] = ssim[i] = __builtin_nan("");
    return;
  }
  const int tiles = a.tiles_y * a.tiles_x;
  const EvPartial *p = a.part + (long long)i * tiles;
  unsigned long long sse = 0;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int u0 = 0; u0 < tiles; u0 += 64) {
    if (u0 + t < tiles) sp[t] = p[u0 + t];
    __syncthreads();
    if (t == 0) {
      const int m = tiles - u0 < 64 ? tiles - u0 : 64;
      for (int u = 0; u < m; ++u) {
        sse += sp[u].sse;
        for (int ch = 0; ch < c; ++ch) s[ch] += sp[u].s[ch];
      }
    }
    __syncthreads();
  }
  if (t != 0) return;
  const long long per = (long long)a.oh * a.ow * c;
  const double mse = (double)sse / (double)per;
  psnr[i] = mse == 0 ? __builtin_inf() : 10.0 * log10(255.0 * 255.0 / mse);
  double m = 0.0;
  for (int ch = 0; ch < c; ++ch) m += s[ch] / ((double)(a.oh - 6) * (a.ow - 6));
  ssim[i] = m / c;
}

// RR_OK, RR_EINVAL, or RR_EUNSUPPORTED (more than 2^31 - 1 workgroups)
static int ev_plan(int n, int c, int oh, int ow, int *tiles_y, int *tiles_x, size_t *total) {
  if (n <= 0 || c < 1 || c > 4 || oh < 7 || ow < 7) return RR_EINVAL;   // skimage: win_size > image side
  *tiles_y = (oh + EV_T - 1) / EV_T;
  *tiles_x = (ow + EV_T - 1) / EV_T;
  const long long groups = (long long)n * *tiles_y * *tiles_x;
  if (groups >= (1LL << 31)) return RR_EUNSUPPORTED;
  *total = (size_t)groups * sizeof(EvPartial);
  return RR_OK;
}

__global__ void ssim_chan_mean_kernel(int n, int C, const double *__restrict__ chan_mean,
                                      double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int c = 0; c < C; ++c) s += chan_mean[(long long)i * C + c];
  out[i] = s / C;
}

}  // namespace

extern "C" int rr_cv_resize_linear_u8(int n, int h, int w, int c, int oh, int ow,
                                      const uint8_t *in, uint8_t *out, int simd_lanes,
                                      rr_stream stream) {
  if (n < 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || c < 1 || c > 4) return RR_EINVAL;
  if (simd_lanes <= 0) simd_lanes = 16;
  if ((simd_lanes & 1) != 0) return RR_EINVAL;
  if (n == 0) return RR_OK;
  if (!in || !out) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (oh == h && ow == w) {                               // cv::resize: same size -> copy
    return rr_copy_bytes(out, in, (size_t)n * h * w * c, st);   // (a kernel: graph-safe, misc.hip)
  }
  // hal::resize: scale = 1 / inv_scale, inv_scale = dst / src (double)
  const double sxs = 1.0 / ((double)ow / (double)w), sys = 1.0 / ((double)oh / (double)h);
  const int ve = cvr_vec_end(ow, c, simd_lanes);
  const long long total = (long long)n * oh * ow;
  const dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
    hipLaunchKernelGGL(cv_resize_linear_kernel<decltype(cc)::value>, g, b, 0, st, n, h, w, oh, ow, sxs, sys,
                       ve, in, out);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

// the arguments rr_cv_resize_ragged_u8 and rr_eval_ragged_u8 share
static bool cvg_args_ok(int n, int c, int max_h, int max_w, int oh, int ow, const void *in, size_t in_bytes,
                        const void *images_dev, int *simd_lanes) {
  if (n <= 0 || c < 1 || c > 4 || max_h <= 0 || max_w <= 0 || oh <= 0 || ow <= 0) return false;
  if (!in || !images_dev || !rg_bytes_ok(in_bytes)) return false;
  if ((long long)oh * ow * c > INT32_MAX) return false;      // x * c + ch, the pixel index: int
  if (*simd_lanes <= 0) *simd_lanes = 16;
  return (*simd_lanes & 1) == 0;
}

extern "C" int rr_cv_resize_ragged_u8(int n, int c, int max_h, int max_w, int oh, int ow,
                                      const uint8_t *in, size_t in_bytes,
                                      const rr_ragged_image *images_dev, uint8_t *out, int simd_lanes,
                                      rr_stream stream) {
  if (!out || !cvg_args_ok(n, c, max_h, max_w, oh, ow, in, in_bytes, images_dev, &simd_lanes)) return RR_EINVAL;
  const long long per = (long long)CVG_T * CVG_PER;
  const long long chunks = ((long long)oh * ow + per - 1) / per;
  if (chunks * n >= (1LL << 31)) return RR_EUNSUPPORTED;
  const int ve = cvr_vec_end(ow, c, simd_lanes);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
    hipLaunchKernelGGL(cv_resize_ragged_kernel<decltype(cc)::value>, dim3((unsigned)(chunks * n)), dim3(CVG_T),
                       0, st, max_h, max_w, oh, ow, (int)chunks, ve, (long long)in_bytes, in, images_dev, out);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" size_t rr_eval_ragged_workspace(int n, int c, int oh, int ow) {
  int ty, tx;
  size_t total;
  return ev_plan(n, c, oh, ow, &ty, &tx, &total) == RR_OK ? total : 0;
}

extern "C" int rr_eval_ragged_u8(int n, int c, int max_h, int max_w, int oh, int ow, const uint8_t *clean,
                                 size_t clean_bytes, const rr_ragged_image *images_dev,
                                 const uint8_t *restored, double *psnr, double *ssim, int simd_lanes,
                                 void *ws, size_t ws_bytes, rr_stream stream) {
  if (!restored || !psnr || !ssim || !ws || ((uintptr_t)ws & 7) != 0) return RR_EINVAL;
  if (!cvg_args_ok(n, c, max_h, max_w, oh, ow, clean, clean_bytes, images_dev, &simd_lanes)) return RR_EINVAL;
  EvArgs a{n, max_h, max_w, oh, ow, 0, 0, 0, (long long)clean_bytes, clean, images_dev, restored,
           (EvPartial *)ws};
  size_t total;
  if (const int rc = ev_plan(n, c, oh, ow, &a.tiles_y, &a.tiles_x, &total)) return rc;
  if (ws_bytes < total) return RR_EWORKSPACE;
  a.vec_end = cvr_vec_end(ow, c, simd_lanes);
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)((long long)n * a.tiles_y * a.tiles_x)), b(EV_THREADS);
  const int rc = rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
    hipLaunchKernelGGL(ev_tile_kernel<decltype(cc)::value>, g, b, 0, st, a);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(ev_final_kernel, dim3(n), dim3(64), 0, st, a, c, psnr, ssim);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" size_t rr_ssim_workspace(int n, int c) {
  return n > 0 && c > 0 ? (size_t)n * c * sizeof(double) : 0;
}

extern "C" int rr_ssim_u8(int n, int h, int w, int c, const uint8_t *a, const uint8_t *b, double *out,
                          void *ws, size_t ws_bytes, rr_stream stream) {
  if (!a || !b || !out || !ws || n <= 0 || c <= 0) return RR_EINVAL;
  if (h < 7 || w < 7) return RR_EINVAL;                     // skimage: win_size > image side
  if (ws_bytes < rr_ssim_workspace(n, c)) return RR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  double *cm = (double *)ws;
  hipLaunchKernelGGL(ssim_kernel, dim3(n * c), dim3(SS_T), 0, st, h, w, c, a, b, cm);
  RR_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_chan_mean_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, c, cm, out);
  RR_CHECK_LAUNCH();
  return RR_OK;
}
