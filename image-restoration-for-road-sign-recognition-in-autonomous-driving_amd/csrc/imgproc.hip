// imgproc.hip -- the image I/O either side of the networks (SURVEY §8f rows 2
// and 4), on device:
//
//   * rr_resize_bilinear_u8: torchvision Resize((oh, ow)) on a PIL image, i.e.
//     PIL Image.resize(BILINEAR) (17:66, 18:28-32), bit-exact: PIL's separable
//     two-pass resample with antialiasing support (filter support scaled by
//     the downscale factor), coefficients normalised in double and rounded to
//     22-bit fixed point, an 8-bit clip after each pass.  Optionally fused with
//     ToTensor (x / 255 in fp32) and Normalize ((x - mean) / std in fp32, 18:31)
//     into an NCHW fp32 batch.
//   * rr_resize_ragged_u8: the same resample for n images of unequal size in
//     one buffer (the reference resizes each GTSRB image on its own, 05:24-29,
//     17:66, 18:28-32): two launches for any n, the intermediate image in LDS.
//   * rr_cv_resize_linear_u8: cv2.resize(img, (ow, oh)) INTER_LINEAR, the
//     clean side of the 08 PSNR leg (08:118-119) -- OpenCV's own fixed-point
//     bilinear (resize.cpp resizeGeneric_ + HResizeLinear / VResizeLinear),
//     not Pillow's: 11-bit weights from float source coordinates, an exact
//     int32 horizontal pass, the vertical pass as the x86 SIMD body computes
//     it (VResizeLinearVec_32s8u) with the scalar 22-bit rounding on the row
//     tail; bit-equal to oracle/imgproc_cpu.cv_resize_linear (parity vs cv2
//     itself unpinned: cv2 is not installed).
//   * rr_cv_resize_ragged_u8: the same for n images of unequal size in one
//     buffer (every clean GTSRB original of the 08 loop has its own size), one
//     launch, the scale taken per image on the device.
//   * rr_eval_ragged_u8: PSNR and SSIM (08:123-125) of those resized clean
//     images against a dense restored batch in two launches; the resized clean
//     image lives in LDS tiles only.
//   * rr_ssim_u8: skimage structural_similarity(a, b, data_range=255,
//     channel_axis=2) (08:125): 7x7 uniform window, sample covariance
//     (49/48), K1 = .01, K2 = .03, mean of S over the interior (3-pixel border
//     cropped), mean over channels, fp64.
//
// Both are HBM-bound byte work: no MFMA, one thread per output pixel (resize)
// or per output column (SSIM), coalesced along the innermost NHWC axis.
#include "common.h"
#include "philox.h"

#include <cmath>

namespace {

// ---------------------------------------------------------------- resize ----
constexpr int RS_PREC = 22;        // PIL PRECISION_BITS = 32 - 8 - 2
constexpr int RS_MAXK = 255;       // taps per output (downscale up to 127x)

struct RsAxis {
  int in_size, out_size, ksize;
  int *bounds;                     // [out][2]: first tap, tap count
  int *kk;                         // [out][ksize] fixed-point coefficients
};

// PIL precompute_coeffs + normalize_coeffs_8bpc (Resample.c), evaluated in
// the same double operations in the same order; contraction into FMA would
// change the rounding, so it is off for this function.
__device__ void rs_coeffs_one(const RsAxis &ax, int xx) {
#pragma clang fp contract(off)
  const double scale = (double)ax.in_size / ax.out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;                  // bilinear support 1.0
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > ax.in_size) xmax = ax.in_size;
  xmax -= xmin;
  // the filter value of tap x (evaluated twice: sum first, then normalise --
  // the same doubles both times, and no private array in scratch)
  auto tap = [&](int x) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    t = t < 0.0 ? -t : t;
    return t < 1.0 ? 1.0 - t : 0.0;
  };
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += tap(x);
  int *o = ax.kk + (long long)xx * ax.ksize;
  for (int x = 0; x < ax.ksize; ++x) {
    double v = 0.0;
    if (x < xmax) v = ww != 0.0 ? tap(x) / ww : tap(x);
    o[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << RS_PREC)) : (int)(0.5 + v * (double)(1 << RS_PREC));
  }
  ax.bounds[2 * xx] = xmin;
  ax.bounds[2 * xx + 1] = xmax;
}

__global__ void rs_coeffs_kernel(RsAxis h, RsAxis v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < h.out_size) rs_coeffs_one(h, i);
  else if (i < h.out_size + v.out_size) rs_coeffs_one(v, i - h.out_size);
}

__device__ __forceinline__ int rs_clip8(int s) {          // PIL clip8: lookups[s >> 22]
  const int v = s >> RS_PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one output sample of a pass: the rounded fixed-point sum of cnt taps of C
// interleaved channels, src advancing by stride bytes per tap (C for the
// horizontal pass, a row of the intermediate for the vertical one)
template <int C, typename Stride>
__device__ __forceinline__ void rs_tap_sum(const uint8_t *__restrict__ src, Stride stride,
                                           const int *__restrict__ k, int cnt, int (&s)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = 1 << (RS_PREC - 1);
  for (int x = 0; x < cnt; ++x) {
    const int kx = k[x];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] += (int)src[x * stride + c] * kx;
  }
}

struct RsNorm { float mean[4], std[4]; };

// the vertical pass's store of output pixel (img, oy, ox): u8 NHWC (MODE 0) or
// fp32 NCHW ToTensor (+ Normalize) (MODE 1)
template <int C, int MODE>
__device__ __forceinline__ void rs_emit(const int (&s)[C], void *__restrict__ out, int img, int oy,
                                        int ox, int oh, int ow, const RsNorm &nm, int normalize) {
  if constexpr (MODE == 0) {
    uint8_t *dst = (uint8_t *)out + (((long long)img * oh + oy) * ow + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = (uint8_t)rs_clip8(s[c]);
  } else {
    float *dst = (float *)out;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v = (float)rs_clip8(s[c]) / 255.0f;                 // ToTensor: .div(255)
      if (normalize) v = (v - nm.mean[c]) / nm.std[c];          // Normalize: sub_, div_
      dst[(((long long)img * C + c) * oh + oy) * ow + ox] = v;
    }
  }
}

// horizontal pass over source rows [y_first, y_first + rows): [n][h][w][C] ->
// tmp [n][rows][ow][C]
template <int C>
__global__ void rs_horiz_kernel(int n, int h, int w, int ow, int y_first, int rows, int ksize,
                                const int *__restrict__ bounds, const int *__restrict__ kk,
                                const uint8_t *__restrict__ in, uint8_t *__restrict__ tmp) {
  const long long total = (long long)n * rows * ow;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    const long long r = i / ow;                    // n * rows + row
    const int img = (int)(r / rows), y = (int)(r % rows) + y_first;
    const int xmin = bounds[2 * ox], xcnt = bounds[2 * ox + 1];
    int s[C];
    rs_tap_sum<C>(in + (((long long)img * h + y) * w + xmin) * C, C, kk + (long long)ox * ksize, xcnt, s);
    uint8_t *dst = tmp + i * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = (uint8_t)rs_clip8(s[c]);
  }
}

// vertical pass: tmp [n][rows][ow][C] -> u8 [n][oh][ow][C] (MODE 0) or fp32
// NCHW ToTensor (+ Normalize) (MODE 1)
template <int C, int MODE>
__global__ void rs_vert_kernel(int n, int rows, int oh, int ow, int ksize, int y_first,
                               const int *__restrict__ bounds, const int *__restrict__ kk,
                               const uint8_t *__restrict__ tmp, void *__restrict__ out, RsNorm nm,
                               int normalize) {
  const long long total = (long long)n * oh * ow;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    const long long r = i / ow;
    const int img = (int)(r / oh), oy = (int)(r % oh);
    const int ymin = bounds[2 * oy] - y_first, ycnt = bounds[2 * oy + 1];
    int s[C];
    rs_tap_sum<C>(tmp + (((long long)img * rows + ymin) * ow + ox) * C, (long long)ow * C,
                  kk + (long long)oy * ksize, ycnt, s);
    rs_emit<C, MODE>(s, out, img, oy, ox, oh, ow, nm, normalize);
  }
}

// same-size "resize": Pillow returns a copy of the image (Image.resize with
// size == self.size), so the passes reduce to the copy / ToTensor (+
// Normalize) of the input -- one pass instead of horiz + vert + coefficients
template <int C, int MODE>
__global__ void rs_same_kernel(long long npix, int hw, const uint8_t *__restrict__ in,
                               void *__restrict__ out, RsNorm nm, int normalize) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < npix;
       i += (long long)gridDim.x * blockDim.x) {
    const uint8_t *src = in + i * C;
    if constexpr (MODE == 0) {
      uint8_t *dst = (uint8_t *)out + i * C;
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c] = src[c];
    } else {
      const long long img = i / hw, px = i - img * hw;
      float *dst = (float *)out;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float v = (float)src[c] / 255.0f;                           // ToTensor: .div(255)
        if (normalize) v = (v - nm.mean[c]) / nm.std[c];          // Normalize: sub_, div_
        dst[(img * C + c) * hw + px] = v;
      }
    }
  }
}

struct RsPlan {
  int kh, kv, y_first, rows;
  size_t off_bh, off_kh, off_bv, off_kv, off_tmp, total;
};

// host mirror of the bound computation for the rows the vertical pass reads
// (PIL ybox_first / ybox_last); same double expressions as rs_coeffs_one
static void rs_vbox(int in_size, int out_size, int *first, int *last) {
  const double scale = (double)in_size / out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  auto lo = [&](int yy) {
    const double c = 0.0 + (yy + 0.5) * scale;
    int a = (int)(c - support + 0.5);
    return a < 0 ? 0 : a;
  };
  auto hi = [&](int yy) {
    const double c = 0.0 + (yy + 0.5) * scale;
    int b = (int)(c + support + 0.5);
    return b > in_size ? in_size : b;
  };
  *first = lo(0);
  *last = hi(out_size - 1);   // bounds[last] start + count = clamped xmax
}

static int rs_ksize(int in_size, int out_size) {
  const double scale = (double)in_size / out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(support) * 2 + 1;
}

static bool rs_plan(int n, int h, int w, int c, int oh, int ow, RsPlan *p) {
  if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || c < 1 || c > 4) return false;
  p->kh = rs_ksize(w, ow);
  p->kv = rs_ksize(h, oh);
  if (p->kh > RS_MAXK || p->kv > RS_MAXK) return false;
  int f, l;
  rs_vbox(h, oh, &f, &l);
  p->y_first = f;
  p->rows = l - f;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  p->off_bh = o; o = al(o + (size_t)ow * 2 * 4);
  p->off_kh = o; o = al(o + (size_t)ow * p->kh * 4);
  p->off_bv = o; o = al(o + (size_t)oh * 2 * 4);
  p->off_kv = o; o = al(o + (size_t)oh * p->kv * 4);
  p->off_tmp = o; o = al(o + (size_t)n * p->rows * ow * c);
  p->total = o;
  return true;
}

// --------------------------------------------------------- ragged resize ----
// The same two passes for n images of unequal size lying in one byte buffer
// (rr_resize_ragged_u8): two launches whatever n is, and no per-image work on
// the host.
//   1. rg_coeffs_kernel: rs_coeffs_one for every (image, axis, output index),
//      each image's tables at a fixed stride in the workspace.  The stride is
//      that of the largest admissible image (max_h x max_w): rs_ksize grows
//      with the input size, and rs_coeffs_one zero-fills the taps past an
//      image's own count.
//   2. rg_resample_kernel: one workgroup per (image, band of output rows).
//      It runs the horizontal pass over the source rows the band's vertical
//      taps cover into an LDS tile [rows][ow][C] of uint8 (PIL's clipped
//      intermediate image), then the vertical pass out of that tile: the
//      intermediate never reaches HBM.
// Both kernels test every table record with rg_valid before they touch the
// image: a record outside [1, max_h] x [1, max_w] or outside the buffer reads
// nothing and its output is zeros.
constexpr int RG_T = 256;
constexpr int RG_BAND_MAX = 16;            // output rows per workgroup, at most
constexpr int RG_MIN_GROUPS = 512;         // bands shrink (down to 4 rows) to launch this many
constexpr size_t RG_LDS_PREF = 32u << 10;  // tile bytes the band height is sized for
constexpr size_t RG_LDS_MAX = 64u << 10;   // tile bytes a one-row band may take

struct RgArgs {
  int n, max_h, max_w, oh, ow, kh, kv, band, tile_rows;
  long long in_bytes;
  const uint8_t *in;
  const rr_ragged_image *tab;
  char *ws;
  size_t per_image, off_bh, off_kh, off_bv, off_kv;
};

__host__ __device__ inline bool rg_valid(const rr_ragged_image &r, int c, int max_h, int max_w,
                                         long long in_bytes) {
  if (r.h < 1 || r.h > max_h || r.w < 1 || r.w > max_w) return false;
  if (r.offset < 0 || r.offset > in_bytes) return false;
  return (long long)r.h * r.w <= (in_bytes - r.offset) / c;
}

__global__ void rg_coeffs_kernel(RgArgs a, int c) {
  const int per = a.ow + a.oh;
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)a.n * per) return;
  const int img = (int)(i / per), j = (int)(i % per);
  const rr_ragged_image r = a.tab[img];
  if (!rg_valid(r, c, a.max_h, a.max_w, a.in_bytes)) return;
  char *base = a.ws + (size_t)img * a.per_image;
  if (j < a.ow)
    rs_coeffs_one(RsAxis{r.w, a.ow, a.kh, (int *)(base + a.off_bh), (int *)(base + a.off_kh)}, j);
  else
    rs_coeffs_one(RsAxis{r.h, a.oh, a.kv, (int *)(base + a.off_bv), (int *)(base + a.off_kv)}, j - a.ow);
}

template <int C, int MODE>
__global__ __launch_bounds__(RG_T) void rg_resample_kernel(RgArgs a, void *__restrict__ out, RsNorm nm,
                                                           int normalize) {
  extern __shared__ uint8_t rg_tile[];                       // [rows][ow][C]
  const int bands = (a.oh + a.band - 1) / a.band;
  const int img = blockIdx.x / bands, oy0 = (blockIdx.x % bands) * a.band;
  const int nb = a.oh - oy0 < a.band ? a.oh - oy0 : a.band;
  const rr_ragged_image r = a.tab[img];
  const char *base = a.ws + (size_t)img * a.per_image;
  const int *bh = (const int *)(base + a.off_bh), *kh = (const int *)(base + a.off_kh);
  const int *bv = (const int *)(base + a.off_bv), *kv = (const int *)(base + a.off_kv);
  // all of this is uniform over the workgroup, so is the early return
  bool ok = rg_valid(r, C, a.max_h, a.max_w, a.in_bytes);
  int y0 = 0, rows = 0;
  if (ok) {
    const int last = oy0 + nb - 1;
    y0 = bv[2 * oy0];
    rows = bv[2 * last] + bv[2 * last + 1] - y0;
    ok = y0 >= 0 && rows >= 0 && rows <= a.tile_rows && y0 + rows <= r.h;
  }
  if (!ok) {
    for (int i = threadIdx.x; i < nb * a.ow; i += RG_T) {
      const int ly = i / a.ow, ox = i - ly * a.ow, oy = oy0 + ly;
      if constexpr (MODE == 0) {
        uint8_t *dst = (uint8_t *)out + (((long long)img * a.oh + oy) * a.ow + ox) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = 0;
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) ((float *)out)[(((long long)img * C + c) * a.oh + oy) * a.ow + ox] = 0.f;
      }
    }
    return;
  }
  const uint8_t *src = a.in + r.offset + (long long)y0 * r.w * C;
  for (int i = threadIdx.x; i < rows * a.ow; i += RG_T) {
    const int ry = i / a.ow, ox = i - ry * a.ow;
    const int xmin = bh[2 * ox], xcnt = bh[2 * ox + 1];
    int s[C];
    rs_tap_sum<C>(src + ((long long)ry * r.w + xmin) * C, C, kh + (long long)ox * a.kh, xcnt, s);
#pragma unroll
    for (int c = 0; c < C; ++c) rg_tile[i * C + c] = (uint8_t)rs_clip8(s[c]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nb * a.ow; i += RG_T) {
    const int ly = i / a.ow, ox = i - ly * a.ow, oy = oy0 + ly;
    const int ymin = bv[2 * oy] - y0, ycnt = bv[2 * oy + 1];
    int s[C];
    rs_tap_sum<C>(rg_tile + (ymin * a.ow + ox) * C, a.ow * C, kv + (long long)oy * a.kv, ycnt, s);
    rs_emit<C, MODE>(s, out, img, oy, ox, a.oh, a.ow, nm, normalize);
  }
}

struct RgPlan {
  int kh, kv, band, tile_rows;
  size_t lds, per_image, off_bh, off_kh, off_bv, off_kv, total;
};

// source rows a band of `band` output rows can cover, for any image up to
// max_h rows: last tap - first tap <= (band - 1) * scale + 2 * support + 1
// (rs_coeffs_one's xmin / xmax, one truncation each way), and both scale and
// support grow with the image's height
static long long rg_tile_rows(int max_h, int oh, int band) {
  const double scale = (double)max_h / oh;
  const double support = scale < 1.0 ? 1.0 : scale;
  const long long rows = (long long)((band - 1) * scale + 2.0 * support + 1.0) + 1;
  return rows < max_h ? rows : max_h;
}

// RR_OK, RR_EINVAL (arguments) or RR_EUNSUPPORTED (more than RS_MAXK taps, or
// a one-row band's tile larger than RG_LDS_MAX)
static int rg_plan(int n, int c, int max_h, int max_w, int oh, int ow, RgPlan *p) {
  if (n <= 0 || max_h <= 0 || max_w <= 0 || oh <= 0 || ow <= 0 || c < 1 || c > 4) return RR_EINVAL;
  // rs_ksize's ceil(scale) * 2 + 1 <= RS_MAXK, without its int overflowing
  if ((max_w - 1) / ow >= RS_MAXK / 2 || (max_h - 1) / oh >= RS_MAXK / 2) return RR_EUNSUPPORTED;
  p->kh = rs_ksize(max_w, ow);
  p->kv = rs_ksize(max_h, oh);
  if (p->kh > RS_MAXK || p->kv > RS_MAXK) return RR_EUNSUPPORTED;
  if ((long long)n * ((long long)oh + ow) > (1LL << 31)) return RR_EUNSUPPORTED;   // grid sizes
  auto tile = [&](int band) { return (size_t)rg_tile_rows(max_h, oh, band) * ow * c; };
  if ((size_t)ow * c > RG_LDS_MAX) return RR_EUNSUPPORTED;
  int band = oh < RG_BAND_MAX ? oh : RG_BAND_MAX;
  while (band > 1 && tile(band) > RG_LDS_PREF) --band;
  if (tile(band) > RG_LDS_MAX) return RR_EUNSUPPORTED;
  while (band > 4 && (long long)n * ((oh + band - 1) / band) < RG_MIN_GROUPS) band = (band + 1) / 2;
  p->band = band;
  p->tile_rows = (int)rg_tile_rows(max_h, oh, band);
  p->lds = tile(band);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t o = 0;
  p->off_bh = o; o = al(o + (size_t)ow * 2 * 4);
  p->off_kh = o; o = al(o + (size_t)ow * p->kh * 4);
  p->off_bv = o; o = al(o + (size_t)oh * 2 * 4);
  p->off_kv = o; o = al(o + (size_t)oh * p->kv * 4);
  p->per_image = o;
  p->total = o * (size_t)n;
  return RR_OK;
}

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
//      is ssim_kernel's fp64 expression; the block's S is summed per channel
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

int rr_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t st);   // misc.hip

extern "C" size_t rr_resize_workspace(int n, int h, int w, int c, int oh, int ow) {
  RsPlan p;
  return rs_plan(n, h, w, c, oh, ow, &p) ? p.total : 0;
}

extern "C" int rr_resize_bilinear_u8(int n, int h, int w, int c, int oh, int ow, const uint8_t *in,
                                     int out_kind, const float *mean, const float *std, void *out,
                                     void *ws, size_t ws_bytes, rr_stream stream) {
  RsPlan p;
  if (!in || !out || !ws || (out_kind != 0 && out_kind != 1)) return RR_EINVAL;
  if (!rs_plan(n, h, w, c, oh, ow, &p)) return RR_EUNSUPPORTED;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  if ((mean == nullptr) != (std == nullptr) || (mean && out_kind != 1)) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (oh == h && ow == w) {
    RsNorm nm{};
    for (int i = 0; i < c; ++i) {
      nm.mean[i] = mean ? mean[i] : 0.f;
      nm.std[i] = std ? std[i] : 1.f;
    }
    const long long np = (long long)n * h * w;
    const dim3 g(rr_grid_cap((np + 255) / 256, 8192)), b(256);
    return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
      constexpr int CC = decltype(cc)::value;
      if (out_kind == 0) hipLaunchKernelGGL((rs_same_kernel<CC, 0>), g, b, 0, st, np, h * w, in, out, nm, 0);
      else hipLaunchKernelGGL((rs_same_kernel<CC, 1>), g, b, 0, st, np, h * w, in, out, nm, mean != nullptr);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  }
  char *base = (char *)ws;
  RsAxis ah{w, ow, p.kh, (int *)(base + p.off_bh), (int *)(base + p.off_kh)};
  RsAxis av{h, oh, p.kv, (int *)(base + p.off_bv), (int *)(base + p.off_kv)};
  hipLaunchKernelGGL(rs_coeffs_kernel, dim3((ow + oh + 63) / 64), dim3(64), 0, st, ah, av);
  RR_CHECK_LAUNCH();
  uint8_t *tmp = (uint8_t *)(base + p.off_tmp);
  const long long th = (long long)n * p.rows * ow, tv = (long long)n * oh * ow;
  const dim3 gh(rr_grid_cap((th + 255) / 256, 8192)), gv(rr_grid_cap((tv + 255) / 256, 8192)), b(256);
  RsNorm nm{};
  for (int i = 0; i < c; ++i) {
    nm.mean[i] = mean ? mean[i] : 0.f;
    nm.std[i] = std ? std[i] : 1.f;
  }
  const int norm = mean != nullptr;
  return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    hipLaunchKernelGGL(rs_horiz_kernel<CC>, gh, b, 0, st, n, h, w, ow, p.y_first, p.rows, p.kh, ah.bounds,
                       ah.kk, in, tmp);
    if (out_kind == 0)
      hipLaunchKernelGGL((rs_vert_kernel<CC, 0>), gv, b, 0, st, n, p.rows, oh, ow, p.kv, p.y_first,
                         av.bounds, av.kk, tmp, out, nm, norm);
    else
      hipLaunchKernelGGL((rs_vert_kernel<CC, 1>), gv, b, 0, st, n, p.rows, oh, ow, p.kv, p.y_first,
                         av.bounds, av.kk, tmp, out, nm, norm);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_ragged_check(int n, int c, size_t in_bytes, const rr_ragged_image *images_host,
                               int max_h, int max_w, int oh, int ow) {
  if (!images_host || n <= 0 || max_h <= 0 || max_w <= 0 || oh <= 0 || ow <= 0 || c < 1 || c > 4)
    return RR_EINVAL;
  if ((max_w - 1) / ow >= RS_MAXK / 2 || (max_h - 1) / oh >= RS_MAXK / 2) return RR_EUNSUPPORTED;
  if (in_bytes > (size_t)INT64_MAX) return RR_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!rg_valid(images_host[i], c, max_h, max_w, (long long)in_bytes)) return RR_EINVAL;
  return RR_OK;
}

extern "C" size_t rr_resize_ragged_workspace(int n, int c, int max_h, int max_w, int oh, int ow) {
  RgPlan p;
  return rg_plan(n, c, max_h, max_w, oh, ow, &p) == RR_OK ? p.total : 0;
}

extern "C" int rr_resize_ragged_u8(int n, int c, int max_h, int max_w, int oh, int ow,
                                   const uint8_t *in, size_t in_bytes,
                                   const rr_ragged_image *images_dev, int out_kind, const float *mean,
                                   const float *std, void *out, void *ws, size_t ws_bytes,
                                   rr_stream stream) {
  RgPlan p;
  if (!in || !images_dev || !out || !ws || (out_kind != 0 && out_kind != 1)) return RR_EINVAL;
  if (in_bytes == 0 || in_bytes > (size_t)INT64_MAX) return RR_EINVAL;
  if (const int rc = rg_plan(n, c, max_h, max_w, oh, ow, &p)) return rc;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  if ((mean == nullptr) != (std == nullptr) || (mean && out_kind != 1)) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const RgArgs a{n, max_h, max_w, oh, ow, p.kh, p.kv, p.band, p.tile_rows, (long long)in_bytes,
                 in, images_dev, (char *)ws, p.per_image, p.off_bh, p.off_kh, p.off_bv, p.off_kv};
  const long long nco = (long long)n * (ow + oh);
  hipLaunchKernelGGL(rg_coeffs_kernel, dim3((unsigned)((nco + 63) / 64)), dim3(64), 0, st, a, c);
  RR_CHECK_LAUNCH();
  RsNorm nm{};
  for (int i = 0; i < c; ++i) {
    nm.mean[i] = mean ? mean[i] : 0.f;
    nm.std[i] = std ? std[i] : 1.f;
  }
  const int norm = mean != nullptr;
  const dim3 g((unsigned)((long long)n * ((oh + p.band - 1) / p.band))), b(RG_T);
  return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
    constexpr int CC = decltype(cc)::value;
    if (out_kind == 0) hipLaunchKernelGGL((rg_resample_kernel<CC, 0>), g, b, p.lds, st, a, out, nm, norm);
    else hipLaunchKernelGGL((rg_resample_kernel<CC, 1>), g, b, p.lds, st, a, out, nm, norm);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

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
  if (!in || !images_dev || in_bytes == 0 || in_bytes > (size_t)INT64_MAX) return false;
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

// ------------------------------------------------------------ distortion ----
// The dynamic distortion generator 14:31-64 (fog -> noise -> motion blur, each
// drawn per image) and the fixed compound variant 16:14-37 (blur -> fog ->
// noise), per image on device, with the reference's numpy dtype semantics:
//   img / 255 in fp32; fog out * f32(t) + f32(A (1 - t)) in fp32; noise added
//   in fp64 (np.random.normal is float64, so the image becomes float64);
//   clip(x * 255, 0, 255).astype(uint8) truncates; cv2.filter2D on uint8 with
//   the fp32-converted kernel: fp32 sum over the taps in row-major order,
//   BORDER_REFLECT_101, anchor (k / 2, k / 2), round half to even, saturate.
// Noise: the caller's fp64 field (parity runs) or Philox4x32-10 normals
// (Box-Muller in fp64) keyed by (seed, element index).

struct DistCfg {
  int n, h, w, c, mode;                 // mode 0: 14:31-64 order, 1: 16:14-37 order
  const uint8_t *in;
  uint8_t *out, *tmp;
  const rr_distort_param *prm;
  const float *taps;                    // [n][RR_DISTORT_KMAX^2], row-major
  const double *noise;                  // [n][h][w][c] or null -> Philox
  unsigned long long seed;
  const int *tap_idx;                   // null, or [n]: image i's taps are taps + tap_idx[i] * KMAX^2
  const unsigned long long *seed_dev;   // null, or the Philox seed in device memory
};

__device__ __forceinline__ unsigned long long dist_seed(const DistCfg &a) {
  return a.seed_dev ? *a.seed_dev : a.seed;
}

// standard normal for element e (Philox4x32-10, two 24-bit uniforms,
// Box-Muller in fp32: np.random.normal's stream cannot be reproduced anyway,
// and the fp32 transcendentals cost a fraction of the fp64 library ones --
// the noise feeds an fp64 add and a uint8 truncation; |z| <= 5.8)
__device__ double philox_normal(unsigned long long seed, unsigned long long e) {
  uint32_t c0 = (uint32_t)e, c1 = (uint32_t)(e >> 32), c2 = 0x9E3779B9u, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const float u1 = (float)((c0 >> 8) + 1) * 0x1p-24f;          // (0, 1]
  const float u2 = (float)(c2 >> 8) * 0x1p-24f;                // [0, 1)
  return (double)(sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958648f * u2));
}

__device__ __forceinline__ uint8_t trunc_u8(double v) {    // np.clip(v, 0, 255).astype(uint8)
  v = v < 0.0 ? 0.0 : (v > 255.0 ? 255.0 : v);
  return (uint8_t)(int)v;
}
__device__ __forceinline__ uint8_t trunc_u8f(float v) {
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (uint8_t)(int)v;
}

// fog then noise on x = img / 255 (fp32); returns clip(x * 255).astype(u8)
// in the dtype the reference holds at that point
__device__ __forceinline__ uint8_t fog_noise(const DistCfg &a, const rr_distort_param &p, float x,
                                             long long e) {
#pragma clang fp contract(off)
  if (p.flags & RR_DISTORT_FOG) x = x * p.fog_mul + p.fog_add;
  if (p.flags & RR_DISTORT_NOISE) {
    const double nz = a.noise ? a.noise[e] : p.sigma * philox_normal(dist_seed(a), (unsigned long long)e);
    return trunc_u8(((double)x + nz) * 255.0);
  }
  return trunc_u8f(x * 255.f);
}

__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// stage 1 (per element): mode 0: fog/noise -> u8 (the blur input, or the
// output if no blur); mode 1: (img / 255 * 255).astype(u8), the blur input
__global__ void distort_pre_kernel(DistCfg a) {
#pragma clang fp contract(off)
  const long long per = (long long)a.h * a.w * a.c, total = per * a.n;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int img = (int)(e / per);
    const rr_distort_param p = a.prm[img];
    const float x = (float)a.in[e] / 255.0f;
    const bool blur = p.flags & RR_DISTORT_BLUR;
    uint8_t v;
    if (a.mode == 0) v = fog_noise(a, p, x, e);
    else v = trunc_u8f(x * 255.f);
    if (blur) a.tmp[e] = v;
    else if (a.mode == 0) a.out[e] = v;
    else a.out[e] = fog_noise(a, p, (float)v / 255.0f, e);
  }
}

// stage 2 (blurred images only): filter2D of tmp, then mode 0: the u8 result
// ((t / 255) * 255 truncated), mode 1: fog + noise on it.  The pixel's a.c
// bytes go to dst; e0 is its first element's noise index (the dense batch:
// the same number as its place in out; a ragged batch: elem_base order)
__device__ __forceinline__ void blur_store(const DistCfg &a, const rr_distort_param &p, long long e0,
                                           uint8_t *dst, const float *s) {
#pragma clang fp contract(off)
  for (int c = 0; c < a.c; ++c) {
    float r = rintf(s[c]);                                   // saturate_cast<uchar>: cvRound
    r = r < 0.f ? 0.f : (r > 255.f ? 255.f : r);
    const float t = (float)(int)r / 255.0f;
    dst[c] = a.mode == 0 ? trunc_u8f(t * 255.f) : fog_noise(a, p, t, e0 + c);
  }
}

__global__ void distort_blur_kernel(DistCfg a) {
#pragma clang fp contract(off)
  const long long hw = (long long)a.h * a.w, total = hw * a.n;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total;
       q += (long long)gridDim.x * blockDim.x) {
    const int img = (int)(q / hw);
    const rr_distort_param p = a.prm[img];
    if (!(p.flags & RR_DISTORT_BLUR)) continue;
    const int rem = (int)(q - (long long)img * hw), y = rem / a.w, x = rem % a.w;
    const int k = p.ksize, anc = k / 2;
    const float *kt = a.taps + (long long)(a.tap_idx ? a.tap_idx[img] : img) * RR_DISTORT_KMAX * RR_DISTORT_KMAX;
    const uint8_t *src = a.tmp + (long long)img * hw * a.c;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < k; ++i) {
      const int yy = reflect101(y + i - anc, a.h);
      for (int j = 0; j < k; ++j) {
        const float kv = kt[i * RR_DISTORT_KMAX + j];
        if (kv == 0.f) continue;                             // cv2 drops zero taps
        const int xx = reflect101(x + j - anc, a.w);
        const uint8_t *px = src + ((long long)yy * a.w + xx) * a.c;
        for (int c = 0; c < a.c; ++c) s[c] = s[c] + kv * (float)px[c];
      }
    }
    blur_store(a, p, q * a.c, a.out + q * a.c, s);
  }
}

// the same with the image's nonzero taps compacted into LDS first (row-major,
// so the sums run in the same order: bit-identical) -- for h * w a multiple
// of 256, where a workgroup's 256 pixels always belong to one image: the
// per-pixel loop then visits the ~k..2k nonzero taps of the rotated line
// kernel instead of testing all k * k, with no per-tap global loads
//
// The source rows the 256 pixels read (their row span + k - 1, reflect-101
// applied at staging, columns -anc .. w - 1 + k - 1 - anc) are staged in LDS
// when they fit: the tap loop then reads bytes at (row, x + j) with no
// reflection and no global load (same values, same order: bit-identical)
#define RR_BLUR_LDS 24576
__global__ __launch_bounds__(256) void distort_blur_tiled_kernel(DistCfg a) {
#pragma clang fp contract(off)
  __shared__ float tv[RR_DISTORT_KMAX * RR_DISTORT_KMAX];
  __shared__ int ti[RR_DISTORT_KMAX * RR_DISTORT_KMAX];
  __shared__ int wcount[4];
  __shared__ uint8_t simg[RR_BLUR_LDS];
  const long long hw = (long long)a.h * a.w, total = hw * a.n;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (long long q0 = blockIdx.x * 256LL; q0 < total; q0 += (long long)gridDim.x * 256) {
    const int img = (int)(q0 / hw);                          // uniform: 256 | hw
    const rr_distort_param p = a.prm[img];
    if (!(p.flags & RR_DISTORT_BLUR)) continue;              // uniform
    const int k = p.ksize, anc = k / 2;
    const float *kt = a.taps + (long long)(a.tap_idx ? a.tap_idx[img] : img) * RR_DISTORT_KMAX * RR_DISTORT_KMAX;
    const int i = t / (k > 0 ? k : 1), j = t - i * (k > 0 ? k : 1);
    const float kv = t < k * k ? kt[i * RR_DISTORT_KMAX + j] : 0.f;
    const bool nz = kv != 0.f;                               // cv2 drops zero taps
    const unsigned long long m = __ballot(nz);
    const int pos = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                         // the previous image's list is read
    if (lane == 0) wcount[wv] = __popcll(m);
    const uint8_t *src = a.tmp + (long long)img * hw * a.c;
    const int rem0 = (int)(q0 - (long long)img * hw);
    const int ya = rem0 / a.w, yb = (rem0 + 255) / a.w;      // row span of the 256 pixels
    const int pw = a.w + k - 1, nr = yb - ya + k;             // staged columns / rows
    const bool lds = nr * pw * a.c <= RR_BLUR_LDS;           // uniform
    if (lds) {
      const int rowb = pw * a.c;
      for (int e = t; e < nr * rowb; e += 256) {
        const int r = e / rowb, rest = e - r * rowb;
        const int cx = rest / a.c, ch = rest - cx * a.c;
        const int yy = reflect101(ya - anc + r, a.h), xx = reflect101(cx - anc, a.w);
        simg[e] = src[((long long)yy * a.w + xx) * a.c + ch];
      }
    }
    __syncthreads();
    int off = 0;
    for (int u = 0; u < wv; ++u) off += wcount[u];
    if (nz) { tv[off + pos] = kv; ti[off + pos] = (i << 8) | j; }
    const int nt = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    __syncthreads();
    const long long q = q0 + t;
    const int rem = (int)(q - (long long)img * hw), y = rem / a.w, x = rem % a.w;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (lds) {
      const uint8_t *base = simg + ((y - ya) * pw + x) * a.c;
      for (int u = 0; u < nt; ++u) {
        const int ij = ti[u];
        const float w = tv[u];
        const uint8_t *px = base + ((ij >> 8) * pw + (ij & 255)) * a.c;
        for (int c = 0; c < a.c; ++c) s[c] = s[c] + w * (float)px[c];
      }
    } else {
      for (int u = 0; u < nt; ++u) {
        const int ij = ti[u];
        const float w = tv[u];
        const int yy = reflect101(y + (ij >> 8) - anc, a.h), xx = reflect101(x + (ij & 255) - anc, a.w);
        const uint8_t *px = src + ((long long)yy * a.w + xx) * a.c;
        for (int c = 0; c < a.c; ++c) s[c] = s[c] + w * (float)px[c];
      }
    }
    blur_store(a, p, q * a.c, a.out + q * a.c, s);
  }
}

static void launch_blur(const DistCfg &a, long long tp, const RrPath &p, hipStream_t st) {
  // the LDS-tiled form where whole 256-pixel tiles fit (RR_PATH
  // blur_tiled=0: the per-pixel kernel, tests)
  if (((long long)a.h * a.w) % 256 == 0 && a.c <= 4 && p.blur_tiled)
    hipLaunchKernelGGL(distort_blur_tiled_kernel, dim3(rr_grid_cap((tp + 255) / 256, 8192)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(distort_blur_kernel, dim3(rr_grid_cap((tp + 255) / 256, 8192)), dim3(256), 0, st, a);
}

// ---------------------------------------------------- on-device draws ----
// The per-image draws of apply_random_distortions (14:36-58) made on device,
// so the whole data step is graph-capturable: the same distributions as the
// reference's Python `random` calls (fog with p 0.5, intensity U(0.3, 0.7),
// t = 1 - intensity * U(0.8, 1.2), A = 0.9; noise with p 0.5, var U(0.01,
// 0.03); blur with p 0.5, degree randint(5, 15), angle randint(0, 360)), drawn
// from Philox4x32-10 keyed by (seed, step) with the image index as counter
// (the reference's stream is unseeded, so only the distributions can match).
// The step counter lives in device memory and advances once per call; the
// blur kernel of (degree, angle) is an index into a table of all 11 x 361
// kernels built once on the host by rr_motion_blur_kernel.
constexpr int DRAW_DEG0 = 5, DRAW_NDEG = 11, DRAW_NANG = 361;

__device__ __forceinline__ double u01(uint32_t hi, uint32_t lo) {       // [0, 1), 53 bits
  return ((((unsigned long long)hi << 21) ^ lo) & ((1ull << 53) - 1)) * 0x1p-53;
}

// the Philox key of step s, image i's draws under it, and the step's noise
// seed: one statement for the dense and the ragged generator, so image i of
// (seed, step) draws the same in both
__device__ __forceinline__ unsigned long long draw_key(unsigned long long seed, long long s) {
  return seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(s + 1));
}

__device__ void distort_draw_one(int i, unsigned long long key, rr_distort_param *prm, int *tap_idx) {
#pragma clang fp contract(off)
  uint32_t a[4] = {(uint32_t)i, 0u, 0x5EED0001u, 0u}, b[4] = {(uint32_t)i, 1u, 0x5EED0001u, 0u};
  philox4(a, key);
  philox4(b, key);
  const double r_fog = u01(a[0], a[1]), r_int = u01(a[2], a[3]);
  const double r_t = u01(b[0], b[1]), r_noise = u01(b[2], b[3]);
  uint32_t c[4] = {(uint32_t)i, 2u, 0x5EED0001u, 0u}, d[4] = {(uint32_t)i, 3u, 0x5EED0001u, 0u};
  philox4(c, key);
  philox4(d, key);
  const double r_var = u01(c[0], c[1]), r_blur = u01(c[2], c[3]);
  const double r_deg = u01(d[0], d[1]), r_ang = u01(d[2], d[3]);
  rr_distort_param p;
  p.sigma = 0.0;
  p.fog_mul = 1.0f;
  p.fog_add = 0.0f;
  p.flags = 0;
  p.ksize = 0;
  int ti = 0;
  if (r_fog < 0.5) {
    const double intensity = 0.3 + (0.7 - 0.3) * r_int;
    const double t = 1.0 - intensity * (0.8 + (1.2 - 0.8) * r_t);
    p.flags |= RR_DISTORT_FOG;
    p.fog_mul = (float)t;
    p.fog_add = (float)(0.9 * (1.0 - t));
  }
  if (r_noise < 0.5) {
    const double var = 0.01 + (0.03 - 0.01) * r_var;
    p.flags |= RR_DISTORT_NOISE;
    p.sigma = sqrt(var);
  }
  if (r_blur < 0.5) {
    const int deg = DRAW_DEG0 + (int)(r_deg * DRAW_NDEG);
    const int ang = (int)(r_ang * DRAW_NANG);
    p.flags |= RR_DISTORT_BLUR;
    p.ksize = deg;
    ti = (deg - DRAW_DEG0) * DRAW_NANG + ang;
  }
  *prm = p;
  *tap_idx = ti;
}

__device__ __forceinline__ unsigned long long draw_noise_seed(unsigned long long key) {
  uint32_t e[4] = {0xFFFFFFFFu, 0u, 0x5EED0002u, 0u};
  philox4(e, key);
  return ((unsigned long long)e[0] << 32) | e[1];
}

__global__ __launch_bounds__(256) void distort_draw_kernel(int n, unsigned long long seed,
                                                           long long *step, rr_distort_param *prm,
                                                           int *tap_idx, unsigned long long *noise_seed) {
  const long long s = *step;
  const unsigned long long key = draw_key(seed, s);
  for (int i = threadIdx.x; i < n; i += blockDim.x) distort_draw_one(i, key, prm + i, tap_idx + i);
  __syncthreads();
  if (threadIdx.x == 0) {
    *noise_seed = draw_noise_seed(key);
    *step = s + 1;
  }
}

// ------------------------------------------------- ragged distortion ----
// The same generator for n images of unequal size in one byte buffer, each at
// its NATIVE size, as the reference distorts them before it resizes anything
// (14:75-93; 16:44-58 for the compound form): two launches whatever n is, no
// per-image host work, the table and the step counter read on the device only.
//   1. rdist_prologue_kernel (one workgroup): elem_base[i], the exclusive
//      prefix sum of h * w * c over the records in table order (an invalid
//      record counts 0): the element index that keys the Philox noise and
//      indexes the explicit noise field.  Images back to back in table order
//      thus use the dense op's element indices, whatever the byte offsets
//      are.  The random variant makes the per-image draws here too.
//   2. rdist_tile_kernel: one workgroup per (image, TH x TW tile of output
//      pixels).  For a blurred image it computes the blur INPUT of its tile
//      plus the k - 1 halo straight into LDS -- the source coordinate
//      reflected (101), the noise taken at the reflected source element's
//      index, so a halo byte is the byte the two-pass form reads back from its
//      staging image -- compacts the nonzero taps (row-major), and after one
//      barrier runs the fp32 tap sum out of LDS.  The staging image never
//      reaches HBM; the price is that a halo element's fog / noise is
//      computed by every tile that reads it.
// A record that fails rd_valid (rg_valid, or a blur flag with ksize outside
// [1, KMAX]) reads nothing and writes nothing.
struct RdArgs {
  DistCfg d;                            // n, mode, in, out, prm, taps, noise, seeds; h, w = max_h, max_w
  const rr_ragged_image *tab;
  long long in_bytes;
  long long *elem_base;                 // [n], workspace
  int tiles_y, tiles_x;                 // tiles of a max_h x max_w image
};

__device__ __forceinline__ bool rd_valid(const rr_ragged_image &r, const rr_distort_param &p, int c,
                                         int max_h, int max_w, long long in_bytes) {
  if ((p.flags & RR_DISTORT_BLUR) && (p.ksize < 1 || p.ksize > RR_DISTORT_KMAX)) return false;
  return rg_valid(r, c, max_h, max_w, in_bytes);
}

// draw != 0: image i's draws of (seed, *step) into prm_out / idx_out (= a.d.prm
// / a.d.tap_idx), the step's noise seed, *step += 1 -- distort_draw_kernel's
// work, by the same device functions
__global__ __launch_bounds__(256) void rdist_prologue_kernel(RdArgs a, int draw, unsigned long long seed,
                                                             long long *step, rr_distort_param *prm_out,
                                                             int *idx_out, unsigned long long *noise_seed) {
  __shared__ long long scan[256];
  const int t = threadIdx.x;
  long long s = 0;
  unsigned long long key = 0;
  if (draw) {
    s = *step;
    key = draw_key(seed, s);
  }
  long long carry = 0;                                      // elements of the records before this chunk
  for (int i0 = 0; i0 < a.d.n; i0 += 256) {
    const int i = i0 + t;
    long long v = 0;
    if (i < a.d.n) {
      rr_distort_param p;
      if (draw) {
        int ti;
        distort_draw_one(i, key, &p, &ti);
        prm_out[i] = p;
        idx_out[i] = ti;
      } else {
        p = a.d.prm[i];
      }
      const rr_ragged_image r = a.tab[i];
      if (rd_valid(r, p, a.d.c, a.d.h, a.d.w, a.in_bytes)) v = (long long)r.h * r.w * a.d.c;
    }
    scan[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                     // inclusive scan of the chunk
      const long long u = t >= o ? scan[t - o] : 0;
      __syncthreads();
      scan[t] += u;
      __syncthreads();
    }
    if (i < a.d.n) a.elem_base[i] = carry + scan[t] - v;
    carry += scan[255];
    __syncthreads();                                        // scan is rewritten by the next chunk
  }
  if (draw && t == 0) {
    *noise_seed = draw_noise_seed(key);
    *step = s + 1;
  }
}

template <int C, int TH, int TW>
__global__ __launch_bounds__(256) void rdist_tile_kernel(RdArgs a) {
#pragma clang fp contract(off)
  constexpr int K2 = RR_DISTORT_KMAX * RR_DISTORT_KMAX;
  // a staged pixel takes PS bytes, 4 for 3 channels: the tap loop then reads a
  // pixel in one aligned LDS load (3-byte pixels made it a misaligned 16-bit
  // load plus a byte load per tap, and the tap loop the slowest part of the
  // call by far)
  constexpr int PS = C == 3 ? 4 : C;
  using Pix = std::conditional_t<PS == 4, uint32_t, std::conditional_t<PS == 2, uint16_t, uint8_t>>;
  __shared__ Pix simg[(TH + RR_DISTORT_KMAX - 1) * (TW + RR_DISTORT_KMAX - 1)];
  __shared__ float tv[K2];
  __shared__ int ti[K2];
  __shared__ int ntaps;
  const int t = threadIdx.x;
  const int tiles = a.tiles_y * a.tiles_x;
  const int img = blockIdx.x / tiles, tl = blockIdx.x - img * tiles;
  const int y0 = (tl / a.tiles_x) * TH, x0 = (tl % a.tiles_x) * TW;
  const rr_ragged_image r = a.tab[img];
  const rr_distort_param p = a.d.prm[img];
  // uniform over the workgroup, and before any barrier
  if (!rd_valid(r, p, C, a.d.h, a.d.w, a.in_bytes) || y0 >= r.h || x0 >= r.w) return;
  const int th = r.h - y0 < TH ? r.h - y0 : TH, tw = r.w - x0 < TW ? r.w - x0 : TW;
  DistCfg d = a.d;
  d.c = C;
  const long long eb = a.elem_base[img];
  const uint8_t *src = d.in + r.offset;
  uint8_t *dst = d.out + r.offset;
  if (!(p.flags & RR_DISTORT_BLUR)) {                        // distort_pre_kernel's expression
    const int rowb = tw * C;
    for (int i = t; i < th * rowb; i += 256) {
      const int ly = i / rowb;
      const long long le = ((long long)(y0 + ly) * r.w + x0) * C + (i - ly * rowb);
      const float x = (float)src[le] / 255.0f;
      if (d.mode == 0) dst[le] = fog_noise(d, p, x, eb + le);
      else dst[le] = fog_noise(d, p, (float)trunc_u8f(x * 255.f) / 255.0f, eb + le);
    }
    return;
  }
  const int k = p.ksize, anc = k / 2;
  // the nonzero taps in row-major order (cv2 drops zero taps), listed by the
  // first wave alone: tap u = lane + 64 j, so the ballots come in tap order
  if (t < 64) {
    const float *kt = d.taps + (long long)(d.tap_idx ? d.tap_idx[img] : img) * K2;
    int off = 0;
#pragma unroll
    for (int j = 0; j < (K2 + 63) / 64; ++j) {
      const int u = t + 64 * j, ki = u / k, kj = u - ki * k;
      const float kv = u < k * k ? kt[ki * RR_DISTORT_KMAX + kj] : 0.f;
      const bool nz = kv != 0.f;
      const unsigned long long m = __ballot(nz);
      if (nz) {
        const int pos = off + __popcll(m & ((1ull << t) - 1ull));
        tv[pos] = kv;
        ti[pos] = (ki << 8) | kj;
      }
      off += __popcll(m);
    }
    if (t == 0) ntaps = off;
  }
  // the blur input of the tile and its halo: rows y0 - anc .. y0 + th + k - 2 -
  // anc, columns likewise, each at its reflected source element
  const int pw = tw + k - 1, nr = th + k - 1, rowb = pw * C;
  for (int e = t; e < nr * rowb; e += 256) {
    const int ry = e / rowb, rest = e - ry * rowb;
    const int cx = rest / C, ch = rest - cx * C;
    const int yy = reflect101(y0 - anc + ry, r.h), xx = reflect101(x0 - anc + cx, r.w);
    const long long le = ((long long)yy * r.w + xx) * C + ch;
    const float x = (float)src[le] / 255.0f;
    ((uint8_t *)simg)[(ry * pw + cx) * PS + ch] = d.mode == 0 ? fog_noise(d, p, x, eb + le) : trunc_u8f(x * 255.f);
  }
  __syncthreads();
  const int nt = ntaps;
  for (int i = t; i < th * tw; i += 256) {
    const int ly = i / tw, lx = i - ly * tw;
    const Pix *base = simg + ly * pw + lx;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int u = 0; u < nt; ++u) {
      const int ij = ti[u];
      const float w = tv[u];
      const uint32_t px = base[(ij >> 8) * pw + (ij & 255)];
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] = s[c] + w * (float)((px >> (8 * c)) & 255u);
    }
    const long long le = ((long long)(y0 + ly) * r.w + (x0 + lx)) * C;
    blur_store(d, p, eb + le, dst + le, s);
  }
}

// workspace of both ragged entry points: elem_base[n], then the random
// variant's draws in rr_distort_random_u8's order (params, table indices, noise
// seed).  No image-sized term: nothing is staged in HBM.
struct RdPlan {
  size_t off_prm, off_idx, off_seed, total;
};

static int rd_plan(int n, int c, int max_h, int max_w, RdPlan *p) {
  if (n <= 0 || c < 1 || c > 4 || max_h < 1 || max_w < 1) return RR_EINVAL;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  p->off_prm = al((size_t)n * sizeof(long long));
  p->off_idx = al(p->off_prm + (size_t)n * sizeof(rr_distort_param));
  p->off_seed = al(p->off_idx + (size_t)n * sizeof(int));
  p->total = p->off_seed + 16;
  return RR_OK;
}

// the tile shape: 32 x 32 unless RR_PATH rdist_tile names one of the other
// two measured shapes (tools/bench_ragged_distort.py)
static int rd_launch(RdArgs a, int c, int max_h, int max_w, int tile, hipStream_t st) {
  auto go = [&](auto th, auto tw) {
    constexpr int TH = decltype(th)::value, TW = decltype(tw)::value;
    a.tiles_y = (max_h + TH - 1) / TH;
    a.tiles_x = (max_w + TW - 1) / TW;
    const long long groups = (long long)a.d.n * a.tiles_y * a.tiles_x;
    if (groups >= (1LL << 31)) return (int)RR_EUNSUPPORTED;
    return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
      hipLaunchKernelGGL((rdist_tile_kernel<decltype(cc)::value, TH, TW>), dim3((unsigned)groups), dim3(256), 0,
                         st, a);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  };
  if (tile == 16) return go(ic<16>{}, ic<16>{});
  if (tile == 64) return go(ic<64>{}, ic<64>{});
  return go(ic<32>{}, ic<32>{});
}

extern "C" size_t rr_distort_workspace(int n, int h, int w, int c) {
  return n > 0 && h > 0 && w > 0 && c > 0 ? (size_t)n * h * w * c : 0;
}

extern "C" int rr_distort_u8(int n, int h, int w, int c, int mode, const uint8_t *in, uint8_t *out,
                             const rr_distort_param *params, const float *taps, const double *noise,
                             unsigned long long seed, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!in || !out || !params || !taps || !ws || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (c < 1 || c > 4 || (mode != 0 && mode != 1)) return RR_EINVAL;
  if (ws_bytes < rr_distort_workspace(n, h, w, c)) return RR_EWORKSPACE;
  DistCfg a{n, h, w, c, mode, in, out, (uint8_t *)ws, params, taps, noise, seed, nullptr, nullptr};
  hipStream_t st = (hipStream_t)stream;
  const long long te = (long long)n * h * w * c, tp = (long long)n * h * w;
  hipLaunchKernelGGL(distort_pre_kernel, dim3(rr_grid_cap((te + 255) / 256, 8192)), dim3(256), 0, st, a);
  RR_CHECK_LAUNCH();
  launch_blur(a, tp, rr_path_read(), st);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

// cv2.getRotationMatrix2D((k / 2, k / 2), angle, 1) + cv2.warpAffine of
// np.diag(np.ones(k)) (INTER_LINEAR, BORDER_CONSTANT 0, dsize (k, k)) / k,
// converted to fp32 as filter2D does (14:55-59, 16:20-21).  Host code: the
// reference builds this kernel on the host per image too; it is <= 225 taps.
// warpAffine: inverted matrix, 10-bit fixed-point source coordinates rounded
// half-even, 1/32-pixel interpolation table of fp32 bilinear weights.
extern "C" int rr_motion_blur_kernel(int k, int angle, float *taps) {
  if (!taps || k < 1 || k > RR_DISTORT_KMAX) return RR_EINVAL;
  const double cx = (float)(k / 2.0), cy = cx;
  const double ang = angle * 3.14159265358979323846 / 180.0;
  const double alpha = std::cos(ang) * 1.0, beta = std::sin(ang) * 1.0;
  double M[6] = {alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy};
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  auto rnd = [](double v) { return (int)std::nearbyint(v); };   // cvRound: half to even
  float tab1[32][2];
  for (int i = 0; i < 32; ++i) {
    const float x = i * (1.f / 32);
    tab1[i][0] = 1.f - x;
    tab1[i][1] = x;
  }
  for (int y = 0; y < k; ++y)
    for (int x = 0; x < k; ++x) {
      const int X0 = rnd((M[1] * y + M[2]) * 1024) + 16, Y0 = rnd((M[4] * y + M[5]) * 1024) + 16;
      const int X = (X0 + rnd(M[0] * x * 1024)) >> 5, Y = (Y0 + rnd(M[3] * x * 1024)) >> 5;
      const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
      const float w[4] = {tab1[fy][0] * tab1[fx][0], tab1[fy][0] * tab1[fx][1],
                          tab1[fy][1] * tab1[fx][0], tab1[fy][1] * tab1[fx][1]};
      auto src = [&](int xx, int yy) -> double {               // np.diag(np.ones(k)), 0 outside
        return xx >= 0 && yy >= 0 && xx < k && yy < k && xx == yy ? 1.0 : 0.0;
      };
      double v = 0.0;
      if (!(sx >= k || sx + 1 < 0 || sy >= k || sy + 1 < 0))
        v = src(sx, sy) * w[0] + src(sx + 1, sy) * w[1] + src(sx, sy + 1) * w[2] + src(sx + 1, sy + 1) * w[3];
      taps[y * RR_DISTORT_KMAX + x] = (float)(v / k);
    }
  for (int y = 0; y < RR_DISTORT_KMAX; ++y)
    for (int x = 0; x < RR_DISTORT_KMAX; ++x)
      if (y >= k || x >= k) taps[y * RR_DISTORT_KMAX + x] = 0.f;
  return RR_OK;
}

// all 11 x 361 motion-blur kernels of the draws above ([deg - 5][angle][KMAX^2])
extern "C" size_t rr_motion_blur_table_floats(void) {
  return (size_t)DRAW_NDEG * DRAW_NANG * RR_DISTORT_KMAX * RR_DISTORT_KMAX;
}

extern "C" int rr_motion_blur_table(float *table) {
  if (!table) return RR_EINVAL;
  for (int d = 0; d < DRAW_NDEG; ++d)
    for (int a = 0; a < DRAW_NANG; ++a) {
      const int rc = rr_motion_blur_kernel(DRAW_DEG0 + d, a,
                                           table + ((size_t)d * DRAW_NANG + a) * RR_DISTORT_KMAX * RR_DISTORT_KMAX);
      if (rc) return rc;
    }
  return RR_OK;
}

// workspace of rr_distort_random_u8: the blur staging image, the n draws, the
// n tap indices and the step's noise seed
static size_t draw_off_prm(int n, int h, int w, int c) {
  return ((size_t)n * h * w * c + 15) / 16 * 16;
}
extern "C" size_t rr_distort_random_workspace(int n, int h, int w, int c) {
  if (n <= 0 || h <= 0 || w <= 0 || c <= 0) return 0;
  return draw_off_prm(n, h, w, c) + (size_t)n * sizeof(rr_distort_param) + ((size_t)n * 4 + 15) / 16 * 16 + 16;
}

extern "C" int rr_distort_random_u8(int n, int h, int w, int c, const uint8_t *in, uint8_t *out,
                                    unsigned long long seed, long long *step, const float *table,
                                    void *ws, size_t ws_bytes, rr_stream stream) {
  if (!in || !out || !step || !table || !ws || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (c < 1 || c > 4) return RR_EINVAL;
  if (ws_bytes < rr_distort_random_workspace(n, h, w, c)) return RR_EWORKSPACE;
  char *base = (char *)ws;
  rr_distort_param *prm = (rr_distort_param *)(base + draw_off_prm(n, h, w, c));
  int *tap_idx = (int *)((char *)prm + (size_t)n * sizeof(rr_distort_param));
  unsigned long long *nseed = (unsigned long long *)((char *)tap_idx + ((size_t)n * 4 + 15) / 16 * 16);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distort_draw_kernel, dim3(1), dim3(256), 0, st, n, seed, step, prm, tap_idx, nseed);
  RR_CHECK_LAUNCH();
  DistCfg a{n, h, w, c, 0, in, out, (uint8_t *)ws, prm, table, nullptr, 0ull, tap_idx, nseed};
  const long long te = (long long)n * h * w * c, tp = (long long)n * h * w;
  hipLaunchKernelGGL(distort_pre_kernel, dim3(rr_grid_cap((te + 255) / 256, 8192)), dim3(256), 0, st, a);
  RR_CHECK_LAUNCH();
  launch_blur(a, tp, rr_path_read(), st);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

// the draws of the last rr_distort_random_u8 call, read back from its
// workspace (tests): params [n], tap indices [n], noise seed
extern "C" int rr_distort_random_draws(int n, int h, int w, int c, const void *ws,
                                       size_t *prm_off, size_t *idx_off, size_t *seed_off) {
  if (!ws || n <= 0 || !prm_off || !idx_off || !seed_off) return RR_EINVAL;
  *prm_off = draw_off_prm(n, h, w, c);
  *idx_off = *prm_off + (size_t)n * sizeof(rr_distort_param);
  *seed_off = *idx_off + ((size_t)n * 4 + 15) / 16 * 16;
  return RR_OK;
}

// ------------------------------------------- ragged distortion: C ABI ----
extern "C" size_t rr_distort_ragged_workspace(int n, int c, int max_h, int max_w) {
  RdPlan p;
  return rd_plan(n, c, max_h, max_w, &p) == RR_OK ? p.total : 0;
}

extern "C" int rr_distort_ragged_u8(int n, int c, int mode, int max_h, int max_w, const uint8_t *in,
                                    size_t in_bytes, const rr_ragged_image *images_dev, uint8_t *out,
                                    const rr_distort_param *params, const float *taps, const int *tap_idx,
                                    const double *noise, unsigned long long seed, void *ws, size_t ws_bytes,
                                    rr_stream stream) {
  RdPlan p;
  if (!in || !images_dev || !out || !params || !taps || !ws || in == out) return RR_EINVAL;   // halo reads: not in place
  if (in_bytes == 0 || in_bytes > (size_t)INT64_MAX || (mode != 0 && mode != 1)) return RR_EINVAL;
  if (const int rc = rd_plan(n, c, max_h, max_w, &p)) return rc;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  RdArgs a{DistCfg{n, max_h, max_w, c, mode, in, out, nullptr, params, taps, noise, seed, tap_idx, nullptr},
           images_dev, (long long)in_bytes, (long long *)ws, 0, 0};
  hipLaunchKernelGGL(rdist_prologue_kernel, dim3(1), dim3(256), 0, st, a, 0, 0ull, (long long *)nullptr,
                     (rr_distort_param *)nullptr, (int *)nullptr, (unsigned long long *)nullptr);
  RR_CHECK_LAUNCH();
  return rd_launch(a, c, max_h, max_w, rr_path_read().rdist_tile, st);
}

extern "C" int rr_distort_random_ragged_u8(int n, int c, int max_h, int max_w, const uint8_t *in,
                                           size_t in_bytes, const rr_ragged_image *images_dev, uint8_t *out,
                                           unsigned long long seed, long long *step, const float *table,
                                           void *ws, size_t ws_bytes, rr_stream stream) {
  RdPlan p;
  if (!in || !images_dev || !out || !step || !table || !ws || in == out) return RR_EINVAL;
  if (in_bytes == 0 || in_bytes > (size_t)INT64_MAX) return RR_EINVAL;
  if (const int rc = rd_plan(n, c, max_h, max_w, &p)) return rc;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  char *base = (char *)ws;
  rr_distort_param *prm = (rr_distort_param *)(base + p.off_prm);
  int *tap_idx = (int *)(base + p.off_idx);
  unsigned long long *nseed = (unsigned long long *)(base + p.off_seed);
  hipStream_t st = (hipStream_t)stream;
  RdArgs a{DistCfg{n, max_h, max_w, c, 0, in, out, nullptr, prm, table, nullptr, 0ull, tap_idx, nseed},
           images_dev, (long long)in_bytes, (long long *)ws, 0, 0};
  hipLaunchKernelGGL(rdist_prologue_kernel, dim3(1), dim3(256), 0, st, a, 1, seed, step, prm, tap_idx, nseed);
  RR_CHECK_LAUNCH();
  return rd_launch(a, c, max_h, max_w, rr_path_read().rdist_tile, st);
}

// the draws of the last rr_distort_random_ragged_u8 call, as rr_distort_random_draws
extern "C" int rr_distort_random_ragged_draws(int n, int c, int max_h, int max_w, const void *ws,
                                              size_t *prm_off, size_t *idx_off, size_t *seed_off) {
  RdPlan p;
  if (!ws || !prm_off || !idx_off || !seed_off) return RR_EINVAL;
  if (const int rc = rd_plan(n, c, max_h, max_w, &p)) return rc;
  *prm_off = p.off_prm;
  *idx_off = p.off_idx;
  *seed_off = p.off_seed;
  return RR_OK;
}
