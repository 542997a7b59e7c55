// resize.hip -- torchvision Resize((oh, ow)) on PIL images,
// on device and bit-exact: PIL Image.resize(BILINEAR) (17:66, 18:28-32), its
// separable two-pass resample with antialiasing support (filter support scaled
// by the downscale factor), coefficients normalised in double and rounded to
// 22-bit fixed point, an 8-bit clip after each pass.  Optionally fused with
// ToTensor (x / 255 in fp32) and Normalize ((x - mean) / std in fp32, 18:31)
// into an NCHW fp32 batch.  rr_resize_bilinear_u8 takes a dense batch (the
// intermediate image in the workspace), rr_resize_ragged_u8 n images of
// unequal size in one buffer (05:24-29; the intermediate image in LDS), and
// rr_ragged_check is the host's test of a ragged table.  Byte work, no MFMA:
// one thread per output pixel, coalesced along the innermost NHWC axis.
#include "imgproc.h"

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

// Normalize's constants of a call (ToTensor alone: mean 0, std 1), and the
// rule for its arguments: mean and std together, and only with the fp32 output
static RsNorm rs_norm(int c, const float *mean, const float *std) {
  RsNorm nm{};
  for (int i = 0; i < c; ++i) {
    nm.mean[i] = mean ? mean[i] : 0.f;
    nm.std[i] = std ? std[i] : 1.f;
  }
  return nm;
}
static bool rs_norm_args_ok(int out_kind, const float *mean, const float *std) {
  return (mean == nullptr) == (std == nullptr) && (!mean || out_kind == 1);
}

// the four coefficient tables of one image (bounds and taps, horizontal then
// vertical), each at a 256-byte boundary; rs_tables -> the bytes they take
struct RsTables { size_t off_bh, off_kh, off_bv, off_kv; };
static size_t rs_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t rs_tables(int oh, int ow, int kh, int kv, RsTables *t) {
  size_t o = 0;
  t->off_bh = o; o = rs_align(o + (size_t)ow * 2 * 4);
  t->off_kh = o; o = rs_align(o + (size_t)ow * kh * 4);
  t->off_bv = o; o = rs_align(o + (size_t)oh * 2 * 4);
  t->off_kv = o; o = rs_align(o + (size_t)oh * kv * 4);
  return o;
}

struct RsPlan : RsTables {
  int kh, kv, y_first, rows;
  size_t off_tmp, total;
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
  p->off_tmp = rs_tables(oh, ow, p->kh, p->kv, p);
  p->total = rs_align(p->off_tmp + (size_t)n * p->rows * ow * c);
  return true;
}

// rs_ksize's ceil(scale) * 2 + 1 <= RS_MAXK for every image up to max_h x
// max_w, tested without its int overflowing
static bool rs_taps_ok(int max_h, int max_w, int oh, int ow) {
  return (max_w - 1) / ow < RS_MAXK / 2 && (max_h - 1) / oh < RS_MAXK / 2;
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

struct RgPlan : RsTables {
  int kh, kv, band, tile_rows;
  size_t lds, per_image, total;
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
  if (!rs_taps_ok(max_h, max_w, oh, ow)) return RR_EUNSUPPORTED;
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
  p->per_image = rs_tables(oh, ow, p->kh, p->kv, p);
  p->total = p->per_image * (size_t)n;
  return RR_OK;
}

}  // namespace

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
  if (!rs_norm_args_ok(out_kind, mean, std)) return RR_EINVAL;
  const RsNorm nm = rs_norm(c, mean, std);
  const int norm = mean != nullptr;               // only with out_kind 1
  hipStream_t st = (hipStream_t)stream;
  if (oh == h && ow == w) {
    const long long np = (long long)n * h * w;
    const dim3 g(rr_grid_cap((np + 255) / 256, 8192)), b(256);
    return rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
      constexpr int CC = decltype(cc)::value;
      if (out_kind == 0) hipLaunchKernelGGL((rs_same_kernel<CC, 0>), g, b, 0, st, np, h * w, in, out, nm, norm);
      else hipLaunchKernelGGL((rs_same_kernel<CC, 1>), g, b, 0, st, np, h * w, in, out, nm, norm);
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
  if (!rs_taps_ok(max_h, max_w, oh, ow)) return RR_EUNSUPPORTED;
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
  if (!rg_bytes_ok(in_bytes)) return RR_EINVAL;
  if (const int rc = rg_plan(n, c, max_h, max_w, oh, ow, &p)) return rc;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  if (!rs_norm_args_ok(out_kind, mean, std)) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const RgArgs a{n, max_h, max_w, oh, ow, p.kh, p.kv, p.band, p.tile_rows, (long long)in_bytes,
                 in, images_dev, (char *)ws, p.per_image, p.off_bh, p.off_kh, p.off_bv, p.off_kv};
  const long long nco = (long long)n * (ow + oh);
  hipLaunchKernelGGL(rg_coeffs_kernel, dim3((unsigned)((nco + 63) / 64)), dim3(64), 0, st, a, c);
  RR_CHECK_LAUNCH();
  const RsNorm nm = rs_norm(c, mean, std);
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
