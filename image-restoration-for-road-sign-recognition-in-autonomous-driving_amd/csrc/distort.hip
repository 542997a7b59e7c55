// distort.hip -- the distortion generator of the training data (SURVEY §8f
// row 1), on device:
//   * rr_distort_u8: a dense [n, h, w, c] batch under the caller's per-image
//     parameters and blur kernels, in two passes (fog / noise per element,
//     then the blur of the images that have one out of a staging image).
//   * rr_distort_random_u8: the same with the per-image draws made on the
//     device from (seed, step), so a captured training step re-draws on every
//     replay.
//   * rr_distort_ragged_u8 / rr_distort_random_ragged_u8: n images of unequal
//     size in one buffer, each at its native size, in two launches, the blur
//     input in LDS and no staging image.
//   * rr_distort_single_ragged_u8: the noise, blur and fog of the offline
//     generators 02-04 and of 13:33-56 in their own spelling, one kind per
//     ragged batch; the blur with 03:29's per-image min-max stretch.
//   * rr_motion_blur_kernel / rr_motion_blur_table: cv2's rotated line kernel
//     restated on the host, one kernel or all 11 x 361 the draws can pick.
// The work is VALU (Philox + logf / cosf for the noise, up to 225 taps per
// blurred pixel), not HBM.
//
// The dynamic distortion generator 14:31-64 (fog -> noise -> motion blur, each
// drawn per image) and the fixed compound variant 16:14-37 (blur -> fog ->
// noise), per image on device, with the reference's numpy dtype semantics:
//   img / 255 in fp32; fog out * f32(t) + f32(A (1 - t)) in fp32; noise added
//   in fp64 (np.random.normal is float64, so the image becomes float64);
//   clip(x * 255, 0, 255).astype(uint8) truncates; cv2.filter2D on uint8 with
//   the fp32-converted kernel: fp32 sum over the taps in row-major order,
//   BORDER_REFLECT_101, anchor (k / 2, k / 2), round half to even, saturate.
// Noise: the caller's fp64 field (parity runs) or Philox4x32-10 normals
// (Box-Muller, philox_normal) keyed by (seed, element index).
#include "imgproc.h"
#include "philox.h"

#include <cfloat>
#include <cmath>

namespace {

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
constexpr int RR_BLUR_LDS = 24576;
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

// the dense generator's two launches: stage 1 over the elements, stage 2 over
// the pixels
static int dist_launch(const DistCfg &a, hipStream_t st) {
  const long long tp = (long long)a.n * a.h * a.w, te = tp * a.c;
  hipLaunchKernelGGL(distort_pre_kernel, dim3(rr_grid_cap((te + 255) / 256, 8192)), dim3(256), 0, st, a);
  RR_CHECK_LAUNCH();
  // the LDS-tiled form where whole 256-pixel tiles fit (RR_PATH
  // blur_tiled=0: the per-pixel kernel, tests)
  if (((long long)a.h * a.w) % 256 == 0 && a.c <= 4 && rr_path_read().blur_tiled)
    hipLaunchKernelGGL(distort_blur_tiled_kernel, dim3(rr_grid_cap((tp + 255) / 256, 8192)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(distort_blur_kernel, dim3(rr_grid_cap((tp + 255) / 256, 8192)), dim3(256), 0, st, a);
  RR_CHECK_LAUNCH();
  return RR_OK;
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

// elem_base[i] = the exclusive prefix sum of count(i) over the n records, by
// one 256-thread workgroup; count(i), the elements of record i (0 for an
// invalid one), is called once, by thread i % 256
template <class Count>
__device__ __forceinline__ void elem_base_scan(int n, long long *elem_base, Count count) {
  __shared__ long long scan[256];
  const int t = threadIdx.x;
  long long carry = 0;                                      // elements of the records before this chunk
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    const long long v = i < n ? count(i) : 0;
    scan[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                     // inclusive scan of the chunk
      const long long u = t >= o ? scan[t - o] : 0;
      __syncthreads();
      scan[t] += u;
      __syncthreads();
    }
    if (i < n) elem_base[i] = carry + scan[t] - v;
    carry += scan[255];
    __syncthreads();                                        // scan is rewritten by the next chunk
  }
}

// draw != 0: image i's draws of (seed, *step) into prm_out / idx_out (= a.d.prm
// / a.d.tap_idx), the step's noise seed, *step += 1 -- distort_draw_kernel's
// work, by the same device functions
__global__ __launch_bounds__(256) void rdist_prologue_kernel(RdArgs a, int draw, unsigned long long seed,
                                                             long long *step, rr_distort_param *prm_out,
                                                             int *idx_out, unsigned long long *noise_seed) {
  const int t = threadIdx.x;
  long long s = 0;
  unsigned long long key = 0;
  if (draw) {
    s = *step;
    key = draw_key(seed, s);
  }
  elem_base_scan(a.d.n, a.elem_base, [&](int i) -> long long {
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
    return rd_valid(r, p, a.d.c, a.d.h, a.d.w, a.in_bytes) ? (long long)r.h * r.w * a.d.c : 0;
  });
  if (draw && t == 0) {
    *noise_seed = draw_noise_seed(key);
    *step = s + 1;
  }
}

// a staged pixel takes PS bytes, 4 for 3 channels: the tap loop then reads a
// pixel in one aligned LDS load (3-byte pixels made it a misaligned 16-bit
// load plus a byte load per tap, and the tap loop the slowest part of the
// call by far)
template <int C> struct TilePix {
  static constexpr int PS = C == 3 ? 4 : C;
  using type = std::conditional_t<PS == 4, uint32_t, std::conditional_t<PS == 2, uint16_t, uint8_t>>;
};

// the nonzero taps of the k x k kernel kt in row-major order (cv2 drops zero
// taps), listed by the first wave alone (t < 64): tap u = lane + 64 j, so the
// ballots come in tap order
__device__ __forceinline__ void list_taps(const float *kt, int k, int t, float *tv, int *ti, int *ntaps) {
  constexpr int K2 = RR_DISTORT_KMAX * RR_DISTORT_KMAX;
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
  if (t == 0) *ntaps = off;
}

// the fp32 tap sum of one output pixel out of the staged tile (pw pixels a
// row), base its top-left tap's pixel
template <int C>
__device__ __forceinline__ void tap_sum(const typename TilePix<C>::type *base, int pw, int nt, const float *tv,
                                        const int *ti, float *s) {
#pragma clang fp contract(off)
  for (int u = 0; u < nt; ++u) {
    const int ij = ti[u];
    const float w = tv[u];
    const uint32_t px = base[(ij >> 8) * pw + (ij & 255)];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = s[c] + w * (float)((px >> (8 * c)) & 255u);
  }
}

template <int C, int TH, int TW>
__global__ __launch_bounds__(256) void rdist_tile_kernel(RdArgs a) {
#pragma clang fp contract(off)
  constexpr int K2 = RR_DISTORT_KMAX * RR_DISTORT_KMAX;
  constexpr int PS = TilePix<C>::PS;
  using Pix = typename TilePix<C>::type;
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
  if (t < 64) list_taps(d.taps + (long long)(d.tap_idx ? d.tap_idx[img] : img) * K2, k, t, tv, ti, &ntaps);
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
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    tap_sum<C>(simg + ly * pw + lx, pw, nt, tv, ti, s);
    const long long le = ((long long)(y0 + ly) * r.w + (x0 + lx)) * C;
    blur_store(d, p, eb + le, dst + le, s);
  }
}

// --------------------------------------- single distortions, ragged ----
// The offline generators 02_gen_noise.py, 03_gen_blur.py and 04_gen_fog.py as
// they spell their arithmetic -- which is not 14's -- and 13:33-56's three
// steps, one kind per call for a whole ragged batch at native size:
//   noise 02:18-26: fp64 from image / 255, clip(x + nz, low, 1) * 255, then
//     np.uint8: truncation toward zero and a wrap modulo 256 (-3.7 -> 253).
//     02:21's `out.min() < 0` picks low = -1 or 0, but when no element is
//     negative the lower clip is inert either way, so clip(out, -1, 1) IS the
//     reference's result for every image: no reduction.  13:37 clips at 0:
//     the caller's `b`.
//   fog 04:17-30 / 13:50-56: clip((x * t + A (1 - t)) * 255, 0, 255) in fp64.
//   blur 03:17-30 / 13:40-48: filter2D of the raw bytes (rdist_tile_kernel's
//     tap sum on a staged tile), and with `stretch` 03:29's cv2.normalize(...,
//     0, 255, NORM_MINMAX) behind it: the minimum and maximum of the blurred
//     bytes of the WHOLE image over all channels, scale and shift in fp64,
//     convertTo's saturate(rintf(v * (float)scale + (float)shift)).
// Launches: rsingle_prologue_kernel (elem_base), one tile kernel, and for the
// blur rsingle_stretch_kernel on the same grid.  The blur kernel leaves one
// (min, max) record per tile it computed in the workspace; a stretch workgroup
// reduces the records of its image's own tiles -- counted from the record's h
// and w, so only what this call wrote is read and the workspace needs no
// initialisation -- and rescales its tile of `out` in place.  Integer min and
// max: no order, no atomics.
struct RsRange { int lo, hi; };
struct RsArgs {
  int n, kind, max_h, max_w;
  const uint8_t *in;
  uint8_t *out;
  const rr_single_param *prm;
  const float *taps;                    // [n][RR_DISTORT_KMAX^2], blur
  const double *noise;                  // packed in elem_base order, or null -> Philox
  unsigned long long seed;
  const rr_ragged_image *tab;
  long long in_bytes;
  long long *elem_base;                 // [n], workspace
  RsRange *range;                       // [n][tiles_y * tiles_x], workspace
  int tiles_y, tiles_x;                 // tiles of a max_h x max_w image
};
constexpr int RS_T = 32;                // the tile side

__device__ __forceinline__ bool rs_valid(const rr_ragged_image &r, const rr_single_param &p, int kind, int c,
                                         int max_h, int max_w, long long in_bytes) {
  if (kind == RR_SINGLE_BLUR && (p.ksize < 1 || p.ksize > RR_DISTORT_KMAX)) return false;
  return rg_valid(r, c, max_h, max_w, in_bytes);
}

// a workgroup's image and tile: false for an invalid record or a tile outside
// its image (uniform over the workgroup: return before any barrier)
struct RsTile { int img, y0, x0, th, tw; };
__device__ __forceinline__ bool rs_tile(const RsArgs &a, int c, const rr_ragged_image &r, const rr_single_param &p,
                                        RsTile *q) {
  q->y0 = ((blockIdx.x % (a.tiles_y * a.tiles_x)) / a.tiles_x) * RS_T;
  q->x0 = ((blockIdx.x % (a.tiles_y * a.tiles_x)) % a.tiles_x) * RS_T;
  if (!rs_valid(r, p, a.kind, c, a.max_h, a.max_w, a.in_bytes) || q->y0 >= r.h || q->x0 >= r.w) return false;
  q->th = r.h - q->y0 < RS_T ? r.h - q->y0 : RS_T;
  q->tw = r.w - q->x0 < RS_T ? r.w - q->x0 : RS_T;
  return true;
}

// min / max over the workgroup's 256 threads: a wave butterfly, the four waves
// through LDS; every thread gets the result (red: 8 ints, one barrier)
__device__ __forceinline__ void rs_group_range(int &lo, int &hi, int *red) {
  for (int o = 32; o > 0; o >>= 1) {
    const int l = __shfl_xor(lo, o, 64), h = __shfl_xor(hi, o, 64);
    lo = l < lo ? l : lo;
    hi = h > hi ? h : hi;
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) {
    red[t >> 6] = lo;
    red[4 + (t >> 6)] = hi;
  }
  __syncthreads();
  for (int u = 0; u < 4; ++u) {
    lo = red[u] < lo ? red[u] : lo;
    hi = red[4 + u] > hi ? red[4 + u] : hi;
  }
}

__global__ __launch_bounds__(256) void rsingle_prologue_kernel(RsArgs a, int c) {
  elem_base_scan(a.n, a.elem_base, [&](int i) -> long long {
    const rr_ragged_image r = a.tab[i];
    return rs_valid(r, a.prm[i], a.kind, c, a.max_h, a.max_w, a.in_bytes) ? (long long)r.h * r.w * c : 0;
  });
}

// noise and fog: per element, the tile's bytes row by row
template <int KIND>
__global__ __launch_bounds__(256) void rsingle_point_kernel(RsArgs a, int c) {
#pragma clang fp contract(off)
  const int img = blockIdx.x / (a.tiles_y * a.tiles_x);
  const rr_ragged_image r = a.tab[img];
  const rr_single_param p = a.prm[img];
  RsTile q;
  if (!rs_tile(a, c, r, p, &q)) return;
  const long long eb = a.elem_base[img];
  const uint8_t *src = a.in + r.offset;
  uint8_t *dst = a.out + r.offset;
  const int rowb = q.tw * c;
  for (int i = threadIdx.x; i < q.th * rowb; i += 256) {
    const int ly = i / rowb;
    const long long le = ((long long)(q.y0 + ly) * r.w + q.x0) * c + (i - ly * rowb);
    const double x = (double)src[le] / 255.0;
    if (KIND == RR_SINGLE_NOISE) {
      const double nz = a.noise ? a.noise[eb + le] : p.a * philox_normal(a.seed, (unsigned long long)(eb + le));
      double v = x + nz;
      v = v < p.b ? p.b : (v > 1.0 ? 1.0 : v);               // np.clip(out, low_clip, 1.0)
      dst[le] = (uint8_t)(int)(v * 255.0);                   // np.uint8: toward zero, then modulo 256
    } else {
      dst[le] = trunc_u8((x * p.a + p.b) * 255.0);
    }
  }
}

template <int C>
__global__ __launch_bounds__(256) void rsingle_blur_kernel(RsArgs a) {
#pragma clang fp contract(off)
  constexpr int K2 = RR_DISTORT_KMAX * RR_DISTORT_KMAX;
  constexpr int PS = TilePix<C>::PS;
  using Pix = typename TilePix<C>::type;
  __shared__ Pix simg[(RS_T + RR_DISTORT_KMAX - 1) * (RS_T + RR_DISTORT_KMAX - 1)];
  __shared__ float tv[K2];
  __shared__ int ti[K2];
  __shared__ int ntaps;
  __shared__ int red[8];
  const int t = threadIdx.x;
  const int img = blockIdx.x / (a.tiles_y * a.tiles_x);
  const rr_ragged_image r = a.tab[img];
  const rr_single_param p = a.prm[img];
  RsTile q;
  if (!rs_tile(a, C, r, p, &q)) return;
  const uint8_t *src = a.in + r.offset;
  uint8_t *dst = a.out + r.offset;
  const int k = p.ksize, anc = k / 2;
  if (t < 64) list_taps(a.taps + (long long)img * K2, k, t, tv, ti, &ntaps);
  // the raw source bytes of the tile and its halo, each at its reflected place
  const int pw = q.tw + k - 1, nr = q.th + k - 1, rowb = pw * C;
  for (int e = t; e < nr * rowb; e += 256) {
    const int ry = e / rowb, rest = e - ry * rowb;
    const int cx = rest / C, ch = rest - cx * C;
    const int yy = reflect101(q.y0 - anc + ry, r.h), xx = reflect101(q.x0 - anc + cx, r.w);
    ((uint8_t *)simg)[(ry * pw + cx) * PS + ch] = src[((long long)yy * r.w + xx) * C + ch];
  }
  __syncthreads();
  const int nt = ntaps;
  int lo = 255, hi = 0;
  for (int i = t; i < q.th * q.tw; i += 256) {
    const int ly = i / q.tw, lx = i - ly * q.tw;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    tap_sum<C>(simg + ly * pw + lx, pw, nt, tv, ti, s);
    const long long le = ((long long)(q.y0 + ly) * r.w + (q.x0 + lx)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v = rintf(s[c]);                                 // saturate_cast<uchar>: cvRound
      v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
      const int b = (int)v;
      dst[le + c] = (uint8_t)b;
      lo = b < lo ? b : lo;
      hi = b > hi ? b : hi;
    }
  }
  if (!p.stretch) return;                                    // uniform
  rs_group_range(lo, hi, red);
  if (t == 0) a.range[blockIdx.x] = RsRange{lo, hi};
}

// 03:29 behind the blur: cv2.normalize(blurred, blurred, 0, 255, NORM_MINMAX)
__global__ __launch_bounds__(256) void rsingle_stretch_kernel(RsArgs a, int c) {
#pragma clang fp contract(off)
  __shared__ int red[8];
  const int tiles = a.tiles_y * a.tiles_x, img = blockIdx.x / tiles;
  const rr_ragged_image r = a.tab[img];
  const rr_single_param p = a.prm[img];
  RsTile q;
  if (!p.stretch || !rs_tile(a, c, r, p, &q)) return;
  const int ny = (r.h - 1) / RS_T + 1, nx = (r.w - 1) / RS_T + 1;   // the image's own tiles
  const RsRange *rec = a.range + (long long)img * tiles;
  int lo = 255, hi = 0;
  for (int j = threadIdx.x; j < ny * nx; j += 256) {
    const RsRange g = rec[(j / nx) * a.tiles_x + j % nx];
    lo = g.lo < lo ? g.lo : lo;
    hi = g.hi > hi ? g.hi : hi;
  }
  rs_group_range(lo, hi, red);
  const double span = (double)(hi - lo);
  const double scale = 255.0 * (span > DBL_EPSILON ? 1.0 / span : 0.0), shift = 0.0 - (double)lo * scale;
  const float fs = (float)scale, fb = (float)shift;          // convertTo works in fp32
  uint8_t *dst = a.out + r.offset;
  const int rowb = q.tw * c;
  for (int i = threadIdx.x; i < q.th * rowb; i += 256) {
    const int ly = i / rowb;
    const long long le = ((long long)(q.y0 + ly) * r.w + q.x0) * c + (i - ly * rowb);
    float v = rintf((float)dst[le] * fs + fb);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    dst[le] = (uint8_t)(int)v;
  }
}

// where a random variant keeps its draws in its workspace: the n params, the n
// table indices, the step's noise seed
struct DrawPlan { size_t off_prm, off_idx, off_seed, total; };
static size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// workspace of rr_distort_random_u8: the blur staging image, then the draws.
// No argument check: its three users each have their own
static DrawPlan draw_plan(int n, int h, int w, int c) {
  DrawPlan p;
  p.off_prm = al16((size_t)n * h * w * c);
  p.off_idx = p.off_prm + (size_t)n * sizeof(rr_distort_param);
  p.off_seed = p.off_idx + al16((size_t)n * sizeof(int));
  p.total = p.off_seed + 16;
  return p;
}

// workspace of both ragged entry points: elem_base[n], then the random
// variant's draws in rr_distort_random_u8's order.  No image-sized term:
// nothing is staged in HBM.
static int rd_plan(int n, int c, int max_h, int max_w, DrawPlan *p) {
  if (n <= 0 || c < 1 || c > 4 || max_h < 1 || max_w < 1) return RR_EINVAL;
  p->off_prm = al16((size_t)n * sizeof(long long));
  p->off_idx = al16(p->off_prm + (size_t)n * sizeof(rr_distort_param));
  p->off_seed = al16(p->off_idx + (size_t)n * sizeof(int));
  p->total = p->off_seed + 16;
  return RR_OK;
}

// the answer of the two *_draws queries
static int draw_offsets(const DrawPlan &p, size_t *prm_off, size_t *idx_off, size_t *seed_off) {
  *prm_off = p.off_prm;
  *idx_off = p.off_idx;
  *seed_off = p.off_seed;
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

// the body of both ragged entry points.  draw: the prologue draws params and
// table indices of (seed, *step) into the workspace, the noise seed beside
// them, and taps is the table of all kernels; else all three are the caller's
static int rd_run(bool draw, int n, int c, int mode, int max_h, int max_w, const uint8_t *in, size_t in_bytes,
                  const rr_ragged_image *images_dev, uint8_t *out, const rr_distort_param *params,
                  const float *taps, const int *tap_idx, const double *noise, unsigned long long seed,
                  long long *step, void *ws, size_t ws_bytes, rr_stream stream) {
  DrawPlan p;
  if (!in || !images_dev || !out || !taps || !ws || in == out) return RR_EINVAL;   // halo reads: not in place
  if (draw ? !step : !params) return RR_EINVAL;
  if (!rg_bytes_ok(in_bytes) || (mode != 0 && mode != 1)) return RR_EINVAL;
  if (const int rc = rd_plan(n, c, max_h, max_w, &p)) return rc;
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  char *base = (char *)ws;
  rr_distort_param *prm_out = draw ? (rr_distort_param *)(base + p.off_prm) : nullptr;
  int *idx_out = draw ? (int *)(base + p.off_idx) : nullptr;
  unsigned long long *nseed = draw ? (unsigned long long *)(base + p.off_seed) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  RdArgs a{DistCfg{n, max_h, max_w, c, mode, in, out, nullptr, draw ? prm_out : params, taps, noise,
                   draw ? 0ull : seed, draw ? idx_out : tap_idx, nseed},
           images_dev, (long long)in_bytes, (long long *)ws, 0, 0};
  hipLaunchKernelGGL(rdist_prologue_kernel, dim3(1), dim3(256), 0, st, a, (int)draw, draw ? seed : 0ull, step,
                     prm_out, idx_out, nseed);
  RR_CHECK_LAUNCH();
  return rd_launch(a, c, max_h, max_w, rr_path_read().rdist_tile, st);
}

// workspace of rr_distort_single_ragged_u8: elem_base[n], then one RsRange per
// (image, tile of a max_h x max_w image); *groups: the workgroups of the tile
// grid, which is the launch's limit
static int rs_plan(int n, int c, int max_h, int max_w, size_t *off_range, size_t *total, long long *groups) {
  if (n <= 0 || c < 1 || c > 4 || max_h < 1 || max_w < 1) return RR_EINVAL;
  const long long tiles = (long long)((max_h - 1) / RS_T + 1) * ((max_w - 1) / RS_T + 1);
  if (tiles > ((1LL << 31) - 1) / n) return RR_EUNSUPPORTED;
  *groups = tiles * n;
  *off_range = al16((size_t)n * sizeof(long long));
  *total = *off_range + (size_t)*groups * sizeof(RsRange);
  return RR_OK;
}

}  // namespace

extern "C" size_t rr_distort_workspace(int n, int h, int w, int c) {
  return n > 0 && h > 0 && w > 0 && c > 0 ? (size_t)n * h * w * c : 0;
}

extern "C" int rr_distort_u8(int n, int h, int w, int c, int mode, const uint8_t *in, uint8_t *out,
                             const rr_distort_param *params, const float *taps, const double *noise,
                             unsigned long long seed, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!in || !out || !params || !taps || !ws || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (c < 1 || c > 4 || (mode != 0 && mode != 1)) return RR_EINVAL;
  if (ws_bytes < rr_distort_workspace(n, h, w, c)) return RR_EWORKSPACE;
  return dist_launch(DistCfg{n, h, w, c, mode, in, out, (uint8_t *)ws, params, taps, noise, seed, nullptr, nullptr},
                     (hipStream_t)stream);
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

extern "C" size_t rr_distort_random_workspace(int n, int h, int w, int c) {
  return n > 0 && h > 0 && w > 0 && c > 0 ? draw_plan(n, h, w, c).total : 0;
}

extern "C" int rr_distort_random_u8(int n, int h, int w, int c, const uint8_t *in, uint8_t *out,
                                    unsigned long long seed, long long *step, const float *table,
                                    void *ws, size_t ws_bytes, rr_stream stream) {
  if (!in || !out || !step || !table || !ws || n <= 0 || h <= 0 || w <= 0) return RR_EINVAL;
  if (c < 1 || c > 4) return RR_EINVAL;
  const DrawPlan p = draw_plan(n, h, w, c);
  if (ws_bytes < p.total) return RR_EWORKSPACE;
  char *base = (char *)ws;
  rr_distort_param *prm = (rr_distort_param *)(base + p.off_prm);
  int *tap_idx = (int *)(base + p.off_idx);
  unsigned long long *nseed = (unsigned long long *)(base + p.off_seed);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(distort_draw_kernel, dim3(1), dim3(256), 0, st, n, seed, step, prm, tap_idx, nseed);
  RR_CHECK_LAUNCH();
  return dist_launch(DistCfg{n, h, w, c, 0, in, out, (uint8_t *)ws, prm, table, nullptr, 0ull, tap_idx, nseed}, st);
}

// where the last rr_distort_random_u8 call left its draws in its workspace
// (tests): params [n], tap indices [n], noise seed
extern "C" int rr_distort_random_draws(int n, int h, int w, int c, const void *ws,
                                       size_t *prm_off, size_t *idx_off, size_t *seed_off) {
  if (!ws || n <= 0 || !prm_off || !idx_off || !seed_off) return RR_EINVAL;
  return draw_offsets(draw_plan(n, h, w, c), prm_off, idx_off, seed_off);
}

// ------------------------------------------- ragged distortion: C ABI ----
extern "C" size_t rr_distort_ragged_workspace(int n, int c, int max_h, int max_w) {
  DrawPlan p;
  return rd_plan(n, c, max_h, max_w, &p) == RR_OK ? p.total : 0;
}

extern "C" int rr_distort_ragged_u8(int n, int c, int mode, int max_h, int max_w, const uint8_t *in,
                                    size_t in_bytes, const rr_ragged_image *images_dev, uint8_t *out,
                                    const rr_distort_param *params, const float *taps, const int *tap_idx,
                                    const double *noise, unsigned long long seed, void *ws, size_t ws_bytes,
                                    rr_stream stream) {
  return rd_run(false, n, c, mode, max_h, max_w, in, in_bytes, images_dev, out, params, taps, tap_idx, noise,
                seed, nullptr, ws, ws_bytes, stream);
}

extern "C" int rr_distort_random_ragged_u8(int n, int c, int max_h, int max_w, const uint8_t *in,
                                           size_t in_bytes, const rr_ragged_image *images_dev, uint8_t *out,
                                           unsigned long long seed, long long *step, const float *table,
                                           void *ws, size_t ws_bytes, rr_stream stream) {
  return rd_run(true, n, c, 0, max_h, max_w, in, in_bytes, images_dev, out, nullptr, table, nullptr, nullptr,
                seed, step, ws, ws_bytes, stream);
}

// the same for rr_distort_random_ragged_u8
extern "C" int rr_distort_random_ragged_draws(int n, int c, int max_h, int max_w, const void *ws,
                                              size_t *prm_off, size_t *idx_off, size_t *seed_off) {
  DrawPlan p;
  if (!ws || !prm_off || !idx_off || !seed_off) return RR_EINVAL;
  if (const int rc = rd_plan(n, c, max_h, max_w, &p)) return rc;
  return draw_offsets(p, prm_off, idx_off, seed_off);
}

// ------------------------------------------ single distortions: C ABI ----
extern "C" size_t rr_distort_single_ragged_workspace(int n, int c, int max_h, int max_w) {
  size_t off, total;
  long long groups;
  return rs_plan(n, c, max_h, max_w, &off, &total, &groups) == RR_OK ? total : 0;
}

extern "C" int rr_distort_single_ragged_u8(int n, int c, int kind, int max_h, int max_w, const uint8_t *in,
                                           size_t in_bytes, const rr_ragged_image *images_dev, uint8_t *out,
                                           const rr_single_param *params, const float *taps, const double *noise,
                                           unsigned long long seed, void *ws, size_t ws_bytes, rr_stream stream) {
  size_t off, total;
  long long groups;
  if (!in || !images_dev || !out || !params || !ws || in == out) return RR_EINVAL;   // halo reads: not in place
  if (kind != RR_SINGLE_NOISE && kind != RR_SINGLE_BLUR && kind != RR_SINGLE_FOG) return RR_EINVAL;
  if ((kind == RR_SINGLE_BLUR && !taps) || !rg_bytes_ok(in_bytes)) return RR_EINVAL;
  if (const int rc = rs_plan(n, c, max_h, max_w, &off, &total, &groups)) return rc;
  if (ws_bytes < total) return RR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  RsArgs a{n, kind, max_h, max_w, in, out, params, taps, noise, seed, images_dev, (long long)in_bytes,
           (long long *)ws, (RsRange *)((char *)ws + off), (max_h - 1) / RS_T + 1, (max_w - 1) / RS_T + 1};
  const dim3 grid((unsigned)groups), block(256);
  hipLaunchKernelGGL(rsingle_prologue_kernel, dim3(1), block, 0, st, a, c);
  RR_CHECK_LAUNCH();
  if (kind == RR_SINGLE_NOISE) {
    hipLaunchKernelGGL(rsingle_point_kernel<RR_SINGLE_NOISE>, grid, block, 0, st, a, c);
  } else if (kind == RR_SINGLE_FOG) {
    hipLaunchKernelGGL(rsingle_point_kernel<RR_SINGLE_FOG>, grid, block, 0, st, a, c);
  } else {
    const int rc = rr_dispatch_int<1, 2, 3, 4>(c, [&](auto cc) {
      hipLaunchKernelGGL(rsingle_blur_kernel<decltype(cc)::value>, grid, block, 0, st, a);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
    if (rc) return rc;
    // the images with `stretch` are known on the device only: the launch is
    // made whatever the table says, and a workgroup without one leaves at once
    hipLaunchKernelGGL(rsingle_stretch_kernel, grid, block, 0, st, a, c);
  }
  RR_CHECK_LAUNCH();
  return RR_OK;
}
