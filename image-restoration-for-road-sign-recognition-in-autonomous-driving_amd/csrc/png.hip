// png.hip -- PNG input, device half: undo the row filters of a whole batch of
// inflated PNG images and write them as packed RGB, as
// Image.open(p).convert('RGB') gives them (17_run_unified_inference.py:69-79,
// 18_test_unified_benchmark.py:35, 07_train_restoration.py:52-66,
// 08_run_inference.py:84-88).  The host half (png.cpp) reads and inflates the
// files; the output is the buffer rr_resize_ragged_u8 consumes.
//
// Structure: one 64-lane wave per image, a skewed wavefront over bands of 64
// rows.  Lane l owns row 64 k + l of band k and at step t reconstructs pixel
// x = t - l, all channels packed in one dword (independent chains).  The three
// neighbours of PNG spec section 9 are then all one step old:
//   a (left)        the lane's own previous result,
//   b (above)       what lane l - 1 produced one step earlier: one __shfl_up,
//   c (upper left)  the lane's previous b.
// A band takes w + rows - 1 steps whatever its filters are.  The row above a
// band's first row is the last row of the previous band: lane 63 leaves its
// pixels in an LDS row (4 bytes per pixel), lane 0 of the next band reads b
// from there.  The wave runs its bands one after the other, so within a band
// lane 63 writes entry t - 63 while lane 0 reads entry t: the write trails the
// read, one row is enough, and the barrier between bands orders the rest.
// LDS bounds the width: 8192 pixels (32 KiB).
//
// Filtered bytes are read a dword at a time per lane (the two aligned dwords
// around the lane's byte position are kept and a pixel is cut out of them;
// rows start at any byte offset); the first and last partial dword of the
// buffer are read by bytes.
#include "common.h"

namespace {

constexpr int PU_LANES = 64;
constexpr int PU_MAX_W = 8192;             // LDS row of packed pixels: 32 KiB

// the table check, host and device: every range in 64-bit, by division
__host__ __device__ inline bool pu_valid(const rr_png_image &r, int max_h, int max_w,
                                         long long in_bytes, long long out_bytes) {
  if (r.h < 1 || r.h > max_h || r.w < 1 || r.w > max_w) return false;
  if (r.channels < 1 || r.channels > 4 || (r.kind != 0 && r.kind != 1)) return false;
  if (r.src < 0 || r.src > in_bytes || r.dst < 0 || r.dst > out_bytes) return false;
  const long long pitch = r.kind + (long long)r.w * r.channels;      // < 2^34
  if (r.h > (in_bytes - r.src) / pitch) return false;
  return (long long)r.h * r.w <= (out_bytes - r.dst) / 3;
}

// reader over the buffer [lo, hi) that fetches aligned dwords: the two dwords
// around the lane's position are kept, a pixel is cut out of them, and moving
// on by one dword costs one load
struct PuReader {
  const uint8_t *lo, *hi;
  uintptr_t w_lo, w_hi;        // aligned dwords wholly inside [lo, hi)
  uintptr_t cur;               // address of the cached low dword (0: none)
  uint32_t word, next;         // the dwords at cur and cur + 4

  __device__ PuReader(const uint8_t *base, long long bytes)
      : lo(base), hi(base + bytes), cur(0), word(0), next(0) {
    w_lo = ((uintptr_t)lo + 3) & ~(uintptr_t)3;
    w_hi = (uintptr_t)hi & ~(uintptr_t)3;
  }
  __device__ __forceinline__ uint32_t load(uintptr_t wa) const {
    if (wa >= w_lo && wa + 4 <= w_hi) return *(const uint32_t *)wa;
    uint32_t v = 0;                             // the buffer's ragged ends by bytes; past them: zeros
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t *q = (const uint8_t *)wa + i;
      if (q >= lo && q < hi) v |= (uint32_t)*q << (8 * i);
    }
    return v;
  }
  // the C bytes at p, low byte first
  template <int C> __device__ __forceinline__ uint32_t get(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p, wa = a & ~(uintptr_t)3;
    if (wa != cur) {
      const bool step = wa == cur + 4;
      const uint32_t keep = next;
      next = load(wa + 4);
      word = step ? keep : load(wa);
      cur = wa;
    }
    const uint64_t v = ((uint64_t)next << 32) | word;
    return (uint32_t)(v >> (8 * (a & 3))) & (C == 4 ? 0xffffffffu : (1u << (8 * C)) - 1u);
  }
};

__device__ __forceinline__ int pu_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);       // ties: a, b, c (png.cpp paeth)
}

// one pixel: C channels packed low byte first
template <int C>
__device__ __forceinline__ uint32_t pu_recon(int ft, uint32_t raw, uint32_t pa, uint32_t pb, uint32_t pc) {
  uint32_t o = 0;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const int x = (raw >> (8 * ch)) & 255, a = (pa >> (8 * ch)) & 255, b = (pb >> (8 * ch)) & 255,
              c = (pc >> (8 * ch)) & 255;
    int pred = 0;
    if (ft == 1) pred = a;
    else if (ft == 2) pred = b;
    else if (ft == 3) pred = (a + b) >> 1;                      // 9-bit sum
    else if (ft == 4) pred = pu_paeth(a, b, c);
    o |= (uint32_t)((x + pred) & 255) << (8 * ch);
  }
  return o;
}

// convert('RGB'): grey replicated, alpha dropped, RGB copied
template <int C> __device__ __forceinline__ void pu_store_rgb(uint8_t *o, uint32_t px) {
  if (C <= 2) {
    o[0] = o[1] = o[2] = (uint8_t)px;
  } else {
    o[0] = (uint8_t)px;
    o[1] = (uint8_t)(px >> 8);
    o[2] = (uint8_t)(px >> 16);
  }
}

template <int C>
__device__ void pu_unfilter_image(long long src, long long dst, int h, int w, const uint8_t *in,
                                  long long in_bytes, uint8_t *out, uint32_t *carry) {
  PuReader rd(in, in_bytes);                            // local, and the record by value: registers
  const int lane = threadIdx.x;
  const long long pitch = 1 + (long long)w * C;
  for (long long row0 = 0; row0 < h; row0 += PU_LANES) {
    const int rows = (int)(h - row0 < PU_LANES ? h - row0 : PU_LANES);
    const bool active = lane < rows;
    const long long row = row0 + lane;
    const uint8_t *rp = in + src + row * pitch;       // the row's filter byte (active lanes)
    uint8_t *op = out + dst + row * w * 3;
    const int ft = active ? (int)rd.template get<1>(rp) : 0;
    uint32_t prev = 0, up_prev = 0;
    const int steps = w + rows - 1;
    for (int t = 0; t < steps; ++t) {
      uint32_t up = __shfl_up(prev, 1);                 // every lane, every step
      if (lane == 0) up = (row0 > 0 && t < w) ? carry[t] : 0u;
      const int x = t - lane;
      uint32_t cur = 0;
      if (active && x >= 0 && x < w) {
        const uint32_t raw = rd.template get<C>(rp + 1 + (long long)x * C);
        cur = pu_recon<C>(ft, raw, x ? prev : 0u, up, x ? up_prev : 0u);
        pu_store_rgb<C>(op + (long long)x * 3, cur);
        if (lane == PU_LANES - 1) carry[x] = cur;       // the next band's row above
      }
      up_prev = up;
      prev = cur;
    }
    __syncthreads();                                    // carry complete before the next band reads it
  }
}

template <int C>
__device__ void pu_copy_image(long long np, const uint8_t *src, uint8_t *dst) {
  for (long long i = threadIdx.x; i < np; i += PU_LANES) {
    uint32_t px = 0;
#pragma unroll
    for (int ch = 0; ch < (C <= 2 ? 1 : 3); ++ch) px |= (uint32_t)src[i * C + ch] << (8 * ch);
    pu_store_rgb<C>(dst + i * 3, px);
  }
}

__global__ __launch_bounds__(PU_LANES) void png_unfilter_kernel(int max_h, int max_w,
                                                                const uint8_t *__restrict__ in,
                                                                long long in_bytes,
                                                                const rr_png_image *__restrict__ images,
                                                                uint8_t *__restrict__ out,
                                                                long long out_bytes) {
  extern __shared__ uint32_t pu_carry[];                // max_w packed pixels
  const rr_png_image r = images[blockIdx.x];
  if (!pu_valid(r, max_h, max_w, in_bytes, out_bytes)) return;       // the whole wave: no read, no write
  if (r.kind == 0) {
    switch (r.channels) {
      case 1: pu_copy_image<1>((long long)r.h * r.w, in + r.src, out + r.dst); break;
      case 2: pu_copy_image<2>((long long)r.h * r.w, in + r.src, out + r.dst); break;
      case 3: pu_copy_image<3>((long long)r.h * r.w, in + r.src, out + r.dst); break;
      default: pu_copy_image<4>((long long)r.h * r.w, in + r.src, out + r.dst); break;
    }
    return;
  }
  switch (r.channels) {
    case 1: pu_unfilter_image<1>(r.src, r.dst, r.h, r.w, in, in_bytes, out, pu_carry); break;
    case 2: pu_unfilter_image<2>(r.src, r.dst, r.h, r.w, in, in_bytes, out, pu_carry); break;
    case 3: pu_unfilter_image<3>(r.src, r.dst, r.h, r.w, in, in_bytes, out, pu_carry); break;
    default: pu_unfilter_image<4>(r.src, r.dst, r.h, r.w, in, in_bytes, out, pu_carry); break;
  }
}

}  // namespace

extern "C" int rr_png_table_check(int n, size_t in_bytes, size_t out_bytes,
                                  const rr_png_image *images_host, int max_h, int max_w) {
  if (!images_host || n <= 0 || max_h <= 0 || max_w <= 0) return RR_EINVAL;
  if (in_bytes > (size_t)INT64_MAX || out_bytes > (size_t)INT64_MAX) return RR_EINVAL;
  if (max_w > PU_MAX_W) return RR_EUNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!pu_valid(images_host[i], max_h, max_w, (long long)in_bytes, (long long)out_bytes)) return RR_EINVAL;
  return RR_OK;
}

extern "C" int rr_png_unfilter(int n, int max_h, int max_w, const uint8_t *in, size_t in_bytes,
                               const rr_png_image *images_dev, uint8_t *out, size_t out_bytes,
                               rr_stream stream) {
  if (n <= 0 || max_h <= 0 || max_w <= 0 || !in || !images_dev || !out) return RR_EINVAL;
  if (in_bytes == 0 || out_bytes == 0 || in_bytes > (size_t)INT64_MAX || out_bytes > (size_t)INT64_MAX)
    return RR_EINVAL;
  if (max_w > PU_MAX_W) return RR_EUNSUPPORTED;
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(PU_LANES), (size_t)max_w * 4,
                     (hipStream_t)stream, max_h, max_w, in, (long long)in_bytes, images_dev, out,
                     (long long)out_bytes);
  RR_CHECK_LAUNCH();
  return RR_OK;
}
