// pool.hip -- pooling and resizing of NHWC activations (gfx950).
//
//  * MaxPool2d(2, 2) fwd with 1-byte argmax, gather-form bwd, 4- and 8-channel
//    kernels, bwd from the pooled values (07:81, 14:125)
//  * AdaptiveAvgPool2d(7) + flatten (VGG16 classifier input)
//  * F.interpolate 'nearest' fwd / bwd (ResUNet skip alignment, 14:169-182)
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
template <typename T>
__global__ void maxpool_fwd_kernel(int n, int h, int w, int C, const T *__restrict__ x,
                                   T *__restrict__ y, uint8_t *__restrict__ idx) {
  const int ho = h / 2, wo = w / 2;
  const int G = C / 4;
  const long long total = (long long)n * ho * wo * G;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const long long op = i / G;
    const int ox = (int)(op % wo);
    const long long t = op / wo;
    const int oy = (int)(t % ho);
    const int nn = (int)(t / ho);
    const long long base = (((long long)nn * h + 2 * oy) * w + 2 * ox) * C + g * 4;
    f32x4 m = load4<T>(x + base);
    uint8_t id[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const long long off = base + ((long long)(k >> 1) * w + (k & 1)) * C;
      const f32x4 v = load4<T>(x + off);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (v[c] > m[c] || (v[c] != v[c] && m[c] == m[c])) { m[c] = v[c]; id[c] = (uint8_t)k; }
    }
    store4<T>(y + op * C + g * 4, m);
    *reinterpret_cast<uchar4 *>(idx + op * C + g * 4) = make_uchar4(id[0], id[1], id[2], id[3]);
  }
}

// 8-channel forms (C % 8 == 0, < 2^31 elements): 16-B accesses, 32-bit
// index math; same routing (first max in window order) and NaN rule
template <typename T>
__global__ void maxpool_fwd8_kernel(int n, int h, int w, int C, const T *__restrict__ x,
                                    T *__restrict__ y, uint8_t *__restrict__ idx) {
  const int ho = h / 2, wo = w / 2, G = C / 8;
  const int total = n * ho * wo * G;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int g = i % G, op = i / G;
    const int ox = op % wo, t = op / wo, oy = t % ho, nn = t / ho;
    const long long base = (((long long)nn * h + 2 * oy) * w + 2 * ox) * C + g * 8;
    f32x4 a0, a1;
    load8<T>(x + base, a0, a1);
    float m[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    uint8_t id[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      f32x4 v0, v1;
      load8<T>(x + base + ((long long)(k >> 1) * w + (k & 1)) * C, v0, v1);
      const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (v[c] > m[c] || (v[c] != v[c] && m[c] == m[c])) { m[c] = v[c]; id[c] = (uint8_t)k; }
    }
    store8<T>(y + (long long)op * C + g * 8, f32x4{m[0], m[1], m[2], m[3]}, f32x4{m[4], m[5], m[6], m[7]});
    *reinterpret_cast<uint2 *>(idx + (long long)op * C + g * 8) =
        uint2{(uint32_t)id[0] | ((uint32_t)id[1] << 8) | ((uint32_t)id[2] << 16) | ((uint32_t)id[3] << 24),
              (uint32_t)id[4] | ((uint32_t)id[5] << 8) | ((uint32_t)id[6] << 16) | ((uint32_t)id[7] << 24)};
  }
}

template <typename T>
__global__ void maxpool_bwd8_kernel(int n, int h, int w, int C, const T *__restrict__ dy,
                                    const uint8_t *__restrict__ idx, T *__restrict__ dx,
                                    int accumulate, const T *__restrict__ mask) {
  const int ho = h / 2, wo = w / 2, G = C / 8;
  const int total = n * h * w * G;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int g = i % G, p = i / G;
    const int xx = p % w, t = p / w, yy = t % h, nn = t / h;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int oy = yy >> 1, ox = xx >> 1;
    if (oy < ho && ox < wo) {
      const long long o = ((long long)(nn * ho + oy) * wo + ox) * C + g * 8;
      const uint2 id = *reinterpret_cast<const uint2 *>(idx + o);
      const int k = (yy & 1) * 2 + (xx & 1);
      f32x4 d0, d1;
      load8<T>(dy + o, d0, d1);
      const float d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = (int)(((j < 4 ? id.x : id.y) >> (8 * (j & 3))) & 0xff) == k ? d[j] : 0.f;
    }
    const long long e = (long long)p * C + g * 8;
    if (accumulate) {
      f32x4 a0, a1;
      load8<T>(dx + e, a0, a1);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] += a0[j]; v[j + 4] += a1[j]; }
    }
    if (mask) {
      f32x4 m0, m1;
      load8<T>(mask + e, m0, m1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = m0[j] > 0.f ? v[j] : 0.f;
        v[j + 4] = m1[j] > 0.f ? v[j + 4] : 0.f;
      }
    }
    store8<T>(dx + e, f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
  }
}

// MaxPool2d(2, 2) backward of a pool whose input is a ReLU output (the
// perceptual VGG slice: conv + ReLU + MaxPool2d, 14:189-196): the ReLU mask
// at a window's argmax is (pooled value > 0) -- the max IS that element --
// and every other element of the window gets 0 anyway, so the mask comes
// from the pooled forward output yp instead of the full-size activation
// (a quarter of the bytes).  Scatter form: one thread per pooled pixel x 8
// channels writes its whole window (h, w even).  Bitwise the gather form of
// maxpool_bwd8_kernel with mask = the full-size ReLU output.
template <typename T>
__global__ void maxpool_bwd8p_kernel(int n, int h, int w, int C, const T *__restrict__ dy,
                                     const uint8_t *__restrict__ idx, const T *__restrict__ yp,
                                     T *__restrict__ dx) {
  const int ho = h / 2, wo = w / 2, G = C / 8;
  const int total = n * ho * wo * G;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int g = i % G, op = i / G;
    const int ox = op % wo, t = op / wo, oy = t % ho, nn = t / ho;
    const long long o = (long long)op * C + g * 8;
    const uint2 id = *reinterpret_cast<const uint2 *>(idx + o);
    f32x4 d0, d1, m0, m1;
    load8<T>(dy + o, d0, d1);
    load8<T>(yp + o, m0, m1);
    const float d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
    const float m[8] = {m0[0], m0[1], m0[2], m0[3], m1[0], m1[1], m1[2], m1[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool at = (int)(((j < 4 ? id.x : id.y) >> (8 * (j & 3))) & 0xff) == k;
        v[j] = at && m[j] > 0.f ? d[j] : 0.f;
      }
      const long long e = (((long long)nn * h + 2 * oy + (k >> 1)) * w + 2 * ox + (k & 1)) * C + g * 8;
      store8<T>(dx + e, f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
    }
  }
}

template <typename T>
__global__ void maxpool_bwd_kernel(int n, int h, int w, int C, const T *__restrict__ dy,
                                   const uint8_t *__restrict__ idx, T *__restrict__ dx,
                                   int accumulate, const T *__restrict__ mask) {
  const int ho = h / 2, wo = w / 2;
  const int G = C / 4;
  const long long total = (long long)n * h * w * G;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const long long p = i / G;
    const int xx = (int)(p % w);
    const long long t = p / w;
    const int yy = (int)(t % h);
    const int nn = (int)(t / h);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int oy = yy >> 1, ox = xx >> 1;
    if (oy < ho && ox < wo) {
      const long long op = ((long long)nn * ho + oy) * wo + ox;
      const uchar4 id = *reinterpret_cast<const uchar4 *>(idx + op * C + g * 4);
      const uint8_t k = (uint8_t)((yy & 1) * 2 + (xx & 1));
      const f32x4 d = load4<T>(dy + op * C + g * 4);
      v[0] = id.x == k ? d[0] : 0.f;
      v[1] = id.y == k ? d[1] : 0.f;
      v[2] = id.z == k ? d[2] : 0.f;
      v[3] = id.w == k ? d[3] : 0.f;
    }
    const long long e = p * C + g * 4;
    if (accumulate) v += load4<T>(dx + e);
    if (mask) {
      const f32x4 m = load4<T>(mask + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = m[c] > 0.f ? v[c] : 0.f;
    }
    store4<T>(dx + e, v);
  }
}

// AdaptiveAvgPool2d((oh, ow)) on NHWC input -> [n][C*oh*ow] in NCHW flatten order
template <typename T>
__global__ void adaptive_avgpool_kernel(int n, int h, int w, int C, int oh, int ow,
                                        const T *__restrict__ x, T *__restrict__ y) {
  const long long total = (long long)n * C * oh * ow;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % ow);
    long long t = i / ow;
    const int oy = (int)(t % oh);
    t /= oh;
    const int c = (int)(t % C);
    const int nn = (int)(t / C);
    // torch: start = floor(o*in/out), end = ceil((o+1)*in/out)
    const int y0 = (oy * h) / oh, y1 = ((oy + 1) * h + oh - 1) / oh;
    const int x0 = (ox * w) / ow, x1 = ((ox + 1) * w + ow - 1) / ow;
    float s = 0.f;
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = x0; xx < x1; ++xx) s += Elt<T>::load(x, (((long long)nn * h + yy) * w + xx) * C + c);
    Elt<T>::store(y, i, s / (float)((y1 - y0) * (x1 - x0)));
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// F.interpolate(x, size=(ho, wo)) default mode 'nearest' (ResUNet skip
// alignment, 14:169-182): ATen's source index, output == input -> identity,
// output == 2 input -> o >> 1, else min(floorf(o * (float)in / out), in - 1)
// in fp32 (as upsample_nearest2d computes it).  NHWC, C % 4 == 0.
__device__ __forceinline__ int nearest_src(int o, int in, int out) {
  if (out == in) return o;
  if (out == 2 * in) return o >> 1;
  const float scale = (float)in / (float)out;
  const int s = (int)floorf((float)o * scale);
  return s < in - 1 ? s : in - 1;
}

template <typename T>
__global__ void nearest_fwd_kernel(int n, int hi, int wi, int ho, int wo, int C,
                                   const T *__restrict__ x, T *__restrict__ y) {
  const int G = C / 4;
  const long long total = (long long)n * ho * wo * G;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const long long op = i / G;
    const int ox = (int)(op % wo);
    const long long t = op / wo;
    const int oy = (int)(t % ho), nn = (int)(t / ho);
    const long long ip = ((long long)nn * hi + nearest_src(oy, hi, ho)) * wi + nearest_src(ox, wi, wo);
    store4<T>(y + op * C + g * 4, load4<T>(x + ip * C + g * 4));
  }
}

// backward in gather form (deterministic): dx[iy][ix] = sum of dy over the
// outputs whose source is (iy, ix), rows then columns in increasing order.
// The source index is monotone, so those outputs form a contiguous range;
// it is found by scanning a window around iy * out / in.
__device__ __forceinline__ void nearest_range(int i, int in, int out, int &lo, int &hi) {
  int o = (int)(((long long)i * out) / in) - 2;
  o = o < 0 ? 0 : o;
  while (o < out && nearest_src(o, in, out) < i) ++o;
  lo = o;
  while (o < out && nearest_src(o, in, out) == i) ++o;
  hi = o;
}

template <typename T>
__global__ void nearest_bwd_kernel(int n, int hi, int wi, int ho, int wo, int C,
                                   const T *__restrict__ dy, T *__restrict__ dx) {
  const int G = C / 4;
  const long long total = (long long)n * hi * wi * G;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % G);
    const long long ip = i / G;
    const int ix = (int)(ip % wi);
    const long long t = ip / wi;
    const int iy = (int)(t % hi), nn = (int)(t / hi);
    int y0, y1, x0, x1;
    nearest_range(iy, hi, ho, y0, y1);
    nearest_range(ix, wi, wo, x0, x1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = y0; oy < y1; ++oy)
      for (int ox = x0; ox < x1; ++ox)
        acc += load4<T>(dy + (((long long)nn * ho + oy) * wo + ox) * C + g * 4);
    store4<T>(dx + ip * C + g * 4, acc);
  }
}

extern "C" int rr_nearest_resize(int dtype, int n, int hi, int wi, int ho, int wo, int C,
                                 const void *x, void *y, rr_stream stream) {
  if (!x || !y || n < 0 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0 || C <= 0 || C % 4) return RR_EINVAL;
  if (!rr_dtype_ok(dtype)) return RR_EINVAL;
  const long long total = (long long)n * ho * wo * (C / 4);
  if (total == 0) return RR_OK;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nearest_fwd_kernel<T>, g, b, 0, st, n, hi, wi, ho, wo, C, (const T *)x, (T *)y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_nearest_resize_bwd(int dtype, int n, int hi, int wi, int ho, int wo, int C,
                                     const void *dy, void *dx, rr_stream stream) {
  if (!dy || !dx || n < 0 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0 || C <= 0 || C % 4) return RR_EINVAL;
  if (!rr_dtype_ok(dtype)) return RR_EINVAL;
  const long long total = (long long)n * hi * wi * (C / 4);
  if (total == 0) return RR_OK;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nearest_bwd_kernel<T>, g, b, 0, st, n, hi, wi, ho, wo, C, (const T *)dy, (T *)dx);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_maxpool2_fwd(int dtype, int n, int h, int w, int C, const void *x, void *y,
                               uint8_t *idx, rr_stream stream) {
  if (!x || !y || !idx || C % 4 || h < 2 || w < 2) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool v8 = C % 8 == 0 && (long long)n * h * w * C < 0x7fffffffLL;
  const long long total = (long long)n * (h / 2) * (w / 2) * (C / (v8 ? 8 : 4));
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  if (v8)
    return rr_dispatch_elt(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(maxpool_fwd8_kernel<T>, g, b, 0, st, n, h, w, C, (const T *)x, (T *)y, idx);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(maxpool_fwd_kernel<T>, g, b, 0, st, n, h, w, C, (const T *)x, (T *)y, idx);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_maxpool2_bwd_pooled(int dtype, int n, int h, int w, int C, const void *dy,
                                      const uint8_t *idx, const void *y_pool, void *dx,
                                      rr_stream stream) {
  if (!dy || !idx || !y_pool || !dx || n < 0 || h < 0 || w < 0) return RR_EINVAL;
  if (!rr_dtype_ok(dtype)) return RR_EINVAL;
  if (C % 8 || h % 2 || w % 2 || (long long)n * h * w * C >= 0x7fffffffLL) return RR_EUNSUPPORTED;
  const long long t8 = (long long)n * (h / 2) * (w / 2) * (C / 8);
  if (t8 == 0) return RR_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 g(rr_grid_cap((t8 + 255) / 256, 8192)), b(256);
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(maxpool_bwd8p_kernel<T>, g, b, 0, st, n, h, w, C, (const T *)dy, idx,
                       (const T *)y_pool, (T *)dx);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_maxpool2_bwd(int dtype, int n, int h, int w, int C, const void *dy,
                               const uint8_t *idx, void *dx, int accumulate, const void *mask,
                               rr_stream stream) {
  if (!dy || !idx || !dx || C % 4) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const bool v8 = C % 8 == 0 && (long long)n * h * w * C < 0x7fffffffLL;
  const long long total = (long long)n * h * w * (C / (v8 ? 8 : 4));
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  if (v8)
    return rr_dispatch_elt(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(maxpool_bwd8_kernel<T>, g, b, 0, st, n, h, w, C, (const T *)dy, idx, (T *)dx,
                         accumulate, (const T *)mask);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(maxpool_bwd_kernel<T>, g, b, 0, st, n, h, w, C, (const T *)dy, idx, (T *)dx,
                       accumulate, (const T *)mask);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_adaptive_avgpool_flatten(int dtype, int n, int h, int w, int C, int oh, int ow,
                                           const void *x, void *y, rr_stream stream) {
  if (!x || !y || oh <= 0 || ow <= 0) return RR_EINVAL;
  const long long total = (long long)n * C * oh * ow;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(adaptive_avgpool_kernel<T>, g, b, 0, st, n, h, w, C, oh, ow, (const T *)x, (T *)y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}
