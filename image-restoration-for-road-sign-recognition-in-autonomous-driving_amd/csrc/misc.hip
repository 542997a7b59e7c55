// misc.hip -- the remaining element-wise ops of the hot path (gfx950, NHWC).
//
//  * PReLU backward for the enc1 activation (14:122)
//  * layout conversion NCHW fp32 <-> NHWC
//  * L1 / MSE / perceptual-MSE losses (14:219, 07:142, 14:196)
//  * fused Adam / AdamW over flat fp32 buffers (14:222, 07:143)
//  * clamp -> x255 -> uint8 truncation (17:84-92), PSNR (08:123),
//    argmax (18:47)
//  * running-loss accumulate, byte zero / copy kernels, rr_version
#include "common.h"

namespace {

// PReLU backward on an NHWC tensor (count elements): dx = dy*(y>0 ? 1 : a);
// alpha partial per block of sum(dy*y_pre*(y_pre<=0)).
template <typename T>
__global__ void prelu_bwd_kernel(long long count, const T *__restrict__ dy, const T *__restrict__ yp,
                                 const float *alpha, T *__restrict__ dx, float *__restrict__ apart) {
  __shared__ float red[256];
  const float a = alpha[0];
  float s = 0.f;
  const long long n4 = count / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
       i += (long long)gridDim.x * blockDim.x) {
    const f32x4 d = load4<T>(dy + i * 4);
    const f32x4 u = load4<T>(yp + i * 4);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o[k] = u[k] > 0.f ? d[k] : a * d[k];
      s += u[k] > 0.f ? 0.f : d[k] * u[k];
    }
    store4<T>(dx + i * 4, o);
  }
  // the count % 4 tail: workgroup 0, one element per thread
  if (blockIdx.x == 0 && (long long)threadIdx.x < count - n4 * 4) {
    const long long i = n4 * 4 + threadIdx.x;
    const float d = Elt<T>::load(dy, i), u = Elt<T>::load(yp, i);
    Elt<T>::store(dx, i, u > 0.f ? d : a * d);
    s += u > 0.f ? 0.f : d * u;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) apart[blockIdx.x] = red[0];
}

__global__ void sum_partials(int n, const float *__restrict__ part, float *out, int accumulate) {
  __shared__ double red[256];
  double s[1] = {0};
  rr_fixed_sum<1>(part + threadIdx.x, blockDim.x, rr_trips(threadIdx.x, n, blockDim.x), s);
  red[threadIdx.x] = s[0];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + (float)red[0] : (float)red[0];
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ void nchw_to_nhwc_kernel(int n, int c, int h, int w, const float *__restrict__ x,
                                    T *__restrict__ y) {
  const long long total = (long long)n * c * h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c);
    const long long p = i / c;
    const long long hw = (long long)h * w;
    const long long nn = p / hw, r = p % hw;
    Elt<T>::store(y, i, x[(nn * c + cc) * hw + r]);
  }
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(int n, int c, int h, int w, const T *__restrict__ x,
                                    float *__restrict__ y) {
  const long long total = (long long)n * c * h * w;
  const long long hw = (long long)h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i % hw;
    const long long t = i / hw;
    const int cc = (int)(t % c);
    const long long nn = t / c;
    y[i] = Elt<T>::load(x, (nn * hw + r) * c + cc);
  }
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ void loss_partial_kernel(int kind, long long count, const T *__restrict__ a,
                                    const T *__restrict__ b, float *__restrict__ part) {
  __shared__ double red[256];
  double s = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count;
       i += (long long)gridDim.x * blockDim.x) {
    const float d = Elt<T>::load(a, i) - Elt<T>::load(b, i);
    s += kind == 0 ? fabsf(d) : d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = (float)red[0];
}

// 8-element forms (count % 8 == 0): 16-B loads, the 8 terms summed in fp32
// in a fixed order, then into the fp64 per-thread sum
template <typename T>
__global__ void loss_partial8_kernel(int kind, long long count, const T *__restrict__ a,
                                     const T *__restrict__ b, float *__restrict__ part) {
  __shared__ double red[256];
  double s = 0;
  const long long n8 = count / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8;
       i += (long long)gridDim.x * blockDim.x) {
    f32x4 a0, a1, b0, b1;
    load8<T>(a + i * 8, a0, a1);
    load8<T>(b + i * 8, b0, b1);
    const f32x4 d0 = a0 - b0, d1 = a1 - b1;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += kind == 0 ? fabsf(d0[k]) : d0[k] * d0[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) t += kind == 0 ? fabsf(d1[k]) : d1[k] * d1[k];
    s += t;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = (float)red[0];
}

template <typename T>
__global__ void loss_bwd8_kernel(int kind, long long count, const T *__restrict__ a,
                                 const T *__restrict__ b, const float *gs, float scale,
                                 T *__restrict__ ga, T *__restrict__ gb, int accumulate,
                                 int mask_a_pos) {
  const float g = (gs ? gs[0] : 1.f) * scale;
  const long long n8 = count / 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8;
       i += (long long)gridDim.x * blockDim.x) {
    f32x4 a0, a1, b0, b1;
    load8<T>(a + i * 8, a0, a1);
    load8<T>(b + i * 8, b0, b1);
    const float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    const float bv[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = av[k] - bv[k];
      v[k] = kind == 0 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 2.f * g * d;
      if (mask_a_pos && !(av[k] > 0.f)) v[k] = 0.f;
    }
    if (ga) {
      f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
      if (accumulate) {
        f32x4 c0, c1;
        load8<T>(ga + i * 8, c0, c1);
        o0 = c0 + o0;
        o1 = c1 + o1;
      }
      store8<T>(ga + i * 8, o0, o1);
    }
    if (gb) {
      f32x4 o0 = {-v[0], -v[1], -v[2], -v[3]}, o1 = {-v[4], -v[5], -v[6], -v[7]};
      if (accumulate) {
        f32x4 c0, c1;
        load8<T>(gb + i * 8, c0, c1);
        o0 = c0 + o0;
        o1 = c1 + o1;
      }
      store8<T>(gb + i * 8, o0, o1);
    }
  }
}

__global__ void loss_finalize(int blocks, const float *__restrict__ part, float *out, double scale,
                              int accumulate) {
  __shared__ double red[256];
  double s[1] = {0};
  rr_fixed_sum<1>(part + threadIdx.x, blockDim.x, rr_trips(threadIdx.x, blocks, blockDim.x), s);
  red[threadIdx.x] = s[0];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.f) + (float)(red[0] * scale);
}

template <typename T>
__global__ void loss_bwd_kernel(int kind, long long count, const T *__restrict__ a,
                                const T *__restrict__ b, const float *gs, float scale,
                                T *__restrict__ ga, T *__restrict__ gb, int accumulate,
                                int mask_a_pos) {
  const float g = (gs ? gs[0] : 1.f) * scale;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count;
       i += (long long)gridDim.x * blockDim.x) {
    const float av = Elt<T>::load(a, i);
    const float d = av - Elt<T>::load(b, i);
    float v = kind == 0 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 2.f * g * d;
    if (mask_a_pos && !(av > 0.f)) v = 0.f;
    if (ga) Elt<T>::store(ga, i, accumulate ? Elt<T>::load(ga, i) + v : v);
    if (gb) Elt<T>::store(gb, i, accumulate ? Elt<T>::load(gb, i) - v : -v);
  }
}

__global__ void adamw_kernel(long long count, float *__restrict__ p, const float *__restrict__ g,
                             float *__restrict__ m, float *__restrict__ v, float lr, float b1,
                             float b2, float eps, float wd, int decoupled, float bc1, float sbc2) {
  const float step = lr / bc1;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count;
       i += (long long)gridDim.x * blockDim.x) {
    float pv = p[i];
    float gv = g[i];
    if (decoupled) pv *= (1.f - lr * wd);
    else if (wd != 0.f) gv += wd * pv;
    float mv = m[i];
    mv = mv + (1.f - b1) * (gv - mv);          // lerp_(g, 1-b1)
    float vv = v[i] * b2 + (1.f - b2) * gv * gv;
    const float denom = sqrtf(vv) / sbc2 + eps;
    pv = pv - step * (mv / denom);
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
}

// capturable form (HIP graphs): the step count lives on the device, bumped
// by its own launch, and the bias corrections are computed per block in
// double from the same float betas the host path uses
__global__ void adamw_step_inc_kernel(int64_t *step) { *step += 1; }

// The learning rate is read from the device too (*lr_dev, a 1-element fp32
// tensor that torch's LR schedulers update in place with fill_), so a
// scheduler.step() between graph replays takes effect (14:223, 248).
__global__ void adamw_dev_kernel(long long count, float *__restrict__ p, const float *__restrict__ g,
                                 float *__restrict__ m, float *__restrict__ v,
                                 const float *__restrict__ lr_dev, float b1,
                                 float b2, float eps, float wd, int decoupled,
                                 const int64_t *__restrict__ step_dev) {
  __shared__ float bc[3];
  if (threadIdx.x == 0) {
    const double st = (double)*step_dev;
    bc[0] = (float)(1.0 - pow((double)b1, st));
    bc[1] = (float)sqrt(1.0 - pow((double)b2, st));
    bc[2] = *lr_dev;
  }
  __syncthreads();
  const float bc1 = bc[0], sbc2 = bc[1], lr = bc[2];
  const float step = lr / bc1;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count;
       i += (long long)gridDim.x * blockDim.x) {
    float pv = p[i];
    float gv = g[i];
    if (decoupled) pv *= (1.f - lr * wd);
    else if (wd != 0.f) gv += wd * pv;
    float mv = m[i];
    mv = mv + (1.f - b1) * (gv - mv);
    float vv = v[i] * b2 + (1.f - b2) * gv * gv;
    const float denom = sqrtf(vv) / sbc2 + eps;
    pv = pv - step * (mv / denom);
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
}

__global__ void to_u8_kernel(int n, int c, int h, int w, const float *__restrict__ x,
                             uint8_t *__restrict__ out, int bgr) {
  const long long total = (long long)n * h * w * c;
  const long long hw = (long long)h * w;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int cc = (int)(i % c);
    const long long p = i / c;
    const long long nn = p / hw, r = p % hw;
    const int sc = bgr ? (c - 1 - cc) : cc;
    float v = x[(nn * c + sc) * hw + r];
    v = fminf(fmaxf(v, 0.f), 1.f);           // torch.clamp(0, 1)
    out[i] = (uint8_t)(v * 255.f);            // astype(uint8): truncation
  }
}

__global__ void psnr_kernel(long long per, const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                            double *out) {
  __shared__ double red[256];
  const uint8_t *pa = a + blockIdx.x * per, *pb = b + blockIdx.x * per;
  double s = 0;
  for (long long i = threadIdx.x; i < per; i += blockDim.x) {
    const double d = (double)pa[i] - (double)pb[i];
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mse = red[0] / (double)per;
    out[blockIdx.x] = mse == 0 ? __builtin_inf() : 10.0 * log10(255.0 * 255.0 / mse);
  }
}

__global__ void argmax_kernel(int n, int k, const float *__restrict__ x, int64_t *out) {
  const int row = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  float best = -__builtin_inff();
  int bi = 0x7fffffff;
  for (int j = lane; j < k; j += 64) {
    const float v = x[(long long)row * k + j];
    if (v > best || (v != v && best == best)) { best = v; bi = j; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const bool onan = ov != ov, bnan = best != best;
    bool take;
    if (onan != bnan) take = onan;
    else take = (ov > best) || (ov == best && oi < bi) || (onan && oi < bi);
    if (take) { best = ov; bi = oi; }
  }
  if (lane == 0) out[row] = bi == 0x7fffffff ? 0 : bi;
}

}  // namespace

extern "C" int rr_prelu_bwd(int dtype, long long count, const void *dy, const void *y_pre,
                            const float *alpha, void *dx, float *alpha_partial, int blocks,
                            float *dalpha, rr_stream stream) {
  if (!dy || !y_pre || !alpha || !dx || !alpha_partial || !dalpha || count <= 0 || blocks <= 0 ||
      blocks > 4096)
    return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int rc = rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(prelu_bwd_kernel<T>, dim3(blocks), dim3(256), 0, st, count, (const T *)dy,
                       (const T *)y_pre, alpha, (T *)dx, alpha_partial);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc != RR_OK) return rc;
  hipLaunchKernelGGL(sum_partials, dim3(1), dim3(256), 0, st, blocks, alpha_partial, dalpha, 0);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_nchw_to_nhwc(int dtype, int n, int c, int h, int w, const float *x, void *y,
                               rr_stream stream) {
  if (!x || !y) return RR_EINVAL;
  const long long total = (long long)n * c * h * w;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<T>, g, b, 0, st, n, c, h, w, x, (T *)y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_nhwc_to_nchw(int dtype, int n, int c, int h, int w, const void *x, float *y,
                               rr_stream stream) {
  if (!x || !y) return RR_EINVAL;
  const long long total = (long long)n * c * h * w;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<T>, g, b, 0, st, n, c, h, w, (const T *)x, y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

static int loss_blocks(long long count) {
  long long b = (count + 4095) / 4096;
  if (b > 1024) b = 1024;
  return (int)(b < 1 ? 1 : b);
}

extern "C" size_t rr_loss_workspace(long long count) {
  return (size_t)loss_blocks(count) * sizeof(float);
}

extern "C" int rr_loss_fwd(int kind, int dtype, long long count, const void *a, const void *b,
                           float *out_scalar, float scale, int accumulate, void *ws,
                           size_t ws_bytes, rr_stream stream) {
  if (!a || !b || !out_scalar || count <= 0 || (kind != 0 && kind != 1)) return RR_EINVAL;
  const int blocks = loss_blocks(count);
  if (!ws || ws_bytes < (size_t)blocks * sizeof(float)) return RR_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const bool v8 = count % 8 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
  const int rc = rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (v8)
      hipLaunchKernelGGL(loss_partial8_kernel<T>, dim3(blocks), dim3(256), 0, st, kind, count,
                         (const T *)a, (const T *)b, (float *)ws);
    else
      hipLaunchKernelGGL(loss_partial_kernel<T>, dim3(blocks), dim3(256), 0, st, kind, count,
                         (const T *)a, (const T *)b, (float *)ws);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc != RR_OK) return rc;
  hipLaunchKernelGGL(loss_finalize, dim3(1), dim3(256), 0, st, blocks, (const float *)ws,
                     out_scalar, (double)scale / (double)count, accumulate);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_loss_bwd(int kind, int dtype, long long count, const void *a, const void *b,
                           const float *gscale_dev, float scale, void *ga, void *gb, int accumulate,
                           int mask_a_pos, rr_stream stream) {
  if (!a || !b || count <= 0 || (kind != 0 && kind != 1)) return RR_EINVAL;
  const bool v8 = count % 8 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)ga | (uintptr_t)gb) % 16 == 0;
  dim3 g(rr_grid_cap(((v8 ? count / 8 : count) + 255) / 256, 8192)), bl(256);
  const float sc = scale / (float)count;
  hipStream_t st = (hipStream_t)stream;
  if (v8)
    return rr_dispatch_elt(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL(loss_bwd8_kernel<T>, g, bl, 0, st, kind, count, (const T *)a, (const T *)b,
                         gscale_dev, sc, (T *)ga, (T *)gb, accumulate, mask_a_pos);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(loss_bwd_kernel<T>, g, bl, 0, st, kind, count, (const T *)a, (const T *)b,
                       gscale_dev, sc, (T *)ga, (T *)gb, accumulate, mask_a_pos);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_adamw(long long count, float *param, const float *grad, float *m, float *v,
                        float lr, float beta1, float beta2, float eps, float weight_decay,
                        int decoupled, int step, rr_stream stream) {
  if (!param || !grad || !m || !v || count <= 0 || step < 1) return RR_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  dim3 g(rr_grid_cap((count + 255) / 256, 8192)), b(256);
  hipLaunchKernelGGL(adamw_kernel, g, b, 0, (hipStream_t)stream, count, param, grad, m, v, lr,
                     beta1, beta2, eps, weight_decay, decoupled, (float)bc1, (float)sqrt(bc2));
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_adamw_dev(long long count, float *param, const float *grad, float *m, float *v,
                            const float *lr_dev, float beta1, float beta2, float eps,
                            float weight_decay, int decoupled, int64_t *step_dev,
                            rr_stream stream) {
  if (count <= 0 || !param || !grad || !m || !v || !step_dev || !lr_dev) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(adamw_step_inc_kernel, dim3(1), dim3(1), 0, st, step_dev);
  RR_CHECK_LAUNCH();
  dim3 g(rr_grid_cap((count + 255) / 256, 8192)), b(256);
  hipLaunchKernelGGL(adamw_dev_kernel, g, b, 0, st, count, param, grad, m, v, lr_dev, beta1, beta2,
                     eps, weight_decay, decoupled, step_dev);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_to_uint8_hwc(int n, int c, int h, int w, const float *x, uint8_t *out, int bgr,
                               rr_stream stream) {
  if (!x || !out) return RR_EINVAL;
  const long long total = (long long)n * c * h * w;
  dim3 g(rr_grid_cap((total + 255) / 256, 8192)), b(256);
  hipLaunchKernelGGL(to_u8_kernel, g, b, 0, (hipStream_t)stream, n, c, h, w, x, out, bgr);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_psnr_u8(int n, long long per_image, const uint8_t *a, const uint8_t *b,
                          double *out, rr_stream stream) {
  if (!a || !b || !out || n <= 0 || per_image <= 0) return RR_EINVAL;
  hipLaunchKernelGGL(psnr_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, per_image, a, b, out);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_argmax_rows(int n, int k, const float *logits, int64_t *out, rr_stream stream) {
  if (!logits || !out || n <= 0 || k <= 0) return RR_EINVAL;
  hipLaunchKernelGGL(argmax_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, n, k,
                     logits, out);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

// running loss on device (14:246 `running_loss += loss.item()` without the
// per-step host sync): acc[0] += x[0] in fp64, count[0] += 1
__global__ void scalar_accumulate_kernel(const float *__restrict__ x, double *acc, int64_t *count) {
  acc[0] += (double)x[0];
  count[0] += 1;
}

extern "C" int rr_scalar_accumulate(const float *x, double *acc, int64_t *count, rr_stream stream) {
  if (!x || !acc || !count) return RR_EINVAL;
  hipLaunchKernelGGL(scalar_accumulate_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, x, acc, count);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

// byte-range zero / copy as kernels (16-B stores over the 16-B aligned
// body, bytes at the ends).  Capturable: recorded in a HIP graph (alone and
// between torch / library nodes) it zeroes on every replay
// (tests/test_lifetime_gpu.py::test_library_zero_in_hip_graph_replays,
// tools/diag_memset*.py; a round-3 observation of garbage after a second
// replay does not reproduce, profiles/r4i_diag_memset2.log).
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__global__ void zero_bytes_kernel(char *__restrict__ dst, long long head, long long nbody, long long bytes) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long k = i; k < nbody; k += stride)
    reinterpret_cast<i32x4_t *>(dst + head)[k] = i32x4_t{0, 0, 0, 0};
  const long long tail0 = head + nbody * 16;
  for (long long k = i; k < head + (bytes - tail0); k += stride) dst[k < head ? k : tail0 + (k - head)] = 0;
}
__global__ void copy_bytes_kernel(char *__restrict__ dst, const char *__restrict__ src, long long head,
                                  long long nbody, long long bytes) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long k = i; k < nbody; k += stride)
    reinterpret_cast<i32x4_t *>(dst + head)[k] = reinterpret_cast<const i32x4_t *>(src + head)[k];
  const long long tail0 = head + nbody * 16;
  for (long long k = i; k < head + (bytes - tail0); k += stride) {
    const long long b = k < head ? k : tail0 + (k - head);
    dst[b] = src[b];
  }
}

// head bytes before the 16-B aligned body (all bytes when src and dst
// alignments differ), body 16-B chunks, blocks
static void bytes_plan(uintptr_t d, uintptr_t s, bool copy, size_t bytes, long long &head,
                       long long &nbody, unsigned &blocks) {
  if (!copy || ((d ^ s) & 15) == 0) {
    head = (long long)((16 - (d & 15)) & 15);
    if (head > (long long)bytes) head = (long long)bytes;
    nbody = ((long long)bytes - head) / 16;
  } else {
    head = (long long)bytes;
    nbody = 0;
  }
  const long long work = nbody > head ? nbody : head;
  long long b = (work + 255) / 256;
  blocks = (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

extern "C" int rr_zero(void *p, size_t bytes, rr_stream stream) {
  if (!p) return RR_EINVAL;
  if (!bytes) return RR_OK;
  long long head, nbody;
  unsigned blocks;
  bytes_plan((uintptr_t)p, 0, false, bytes, head, nbody, blocks);
  hipLaunchKernelGGL(zero_bytes_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (char *)p, head,
                     nbody, (long long)bytes);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

int rr_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (!dst || !src) return RR_EINVAL;
  if (!bytes) return RR_OK;
  long long head, nbody;
  unsigned blocks;
  bytes_plan((uintptr_t)dst, (uintptr_t)src, true, bytes, head, nbody, blocks);
  hipLaunchKernelGGL(copy_bytes_kernel, dim3(blocks), dim3(256), 0, st, (char *)dst, (const char *)src,
                     head, nbody, (long long)bytes);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

// conv_in.hip and conv_out.hip launch this file's copy of the static
// rr_colreduce_kernel: hipcc schedules the copy in a unit that also holds
// sum_partials differently (same sums, other instruction bytes), and those
// calls have always run this one.
int rr_colreduce_misc(const float *in, int rows, int cols, double *out, hipStream_t st) {
  return rr_colreduce(in, rows, cols, out, st);
}

extern "C" const char *rr_version(void) { return "roadrestore-gfx950 0.1"; }
