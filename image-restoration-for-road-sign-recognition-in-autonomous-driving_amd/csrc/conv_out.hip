// conv_out.hip -- the last layer, conv1x1 64->3 into NCHW fp32 (07:96,
// 14:149) (gfx950, NHWC in).
//
//  * fwd
//  * bwd: dx + per-block dw / db partials (general, and the 64 -> 3 form),
//    column reduce, finalize
//  * the 64 -> 3 bwd that also reduces the BN backward of the block feeding
//    it (rr_conv_out_bwd_bnred; its apply is rr_bn_bwd_apply_convout, bn.hip)
#include "common.h"

namespace {

// ---------------------------------------------------------------------------
// last layer: y[n][co][h][w] = b[co] + sum_ci x[p][ci] w[co][ci]; thread = pixel
template <typename T>
__global__ void conv_out_fwd_kernel(int n, int h, int w, int cin, int cout, const T *__restrict__ x,
                                    const float *__restrict__ wt, const float *__restrict__ b,
                                    float *__restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float sw[];   // [cout][cin]
  for (int i = threadIdx.x; i < cin * cout; i += blockDim.x) sw[i] = wt[i];
  __syncthreads();
  const long long P = (long long)n * h * w;
  const long long hw = (long long)h * w;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < P;
       p += (long long)gridDim.x * blockDim.x) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const T *xp = x + p * cin;
    for (int c = 0; c < cin; c += 4) {
      const f32x4 v = load4<T>(xp + c);
      for (int co = 0; co < cout && co < 4; ++co) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(sw + co * cin + c);
        acc[co] += v[0] * wv[0] + v[1] * wv[1] + v[2] * wv[2] + v[3] * wv[3];
      }
    }
    const long long nn = p / hw, r = p % hw;
    for (int co = 0; co < cout && co < 4; ++co)
      y[(nn * cout + co) * hw + r] = acc[co] + (b ? b[co] : 0.f);
  }
}

// last layer backward (cin <= 64, cout <= 4).  dx[p][ci] = sum_co dy[n][co][p]
// w[co][ci] (optionally masked by x > 0); per-workgroup partial dW / db sums.
// block: 256 threads = 4 pixel rows x 64 channel lanes
template <typename T>
__global__ void conv_out_bwd_kernel(int n, int h, int w, int cin, int cout,
                                    const float *__restrict__ dy, const T *__restrict__ x,
                                    const float *__restrict__ wt, T *__restrict__ dx, int mask_relu,
                                    float *__restrict__ part, long long px_per_block) {
  __shared__ float red[4][64][4];
  __shared__ float redb[4][4];
  const int ci = threadIdx.x & 63, row = threadIdx.x >> 6;
  const long long hw = (long long)h * w;
  const long long P = (long long)n * hw;
  const long long pb = blockIdx.x * px_per_block;
  const long long pe = min(P, pb + px_per_block);
  float wv[4] = {0.f, 0.f, 0.f, 0.f};
  for (int co = 0; co < cout; ++co) wv[co] = ci < cin ? wt[co * cin + ci] : 0.f;
  float sw[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long p = pb + row; p < pe; p += 4) {
    const long long nn = p / hw, r = p - nn * hw;
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    for (int co = 0; co < cout; ++co) d[co] = dy[(nn * cout + co) * hw + r];
    if (ci < cin) {
      const float xv = Elt<T>::load(x, p * cin + ci);
      float g = 0.f;
      for (int co = 0; co < cout; ++co) {
        g += d[co] * wv[co];
        sw[co] += d[co] * xv;
      }
      if (mask_relu && !(xv > 0.f)) g = 0.f;
      if (dx) Elt<T>::store(dx, p * cin + ci, g);
    }
    for (int co = 0; co < cout; ++co) sb[co] += d[co];
  }
  for (int co = 0; co < 4; ++co) red[row][ci][co] = sw[co];
  if (ci == 0)
    for (int co = 0; co < 4; ++co) redb[row][co] = sb[co];
  __syncthreads();
  if (row == 0 && ci < cin)
    for (int co = 0; co < cout; ++co)
      part[((long long)blockIdx.x * (cout + 1) + co) * cin + ci] =
          red[0][ci][co] + red[1][ci][co] + red[2][ci][co] + red[3][ci][co];
  if (threadIdx.x < cout) {
    const int co = threadIdx.x;
    part[((long long)blockIdx.x * (cout + 1) + cout) * cin + co] =
        redb[0][co] + redb[1][co] + redb[2][co] + redb[3][co];
  }
}

// cin == 64 variant: 8 threads per pixel x 8 channels (16-B bf16 / 2 x 16-B
// f32 vectors), 32 pixels per block pass, 2 passes in flight per iteration.
// dW partials: shuffle over the 8 pixel lanes of a wave that share a channel
// group, then the 4 waves through LDS (fixed order).
template <typename T, int COUT>
__global__ __launch_bounds__(256) void conv_out_bwd64_kernel(
    int n, int h, int w, const float *__restrict__ dy, const T *__restrict__ x,
    const float *__restrict__ wt, T *__restrict__ dx, int mask_relu, float *__restrict__ part,
    long long px_per_block) {
  constexpr int CIN = 64;
  __shared__ float red[4][COUT + 1][CIN];
  const int cg = threadIdx.x & 7, pl = threadIdx.x >> 3;      // channel group, pixel lane
  const long long hw = (long long)h * w;
  const long long P = (long long)n * hw;
  const long long pb = blockIdx.x * px_per_block;
  const long long pe = min(P, pb + px_per_block);
  float wv[COUT][8];
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int j = 0; j < 8; ++j) wv[co][j] = wt[co * CIN + cg * 8 + j];
  float sw[COUT][8], sb[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    sb[co] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sw[co][j] = 0.f;
  }
  auto one = [&](long long p) __attribute__((always_inline)) {
    const long long nn = p / hw, r = p - nn * hw;
    float d[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) d[co] = dy[(nn * COUT + co) * hw + r];
    const T *xp = x + p * CIN + cg * 8;
    const f32x4 x0 = load4<T>(xp), x1 = load4<T>(xp + 4);
    const float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    float g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = 0.f;
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        t += d[co] * wv[co][j];
        sw[co][j] += d[co] * xv[j];
      }
      g[j] = (mask_relu && !(xv[j] > 0.f)) ? 0.f : t;
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) sb[co] += d[co];
    if (dx) store8<T>(dx + p * CIN + cg * 8, f32x4{g[0], g[1], g[2], g[3]}, f32x4{g[4], g[5], g[6], g[7]});
  };
  long long p = pb + pl;
  for (; p + 32 < pe; p += 64) {
    one(p);
    one(p + 32);
  }
  if (p < pe) one(p);
  // reduce over the 8 pixel lanes of this wave with the same cg (lane bits 3..5)
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = sw[co][j];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      sw[co][j] = v;
    }
    float v = sb[co];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    sb[co] = v;
  }
  const int wv_ = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < 8) {
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wv_][co][cg * 8 + j] = sw[co][j];
      if (cg == 0) red[wv_][COUT][co] = sb[co];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < COUT * CIN + COUT; i += 256) {
    const int co = i / CIN, ci = i - co * CIN;
    part[(long long)blockIdx.x * (COUT + 1) * CIN + i] =
        red[0][co][ci] + red[1][co][ci] + red[2][co][ci] + red[3][co][ci];
  }
}

// the final conv's backward fused with the BN-backward reduce of the block
// that produced its input (ResUNet dec1's residual tail, 14:99-115 + 14:149):
// the final 1x1 conv's dW / db partials as conv_out_bwd64_kernel, and per
// channel sum(gm), sum(gm xhat0), sum(gm xhat1) of gm = dL/d(block out)
// masked by the block's ReLU (out > 0 <=> the pre-ReLU sum > 0), where
// dL/d(block out) = the conv's input grad (rounded to T as rr_conv_out_bwd
// stores it) -- never written: rr_bn_bwd_apply_convout recomputes it.  One
// workgroup per BN partial row ([blocks][64][3], rr_bn_bwd_finalize's layout).
template <typename T, int COUT>
__global__ __launch_bounds__(256) void conv_out_bwd64_bnred_kernel(
    int n, int h, int w, const float *__restrict__ dy, const T *__restrict__ x,
    const float *__restrict__ wt, const T *__restrict__ t0, const float *__restrict__ mean0,
    const float *__restrict__ inv0, const T *__restrict__ t1, const float *__restrict__ mean1,
    const float *__restrict__ inv1, float *__restrict__ part, float *__restrict__ bnpart,
    long long px_per_block) {
  constexpr int CIN = 64;
  __shared__ float red[4][COUT + 1][CIN];
  __shared__ float bred[4][CIN][3];
  const int cg = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const long long hw = (long long)h * w;
  const long long P = (long long)n * hw;
  const long long pb = blockIdx.x * px_per_block;
  const long long pe = min(P, pb + px_per_block);
  float wv[COUT][8], m0[8], i0[8], m1[8], i1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int co = 0; co < COUT; ++co) wv[co][j] = wt[co * CIN + cg * 8 + j];
    m0[j] = mean0[cg * 8 + j]; i0[j] = inv0[cg * 8 + j];
    m1[j] = mean1[cg * 8 + j]; i1[j] = inv1[cg * 8 + j];
  }
  float sw[COUT][8], sb[COUT], bs[3][8];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    sb[co] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sw[co][j] = 0.f;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { bs[0][j] = 0.f; bs[1][j] = 0.f; bs[2][j] = 0.f; }
  auto one = [&](long long p) __attribute__((always_inline)) {
    const long long nn = p / hw, r = p - nn * hw;
    float d[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) d[co] = dy[(nn * COUT + co) * hw + r];
    const long long e = p * CIN + cg * 8;
    f32x4 x0, x1, a0, a1, b0, b1;
    load8<T>(x + e, x0, x1);
    load8<T>(t0 + e, a0, a1);
    load8<T>(t1 + e, b0, b1);
    const float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    const float ta[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    const float tb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = 0.f;
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        t += d[co] * wv[co][j];
        sw[co][j] += d[co] * xv[j];
      }
      const float gm = xv[j] > 0.f ? Elt<T>::round(t) : 0.f;
      bs[0][j] += gm;
      bs[1][j] += gm * ((ta[j] - m0[j]) * i0[j]);
      bs[2][j] += gm * ((tb[j] - m1[j]) * i1[j]);
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co) sb[co] += d[co];
  };
  long long p = pb + pl;
  for (; p + 32 < pe; p += 64) {
    one(p);
    one(p + 32);
  }
  if (p < pe) one(p);
  // over the 8 pixel lanes of this wave with the same cg (lane bits 3..5)
  auto lanes8 = [](float v) __attribute__((always_inline)) {
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
  };
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
#pragma unroll
    for (int j = 0; j < 8; ++j) sw[co][j] = lanes8(sw[co][j]);
    sb[co] = lanes8(sb[co]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[k][j] = lanes8(bs[k][j]);
  const int wv_ = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane < 8) {
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wv_][co][cg * 8 + j] = sw[co][j];
      if (cg == 0) red[wv_][COUT][co] = sb[co];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < 3; ++k) bred[wv_][cg * 8 + j][k] = bs[k][j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < COUT * CIN + COUT; i += 256) {
    const int co = i / CIN, ci = i - co * CIN;
    part[(long long)blockIdx.x * (COUT + 1) * CIN + i] =
        red[0][co][ci] + red[1][co][ci] + red[2][co][ci] + red[3][co][ci];
  }
  if (threadIdx.x < CIN * 3) {
    const int c = threadIdx.x / 3, k = threadIdx.x - c * 3;
    bnpart[(long long)blockIdx.x * CIN * 3 + threadIdx.x] =
        bred[0][c][k] + bred[1][c][k] + bred[2][c][k] + bred[3][c][k];
  }
}

__global__ void conv_out_bwd_finalize(int cin, int cout, int blocks, const double *__restrict__ part,
                                      float *dw, float *db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over cout*cin + cout
  if (i >= cout * cin + cout) return;
  double s = 0;
  if (i < cout * cin) {
    double sv[1] = {0};
    rr_fixed_sum<1>(part + i, (long long)(cout + 1) * cin, blocks, sv);
    s = sv[0];
    if (dw) dw[i] = (float)s;
  } else {
    const int co = i - cout * cin;
    double sv[1] = {0};
    rr_fixed_sum<1>(part + (long long)cout * cin + co, (long long)(cout + 1) * cin, blocks, sv);
    s = sv[0];
    if (db) db[co] = (float)s;
  }
}

}  // namespace

extern "C" int rr_conv_out_fwd(int dtype, int n, int h, int w, int cin, int cout, const void *x,
                               const float *wt, const float *b, float *y, rr_stream stream) {
  if (!x || !wt || !y || cout > 4 || cout <= 0 || cin % 4) return RR_EINVAL;
  const long long P = (long long)n * h * w;
  dim3 g(rr_grid_cap((P + 255) / 256, 8192)), bl(256);
  const size_t shm = (size_t)cin * cout * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv_out_fwd_kernel<T>, g, bl, shm, st, n, h, w, cin, cout, (const T *)x, wt,
                       b, y);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

int rr_colreduce_misc(const float *in, int rows, int cols, double *out, hipStream_t st);   // misc.hip
static int conv_out_blocks(int n, int h, int w) {
  const long long P = (long long)n * h * w;
  long long b = (P + 1023) / 1024;
  if (b > 2048) b = 2048;
  return (int)(b < 1 ? 1 : b);
}

extern "C" size_t rr_conv_out_bwd_workspace(int n, int h, int w, int cin, int cout) {
  const int blocks = conv_out_blocks(n, h, w);
  return (size_t)blocks * (cout + 1) * cin * sizeof(float) +
         rr_colreduce_bytes(blocks, (cout + 1) * cin);
}

extern "C" int rr_conv_out_bwd(int dtype, int n, int h, int w, int cin, int cout, const float *dy,
                               const void *x, const float *wt, void *dx, int mask_relu, float *dw,
                               float *db, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!dy || !x || !wt || cout > 4 || cout <= 0 || cin > 64) return RR_EINVAL;
  const int blocks = conv_out_blocks(n, h, w);
  const size_t pbytes = (size_t)blocks * (cout + 1) * cin * sizeof(float);
  if (!ws || ws_bytes < pbytes + rr_colreduce_bytes(blocks, (cout + 1) * cin)) return RR_EWORKSPACE;
  const long long P = (long long)n * h * w;
  const long long ppb = (P + blocks - 1) / blocks;
  hipStream_t st = (hipStream_t)stream;
  const int rc = cin == 64 && cout == 3 ? rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((conv_out_bwd64_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, n, h, w, dy,
                       (const T *)x, wt, (T *)dx, mask_relu, (float *)ws, ppb);
    RR_CHECK_LAUNCH();
    return RR_OK;
  }) : rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(conv_out_bwd_kernel<T>, dim3(blocks), dim3(256), 0, st, n, h, w, cin, cout, dy,
                       (const T *)x, wt, (T *)dx, mask_relu, (float *)ws, ppb);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc != RR_OK) return rc;
  double *red = (double *)((char *)ws + pbytes);
  const int chunks = rr_colreduce_misc((const float *)ws, blocks, (cout + 1) * cin, red, st);
  if (chunks < 0) return RR_ELAUNCH;
  hipLaunchKernelGGL(conv_out_bwd_finalize, dim3((cout * cin + cout + 255) / 256), dim3(256), 0,
                     st, cin, cout, chunks, (const double *)red, dw, db);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" size_t rr_conv_out_bwd_bnred_workspace(long long P, int cin, int cout) {
  const int blocks = rr_bn_stats_blocks(P);
  return (size_t)blocks * (cout + 1) * cin * sizeof(float) + rr_colreduce_bytes(blocks, (cout + 1) * cin);
}

extern "C" int rr_conv_out_bwd_bnred(const rr_bnbwd_desc *d, int n, int h, int w, int cout,
                                     const float *dy, const void *x, const float *wt, const void *t0,
                                     const float *mean0, const float *invstd0, const void *t1,
                                     const float *mean1, const float *invstd1, float *dw, float *db,
                                     float *bn_partial, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!d || !dy || !x || !wt || !t0 || !mean0 || !invstd0 || !t1 || !mean1 || !invstd1 || !dw || !db ||
      !bn_partial)
    return RR_EINVAL;
  const long long P = (long long)n * h * w;
  if (d->P != P || d->nbn != 2 || d->mask_kind != 4 || d->eval) return RR_EINVAL;
  if (d->C != 64 || cout != 3) return RR_EUNSUPPORTED;
  const int blocks = rr_bn_stats_blocks(P);
  if (blocks != rr_bn_bwd_blocks(d)) return RR_EINVAL;
  const size_t pbytes = (size_t)blocks * (cout + 1) * d->C * sizeof(float);
  if (!ws || ws_bytes < rr_conv_out_bwd_bnred_workspace(P, d->C, cout)) return RR_EWORKSPACE;
  const long long ppb = (P + blocks - 1) / blocks;
  hipStream_t st = (hipStream_t)stream;
  const int rc = rr_dispatch_elt(d->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((conv_out_bwd64_bnred_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, n, h, w, dy,
                       (const T *)x, wt, (const T *)t0, mean0, invstd0, (const T *)t1, mean1, invstd1,
                       (float *)ws, bn_partial, ppb);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
  if (rc != RR_OK) return rc;
  double *red = (double *)((char *)ws + pbytes);
  const int chunks = rr_colreduce_misc((const float *)ws, blocks, (cout + 1) * d->C, red, st);
  if (chunks < 0) return RR_ELAUNCH;
  hipLaunchKernelGGL(conv_out_bwd_finalize, dim3((cout * d->C + cout + 255) / 256), dim3(256), 0, st, d->C,
                     cout, chunks, (const double *)red, dw, db);
  RR_CHECK_LAUNCH();
  return RR_OK;
}
