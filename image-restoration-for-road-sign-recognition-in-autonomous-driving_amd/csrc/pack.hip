// pack.hip -- weight packing: fp32 torch layout -> compute layout / dtype
// (gfx950).
//
//  * conv 3x3 / 1x1 weights, one layer or a batch of jobs, with the
//    tap-reuse conv's weight tiles (conv3r.hip) after the bf16 3x3 packs
//  * ConvTranspose2d(2, 2) weights, the bias tiled 4x for its scatter
//  * first-layer weights (+ bias) -> the [co][kpad] GEMM layout of
//    rr_conv_in_mfma / rr_im2col3, and the gradient back out of it
#include "common.h"

namespace {

// The tap-reuse conv's weight tiles (conv3r.hip), written after the
// [c_out][9][c_in] pack of every bf16 3x3 conv with c_in, c_out multiples of
// 32: 1-KB A-fragment blocks [32-channel input chunk c][tap column dx][tap
// row dy][16-row output block mb] of [plane q = (ci % 32) / 8][row co % 16]
// [ci % 8], so a (chunk, dx) stage of a column block is 3 contiguous runs.
__host__ __device__ inline bool r3_tiled(int k, int co_n, int ci_n) {
  return k == 3 && co_n % 32 == 0 && ci_n % 32 == 0;
}
__device__ __forceinline__ long long r3_tile_off(int co_n, int co, int ci, int ky, int kx) {
  const int c = ci >> 5, q = (ci & 31) >> 3, e = ci & 7;
  return ((((long long)c * 3 + kx) * 3 + ky) * (co_n >> 4) + (co >> 4)) * 512 + q * 128 +
         (co & 15) * 8 + e;
}

template <typename T>
__global__ void pack_conv_kernel(int co_n, int ci_n, int k, const float *__restrict__ w,
                                 T *__restrict__ wf, T *__restrict__ wd) {
  const int kk = k * k;
  const long long total = (long long)co_n * ci_n * kk;
  const bool tiled = sizeof(T) == 2 && r3_tiled(k, co_n, ci_n);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i % kk);
    const long long r = i / kk;
    const int ci = (int)(r % ci_n);
    const int co = (int)(r / ci_n);
    const float v = w[i];
    const int ky = t / k, kx = t % k;
    if (wf) {
      Elt<T>::store(wf, ((long long)co * kk + t) * ci_n + ci, v);
      if (tiled) Elt<T>::store(wf + total, r3_tile_off(co_n, co, ci, ky, kx), v);
    }
    if (wd) {
      const int tf = (k - 1 - ky) * k + (k - 1 - kx);
      Elt<T>::store(wd, ((long long)ci * kk + tf) * co_n + co, v);
      if (tiled) Elt<T>::store(wd + total, r3_tile_off(ci_n, ci, co, k - 1 - ky, k - 1 - kx), v);
    }
  }
}

// all conv packs of a network in one launch.  A work item is one output
// channel x 8 consecutive input channels of one job (phase 0, the fwd pack
// [co][tap][ci] and its conv3r tiles) or one input channel x 8 consecutive
// output channels (phase 1, the dgrad pack [ci][flipped tap][co] and its
// tiles): the item's 8 x k*k fp32 weights are read once and every tap is
// written as one run of 8 consecutive pack elements -- a 16-B store in bf16
// to the row pack and to the tile pack alike (the tile's innermost 8 elements
// are 8 consecutive channels of one row).  Lanes walk the 8-channel groups
// fastest, so a wave's row stores are contiguous.  (The (co, ci)-pair items
// before wrote 2-byte stores: 98 us and 423 MB of HBM traffic per launch for
// the 12.4 M ResUNet weights with their tiles, profiles/r3r_pmc_traffic.json,
// against ~150 MB algorithmic.)  Channel counts that are not a multiple of 8
// leave a partial last group, written element by element.  Item offsets per
// job come from LDS scans; a thread finds its job by binary search.
constexpr int PACKB_MAX = 256;
template <typename T, int KK>
__device__ __forceinline__ void pack_group(const rr_pack_job &jb, int phase, long long q, bool tiled) {
  constexpr int k = KK == 9 ? 3 : 1;
  const long long tot = (long long)jb.c_out * jb.c_in * KK;
  const int cg = phase == 0 ? jb.c_in : jb.c_out;     // the grouped (contiguous in the pack) channel
  const int ng = (cg + 7) >> 3;
  const int g0 = (int)(q % ng) * 8, r = (int)(q / ng);
  const int n = cg - g0 < 8 ? cg - g0 : 8;
  float v[8][KK];
  if (phase == 0) {
    // w[r][g0 + e][tp]: n * KK contiguous floats
    const float *src = jb.w + ((long long)r * jb.c_in + g0) * KK;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int tp = 0; tp < KK; ++tp) v[e][tp] = src[(e < n ? e : 0) * KK + tp];
  } else {
    // w[g0 + e][r][tp]: n runs of KK floats, c_in * KK apart
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float *src = jb.w + ((long long)(g0 + (e < n ? e : 0)) * jb.c_in + r) * KK;
#pragma unroll
      for (int tp = 0; tp < KK; ++tp) v[e][tp] = src[tp];
    }
  }
  T *rows = (T *)(phase == 0 ? jb.w_fwd : jb.w_dgrad);
#pragma unroll
  for (int tp = 0; tp < KK; ++tp) {
    const int ky = tp / k, kx = tp - ky * k;
    // phase 0: row (r = co, tap tp); phase 1: row (r = ci, flipped tap)
    const int tr = phase == 0 ? tp : (k - 1 - ky) * k + (k - 1 - kx);
    const long long ro = ((long long)r * KK + tr) * cg + g0;
    const long long to = tiled ? (phase == 0 ? r3_tile_off(jb.c_out, r, g0, ky, kx)
                                             : r3_tile_off(jb.c_in, r, g0, 2 - ky, 2 - kx))
                               : 0;
    if (n == 8 && (cg & 7) == 0) {                   // 16-B aligned runs
      store8<T>(rows + ro, f32x4{v[0][tp], v[1][tp], v[2][tp], v[3][tp]},
                f32x4{v[4][tp], v[5][tp], v[6][tp], v[7][tp]});
      if (tiled)
        store8<T>(rows + tot + to, f32x4{v[0][tp], v[1][tp], v[2][tp], v[3][tp]},
                  f32x4{v[4][tp], v[5][tp], v[6][tp], v[7][tp]});
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < n) Elt<T>::store(rows, ro + e, v[e][tp]);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_conv_batch_kernel(int count, const rr_pack_job *__restrict__ jobs,
                                                              long long total) {
  __shared__ long long pb[2][PACKB_MAX + 1];
  (void)total;
  const int t = threadIdx.x;
  if (t < count) {
    const rr_pack_job &j = jobs[t];
    pb[0][t + 1] = j.w_fwd ? (long long)j.c_out * ((j.c_in + 7) >> 3) : 0;
    pb[1][t + 1] = j.w_dgrad ? (long long)j.c_in * ((j.c_out + 7) >> 3) : 0;
  } else {
    pb[0][t + 1] = 0;
    pb[1][t + 1] = 0;
  }
  if (t == 0) { pb[0][0] = 0; pb[1][0] = 0; }
  __syncthreads();
  for (int o = 1; o < PACKB_MAX; o <<= 1) {            // inclusive scans of pb[*][1..256]
    const long long v0 = t >= o ? pb[0][t + 1 - o] : 0, v1 = t >= o ? pb[1][t + 1 - o] : 0;
    __syncthreads();
    pb[0][t + 1] += v0;
    pb[1][t + 1] += v1;
    __syncthreads();
  }
  const long long n0 = pb[0][count], n1 = pb[1][count];
  for (long long w = blockIdx.x * (long long)blockDim.x + t; w < n0 + n1;
       w += (long long)gridDim.x * blockDim.x) {
    const int phase = w >= n0;
    const long long e = phase ? w - n0 : w;
    const long long *p = pb[phase];
    int lo = 0, hi = count - 1;                         // last j with p[j] <= e
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (p[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const rr_pack_job jb = jobs[lo];
    const long long q = e - p[lo];
    const bool tiled = sizeof(T) == 2 && r3_tiled(jb.k, jb.c_out, jb.c_in);
    if (jb.k == 3) pack_group<T, 9>(jb, phase, q, tiled);
    else pack_group<T, 1>(jb, phase, q, false);
  }
}

template <typename T>
__global__ void pack_convT_kernel(int ci_n, int co_n, const float *__restrict__ w,
                                  T *__restrict__ wu, T *__restrict__ wdn) {
  const long long total = (long long)ci_n * co_n * 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int t = (int)(i & 3);
    const long long r = i >> 2;
    const int co = (int)(r % co_n);
    const int ci = (int)(r / co_n);
    const float v = w[i];
    if (wu) Elt<T>::store(wu, ((long long)t * co_n + co) * ci_n + ci, v);
    if (wdn) Elt<T>::store(wdn, ((long long)ci * 4 + t) * co_n + co, v);
  }
}

__global__ void bias_tile4_kernel(int co_n, const float *b, float *b4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * co_n) b4[i] = b[i % co_n];
}

// first-layer weights [co][ci][3][3] (+ bias) -> [co][kpad] GEMM layout
template <typename T>
__global__ void pack_in_kernel(int cout, int cin, int kpad, const float *__restrict__ w,
                               const float *__restrict__ b, T *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cout * kpad) return;
  const int co = i / kpad, j = i % kpad, kk = cin * 9;
  float v = 0.f;
  if (j < kk) v = w[(long long)co * kk + j];
  else if (j == kk && b) v = b[co];
  Elt<T>::store(out, i, v);
}

__global__ void unpack_in_grad_kernel(int cout, int cin, int kpad, const float *__restrict__ g,
                                      float *dw, float *db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int kk = cin * 9;
  if (i >= cout * (kk + 1)) return;
  const int co = i / (kk + 1), j = i % (kk + 1);
  const float v = g[(long long)co * kpad + j];
  if (j < kk) dw[(long long)co * kk + j] = v;
  else if (db) db[co] = v;
}

}  // namespace

extern "C" long long rr_pack_conv_elems(int dtype, int c_out, int c_in, int k) {
  const long long n = (long long)c_out * c_in * k * k;
  return dtype == RR_BF16 && r3_tiled(k, c_out, c_in) ? 2 * n : n;
}

extern "C" int rr_pack_conv(int dtype, int c_out, int c_in, int k, const float *w, void *w_fwd,
                            void *w_dgrad, rr_stream stream) {
  if (!w || c_out <= 0 || c_in <= 0 || (k != 1 && k != 3)) return RR_EINVAL;
  const long long total = (long long)c_out * c_in * k * k;
  dim3 g(rr_grid_cap((total + 255) / 256)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pack_conv_kernel<T>, g, b, 0, st, c_out, c_in, k, w, (T *)w_fwd, (T *)w_dgrad);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_pack_conv_batch(int dtype, int count, const rr_pack_job *jobs, long long total,
                                  rr_stream stream) {
  if (!jobs || count <= 0 || count > PACKB_MAX || total <= 0) return RR_EINVAL;
  // ~total / 36 items (8 channels x 9 taps each, two phases); the 1x1 jobs
  // have 9x more per element, so size for ~total / 16 and grid-stride the rest
  dim3 g(rr_grid_cap((total / 16 + 255) / 256, 8192)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pack_conv_batch_kernel<T>, g, b, 0, st, count, jobs, total);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_pack_convT(int dtype, int c_in, int c_out, const float *w, void *w_up,
                             void *w_down, rr_stream stream) {
  if (!w || c_out <= 0 || c_in <= 0) return RR_EINVAL;
  const long long total = (long long)c_out * c_in * 4;
  dim3 g(rr_grid_cap((total + 255) / 256)), b(256);
  hipStream_t st = (hipStream_t)stream;
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pack_convT_kernel<T>, g, b, 0, st, c_in, c_out, w, (T *)w_up, (T *)w_down);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_bias_tile4(int c_out, const float *b, float *b4, rr_stream stream) {
  if (!b || !b4 || c_out <= 0) return RR_EINVAL;
  hipLaunchKernelGGL(bias_tile4_kernel, dim3((4 * c_out + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, c_out, b, b4);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_pack_conv_in(int dtype, int cout, int cin, int kpad, const float *w,
                               const float *b, void *out, rr_stream stream) {
  if (!w || !out || kpad < 9 * cin + 1) return RR_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  dim3 g((cout * kpad + 255) / 256), bl(256);
  return rr_dispatch_elt(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pack_in_kernel<T>, g, bl, 0, st, cout, cin, kpad, w, b, (T *)out);
    RR_CHECK_LAUNCH();
    return RR_OK;
  });
}

extern "C" int rr_unpack_conv_in_grad(int cout, int cin, int kpad, const float *g, float *dw,
                                      float *db, rr_stream stream) {
  if (!g || !dw || kpad < 9 * cin + 1) return RR_EINVAL;
  hipLaunchKernelGGL(unpack_in_grad_kernel, dim3((cout * (9 * cin + 1) + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, cout, cin, kpad, g, dw, db);
  RR_CHECK_LAUNCH();
  return RR_OK;
}
