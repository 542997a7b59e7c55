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
// REC: x is not read but recomputed from t0 / t1 and the forward affines
// aff_s / aff_b [2][64] (rows: BN0, BN1), v = t0*s0 + b0; q = t1*s1 + b1;
// v += q; x = round_T(max(v, 0)) -- affine_act8_kernel's expression in
// bwd_gm8's mask-kind-4 form, so x is bitwise the stored block output.
template <typename T, int COUT, bool REC = false>
__global__ __launch_bounds__(256) void conv_out_bwd64_bnred_kernel(
    int n, int h, int w, const float *__restrict__ dy, const T *__restrict__ x,
    const float *__restrict__ wt, const T *__restrict__ t0, const float *__restrict__ mean0,
    const float *__restrict__ inv0, const T *__restrict__ t1, const float *__restrict__ mean1,
    const float *__restrict__ inv1, float *__restrict__ part, float *__restrict__ bnpart,
    long long px_per_block, const float *__restrict__ aff_s = nullptr,
    const float *__restrict__ aff_b = nullptr) {
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
  // REC: the forward affines sit in LDS ([s0 s1 b0 b1][64]) and are read per
  // pixel: 32 more coefficient registers would halve the occupancy
  __shared__ __attribute__((aligned(16))) float faff[REC ? 4 * CIN : 4];
  if constexpr (REC) {
    faff[threadIdx.x] = threadIdx.x < 2 * CIN ? aff_s[threadIdx.x] : aff_b[threadIdx.x - 2 * CIN];
    __syncthreads();
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
    load8<T>(t0 + e, a0, a1);
    load8<T>(t1 + e, b0, b1);
    if constexpr (REC) {
      int o = cg * 8;
      asm volatile("" : "+v"(o));           // (keeps the reads here: not hoisted into registers)
      const f32x4 *fa = reinterpret_cast<const f32x4 *>(faff + o);
      // f32x4 units: +16 per [64] row, +1 for the upper channel half
      f32x4 v0 = a0 * fa[0] + fa[32], v1 = a1 * fa[1] + fa[33];
      f32x4 q0 = b0 * fa[16] + fa[48], q1 = b1 * fa[17] + fa[49];
      v0 += q0;
      v1 += q1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x0[k] = Elt<T>::round(fmaxf(v0[k], 0.f));
        x1[k] = Elt<T>::round(fmaxf(v1[k], 0.f));
      }
    } else {
      load8<T>(x + e, x0, x1);
    }
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

// ---------------------------------------------------------------------------
// The BN-shortcut residual tail and the final 1x1 conv it feeds in one pass
// (ResUNet dec1 -> final, 14:114-115 + 14:149), bf16, C = 64, cout <= 4:
//   y = relu(x*scale + shift + (res*rs + rb))   affine_act8_kernel's fp32
//       expression, rounded to bf16 (stored only when y != null)
//   out[n][co][h][w] = bias[co] + sum_c y[c] w[co][c], fp32 NCHW
// The 1x1 is stream1_kernel<1,2,..,NCHW>'s arithmetic: one 16x16x32 bf16 MFMA
// per 32-channel k-block from a zero accumulator, k-block 0 then 1, then the
// bias; A = the packed weights [cout][64] (rows >= cout zero), B = 16 pixels.
// A lane owns pixel l & 15 and channels 8 (l >> 4) .. +7 of each k-block: what
// the tail arithmetic leaves in its registers IS its B fragment (two 16-B
// loads per input tensor, no LDS).  A wave walks 16-pixel blocks gw, gw + NWT,
// ... TCO_D at a time (all waves together sweep one window of memory).
constexpr int TCO_D = 2;
__global__ __launch_bounds__(256) void tail_conv_out_kernel(
    int P, int hw, int cout, const bf16_t *__restrict__ x, const float *__restrict__ scale,
    const float *__restrict__ shift, const bf16_t *__restrict__ res, const float *__restrict__ rs,
    const float *__restrict__ rb, const bf16_t *__restrict__ wp, const float *__restrict__ bias,
    bf16_t *__restrict__ y, float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int nblk = (P + 15) >> 4;
  const int gw = blockIdx.x * 4 + wv, NWT = gridDim.x * 4;
  bf16x8 wr[2];
  f32x4 s[2][2], b[2][2], qs[2][2], qb[2][2];       // [k-block][channel half]
#pragma unroll
  for (int kb = 0; kb < 2; ++kb) {
    bf16x8 v = {};
    if (fr < cout) v = *reinterpret_cast<const bf16x8 *>(wp + fr * 64 + kb * 32 + fq * 8);
    wr[kb] = v;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int c = kb * 32 + fq * 8 + 4 * hf;
      s[kb][hf] = *reinterpret_cast<const f32x4 *>(scale + c);
      b[kb][hf] = *reinterpret_cast<const f32x4 *>(shift + c);
      qs[kb][hf] = *reinterpret_cast<const f32x4 *>(rs + c);
      qb[kb][hf] = *reinterpret_cast<const f32x4 *>(rb + c);
    }
  }
  float bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bv[j] = j < cout ? bias[j] : 0.f;
  struct Blk {
    uint4 t[2], r[2];
  };
  // block bi's operands: pixel bi*16 + fr (clamped: loads stay unconditional)
  auto load_blk = [&](int bi, Blk &bk) __attribute__((always_inline)) {
    const int p = min(bi * 16 + fr, P - 1);
    const long long e = (long long)p * 64 + fq * 8;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      bk.t[kb] = *reinterpret_cast<const uint4 *>(x + e + kb * 32);
      bk.r[kb] = *reinterpret_cast<const uint4 *>(res + e + kb * 32);
    }
  };
  auto unpack = [](uint4 r, f32x4 &lo, f32x4 &hi) __attribute__((always_inline)) {   // load8<bf16_t>
    lo[0] = __uint_as_float(r.x << 16); lo[1] = __uint_as_float(r.x & 0xffff0000u);
    lo[2] = __uint_as_float(r.y << 16); lo[3] = __uint_as_float(r.y & 0xffff0000u);
    hi[0] = __uint_as_float(r.z << 16); hi[1] = __uint_as_float(r.z & 0xffff0000u);
    hi[2] = __uint_as_float(r.w << 16); hi[3] = __uint_as_float(r.w & 0xffff0000u);
  };
  auto run = [&](const Blk &bk, int bi) __attribute__((always_inline)) {
    const int p = bi * 16 + fr;
    const bool live = p < P;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x4 v0, v1, q0, q1;
      unpack(bk.t[kb], v0, v1);
      unpack(bk.r[kb], q0, q1);
      v0 = v0 * s[kb][0] + b[kb][0];
      v1 = v1 * s[kb][1] + b[kb][1];
      q0 = q0 * qs[kb][0] + qb[kb][0];
      q1 = q1 * qs[kb][1] + qb[kb][1];
      v0 += q0;
      v1 += q1;
#pragma unroll
      for (int k = 0; k < 4; ++k) { v0[k] = fmaxf(v0[k], 0.f); v1[k] = fmaxf(v1[k], 0.f); }
      u16x8 r;                                    // store8<bf16_t>'s rounding
      r[0] = f32_to_bf16(v0[0]); r[1] = f32_to_bf16(v0[1]); r[2] = f32_to_bf16(v0[2]); r[3] = f32_to_bf16(v0[3]);
      r[4] = f32_to_bf16(v1[0]); r[5] = f32_to_bf16(v1[1]); r[6] = f32_to_bf16(v1[2]); r[7] = f32_to_bf16(v1[3]);
      if (y && live) *reinterpret_cast<u16x8 *>(y + (long long)p * 64 + kb * 32 + fq * 8) = r;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[kb], __builtin_bit_cast(bf16x8, r), acc, 0, 0, 0);
    }
    // accumulator rows 4 fq + j = output channels: the fq == 0 lanes hold
    // them all; 16 lanes = 16 consecutive pixels of one plane
    if (live && fq == 0) {
      const int n = p / hw, rem = p - n * hw;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cout) out[((long long)n * cout + j) * hw + rem] = acc[j] + bv[j];
    }
  };
  for (int b0 = gw; b0 < nblk; b0 += TCO_D * NWT) {
    Blk bk[TCO_D];
#pragma unroll
    for (int j = 0; j < TCO_D; ++j) load_blk(min(b0 + j * NWT, nblk - 1), bk[j]);
#pragma unroll
    for (int j = 0; j < TCO_D; ++j)
      if (b0 + j * NWT < nblk) run(bk[j], b0 + j * NWT);      // wave-uniform
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
  // cin >= cout: the db row of a partial slab has cin slots and holds cout values
  if (!dy || !x || !wt || cout > 4 || cout <= 0 || cin > 64 || cin < cout) return RR_EINVAL;
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

// x given: the stored block output is read; x null: recomputed from t0 / t1
// and the forward affines aff_s / aff_b [2][C] (bf16 only)
static int conv_out_bwd_bnred(const rr_bnbwd_desc *d, int n, int h, int w, int cout, const float *dy,
                              const void *x, const float *aff_s, const float *aff_b, const float *wt,
                              const void *t0, const float *mean0, const float *invstd0, const void *t1,
                              const float *mean1, const float *invstd1, float *dw, float *db,
                              float *bn_partial, void *ws, size_t ws_bytes, rr_stream stream) {
  const bool rec = x == nullptr;
  if (!d || !dy || !wt || !t0 || !mean0 || !invstd0 || !t1 || !mean1 || !invstd1 || !dw || !db ||
      !bn_partial || (rec && (!aff_s || !aff_b)))
    return RR_EINVAL;
  const long long P = (long long)n * h * w;
  if (d->P != P || d->nbn != 2 || d->mask_kind != 4 || d->eval) return RR_EINVAL;
  if (rec && !rr_dtype_ok(d->dtype)) return RR_EINVAL;
  if (d->C != 64 || cout != 3 || (rec && d->dtype != RR_BF16)) return RR_EUNSUPPORTED;
  const int blocks = rr_bn_stats_blocks(P);
  if (blocks != rr_bn_bwd_blocks(d)) return RR_EINVAL;
  const size_t pbytes = (size_t)blocks * (cout + 1) * d->C * sizeof(float);
  if (!ws || ws_bytes < rr_conv_out_bwd_bnred_workspace(P, d->C, cout)) return RR_EWORKSPACE;
  const long long ppb = (P + blocks - 1) / blocks;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (rec) {
    using T = bf16_t;
    hipLaunchKernelGGL((conv_out_bwd64_bnred_kernel<T, 3, true>), dim3(blocks), dim3(256), 0, st, n, h, w,
                       dy, (const T *)nullptr, wt, (const T *)t0, mean0, invstd0, (const T *)t1, mean1,
                       invstd1, (float *)ws, bn_partial, ppb, aff_s, aff_b);
    RR_CHECK_LAUNCH();
    rc = RR_OK;
  } else {
    rc = rr_dispatch_elt(d->dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((conv_out_bwd64_bnred_kernel<T, 3>), dim3(blocks), dim3(256), 0, st, n, h, w, dy,
                         (const T *)x, wt, (const T *)t0, mean0, invstd0, (const T *)t1, mean1, invstd1,
                         (float *)ws, bn_partial, ppb, (const float *)nullptr, (const float *)nullptr);
      RR_CHECK_LAUNCH();
      return RR_OK;
    });
  }
  if (rc != RR_OK) return rc;
  double *red = (double *)((char *)ws + pbytes);
  const int chunks = rr_colreduce_misc((const float *)ws, blocks, (cout + 1) * d->C, red, st);
  if (chunks < 0) return RR_ELAUNCH;
  hipLaunchKernelGGL(conv_out_bwd_finalize, dim3((cout * d->C + cout + 255) / 256), dim3(256), 0, st, d->C,
                     cout, chunks, (const double *)red, dw, db);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

extern "C" int rr_conv_out_bwd_bnred(const rr_bnbwd_desc *d, int n, int h, int w, int cout,
                                     const float *dy, const void *x, const float *wt, const void *t0,
                                     const float *mean0, const float *invstd0, const void *t1,
                                     const float *mean1, const float *invstd1, float *dw, float *db,
                                     float *bn_partial, void *ws, size_t ws_bytes, rr_stream stream) {
  if (!x) return RR_EINVAL;
  return conv_out_bwd_bnred(d, n, h, w, cout, dy, x, nullptr, nullptr, wt, t0, mean0, invstd0, t1, mean1,
                            invstd1, dw, db, bn_partial, ws, ws_bytes, stream);
}

extern "C" int rr_conv_out_bwd_bnred_rec(int n, int h, int w, int cout, const rr_bnbwd_desc *d,
                                         const float *dy, const float *wt, const float *aff_s,
                                         const float *aff_b, const void *t0, const float *mean0,
                                         const float *invstd0, const void *t1, const float *mean1,
                                         const float *invstd1, float *dw, float *db, float *bn_partial,
                                         void *ws, size_t ws_bytes, rr_stream stream) {
  return conv_out_bwd_bnred(d, n, h, w, cout, dy, nullptr, aff_s, aff_b, wt, t0, mean0, invstd0, t1,
                            mean1, invstd1, dw, db, bn_partial, ws, ws_bytes, stream);
}

extern "C" int rr_affine_act_conv_out(int x_dtype, int n, int h, int w, int C, int cout, const void *x,
                                      const float *scale, const float *shift, const void *res,
                                      const float *res_scale, const float *res_shift,
                                      const void *wpack, const float *bias, void *y, float *out,
                                      rr_stream stream) {
  if (!rr_dtype_ok(x_dtype) || n <= 0 || h <= 0 || w <= 0 || C <= 0 || cout <= 0 || !x || !scale ||
      !shift || !res || !res_scale || !res_shift || !wpack || !bias || !out)
    return RR_EINVAL;
  const long long P = (long long)n * h * w;
  if (x_dtype != RR_BF16 || C != 64 || cout > 4 || P > 0x7fffffffLL - 16) return RR_EUNSUPPORTED;
  const int nblk = (int)((P + 15) / 16);
  // one wave per TCO_D blocks in flight; up to 8 workgroups per CU's worth of grid
  const int grid = rr_grid_cap(((long long)nblk + 4 * TCO_D - 1) / (4 * TCO_D), 2048);
  hipLaunchKernelGGL(tail_conv_out_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)P, h * w,
                     cout, (const bf16_t *)x, scale, shift, (const bf16_t *)res, res_scale, res_shift,
                     (const bf16_t *)wpack, bias, (bf16_t *)y, out);
  RR_CHECK_LAUNCH();
  return RR_OK;
}

