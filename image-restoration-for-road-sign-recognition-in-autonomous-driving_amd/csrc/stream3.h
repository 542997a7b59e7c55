// stream3.h -- argument block of the row-streaming 3x3 conv (stream3.hip); its
// entry points are in route.h.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/roadrestore.h"

struct S3Args {
  const char *x;             // NHWC bf16 input [n][h][w][64]
  const char *x2;            // second 64-channel source of a concat input (two passes) or null
  const char *wt;            // packed bf16 weights [64][9][wld] (fwd or dgrad pack)
  int wld, woff;             // packed row length (c_in) and the pass's channel offset
  const float *bias;         // [64] or null
  char *y;                   // NHWC bf16 output [n][h][w][64]
  const char *mask;          // relu-backward mask (NHWC bf16) or null
  float *stats;              // [nwg][64][2] pre-bias partial sums or null
  int n, h, w;               // w: the image width (the template width, or a multiple: column strips)
  int act, accumulate;
  // BN -> PReLU backward epilogue (rr_igemm_bnbwd), bt != null selects it
  const char *bt;
  const float *bmean, *binv, *baff_s, *baff_b, *balpha;
  float *bpart, *bapart;     // [nwg][64][3], [nwg]
  // pool epilogue (rr_igemm_pool): 2x2 max-pool of the ReLU output and
  // its first-max window index, [n][h/2][w/2][64] (no full-size output)
  char *ypool;
  uint8_t *pidx;
  // 1x1 second source (rr_igemm_dgrad_sc): NHWC bf16 [n][h][w][64] and its
  // weights [64 out][64] (rows of the 1x1 dgrad pack)
  const char *xsc, *wsc;
  // eval epilogues (rr_igemm_ex): PReLU alpha [1], identity residual NHWC bf16
  const float *alpha;
  const char *res;
  // input transform (rr_igemm_pre): x is the pre-BN t1, the conv reads
  // PReLU(t1 * pre_s + pre_b) ([64] fp32 each, pre_alpha [1])
  const float *pre_s, *pre_b, *pre_alpha;
};
