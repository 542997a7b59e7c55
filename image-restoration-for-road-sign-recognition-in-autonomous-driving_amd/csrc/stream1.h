// stream1.h -- argument block of the wave-streaming 1x1 / convT GEMM
// (stream1.hip); its entry points are in route.h.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

struct S1Args {
  const char *x1, *x2;       // NHWC bf16 sources (x2: second half of a concat input)
  const char *wt;            // packed bf16 weights [c_out][K] (the rr_igemm pack)
  const float *bias;         // per GEMM column or null
  char *y1, *y2;             // outputs (y2: columns >= split)
  const char *mask;          // relu-backward mask (y1 layout) or null
  float *stats;              // [G][c_out][2] pre-bias partial sums or null
  int mode, P, h, w, hw, lw, lhw;
  FastDiv fd_hw, fd_w;       // coarse pixel -> (image, row, column) for any h, w (convT up / down)
  int c1, c2, cout, cout_t, split, K, G, flags;
  int ksrc[16], kch[16], ktap[16];   // per 32-deep k fragment: source, channel, fine-grid tap offset
};
