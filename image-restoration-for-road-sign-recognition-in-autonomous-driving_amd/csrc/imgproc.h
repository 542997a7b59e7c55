// imgproc.h -- what more than one of resize.hip, quality.hip and distort.hip
// needs.
#pragma once
#include "common.h"

// a record of a ragged batch the device code may follow: inside [1, max_h] x
// [1, max_w] and inside the buffer.  rr_ragged_check on the host, and every
// ragged kernel before it touches the image
__host__ __device__ static inline bool rg_valid(const rr_ragged_image &r, int c, int max_h, int max_w,
                                                long long in_bytes) {
  if (r.h < 1 || r.h > max_h || r.w < 1 || r.w > max_w) return false;
  if (r.offset < 0 || r.offset > in_bytes) return false;
  return (long long)r.h * r.w <= (in_bytes - r.offset) / c;
}

// the size of a ragged buffer: not empty, and a long long on the device
static inline bool rg_bytes_ok(size_t in_bytes) { return in_bytes != 0 && in_bytes <= (size_t)INT64_MAX; }

int rr_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t st);   // a kernel, misc.hip
