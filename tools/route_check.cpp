// route_check -- host-only sanitizer harness for the routing queries: every
// kernel-name, partial-row and workspace query of the library over the sweep
// of tests/route_sweep.py, from 8 threads at once.  Built with ASan + UBSan on
// the host side and linked against the routing objects alone (csrc/Makefile,
// `make routecheck`); needs no GPU and launches nothing.  Each thread folds
// its answers into a hash: all threads must agree, and the sanitizers must
// stay silent.  RR_PATH is taken from the environment, as the library does.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../include/roadrestore.h"

static const int GEOMS[][3] = {{512, 64, 64}, {512, 32, 32}, {512, 16, 16}, {512, 8, 8}, {2, 16, 16}, {3, 16, 16},
                               {1, 8, 8}, {2, 8, 8}, {3, 8, 8}, {16, 224, 224}, {1, 224, 224}, {2, 220, 224},
                               {8, 112, 112}, {16, 56, 56}, {16, 28, 28}, {16, 14, 14}, {2, 60, 60}, {2, 36, 52},
                               {4, 104, 160}, {5, 128, 128}, {10, 40, 224}, {64, 64, 64}, {1, 64, 64}, {256, 32, 32}};
static const int CHANS[][3] = {{64, 0, 64}, {64, 64, 64}, {64, 0, 128}, {128, 64, 64}, {128, 0, 128}, {128, 0, 256},
                               {256, 0, 256}, {256, 128, 128}, {256, 0, 512}, {512, 0, 512}, {512, 0, 256},
                               {512, 256, 256}, {64, 0, 3}, {32, 0, 64}, {64, 0, 256}, {192, 0, 64}};
// out_split, act, accumulate, has_bias, has_mask, want_stats, out_nchw
static const int FLAGS[][7] = {{0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 1, 0, 1, 0}, {0, 1, 0, 1, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0},
                               {0, 0, 0, 0, 1, 0, 0}, {0, 0, 1, 0, 1, 0, 0}, {0, 0, 0, 1, 0, 0, 0}, {0, 2, 0, 1, 0, 0, 0},
                               {0, 5, 0, 1, 0, 0, 0}, {0, 13, 0, 1, 0, 0, 0}, {0, 25, 0, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 1},
                               {64, 0, 1, 0, 0, 0, 0}, {0, 1, 0, 0, 0, 0, 0}};

static uint64_t fold(uint64_t h, uint64_t v) { return (h ^ v) * 0x100000001b3ull; }
static uint64_t fold(uint64_t h, const char *s) {
  if (!s) return fold(h, 0xdeadull);       // (never null by contract: would change the hash)
  for (size_t i = 0, n = strlen(s); i < n; ++i) h = fold(h, (uint64_t)(unsigned char)s[i]);
  return h;
}

static uint64_t sweep() {
  uint64_t h = 0xcbf29ce484222325ull;
  for (int dt = 0; dt < 2; ++dt)
    for (int mode = 0; mode < 4; ++mode)
      for (const auto &g : GEOMS)
        for (const auto &c : CHANS) {
          for (const auto &f : FLAGS) {
            const rr_igemm_desc d = {dt, mode, g[0], g[1], g[2], c[0], c[1], c[2], f[0], f[1], f[2], f[3], f[4], f[5], f[6]};
            h = fold(h, rr_igemm_kernel_name(&d, 0));
            h = fold(h, rr_igemm_kernel_name(&d, 1));
            h = fold(h, (uint64_t)rr_igemm_stat_blocks(&d));
            h = fold(h, (uint64_t)rr_igemm_bnbwd_rows(&d));
            h = fold(h, (uint64_t)rr_igemm_bnbwd_workspace(&d));
            h = fold(h, rr_igemm_pool_kernel_name(&d, 0));
            h = fold(h, rr_igemm_pool_kernel_name(&d, 1));
            h = fold(h, rr_igemm_dgrad_sc_kernel_name(&d, 64));
            h = fold(h, (uint64_t)rr_igemm_pre_ok(&d));
          }
          for (int acc = 0; acc < 2; ++acc) {
            const rr_wgrad_desc d = {dt, mode, g[0], g[1], g[2], c[0], c[1], c[2], acc};
            h = fold(h, rr_wgrad_kernel_name(&d));
            h = fold(h, (uint64_t)rr_wgrad_workspace(&d));
            h = fold(h, (uint64_t)rr_wgrad_pre_ok(&d));
          }
        }
  return h;
}

int main() {
  const int NT = 8;
  uint64_t got[NT] = {};
  std::vector<std::thread> th;
  for (int i = 0; i < NT; ++i) th.emplace_back([&got, i] { got[i] = sweep(); });
  for (auto &t : th) t.join();
  for (int i = 1; i < NT; ++i)
    if (got[i] != got[0]) {
      fprintf(stderr, "route_check: thread %d answered %016llx, thread 0 %016llx\n", i,
              (unsigned long long)got[i], (unsigned long long)got[0]);
      return 1;
    }
  printf("route_check: 8 threads agree, hash %016llx\n", (unsigned long long)got[0]);
  return 0;
}
