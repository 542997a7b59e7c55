// route_check -- host-only sanitizer harness of the routing sources, two
// builds of one file (csrc/Makefile), both with ASan + UBSan on the host side,
// linked against the routing objects alone; no GPU, nothing is launched.
//
// `make routecheck`: every kernel-name, partial-row and workspace query of
// the library over the sweep of tests/route_sweep.py, from 8 threads at once.
// Each thread folds its answers into a hash: all threads must agree, and the
// sanitizers must stay silent.  RR_PATH is taken from the environment, as the
// library does.
//
// `make launchcheck` (-DRR_DRYRUN, against the objects built with it): the
// launching entry points over the same sweep, with fake device pointers.  The
// objects hand every launch to rr_dry_launch below instead of performing it
// (csrc/common.h), so each call leaves one row: its descriptor, its status
// and, per launch in order, the kernel instance with its full template
// argument list, the grid and the block.  The instance is the kernel handle's
// symbol: the harness is linked -no-pie and reads `nm` of itself (argv[1]).
// One SHA-256 per RR_PATH setting over the rows, and the readable rows of the
// model shapes, are written as tests/golden/launch_*.json are; the make target
// compares them byte for byte.  argv[3]: also write every row there.
#include <cxxabi.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
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

#ifndef RR_DRYRUN

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

#else   // RR_DRYRUN: the launch table

// the ten RR_PATH settings of tests/test_routing_cpu.py
static const char *const PATHS[] = {"", "stream3=0", "conv3r=0", "stream3=0,conv3r=0", "swgrad=0",
                                    "swgrad=0,wgrad_halo=0", "stream1=0", "conv3r_wg=8", "stream3_strips=0",
                                    "stream1_minp=256"};
// Descriptors of the launch sweep alone (tests/route_sweep.py and its digests
// stay as they are), on the 64 -> 64 bf16 3x3 maps: the two stream3 flag sets
// the table above does not reach -- the BN statistics without bias, and the
// index-free pool that also keeps the full-size output (ReLU | POOL)
static const int MORE_GEOMS[][3] = {{512, 64, 64}, {512, 32, 32}, {16, 224, 224}};
static const int MORE_FLAGS[][7] = {{0, 0, 0, 0, 0, 1, 0}, {0, 9, 0, 1, 0, 0, 0}};

// ---- SHA-256 (FIPS 180-4) ----
struct Sha256 {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint8_t buf[64];
  uint64_t len = 0;
  static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t *p) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98,
        0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786,
        0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8,
        0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819,
        0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a,
        0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7,
        0xc67178f2};
    uint32_t w[64], v[8];
    for (int i = 0; i < 16; ++i)
      w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i)
      w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] +
             (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10));
    memcpy(v, h, sizeof v);
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = v[7] + (ror(v[4], 6) ^ ror(v[4], 11) ^ ror(v[4], 25)) + ((v[4] & v[5]) ^ (~v[4] & v[6])) +
                          K[i] + w[i];
      const uint32_t t2 = (ror(v[0], 2) ^ ror(v[0], 13) ^ ror(v[0], 22)) + ((v[0] & v[1]) ^ (v[0] & v[2]) ^ (v[1] & v[2]));
      for (int j = 7; j > 0; --j) v[j] = v[j - 1];
      v[4] += t1;
      v[0] = t1 + t2;
    }
    for (int i = 0; i < 8; ++i) h[i] += v[i];
  }
  void add(const void *data, size_t n) {
    const uint8_t *p = (const uint8_t *)data;
    for (size_t i = 0; i < n; ++i) {
      buf[len++ % 64] = p[i];
      if (len % 64 == 0) block(buf);
    }
  }
  std::string hex() {
    const uint64_t bits = len * 8;
    const uint8_t one = 0x80, zero = 0;
    add(&one, 1);
    while (len % 64 != 56) add(&zero, 1);
    for (int i = 7; i >= 0; --i) {
      const uint8_t b = (uint8_t)(bits >> (8 * i));
      add(&b, 1);
    }
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

// ---- the recorder ----
static std::map<uintptr_t, std::string> g_syms;   // kernel handle -> instance
static std::string g_launches;                    // of the call in flight
static std::map<std::string, int> g_instances;    // every instance seen -> launches

extern "C" void rr_dry_launch(const void *kernel, const unsigned *g, const unsigned *b) {
  const auto it = g_syms.find((uintptr_t)kernel);
  if (it == g_syms.end()) {
    fprintf(stderr, "launch_check: no symbol at kernel handle %p\n", kernel);
    exit(2);
  }
  ++g_instances[it->second];
  char dims[96];
  snprintf(dims, sizeof dims, " grid %u,%u,%u block %u,%u,%u", g[0], g[1], g[2], b[0], b[1], b[2]);
  g_launches += " | " + it->second + dims;
}

// `nm` lines "addr type symbol": the data symbols that are kernel handles
// (ASan pads them under a suffixed name), demangled and cut down to
// "kernel<arguments>" (return type, namespaces and parameter list dropped)
static bool load_syms(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) return false;
  char line[4096];
  while (fgets(line, sizeof line, f)) {
    char *end;
    const unsigned long long addr = strtoull(line, &end, 16);
    if (end == line || end[0] != ' ' || !strchr("rRdDbBvV", end[1]) || end[2] != ' ') continue;
    std::string s(end + 3);
    while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
    if (s.find("_kernel") == std::string::npos && s.find("wgrad_reduce") == std::string::npos) continue;
    const size_t pad = s.find("__sanitized_padded_global");
    if (pad != std::string::npos) s.erase(pad);
    int st = 0;
    char *dm = abi::__cxa_demangle(s.c_str(), nullptr, nullptr, &st);
    if (dm) s = dm;
    free(dm);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    for (size_t p; (p = s.find("(anonymous namespace)::")) != std::string::npos;) s.erase(p, 23);
    int depth = 0;
    for (size_t i = 0; i < s.size(); ++i) {
      depth += s[i] == '<' ? 1 : s[i] == '>' ? -1 : 0;
      if (s[i] == '(' && depth == 0) {
        s.erase(i);
        break;
      }
    }
    g_syms[(uintptr_t)addr] = s;
  }
  fclose(f);
  return !g_syms.empty();
}

// one RR_PATH setting's table
struct Table {
  Sha256 sha;
  long rows = 0, ok = 0;
  FILE *full = nullptr;
  std::vector<std::string> *keep = nullptr;   // the model shapes' rows
  void row(const char *entry, const int *desc, int nd, bool model, const std::string &status) {
    std::string r = entry;
    for (int i = 0; i < nd; ++i) r += (i ? "," : " ") + std::to_string(desc[i]);
    r += " -> " + status + g_launches;
    g_launches.clear();
    sha.add(r.data(), r.size());
    sha.add("\n", 1);
    ++rows;
    if (full) fprintf(full, "%s\n", r.c_str());
    // (of the model shapes, the calls that launch)
    if (keep && model && r.find(" | ") != std::string::npos) keep->push_back(r);
  }
  void row(const char *entry, const int *desc, int nd, bool model, int status) {
    ok += status == RR_OK;
    row(entry, desc, nd, model, std::to_string(status));
  }
};

// distinct fake device pointers: the host side never reads through them
static void *fake(int i) { return (void *)(uintptr_t)(0x10000000ull * (unsigned)(i + 1)); }

static void conv_rows(Table &t, const rr_igemm_desc &d, bool model) {
  int k[15];
  static_assert(sizeof k == sizeof d, "rr_igemm_desc: 15 int32 fields");
  memcpy(k, &d, sizeof k);
  const void *x1 = fake(0), *x2 = d.c_in2 ? fake(1) : nullptr, *w = fake(2), *mask = d.has_mask ? fake(5) : nullptr;
  const float *bias = d.has_bias ? (const float *)fake(3) : nullptr;
  void *y1 = fake(6), *y2 = d.out_split ? fake(7) : nullptr;
  float *stats = d.want_stats ? (float *)fake(8) : nullptr;
  t.row("igemm", k, 15, model, rr_igemm(&d, x1, x2, w, bias, y1, y2, mask, stats, nullptr));
  const bool ex = d.act > 0;
  t.row("igemm_ex", k, 15, model,
        rr_igemm_ex(&d, x1, x2, w, bias, ex && (d.act & 3) == RR_ACT_PRELU ? (const float *)fake(9) : nullptr,
                    ex && (d.act & RR_ACT_RES) ? fake(10) : nullptr, ex && (d.act & RR_ACT_NOFULL) ? nullptr : y1,
                    ex && (d.act & RR_ACT_POOL) ? fake(11) : nullptr, mask, stats, nullptr));
  t.row("igemm_pre", k, 15, model,
        rr_igemm_pre(&d, x1, w, (const float *)fake(3), (const float *)fake(12), (const float *)fake(13),
                     (const float *)fake(14), y1, (float *)fake(8), nullptr));
  t.row("igemm_pool", k, 15, model, rr_igemm_pool(&d, x1, x2, w, bias, fake(11), nullptr, nullptr));
  t.row("igemm_pool_idx", k, 15, model, rr_igemm_pool(&d, x1, x2, w, bias, fake(11), (uint8_t *)fake(15), nullptr));
  t.row("igemm_dgrad_sc", k, 15, model, rr_igemm_dgrad_sc(&d, x1, w, fake(16), fake(17), 64, y1, nullptr));
  t.row("igemm_bnbwd", k, 15, model,
        rr_igemm_bnbwd(&d, x1, w, fake(18), (const float *)fake(19), (const float *)fake(20), (const float *)fake(21),
                       (const float *)fake(22), (const float *)fake(9), y1, (float *)fake(23), nullptr));
}

static void wgrad_rows(Table &t, const rr_wgrad_desc &d, bool model) {
  int k[9];
  static_assert(sizeof k == sizeof d, "rr_wgrad_desc: 9 int32 fields");
  memcpy(k, &d, sizeof k);
  const void *dy = fake(0), *x1 = fake(1), *x2 = d.c_in2 ? fake(2) : nullptr;
  float *dw = (float *)fake(3);
  void *ws = fake(4);
  const size_t wsb = rr_wgrad_workspace(&d);
  t.row("wgrad", k, 9, model, rr_wgrad(&d, dy, x1, x2, dw, ws, wsb, nullptr));
  const int p = rr_wgrad_partial(&d, dy, x1, x2, ws, wsb, nullptr);
  const int r = rr_wgrad_reduce(&d, ws, wsb, dw, nullptr);
  t.ok += p == RR_OK && r == RR_OK;
  t.row("wgrad_partial+reduce", k, 9, model, std::to_string(p) + "," + std::to_string(r));
  t.row("wgrad_pre", k, 9, model,
        rr_wgrad_pre(&d, dy, x1, (const float *)fake(5), (const float *)fake(6), (const float *)fake(7), dw, ws, wsb,
                     nullptr));
}

static void launch_sweep(Table &t) {
  for (int dt = 0; dt < 2; ++dt)
    for (int mode = 0; mode < 4; ++mode)
      for (const auto &g : GEOMS)
        for (const auto &c : CHANS) {
          // (the model shapes of tests/route_sweep.py)
          const bool model = mode < 2 && ((g[0] == 512 && g[1] == 64) || (g[0] == 16 && g[1] == 224)) && c[0] == 64 &&
                             (c[2] == 64 || c[2] == 3);
          for (const auto &f : FLAGS)
            conv_rows(t, {dt, mode, g[0], g[1], g[2], c[0], c[1], c[2], f[0], f[1], f[2], f[3], f[4], f[5], f[6]}, model);
          for (int acc = 0; acc < 2; ++acc) wgrad_rows(t, {dt, mode, g[0], g[1], g[2], c[0], c[1], c[2], acc}, model);
        }
  for (const auto &g : MORE_GEOMS)
    for (const auto &f : MORE_FLAGS)
      conv_rows(t, {RR_BF16, RR_CONV3X3, g[0], g[1], g[2], 64, 0, 64, f[0], f[1], f[2], f[3], f[4], f[5], f[6]}, false);
}

int main(int argc, char **argv) {
  if (argc < 3 || !load_syms(argv[1])) {
    fprintf(stderr, "usage: launch_check <nm of this binary> <output directory> [full table]\n");
    return 2;
  }
  const std::string dir = argv[2];
  FILE *full = argc > 3 ? fopen(argv[3], "w") : nullptr;
  FILE *dg = fopen((dir + "/launch_sweep_digest.json").c_str(), "w");
  FILE *mr = fopen((dir + "/launch_model_rows.json").c_str(), "w");
  if (!dg || !mr || (argc > 3 && !full)) {
    fprintf(stderr, "launch_check: cannot write under %s\n", dir.c_str());
    return 2;
  }
  fprintf(dg, "{\n \"paths\": {\n");
  std::vector<std::string> model;
  for (size_t i = 0; i < sizeof PATHS / sizeof PATHS[0]; ++i) {
    setenv("RR_PATH", PATHS[i], 1);
    Table t;
    t.full = full;
    t.keep = i == 0 ? &model : nullptr;
    if (full) fprintf(full, "RR_PATH=%s\n", PATHS[i]);
    launch_sweep(t);
    fprintf(dg, "  \"%s\": {\"rows\": %ld, \"ok\": %ld, \"sha256\": \"%s\"}%s\n", PATHS[i], t.rows, t.ok,
            t.sha.hex().c_str(), i + 1 < sizeof PATHS / sizeof PATHS[0] ? "," : "");
  }
  // distinct kernel instances the ten tables name, per kernel template
  std::map<std::string, int> fam;
  for (const auto &kv : g_instances) ++fam[kv.first.substr(0, kv.first.find('<'))];
  fprintf(dg, " },\n \"instances\": {");
  const char *sep = "";
  for (const auto &kv : fam) {
    fprintf(dg, "%s\"%s\": %d", sep, kv.first.c_str(), kv.second);
    sep = ", ";
  }
  fprintf(dg, "}\n}\n");
  fprintf(mr, "{\n\"\": [\n");
  for (size_t i = 0; i < model.size(); ++i) fprintf(mr, "  \"%s\"%s\n", model[i].c_str(), i + 1 < model.size() ? "," : "");
  fprintf(mr, "]\n}\n");
  fclose(dg);
  fclose(mr);
  if (full) {
    fprintf(full, "instances\n");
    for (const auto &kv : g_instances) fprintf(full, "%s %d\n", kv.first.c_str(), kv.second);
    fclose(full);
  }
  printf("launch_check: %zu kernel instances launched over %zu RR_PATH settings\n", g_instances.size(),
         sizeof PATHS / sizeof PATHS[0]);
  return 0;
}

#endif
