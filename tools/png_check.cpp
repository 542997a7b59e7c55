// png_check.cpp -- host sanitizer harness of the PNG reader's host half
// (csrc/png.cpp: rr_png_probe, rr_png_inflate).  Built by `make -C csrc
// pngcheck` with png.cpp under ASan + UBSan, linked with zlib and nothing
// else, and run on the build machine: no GPU, no Python.
//
// It writes a small valid file and feeds probe and inflate with damaged
// copies of it.  Every case must come back with a status; the destination
// slot is a heap block of exactly h * (1 + w * c) bytes, so ASan's redzone
// stands right behind (and in front of) it and any write outside the slot
// stops the run.
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/roadrestore.h"

namespace {

typedef std::vector<uint8_t> Bytes;
int failures = 0, cases = 0;
std::string tmp_path;

void put32(Bytes &o, uint32_t v) {
  o.push_back(v >> 24); o.push_back((v >> 16) & 255); o.push_back((v >> 8) & 255); o.push_back(v & 255);
}

void chunk(Bytes &o, const char *type, const Bytes &data) {
  put32(o, (uint32_t)data.size());
  const size_t t0 = o.size();
  o.insert(o.end(), type, type + 4);
  o.insert(o.end(), data.begin(), data.end());
  put32(o, (uint32_t)crc32(0L, o.data() + t0, (uInt)(data.size() + 4)));
}

Bytes header(uint32_t w, uint32_t h, int depth, int colour, int lace) {
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  Bytes o(sig, sig + 8), ihdr;
  put32(ihdr, w); put32(ihdr, h);
  ihdr.push_back(depth); ihdr.push_back(colour); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(lace);
  chunk(o, "IHDR", ihdr);
  return o;
}

Bytes deflate(const Bytes &raw) {
  uLongf n = compressBound((uLong)raw.size());
  Bytes z(n);
  if (compress2(z.data(), &n, raw.data(), (uLong)raw.size(), 6) != Z_OK) abort();
  z.resize(n);
  return z;
}

// a whole file around a scanline stream, the zlib data cut into `piece`-byte IDAT chunks
Bytes file_of(int w, int h, int colour, const Bytes &stream, size_t piece = 0) {
  Bytes o = header(w, h, 8, colour, 0), z = deflate(stream);
  if (!piece) piece = z.size();
  for (size_t a = 0; a < z.size(); a += piece)
    chunk(o, "IDAT", Bytes(z.begin() + a, z.begin() + std::min(z.size(), a + piece)));
  chunk(o, "IEND", Bytes());
  return o;
}

struct Result { int probe_rc, inflate_rc; rr_png_info probe, inflate; Bytes slot; };

// probe + inflate of `file` with a record of (h, w, c); the slot is its own heap block
Result run(const Bytes &file, int h, int w, int c, long long slot_bytes = -1) {
  FILE *f = fopen(tmp_path.c_str(), "wb");
  if (!f || (!file.empty() && fwrite(file.data(), 1, file.size(), f) != file.size())) { perror("png_check: tmp file"); exit(2); }
  fclose(f);
  Result r;
  const char *paths[1] = {tmp_path.c_str()};
  r.probe_rc = rr_png_probe(1, paths, &r.probe, 1);
  const long long need = slot_bytes >= 0 ? slot_bytes : (long long)h * (1 + (long long)w * c);
  uint8_t *slot = (uint8_t *)malloc(need ? need : 1);
  memset(slot, 0xEE, need ? need : 1);
  const rr_png_image rec = {0, 0, h, w, c, 1};
  r.inflate_rc = rr_png_inflate(1, paths, &rec, slot, (size_t)need, &r.inflate, 1);
  r.slot.assign(slot, slot + need);
  free(slot);
  ++cases;
  return r;
}

void expect(bool ok, const char *what, long long detail = -1) {
  if (ok) return;
  ++failures;
  if (failures <= 20) fprintf(stderr, "png_check: FAILED %s (%lld)\n", what, detail);
}

bool refused(const Result &r) {
  return r.inflate_rc != RR_OK && r.inflate.status == r.inflate_rc &&
         (r.inflate_rc == RR_EINVAL || r.inflate_rc == RR_EUNSUPPORTED) && r.inflate.reason != RR_PNG_OK;
}

}  // namespace

int main() {
  const char *dir = getenv("TMPDIR");
  tmp_path = std::string(dir && *dir ? dir : "/tmp") + "/rr_png_check_XXXXXX";
  const int fd = mkstemp(&tmp_path[0]);
  if (fd < 0) { perror("png_check: mkstemp"); return 2; }

  const int H = 6, W = 5, C = 3;
  Bytes img((size_t)H * W * C);
  for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)(i * 37 + (i >> 3) * 11);
  // the library's own writer makes the valid file
  const long long cap = rr_png_encode(H, W, C, img.data(), 6, nullptr, 0);
  Bytes good((size_t)cap);
  if (cap <= 0 || rr_png_encode(H, W, C, img.data(), 6, good.data(), cap) != cap) return 2;

  Result r = run(good, H, W, C);
  expect(r.probe_rc == RR_OK && r.probe.h == H && r.probe.w == W && r.probe.channels == C, "probe of the valid file");
  expect(r.inflate_rc == RR_OK && r.inflate.status == RR_OK, "inflate of the valid file", r.inflate.reason);
  const Bytes stream = r.slot;                         // its filtered scanlines
  for (int y = 0; y < H; ++y) expect(stream[(size_t)y * (1 + W * C)] <= 4, "filter byte of the valid file", y);

  // the same stream in 1-byte IDAT chunks, and with empty chunks between
  r = run(file_of(W, H, 2, stream, 1), H, W, C);
  expect(r.inflate_rc == RR_OK && r.slot == stream, "1-byte IDAT chunks");

  // truncated at every length
  for (size_t n = 0; n < good.size(); ++n) {
    r = run(Bytes(good.begin(), good.begin() + n), H, W, C);
    expect(refused(r), "truncation accepted at length", (long long)n);
    expect(r.probe_rc == RR_OK || r.probe.status == r.probe_rc, "probe status of a truncation", (long long)n);
  }

  // every single-byte corruption of the header and the chunk framing: the
  // signature, the IHDR chunk, and length / type / CRC of IDAT and IEND
  std::vector<size_t> framing;
  for (size_t i = 0; i < 33; ++i) framing.push_back(i);
  for (size_t i = 33; i < 41; ++i) framing.push_back(i);                          // IDAT length, type
  for (size_t i = good.size() - 16; i < good.size(); ++i) framing.push_back(i);   // IDAT CRC, IEND
  const uint8_t masks[] = {0x01, 0x20, 0x80, 0xFF};
  for (size_t pos : framing)
    for (uint8_t m : masks) {
      Bytes bad = good;
      bad[pos] ^= m;
      r = run(bad, H, W, C);
      expect(refused(r), "corrupted framing byte accepted", (long long)pos);
    }
  // ... and of every data byte of IDAT: a status, whichever
  for (size_t pos = 41; pos < good.size() - 16; ++pos) {
    Bytes bad = good;
    bad[pos] ^= 0x10;
    r = run(bad, H, W, C);
    expect(refused(r), "corrupted IDAT byte accepted (CRC)", (long long)pos);
  }

  // a chunk length past the end of the file
  const uint32_t idat_len = ((uint32_t)good[33] << 24) | (good[34] << 16) | (good[35] << 8) | good[36];
  for (uint32_t len : {idat_len + 1, idat_len + 13, 0x7fffffffu, 0x80000000u, 0xffffffffu}) {
    Bytes bad = good;
    bad[33] = len >> 24; bad[34] = (len >> 16) & 255; bad[35] = (len >> 8) & 255; bad[36] = len & 255;
    r = run(bad, H, W, C);
    expect(refused(r), "chunk length past the end accepted", len);
  }

  // an IHDR of (2^31 - 1) x (2^31 - 1): refused without allocating
  {
    const uint32_t big = 0x7fffffffu;
    Bytes rgb = header(big, big, 8, 2, 0);             // h * (1 + 3 w) leaves int64
    chunk(rgb, "IDAT", deflate(Bytes(16)));
    chunk(rgb, "IEND", Bytes());
    r = run(rgb, (int)big, (int)big, 3, 64);
    expect(r.probe_rc == RR_EINVAL && r.probe.reason == RR_PNG_EHEADER, "2^31-1 squared RGB probe");
    expect(refused(r), "2^31-1 squared RGB inflate");
    Bytes grey = header(big, big, 8, 0, 0);            // fits int64, not the slot
    chunk(grey, "IDAT", deflate(Bytes(16)));
    chunk(grey, "IEND", Bytes());
    r = run(grey, (int)big, (int)big, 1, 64);
    expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESLOT, "2^31-1 squared grey inflate");
  }

  // IDAT streams one byte short and one byte long; a filter byte of 5
  {
    Bytes s(stream.begin(), stream.end() - 1);
    r = run(file_of(W, H, 2, s), H, W, C);
    expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESIZE, "one byte short");
    s = stream;
    s.push_back(0);
    r = run(file_of(W, H, 2, s), H, W, C);
    expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESIZE, "one byte long");
    s.insert(s.end(), 70000, 7);                       // much longer: still nothing past the slot
    r = run(file_of(W, H, 2, s, 1000), H, W, C);
    expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESIZE, "70000 bytes long");
    s = stream;
    s[(size_t)3 * (1 + W * C)] = 5;
    r = run(file_of(W, H, 2, s), H, W, C);
    expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_EFILTER, "filter byte 5");
  }

  // a slot one byte smaller than the file needs, and a record of another size
  r = run(good, H, W, C, (long long)stream.size() - 1);
  expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESLOT, "slot one byte small");
  r = run(good, H + 1, W, C);
  expect(r.inflate_rc == RR_EINVAL && r.inflate.reason == RR_PNG_ESLOT, "record of another height");

  // unsupported kinds, by name
  for (int k = 0; k < 3; ++k) {
    Bytes f = header(W, H, k == 1 ? 16 : 8, k == 0 ? 3 : 2, k == 2 ? 1 : 0);
    chunk(f, "IDAT", deflate(stream));
    chunk(f, "IEND", Bytes());
    r = run(f, H, W, C);
    expect(r.probe_rc == RR_EUNSUPPORTED && r.probe.reason == RR_PNG_EKIND, "unsupported kind (probe)", k);
    expect(r.inflate_rc == RR_EUNSUPPORTED && r.inflate.reason == RR_PNG_EKIND, "unsupported kind (inflate)", k);
  }

  close(fd);
  remove(tmp_path.c_str());
  printf("png_check: %d cases, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
