// png.cpp -- host-side batched PNG encoder for the restored images
// (17_run_unified_inference.py:89-99: clamp -> x255 -> uint8 -> RGB2BGR ->
// cv2.imwrite per image).  cv2.imwrite of the BGR array stores the RGB
// pixels, so the file content is the RGB uint8 image: this writes it
// directly from the NHWC uint8 batch that rr_to_uint8_hwc produced.
//
// Format: 8-bit truecolour (c = 3) or greyscale (c = 1), no interlace, one
// IDAT from zlib (deflate level `level`); per-row filter chosen by the
// minimum-sum-of-absolute-differences heuristic over the five PNG filters
// (libpng's default adaptive choice).  Images are encoded on `threads`
// host threads (one file each); the GPU is not involved.
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/roadrestore.h"

namespace {

void put32(std::vector<uint8_t> &o, uint32_t v) {
  o.push_back(v >> 24); o.push_back((v >> 16) & 255); o.push_back((v >> 8) & 255); o.push_back(v & 255);
}

void chunk(std::vector<uint8_t> &o, const char *type, const uint8_t *data, size_t len) {
  put32(o, (uint32_t)len);
  const size_t t0 = o.size();
  o.insert(o.end(), type, type + 4);
  if (len) o.insert(o.end(), data, data + len);
  const uint32_t crc = (uint32_t)crc32(0L, o.data() + t0, (uInt)(len + 4));
  put32(o, crc);
}

inline uint8_t paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (uint8_t)(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

// filtered scanlines (filter byte + row) of one image
void filter_rows(int h, int w, int c, const uint8_t *img, std::vector<uint8_t> &out) {
  const size_t row = (size_t)w * c;
  out.resize((size_t)h * (row + 1));
  std::vector<uint8_t> cand[5];
  for (auto &v : cand) v.resize(row);
  for (int y = 0; y < h; ++y) {
    const uint8_t *cur = img + (size_t)y * row;
    const uint8_t *up = y ? cur - row : nullptr;
    long best = -1;
    int bf = 0;
    for (int f = 0; f < 5; ++f) {
      uint8_t *d = cand[f].data();
      long sum = 0;
      for (size_t i = 0; i < row; ++i) {
        const int a = i >= (size_t)c ? cur[i - c] : 0;
        const int b = up ? up[i] : 0;
        const int cc = (up && i >= (size_t)c) ? up[i - c] : 0;
        int v = cur[i];
        switch (f) {
          case 1: v -= a; break;
          case 2: v -= b; break;
          case 3: v -= (a + b) >> 1; break;
          case 4: v -= paeth(a, b, cc); break;
          default: break;
        }
        d[i] = (uint8_t)v;
        sum += d[i] < 128 ? d[i] : 256 - d[i];
      }
      if (best < 0 || sum < best) { best = sum; bf = f; }
    }
    uint8_t *o = out.data() + (size_t)y * (row + 1);
    o[0] = (uint8_t)bf;
    memcpy(o + 1, cand[bf].data(), row);
  }
}

int encode(int h, int w, int c, const uint8_t *img, int level, std::vector<uint8_t> &png) {
  std::vector<uint8_t> raw;
  filter_rows(h, w, c, img, raw);
  uLongf zlen = compressBound((uLong)raw.size());
  std::vector<uint8_t> z(zlen);
  if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), level) != Z_OK) return RR_ELAUNCH;
  static const uint8_t sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
  png.assign(sig, sig + 8);
  uint8_t ihdr[13];
  const uint32_t W = (uint32_t)w, H = (uint32_t)h;
  ihdr[0] = W >> 24; ihdr[1] = (W >> 16) & 255; ihdr[2] = (W >> 8) & 255; ihdr[3] = W & 255;
  ihdr[4] = H >> 24; ihdr[5] = (H >> 16) & 255; ihdr[6] = (H >> 8) & 255; ihdr[7] = H & 255;
  ihdr[8] = 8;                       // bit depth
  ihdr[9] = c == 3 ? 2 : 0;          // truecolour / greyscale
  ihdr[10] = ihdr[11] = ihdr[12] = 0;
  chunk(png, "IHDR", ihdr, 13);
  chunk(png, "IDAT", z.data(), zlen);
  chunk(png, "IEND", nullptr, 0);
  return RR_OK;
}

}  // namespace

extern "C" long long rr_png_encode(int h, int w, int c, const uint8_t *hwc, int level, uint8_t *out,
                                   long long cap) {
  if (!hwc || h <= 0 || w <= 0 || (c != 1 && c != 3) || level < 0 || level > 9) return RR_EINVAL;
  std::vector<uint8_t> png;
  if (const int rc = encode(h, w, c, hwc, level, png)) return rc;
  if (out && (long long)png.size() <= cap) memcpy(out, png.data(), png.size());
  return (long long)png.size();
}

extern "C" int rr_png_write_batch(int n, int h, int w, int c, const uint8_t *hwc,
                                  const char *const *paths, int level, int threads) {
  if (n < 0 || !paths || (n > 0 && !hwc) || h <= 0 || w <= 0 || (c != 1 && c != 3) || level < 0 ||
      level > 9)
    return RR_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!paths[i]) return RR_EINVAL;
  int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
  T = std::max(1, std::min(T, n));
  std::atomic<int> next(0), status(RR_OK);
  const size_t img = (size_t)h * w * c;
  auto work = [&]() {
    std::vector<uint8_t> png;
    for (int i = next++; i < n; i = next++) {
      if (encode(h, w, c, hwc + img * i, level, png) != RR_OK) { status = RR_ELAUNCH; continue; }
      FILE *f = fopen(paths[i], "wb");
      if (!f || fwrite(png.data(), 1, png.size(), f) != png.size()) status = RR_EINVAL;
      if (f) fclose(f);
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < T; ++t) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  return status.load();
}

// ---------------------------------------------------------------------------
// PNG input, host half: probe (signature + IHDR) and inflate (IDAT -> filtered
// scanlines) of the files the reference opens with Image.open(p).convert('RGB')
// (17_run_unified_inference.py:69-79, 18_test_unified_benchmark.py:35,
// 07_train_restoration.py:52-66, 08_run_inference.py:84-88).  The row filters
// are undone on the device (png.hip).  Every length that comes out of a file
// is checked against the bytes present before it is used; nothing is sized
// from IHDR alone.
namespace {

constexpr size_t PNG_HEAD = 8 + 8 + 13 + 4;        // signature, IHDR chunk
const uint8_t PNG_SIG[8] = {137, 80, 78, 71, 13, 10, 26, 10};

inline uint32_t get32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

void fail(rr_png_info *o, int status, int reason) {
  o->status = status;
  o->reason = reason;
}

// signature + IHDR of buf[0, len): fills o (status RR_OK on success)
void parse_head(const uint8_t *buf, size_t len, rr_png_info *o) {
  *o = rr_png_info{0, 0, 0, RR_OK, RR_PNG_OK};
  if (len < 8)
    return fail(o, RR_EINVAL, len && memcmp(buf, PNG_SIG, len) ? RR_PNG_ESIGNATURE : RR_PNG_ETRUNCATED);
  if (memcmp(buf, PNG_SIG, 8)) return fail(o, RR_EINVAL, RR_PNG_ESIGNATURE);
  if (len < PNG_HEAD) return fail(o, RR_EINVAL, RR_PNG_ETRUNCATED);
  if (get32(buf + 8) != 13 || memcmp(buf + 12, "IHDR", 4)) return fail(o, RR_EINVAL, RR_PNG_EHEADER);
  if ((uint32_t)crc32(0L, buf + 12, 17) != get32(buf + 29)) return fail(o, RR_EINVAL, RR_PNG_ECRC);
  const uint32_t W = get32(buf + 16), H = get32(buf + 20);
  const int depth = buf[24], colour = buf[25], comp = buf[26], filt = buf[27], lace = buf[28];
  if (W == 0 || H == 0 || W > 0x7fffffffu || H > 0x7fffffffu) return fail(o, RR_EINVAL, RR_PNG_EHEADER);
  bool legal;
  switch (colour) {
    case 0: legal = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16; break;
    case 3: legal = depth == 1 || depth == 2 || depth == 4 || depth == 8; break;
    case 2: case 4: case 6: legal = depth == 8 || depth == 16; break;
    default: legal = false;
  }
  if (!legal || comp != 0 || filt != 0 || lace > 1) return fail(o, RR_EINVAL, RR_PNG_EHEADER);
  o->h = (int32_t)H;
  o->w = (int32_t)W;
  if (colour == 3 || depth != 8 || lace) return fail(o, RR_EUNSUPPORTED, RR_PNG_EKIND);
  const int c = colour == 0 ? 1 : colour == 4 ? 2 : colour == 2 ? 3 : 4;
  const int64_t pitch = 1 + (int64_t)W * c;                     // < 2^34
  if ((int64_t)H > INT64_MAX / pitch) return fail(o, RR_EINVAL, RR_PNG_EHEADER);
  o->channels = c;
}

int64_t png_slot(int h, int w, int c) { return (int64_t)h * (1 + (int64_t)w * c); }

// one file -> its filtered scanlines in slot[0, need)
void inflate_file(const char *path, const rr_png_image &r, uint8_t *base, size_t dst_bytes,
                  rr_png_info *o) {
  *o = rr_png_info{0, 0, 0, RR_OK, RR_PNG_OK};
  FILE *f = fopen(path, "rb");
  if (!f) return fail(o, RR_EINVAL, RR_PNG_EOPEN);
  std::vector<uint8_t> file;
  {
    uint8_t tmp[1 << 16];
    size_t got;
    while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) file.insert(file.end(), tmp, tmp + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(o, RR_EINVAL, RR_PNG_EOPEN);
  }
  parse_head(file.data(), file.size(), o);
  if (o->status != RR_OK) return;
  // the record is what the buffer was sized from: it must be this file's
  if (r.kind != 1 || r.h != o->h || r.w != o->w || r.channels != o->channels)
    return fail(o, RR_EINVAL, RR_PNG_ESLOT);
  const int64_t need = png_slot(o->h, o->w, o->channels);
  if (r.src < 0 || dst_bytes > (size_t)INT64_MAX || r.src > (int64_t)dst_bytes ||
      need > (int64_t)dst_bytes - r.src)
    return fail(o, RR_EINVAL, RR_PNG_ESLOT);
  uint8_t *slot = base + r.src;

  // chunk walk: CRC of every chunk, the IDAT run gathered
  std::vector<uint8_t> idat;
  const uint8_t *p = file.data();
  const size_t size = file.size();
  size_t pos = PNG_HEAD;
  int seen = 0;                  // 0 before IDAT, 1 inside the run, 2 after it
  bool end = false;
  while (!end) {
    if (size - pos < 12) return fail(o, RR_EINVAL, RR_PNG_ETRUNCATED);
    const uint32_t len = get32(p + pos);
    if (len > 0x7fffffffu) return fail(o, RR_EINVAL, RR_PNG_ECHUNK);
    if (size - pos - 12 < len) return fail(o, RR_EINVAL, RR_PNG_ETRUNCATED);
    const uint8_t *type = p + pos + 4, *data = type + 4;
    uLong crc = crc32(0L, type, 4);
    for (size_t done = 0; done < len;) {             // uInt-sized pieces
      const size_t step = std::min<size_t>(len - done, 1u << 30);
      crc = crc32(crc, data + done, (uInt)step);
      done += step;
    }
    if ((uint32_t)crc != get32(data + len)) return fail(o, RR_EINVAL, RR_PNG_ECRC);
    if (!memcmp(type, "IDAT", 4)) {
      if (seen == 2) return fail(o, RR_EINVAL, RR_PNG_ECHUNK);
      seen = 1;
      idat.insert(idat.end(), data, data + len);
    } else {
      if (seen == 1) seen = 2;
      if (!memcmp(type, "IEND", 4)) end = true;
      else if (!memcmp(type, "IHDR", 4)) return fail(o, RR_EINVAL, RR_PNG_ECHUNK);
      else if (!(type[0] & 0x20) && memcmp(type, "PLTE", 4)) return fail(o, RR_EINVAL, RR_PNG_ECHUNK);
    }
    pos += 12 + (size_t)len;
  }
  if (!seen) return fail(o, RR_EINVAL, RR_PNG_ECHUNK);

  // inflate into the slot, then one spare byte: a stream that still has
  // output after `need` bytes is one byte too long at least
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit(&zs) != Z_OK) return fail(o, RR_EINVAL, RR_PNG_EZLIB);
  size_t in_pos = 0;
  int64_t out_pos = 0;
  uint8_t spare = 0;
  int reason = RR_PNG_OK;
  for (;;) {
    if (zs.avail_in == 0 && in_pos < idat.size()) {
      const size_t step = std::min<size_t>(idat.size() - in_pos, 1u << 30);
      zs.next_in = idat.data() + in_pos;
      zs.avail_in = (uInt)step;
      in_pos += step;
    }
    const bool full = out_pos == need;
    const int64_t room = full ? 1 : std::min<int64_t>(need - out_pos, 1 << 30);
    zs.next_out = full ? &spare : slot + out_pos;
    zs.avail_out = (uInt)room;
    const int rc = inflate(&zs, Z_NO_FLUSH);
    const int64_t wrote = room - zs.avail_out;
    if (full && wrote) { reason = RR_PNG_ESIZE; break; }
    if (!full) out_pos += wrote;
    if (rc == Z_STREAM_END) { reason = out_pos == need ? RR_PNG_OK : RR_PNG_ESIZE; break; }
    if (rc == Z_BUF_ERROR || (rc == Z_OK && zs.avail_in == 0 && in_pos == idat.size() && zs.avail_out)) {
      reason = RR_PNG_EZLIB;             // the input ran out before the stream's end
      break;
    }
    if (rc != Z_OK) { reason = RR_PNG_EZLIB; break; }
  }
  inflateEnd(&zs);
  if (reason != RR_PNG_OK) return fail(o, RR_EINVAL, reason);
  const int64_t pitch = 1 + (int64_t)o->w * o->channels;
  for (int64_t y = 0; y < o->h; ++y)
    if (slot[y * pitch] > 4) return fail(o, RR_EINVAL, RR_PNG_EFILTER);
}

template <typename F> int png_pool(int n, int threads, rr_png_info *info, F one) {
  int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
  T = std::max(1, std::min(T, n));
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int i = next++; i < n; i = next++) one(i);
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < T; ++t) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
  for (int i = 0; i < n; ++i)
    if (info[i].status != RR_OK) return info[i].status;
  return RR_OK;
}

}  // namespace

extern "C" int rr_png_probe(int n, const char *const *paths, rr_png_info *info, int threads) {
  if (n <= 0 || !paths || !info) return RR_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!paths[i]) return RR_EINVAL;
  return png_pool(n, threads, info, [&](int i) {
    uint8_t head[PNG_HEAD];
    FILE *f = fopen(paths[i], "rb");
    if (!f) {
      info[i] = rr_png_info{0, 0, 0, RR_EINVAL, RR_PNG_EOPEN};
      return;
    }
    const size_t got = fread(head, 1, sizeof head, f);
    fclose(f);
    parse_head(head, got, &info[i]);
  });
}

extern "C" int rr_png_inflate(int n, const char *const *paths, const rr_png_image *images_host,
                              uint8_t *dst, size_t dst_bytes, rr_png_info *info, int threads) {
  if (n <= 0 || !paths || !images_host || !dst || !info) return RR_EINVAL;
  for (int i = 0; i < n; ++i)
    if (images_host[i].kind == 1 && !paths[i]) return RR_EINVAL;
  return png_pool(n, threads, info, [&](int i) {
    if (images_host[i].kind == 1) inflate_file(paths[i], images_host[i], dst, dst_bytes, &info[i]);
    else info[i] = rr_png_info{images_host[i].h, images_host[i].w, images_host[i].channels, RR_OK, RR_PNG_OK};
  });
}
