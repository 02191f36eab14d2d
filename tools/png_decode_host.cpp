// The PNG reader's shared core (rcdms_amd/csrc/png_inflate.h) on one CPU thread: the same inflate, the same checks and the
// same status codes as rcdm_png_decode, with serial copies in place of the wave's.  It is how the decoder's logic meets
// corrupt files before a GPU does, and it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/png_decode_host.cpp -o png_decode_host
//   png_decode_host [--bgr] a.png b.png ...
// prints one line per file: `<status> <crc32 of the h * w * 3 pixel bytes, hex> <w> <h>`; status -1: not a file the host
// walk of rcdms_amd/image.py would pass on (bit depth, interlace, missing chunks), -2: unreadable.  Every buffer is
// allocated at its exact size, so that a read or write one byte outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "png_inflate.h"

namespace {

struct HostIO {
  static constexpr int LANES = 1;
  int lane = 0;
  const uint8_t* z;
  uint64_t zbytes;
  uint8_t* out;

  uint32_t uni(uint32_t v) const { return v; }
  void sync() const {}
  uint32_t word(uint32_t i) const {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k) {
      uint64_t at = (uint64_t)i * 4 + k;
      if (at < zbytes) v |= (uint32_t)z[at] << (8 * k);
    }
    return v;
  }
  void literal(uint32_t pos, uint8_t b) { out[pos] = b; }
  void match(uint32_t pos, uint32_t L, uint32_t D) {
    for (uint32_t i = 0; i < L; ++i) out[pos + i] = out[pos - D + i % D];
  }
  void stored(uint64_t at, uint32_t pos, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) out[pos + i] = z[at + i];
  }
  uint32_t adler(uint32_t pos) const {
    uint32_t s1 = 1, s2 = 0;
    for (uint32_t at = 0; at < pos;) {
      uint32_t n = pos - at < 4096 ? pos - at : 4096, sum = 0, weighted = 0;
      for (uint32_t p = 0; p < n; ++p) {
        sum += out[at + p];
        weighted += (n - p) * out[at + p];
      }
      pngd::adler_advance(s1, s2, n, sum, weighted);
      at += n;
    }
    return (s2 << 16) | s1;
  }
};

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

uint32_t crc32(const uint8_t* p, size_t n) {
  static uint32_t table[256];
  if (!table[1])
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      table[i] = c;
    }
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// -> status; pixels: h * w * 3
int decode(const std::vector<uint8_t>& f, bool bgr, std::vector<uint8_t>& pixels, uint32_t& w, uint32_t& h) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  w = h = 0;
  if (f.size() < 8 || memcmp(f.data(), sig, 8)) return -1;
  uint32_t ct = 0, plte_entries = 0;
  bool ihdr = false;
  std::vector<uint8_t> z, plte;
  for (size_t off = 8; off + 12 <= f.size();) {
    uint32_t n = be32(&f[off]);
    if (n > f.size() - off - 12) return -1;
    const uint8_t* kind = &f[off + 4];
    const uint8_t* body = &f[off + 8];
    if (!memcmp(kind, "IHDR", 4)) {
      if (n != 13 || body[8] != 8 || body[10] || body[11] || body[12]) return -1;
      w = be32(body);
      h = be32(body + 4);
      ct = body[9];
      if (!pngd::bytes_per_pixel(ct) || w < 1 || h < 1 || w > 8192 || h > 8192) return -1;
      ihdr = true;
    } else if (!memcmp(kind, "PLTE", 4)) {
      plte.assign(body, body + n);
      plte_entries = n / 3 > 256 ? 256 : n / 3;
    } else if (!memcmp(kind, "IDAT", 4)) {
      z.insert(z.end(), body, body + n);
    } else if (!memcmp(kind, "IEND", 4)) {
      break;
    }
    off += 12 + (size_t)n;
  }
  if (!ihdr || z.empty() || (ct == 3 && plte.empty())) return -1;
  const int bpp = pngd::bytes_per_pixel(ct);
  const size_t S = 1 + (size_t)bpp * w;
  std::vector<uint8_t> raw(h * S);
  pngd::Tables* T = new pngd::Tables;
  HostIO io;
  io.z = z.data();
  io.zbytes = z.size();
  io.out = raw.data();
  int st = pngd::inflate(io, *T, z.size(), (uint32_t)raw.size());
  delete T;
  if (st) return st;
  for (uint32_t r = 0; r < h; ++r)
    if (raw[r * S] > 4) return pngd::EFILTER;
  pixels.assign((size_t)h * w * 3, 0);
  for (uint32_t r = 0; r < h; ++r) {
    uint8_t* row = &raw[r * S + 1];
    const uint8_t* up = r ? &raw[(r - 1) * S + 1] : nullptr;
    uint32_t ft = raw[r * S];
    for (uint32_t x = 0; x < w; ++x) {
      uint32_t px = 0;
      for (int k = 0; k < bpp; ++k) {
        size_t i = (size_t)x * bpp + k;
        uint32_t a = x ? row[i - bpp] : 0, b = up ? up[i] : 0, c = (x && up) ? up[i - bpp] : 0;
        row[i] = (uint8_t)pngd::unfilter_byte(ft, row[i], a, b, c);
        px |= (uint32_t)row[i] << (8 * k);
      }
      uint32_t rgb = pngd::to_rgb(ct, px, plte.data(), plte_entries);
      uint8_t* o = &pixels[((size_t)r * w + x) * 3];
      o[bgr ? 2 : 0] = (uint8_t)rgb;
      o[1] = (uint8_t)(rgb >> 8);
      o[bgr ? 0 : 2] = (uint8_t)(rgb >> 16);
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  bool bgr = false;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--bgr")) {
      bgr = true;
      continue;
    }
    std::vector<uint8_t> f, pixels;
    uint32_t w = 0, h = 0;
    int st = -2;
    if (FILE* fp = fopen(argv[a], "rb")) {
      uint8_t buf[65536];
      for (size_t n; (n = fread(buf, 1, sizeof buf, fp)) > 0;) f.insert(f.end(), buf, buf + n);
      fclose(fp);
      st = decode(f, bgr, pixels, w, h);
    }
    printf("%d %08x %u %u\n", st, st == 0 ? crc32(pixels.data(), pixels.size()) : 0u, w, h);
  }
  return 0;
}
