// The arithmetic of the LPIPS distance head (rcdms_amd/csrc/lpips_core.h) on one CPU thread: the same per-lane sums, group
// trees, float64 tile tree and fixed sum over the tile partials as lpips.hip, with loops where the device has lanes and
// workgroups.  It is how the core is checked against the numpy model (tests/lpips_oracle.py: the same bits) before a GPU runs
// it, and it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/lpips_host.cpp -o lpips_host
//   lpips_host pairs hw c lda ldb a.raw b.raw lin.raw
// a.raw / b.raw hold pairs * hw * lda / ldb uint16 values, the bit patterns of the f16 pixel rows (columns c .. ld - 1 are
// never read); lin.raw holds c float32 values.  Prints one line per pair: the distance (17 significant digits).
// Exit status 2: bad arguments or an unreadable file.  Every buffer is allocated at its exact size, so that a read or write
// one element outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lpips_core.h"

namespace {

template <typename T>
bool read_raw(const char* path, size_t count, std::vector<T>& out) {
  out.assign(count, T(0));
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  const size_t got = fread(out.data(), sizeof(T), count, fp);
  const bool at_end = fgetc(fp) == EOF;
  fclose(fp);
  return got == count && at_end;
}

// IEEE binary16 bits -> float, exact
float widen(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u, man = h & 1023u;
  uint32_t bits;
  if (exp == 31u) {
    bits = sign | 0x7f800000u | (man << 13);
  } else if (exp != 0u) {
    bits = sign | ((exp + 112u) << 23) | (man << 13);
  } else if (man == 0u) {
    bits = sign;
  } else {
    uint32_t m = man, e = 113u;
    while (!(m & 1024u)) m <<= 1, --e;
    bits = sign | (e << 23) | ((m & 1023u) << 13);
  }
  float f;
  memcpy(&f, &bits, sizeof f);
  return f;
}

// lane k's chunk of one pixel row, zeros for a lane past the channels
void chunk(const uint16_t* row, int c, int k, float* v) {
  for (int e = 0; e < lp::CHUNK; ++e) v[e] = k * lp::CHUNK < c ? widen(row[k * lp::CHUNK + e]) : 0.0f;
}

float pixel(const uint16_t* ra, const uint16_t* rb, const float* lin, int c) {
  const int L = lp::lanes(c);
  std::vector<float> sa(L), sb(L), term(L), fa((size_t)L * lp::CHUNK), fb((size_t)L * lp::CHUNK);
  for (int k = 0; k < L; ++k) {
    chunk(ra, c, k, &fa[(size_t)k * lp::CHUNK]);
    chunk(rb, c, k, &fb[(size_t)k * lp::CHUNK]);
    sa[k] = lp::sumsq8(&fa[(size_t)k * lp::CHUNK]);
    sb[k] = lp::sumsq8(&fb[(size_t)k * lp::CHUNK]);
  }
  const float na = lp::norm(lp::group_tree(sa.data(), L)), nb = lp::norm(lp::group_tree(sb.data(), L));
  for (int k = 0; k < L; ++k) {
    float w[lp::CHUNK];
    for (int e = 0; e < lp::CHUNK; ++e) w[e] = k * lp::CHUNK < c ? lin[k * lp::CHUNK + e] : 0.0f;
    term[k] = lp::term8(&fa[(size_t)k * lp::CHUNK], &fb[(size_t)k * lp::CHUNK], na, nb, w);
  }
  return lp::group_tree(term.data(), L);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: lpips_host pairs hw c lda ldb a.raw b.raw lin.raw\n");
    return 2;
  }
  const int pairs = atoi(argv[1]), c = atoi(argv[3]);
  const long long hw = atoll(argv[2]), lda = atoll(argv[4]), ldb = atoll(argv[5]);
  if (pairs < 1 || pairs > lp::MAX_PAIRS || hw < 1 || hw > (1ll << 26) || c < 8 || c > lp::MAX_C || c % 8 || lda < c || ldb < c ||
      lda % 8 || ldb % 8 || lda > 65536 || ldb > 65536) {
    fprintf(stderr, "lpips_host: pairs 1..%d, hw 1..2^26, c a multiple of 8 up to %d, ld a multiple of 8 from c to 65536\n",
            lp::MAX_PAIRS, lp::MAX_C);
    return 2;
  }
  std::vector<uint16_t> a, b;
  std::vector<float> lin;
  if (!read_raw(argv[6], (size_t)pairs * hw * lda, a) || !read_raw(argv[7], (size_t)pairs * hw * ldb, b) ||
      !read_raw(argv[8], (size_t)c, lin)) {
    fprintf(stderr, "lpips_host: the row files must hold exactly pairs * hw * ld uint16 values, the lin file c float32 values\n");
    return 2;
  }
  const int64_t tiles = lp::tiles(hw);
  for (int p = 0; p < pairs; ++p) {
    std::vector<double> partials((size_t)tiles), vals(lp::TILE), lanes(fr::LANES, 0.0);
    for (int64_t t = 0; t < tiles; ++t) {
      for (int q = 0; q < lp::TILE; ++q) {
        const int64_t pix = t * lp::TILE + q;
        const size_t row = (size_t)p * hw + pix;
        vals[q] = pix < hw ? (double)pixel(&a[row * lda], &b[row * ldb], lin.data(), c) : 0.0;
      }
      partials[(size_t)t] = lp::tile_tree(vals.data());
    }
    for (int t = 0; t < fr::LANES; ++t)
      for (int64_t k = t; k < tiles; k += fr::LANES) lanes[t] += partials[(size_t)k];
    printf("%.17g\n", lp::pair_mean(fr::tree_sum(lanes.data()), hw));
  }
  return 0;
}
