// The rules of the denoising objective (rcdms_amd/csrc/objective_core.h) on one CPU thread: the same target, add-noise
// expression, row layout, chunking and fixed-order sums as objective.hip, with loops where the device has lanes and blocks.
// It is how the core is checked against the numpy model (tests/objective_oracle.py) before a GPU runs it, and it builds with
// sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/objective_host.cpp -o objective_host
//   objective_host rows B f H W ld c_pad T offs_scale x0.raw noise.raw t.raw table.raw mask.raw masked.raw [offs.raw]
//       x0, noise, masked: B*4*f*H*W float32; mask: B*f*H*W float32; t: B int64; table: T*2 float32; offs: B*4*f float32 (left
//       out: no offset, offs_scale is not read).  Prints the B*f*H*W rows, ld hexadecimal 16-bit words each; a column the
//       core does not write prints as ffff.
//   objective_host sqerr B f H W ld offs_scale eps.raw noise.raw [offs.raw]
//       eps.raw: B*f*H*W rows of ld 16-bit words (f16 bits), channels 0..3 read.  Prints the B*f sums, one per line, as the 16
//       hexadecimal digits of the float64.
// Exit status 2: bad arguments or an unreadable file.  Every buffer is allocated at its exact size, so that a read or write one
// element outside it is seen.  Needs a compiler with _Float16 (clang, or gcc 12 and later on x86-64).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "objective_core.h"

#pragma clang fp contract(off)

namespace {

typedef _Float16 f16;

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

int usage() {
  fprintf(stderr, "usage: objective_host rows B f H W ld c_pad T offs_scale x0.raw noise.raw t.raw table.raw mask.raw masked.raw [offs.raw]\n"
                  "       objective_host sqerr B f H W ld offs_scale eps.raw noise.raw [offs.raw]\n");
  return 2;
}

uint16_t bits_of(f16 v) {
  uint16_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

f16 half_of(uint16_t u) {
  f16 v;
  memcpy(&v, &u, sizeof v);
  return v;
}

bool geometry(char** argv, int64_t& B, int64_t& F, int64_t& H, int64_t& W) {
  B = atoll(argv[2]);
  F = atoll(argv[3]);
  H = atoll(argv[4]);
  W = atoll(argv[5]);
  if (B < 1 || F < 1 || H < 1 || W < 1 || (double)B * F * H * W >= (double)ob::MAX_ROWS) {
    fprintf(stderr, "objective_host: B, f, H, W are at least 1 and B f H W is below 2^31\n");
    return false;
  }
  return true;
}

int rows_main(int argc, char** argv) {
  if (argc != 16 && argc != 17) return usage();
  int64_t B, F, H, W;
  if (!geometry(argv, B, F, H, W)) return 2;
  const int64_t ld = atoll(argv[6]), c_pad = atoll(argv[7]), T = atoll(argv[8]);
  const float offs_scale = (float)atof(argv[9]);
  if (c_pad < 2 * ob::GROUP || c_pad > 1024 || c_pad % ob::GROUP || ld < c_pad || ld % ob::GROUP || T < 1) {
    fprintf(stderr, "objective_host: c_pad is a multiple of 8 in 16..1024, ld a multiple of 8 and at least c_pad, T at least 1\n");
    return 2;
  }
  const int64_t hw = H * W, fhw = F * hw, rows = B * fhw;
  std::vector<float> x0, noise, table, mask, masked, offs;
  std::vector<int64_t> t;
  const bool has_offs = argc == 17;
  if (!read_raw(argv[10], (size_t)(4 * rows), x0) || !read_raw(argv[11], (size_t)(4 * rows), noise) || !read_raw(argv[12], (size_t)B, t) ||
      !read_raw(argv[13], (size_t)(2 * T), table) || !read_raw(argv[14], (size_t)rows, mask) ||
      !read_raw(argv[15], (size_t)(4 * rows), masked) || (has_offs && !read_raw(argv[16], (size_t)(B * 4 * F), offs))) {
    fprintf(stderr, "objective_host: a file is missing or does not hold exactly its operand\n");
    return 2;
  }
  std::vector<uint16_t> out((size_t)(rows * ld), 0xFFFF);
  const int groups = (int)(c_pad / ob::GROUP);
  for (int64_t row = 0; row < rows; ++row)
    for (int g = 0; g < groups; ++g) {                 // a thread of the device: one group of one row
      const int64_t b = row / fhw, rem = row - b * fhw;
      uint16_t o[ob::GROUP] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (g == 0) {
        const int64_t ts = t[(size_t)b];
        const bool valid = ob::timestep_valid(ts, (int)T);
        const float sa = valid ? table[(size_t)(2 * ts)] : 0.0f, s1m = valid ? table[(size_t)(2 * ts + 1)] : 0.0f;
        const int64_t f = rem / hw;
        for (int c = 0; c < ob::LATENT_CHANNELS; ++c) {
          const int64_t e = (b * ob::LATENT_CHANNELS + c) * fhw + rem;
          float n = noise[(size_t)e];
          if (has_offs) n = ob::target(n, offs_scale, offs[(size_t)((b * ob::LATENT_CHANNELS + c) * F + f)]);
          o[c] = valid ? bits_of((f16)ob::add_noise(sa, x0[(size_t)e], s1m, n)) : ob::F16_NAN;
        }
        o[ob::MASK_CHANNEL] = bits_of((f16)mask[(size_t)(b * fhw + rem)]);
        for (int c = 0; c < 3; ++c) o[5 + c] = bits_of((f16)masked[(size_t)((b * ob::LATENT_CHANNELS + c) * fhw + rem)]);
      } else if (g == 1) {
        o[0] = bits_of((f16)masked[(size_t)((b * ob::LATENT_CHANNELS + 3) * fhw + rem)]);
      }
      for (int k = 0; k < ob::GROUP; ++k) out[(size_t)(row * ld + g * ob::GROUP + k)] = o[k];
    }
  for (int64_t row = 0; row < rows; ++row) {
    for (int64_t c = 0; c < ld; ++c) printf(c ? " %04x" : "%04x", (unsigned)out[(size_t)(row * ld + c)]);
    printf("\n");
  }
  return 0;
}

int sqerr_main(int argc, char** argv) {
  if (argc != 10 && argc != 11) return usage();
  int64_t B, F, H, W;
  if (!geometry(argv, B, F, H, W)) return 2;
  const int64_t ld = atoll(argv[6]);
  const float offs_scale = (float)atof(argv[7]);
  if (ld < ob::LATENT_CHANNELS || ld % 4) {
    fprintf(stderr, "objective_host: ld is a multiple of 4, at least 4\n");
    return 2;
  }
  const int64_t hw = H * W, rows = B * F * hw;
  std::vector<uint16_t> eps;
  std::vector<float> noise, offs;
  const bool has_offs = argc == 11;
  if (!read_raw(argv[8], (size_t)(rows * ld), eps) || !read_raw(argv[9], (size_t)(4 * rows), noise) ||
      (has_offs && !read_raw(argv[10], (size_t)(B * 4 * F), offs))) {
    fprintf(stderr, "objective_host: a file is missing or does not hold exactly its operand\n");
    return 2;
  }
  const int64_t cpf = ob::chunks_per_frame(hw);
  std::vector<double> part((size_t)(B * F * cpf)), slots(ob::CHUNK);
  // launch 1: a chunk of one frame at a time
  for (int64_t j = 0; j < B * F * cpf; ++j) {
    const int64_t bf = j / cpf, b = bf / F, f = bf - b * F;
    for (int i = 0; i < ob::CHUNK; ++i) {
      const int64_t p = (j - bf * cpf) * ob::CHUNK + i;
      double q = 0.0;
      if (p < hw) {
        float ev[4], nv[4];
        for (int c = 0; c < ob::LATENT_CHANNELS; ++c) {
          const int64_t bc = b * ob::LATENT_CHANNELS + c;
          float n = noise[(size_t)((bc * F + f) * hw + p)];
          if (has_offs) n = ob::target(n, offs_scale, offs[(size_t)(bc * F + f)]);
          ev[c] = (float)half_of(eps[(size_t)((bf * hw + p) * ld + c)]);
          nv[c] = n;
        }
        q = ob::pixel_sqerr(ev, nv);
      }
      slots[(size_t)i] = q;
    }
    part[(size_t)j] = ob::chunk_tree(slots.data());
  }
  // launch 2: the chunks of a frame in order
  for (int64_t bf = 0; bf < B * F; ++bf) {
    double s = 0.0;
    for (int64_t j = 0; j < cpf; ++j) s += part[(size_t)(bf * cpf + j)];
    uint64_t u;
    memcpy(&u, &s, sizeof u);
    printf("%016llx\n", (unsigned long long)u);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  if (!strcmp(argv[1], "rows")) return rows_main(argc, argv);
  if (!strcmp(argv[1], "sqerr")) return sqerr_main(argc, argv);
  return usage();
}
