// The operand addressing of the implicit-GEMM tile kernels (rcdms_amd/csrc/igemm_loader.h) on one CPU thread: the tile
// order, the k-step decode, the pixel-row decode and the activation / weight byte offsets, with loops where the device has
// blocks, waves and lanes.  It is how the addressing is checked against the numpy model (tests/gemm_exact.py: gathering the
// operands through the printed offsets gives the model's A and W matrices) before a GPU runs it, and it builds with
// sanitizers as it stands (host code with its own main):
//   hipcc -x hip --cuda-host-only -std=c++17 -O2 [-fsanitize=address,undefined] -I rcdms_amd/csrc tools/igemm_loader_host.cpp -o igemm_loader_host
//   igemm_loader_host TAPS BM BN M N Cin Ktot Hi Wi Ho Wo stride up pad lda nk nk1 Cin2 lda2 ph_rows tilesM tilesN
// (the IgemmArgs fields of igemm_args.h as the planner fills them; nk1 = 2147483647: no second input; TAPS = 4: the phase form.)
// Prints one line of seven integers per record:
//   3 lin m0 n0 0 0 0          tile `lin` of the linear order starts at row m0, column n0
//   0|1 lin ks row lch c off   activation piece: operand A (0) or A2 (1), k-step, tile row, the DMA lane's 16-byte chunk, the
//                              first of its eight channels within the k-step's 64 (the swizzle), byte offset or -1 (out of bounds)
//   2 lin ks row lch c off     weight piece, likewise
// With nk = 0 only the tile lines are printed.  Exit status 2: bad arguments.
//
// Winograd mode — the batched GEMM of the Winograd conv3x3 (rcdms_amd/csrc/wino_loader.h, wino.hip wino_gemm_kernel):
//   igemm_loader_host wino n_img H W K K2 N lda2 splits tilesM tilesN nk
// (K2 = 0: no second input, 16 entries; else 20.  tilesM / tilesN are taken as given, like the launch's.)  Per block `lin`:
//   3 lin m0 n0 entry split 0  the work item: entry, split-K slice, first tile row and column
//   0|1 lin ks row lch c off   piece of the entry's A operand at k-step ks < nk: 0 = V[entry] (offset inside that position's
//                              [T][K] panel), 1 = the second input in2 (entries 16 + 2a + b)
//   2 lin ks row lch c off     piece of its weight operand: inside U[entry] ([N][K]), or W2 ([N][K2]) for entries >= 16
// nk is the number of k-steps WALKED for every item (the kernel walks its slice of K / 64 or K2 / 64): a step past an entry's
// contraction width must print as out of bounds.  nk = 0: item lines only.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "wino_loader.h"

namespace {

long long shown(unsigned off) { return off == kIgemmOOB ? -1ll : (long long)off; }

template <int TAPS, int BM, int BN>
void walk(const IgemmArgs& p) {
  const int Hv = p.Hi << p.up, Wv = p.Wi << p.up;
  for (int lin = 0; lin < p.tilesM * p.tilesN; ++lin) {
    int m0, n0;
    igemm_tile_origin<BM, BN>(p, lin, m0, n0);
    printf("3 %d %d %d 0 0 0\n", lin, m0, n0);
    const int phase = TAPS == 4 ? m0 / p.ph_rows : 0;
    for (int ks = 0; ks < p.nk; ++ks) {
      const IgemmKStep k = igemm_kstep<TAPS>(p, ks);
      for (int row = 0; row < BM; ++row) {
        const IgemmPixelRow pr = igemm_pixel_row<TAPS>(p, m0 + row, m0 + row < p.M, phase);
        for (int lch = 0; lch < 8; ++lch) {
          const int c = igemm_swizzle_chunk(row, lch);
          printf("%d %d %d %d %d %d %lld\n", k.s2 ? 1 : 0, lin, ks, row, lch, c, shown(igemm_pixel_offset<TAPS>(p, k, pr, k.c0 + c, Hv, Wv)));
        }
      }
      for (int row = 0; row < BN; ++row) {
        const unsigned w_off = igemm_weight_row(p, n0 + row, phase);
        for (int lch = 0; lch < 8; ++lch) {
          const int c = igemm_swizzle_chunk(row, lch);
          printf("2 %d %d %d %d %d %lld\n", lin, ks, row, lch, c, shown(igemm_weight_offset(p, k, w_off, k.c0 + c)));
        }
      }
    }
  }
}

template <int TAPS>
bool walk_tile(const IgemmArgs& p, int bm, int bn) {
#define TILE(BM_, BN_) if (bm == BM_ && bn == BN_) { walk<TAPS, BM_, BN_>(p); return true; }
  TILE(64, 64) TILE(128, 64) TILE(128, 128) TILE(160, 160) TILE(160, 256) TILE(160, 320) TILE(256, 256)
#undef TILE
  return false;
}

int wino_main(int argc, char** argv) {
  if (argc != 13) {
    fprintf(stderr, "usage: igemm_loader_host wino n_img H W K K2 N lda2 splits tilesM tilesN nk\n");
    return 2;
  }
  int v[13];
  for (int i = 2; i < 13; ++i) v[i] = atoi(argv[i]);
  WinoArgs p{};
  p.n_img = v[2]; p.H = v[3]; p.W = v[4]; p.K = v[5]; p.K2 = v[6]; p.N = v[7]; p.lda2 = v[8]; p.splits = v[9];
  p.tilesM = v[10]; p.tilesN = v[11];
  const int nk = v[12];
  if (p.n_img <= 0 || p.H <= 0 || p.W <= 0 || (p.H & 1) || (p.W & 1) || p.K <= 0 || (p.K & 63) || p.K2 < 0 || (p.K2 & 63) || p.N <= 0 ||
      (p.K2 && p.lda2 < p.K2) || p.splits <= 0 || p.tilesM <= 0 || p.tilesN <= 0 || nk < 0) {
    fprintf(stderr, "igemm_loader_host wino: H and W even, K and K2 multiples of 64, lda2 >= K2\n");
    return 2;
  }
  p.th = p.H / 2; p.tw = p.W / 2; p.T = p.n_img * p.th * p.tw;
  p.E = p.K2 ? 20 : 16;
  for (int lin = 0; lin < p.E * p.splits * p.tilesM * p.tilesN; ++lin) {
    const WinoItem it = wino_item(p, lin);
    printf("3 %d %d %d %d %d 0\n", lin, it.m0, it.n0, it.entry, it.split);
    const int Kd = wino_kd(p, it.entry);
    for (int ks = 0; ks < nk; ++ks) {
      for (int op = 0; op < 2; ++op)
        for (int row = 0; row < kWinoTile; ++row) {
          const unsigned r_off = op ? wino_w_row(p, it.entry, it.n0 + row) : wino_a_row(p, it.entry, it.m0 + row);
          for (int lch = 0; lch < 8; ++lch) {
            const int c = igemm_swizzle_chunk(row, lch);
            printf("%d %d %d %d %d %d %lld\n", op ? 2 : it.entry >= 16 ? 1 : 0, lin, ks, row, lch, c, shown(wino_piece_offset(r_off, ks * BK + c, Kd)));
          }
        }
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "wino")) return wino_main(argc, argv);
  if (argc != 23) {
    fprintf(stderr, "usage: igemm_loader_host TAPS BM BN M N Cin Ktot Hi Wi Ho Wo stride up pad lda nk nk1 Cin2 lda2 ph_rows tilesM tilesN\n");
    return 2;
  }
  int v[23];
  for (int i = 1; i < 23; ++i) v[i] = atoi(argv[i]);
  IgemmArgs p{};
  const int taps = v[1], bm = v[2], bn = v[3];
  p.M = v[4]; p.N = v[5]; p.Cin = v[6]; p.Ktot = v[7];
  p.Hi = v[8]; p.Wi = v[9]; p.Ho = v[10]; p.Wo = v[11]; p.stride = v[12]; p.up = v[13]; p.pad = v[14];
  p.lda = v[15]; p.nk = v[16]; p.nk1 = v[17]; p.Cin2 = v[18]; p.lda2 = v[19]; p.ph_rows = v[20];
  p.tilesM = v[21]; p.tilesN = v[22];
  const bool shape_ok = p.M > 0 && p.N > 0 && p.Cin > 0 && p.Ktot > 0 && p.Hi > 0 && p.Wi > 0 && p.Ho > 0 && p.Wo > 0 &&
                        (p.stride == 1 || p.stride == 2) && (p.up == 0 || p.up == 1) && (p.pad == 0 || p.pad == 1) && p.lda > 0 &&
                        p.nk >= 0 && p.tilesM > 0 && p.tilesN > 0 && (taps != 4 || (p.ph_rows > 0 && p.ph_rows % bm == 0)) &&
                        (p.nk1 == kNoSeg2 || (taps == 9 && p.Cin2 > 0 && p.lda2 > 0));
  const bool ran = shape_ok && (taps == 1 ? walk_tile<1>(p, bm, bn) : taps == 9 ? walk_tile<9>(p, bm, bn) : taps == 4 ? walk_tile<4>(p, bm, bn) : false);
  if (!ran) {
    fprintf(stderr, "igemm_loader_host: TAPS is 1, 9 or 4 (4: ph_rows a multiple of BM), BM x BN one of the kernels' tiles, nk1 set only with TAPS 9\n");
    return 2;
  }
  return 0;
}
