#include "png.hip"
// usage: main h w stream.bin out.png — png_match_block_kernel + png_assemble_kernel on a host-filtered stream (the filter
// kernel needs wave shuffles, which the stand-in does not model); the workspace is poisoned with 0xEE first
int main(int argc, char** argv) {
  rcdm_png_desc d{};
  d.n = 1; d.h = atoi(argv[1]); d.w = atoi(argv[2]); d.channels = 3; d.filter = -1; d.src_pitch = 3 * d.w;
  const Geo g = png_geo(&d);
  const size_t wsb = rcdm_png_match_workspace_bytes(&d), bound = rcdm_png_bound(&d);
  uint8_t* ws = (uint8_t*)aligned_alloc(256, (wsb + 255) & ~(size_t)255);
  memset(ws, 0xEE, wsb);
  FILE* f = fopen(argv[3], "rb");
  if (fread(ws, 1, g.total, f) != (size_t)g.total) return 2;
  fclose(f);
  uint8_t* dst = (uint8_t*)malloc(bound);
  memset(dst, 0xCC, bound);
  uint64_t size = 0;
  static const CrcOps ops = png_crc_ops();
  hipLaunchKernelGGL(png_match_block_kernel, dim3(g.nblk, 1), dim3(MT), 0, 0, g, ops, 1 + 3 * d.w, (const uint8_t*)ws, ws + g.slots_off, (Rec*)(ws + g.recs_off));
  hipLaunchKernelGGL(png_assemble_kernel, dim3(g.nblk, 1), dim3(NT), 0, 0, d, g, (const uint8_t*)(ws + g.slots_off), (const Rec*)(ws + g.recs_off), dst, &size);
  f = fopen(argv[4], "wb");
  fwrite(dst, 1, size, f);
  fclose(f);
  printf("%llu bytes (bound %zu)\n", (unsigned long long)size, bound);
  free(dst); free(ws);
  return 0;
}
