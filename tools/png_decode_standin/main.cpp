#include "png_decode.hip"
// usage: main n n_idat order records.bin idats.bin src.bin dst_bytes out.bin — both kernels of rcdm_png_decode on the buffers
// rcdms_amd.image.png_decode_plan laid out; every buffer is allocated at its exact size (a byte outside is a sanitizer
// report), the workspace poisoned with 0xEE, dst with 0xA5; out.bin = n status words, then dst
static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}
int main(int argc, char** argv) {
  if (argc != 9) return 2;
  const int n = atoi(argv[1]), n_idat = atoi(argv[2]), order = atoi(argv[3]);
  std::vector<uint8_t> rec = slurp(argv[4]), idat = slurp(argv[5]), src = slurp(argv[6]);
  const size_t dst_bytes = strtoull(argv[7], nullptr, 10);
  if (rec.size() != n * sizeof(rcdm_png_file) || idat.size() != n_idat * sizeof(rcdm_png_idat)) return 3;
  const rcdm_png_file* files = (const rcdm_png_file*)rec.data();
  const size_t wsb = rcdm_png_decode_workspace_bytes(files, n);
  if (!wsb) return 4;
  uint8_t* ws = (uint8_t*)aligned_alloc(16, wsb);
  memset(ws, 0xEE, wsb);
  std::vector<uint8_t> dst(dst_bytes, 0xA5);
  std::vector<int32_t> status(n, -1);
  int rc = rcdm_png_decode(files, (const rcdm_png_idat*)idat.data(), n, n_idat, order, src.data(), ws, dst.data(), status.data(), nullptr);
  if (rc) return 5;
  FILE* f = fopen(argv[8], "wb");
  fwrite(status.data(), 4, n, f);
  fwrite(dst.data(), 1, dst.size(), f);
  fclose(f);
  free(ws);
  return 0;
}
