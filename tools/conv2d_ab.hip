// A/B outside the library: rcdm_conv2d's kernel (operands staged through LDS) against the same tile with the MFMA fragments
// loaded straight from global memory (no LDS in the k-loop, no barrier; the next step's fragments prefetched into a second
// register set), on conv shapes of the Inception network at n = 50.  Same k order per MFMA, so the outputs must be equal bits.
// The result (profiles/inception_conv_ab.txt) is why the library stages through LDS; the direct kernel is not shipped.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize tools/conv2d_ab.hip -o conv2d_ab ; run: ./conv2d_ab
#include "../rcdms_amd/csrc/conv2d.hip"
#include <algorithm>
#include <cstdio>
#include <vector>
thread_local int g_rcdm_last_hip_error = 0;

namespace {
__global__ __launch_bounds__(NT) void conv2d_direct(rcdm_conv2d_desc d, int h_out, int w_out, int M, int K,
                                                    const f16* __restrict__ in, const f16* __restrict__ W,
                                                    const float* __restrict__ bias, f16* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) f16 so[BM * LDO];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int fr = lane & 15, fq = lane >> 4;
  const f16* abase[2]; int iy0[2], ix0[2]; bool mok[2];
  const f16* wrow[2]; bool nok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 32 + i * 16 + fr;
    mok[i] = m < M; iy0[i] = ix0[i] = 0; abase[i] = in;
    if (mok[i]) {
      const int hw = h_out * w_out, img = m / hw, rem = m - img * hw, oy = rem / w_out, ox = rem - oy * w_out;
      iy0[i] = oy * d.stride_h - d.pad_h; ix0[i] = ox * d.stride_w - d.pad_w;
      abase[i] = in + (size_t)img * d.h_in * d.w_in * (size_t)d.lda;
    }
    const int n = n0 + wn * 32 + i * 16 + fr;
    nok[i] = n < d.c_out;
    wrow[i] = W + (size_t)(nok[i] ? n : 0) * (size_t)K;
  }
  int c = fq * 8, kx = 0, ky = 0, k = fq * 8;
  while (c >= d.c_in) { c -= d.c_in; if (++kx == d.kw) { kx = 0; ++ky; } }
  auto la = [&](int i) -> uint4 {
    const int iy = iy0[i] + ky, ix = ix0[i] + kx;
    if (mok[i] && k < K && iy >= 0 && iy < d.h_in && ix >= 0 && ix < d.w_in)
      return *(const uint4*)(abase[i] + ((size_t)iy * d.w_in + ix) * (size_t)d.lda + c);
    return make_uint4(0, 0, 0, 0);
  };
  auto lb = [&](int i) -> uint4 {
    if (nok[i] && k < K) return *(const uint4*)(wrow[i] + k);
    return make_uint4(0, 0, 0, 0);
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int steps = (K + BK - 1) / BK;
  Pack16 a0, a1, b0, b1, na0, na1, nb0, nb1;
  a0.u = la(0); a1.u = la(1); b0.u = lb(0); b1.u = lb(1);
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {
      k += BK; c += BK;
      while (c >= d.c_in) { c -= d.c_in; if (++kx == d.kw) { kx = 0; ++ky; } }
      na0.u = la(0); na1.u = la(1); nb0.u = lb(0); nb1.u = lb(1);
    }
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0.h, b0.h, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0.h, b1.h, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1.h, b0.h, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1.h, b1.h, acc[1][1], 0, 0, 0);
    a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
  }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = wn * 32 + ni * 16 + fr;
    float bv = 0.0f;
    if ((d.epilogue & RCDM_EPI_BIAS) && n0 + col < d.c_out) bv = bias[n0 + col];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = acc[mi][ni][j] + bv;
        if (d.epilogue & RCDM_EPI_RELU) v = relu_f(v);
        so[(wm * 32 + mi * 16 + fq * 4 + j) * LDO + col] = (f16)v;
      }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < (BM * BN / 8) / NT; ++i) {
    const int idx = tid + i * NT;
    const int r = idx >> 3, cc = (idx & 7) * 8;
    if (m0 + r < M && n0 + cc < d.c_out)
      *(uint4*)(out + (size_t)(m0 + r) * (size_t)d.ldc + n0 + cc) = *(const uint4*)(so + r * LDO + cc);
  }
}
}  // namespace

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

int main() {
  struct Shape { const char* name; int n, h, w, ci, co, kh, kw, s, ph, pw; };
  const Shape shapes[] = {{"2b 3x3 p1 32->64 @147", 50, 147, 147, 32, 64, 3, 3, 1, 1, 1},
                          {"5c 1x1 256->64 @35", 50, 35, 35, 256, 64, 1, 1, 1, 0, 0},
                          {"5b 5x5 p2 48->64 @35", 50, 35, 35, 48, 64, 5, 5, 1, 2, 2},
                          {"5b 3x3 p1 96->96 @35", 50, 35, 35, 96, 96, 3, 3, 1, 1, 1},
                          {"6c 1x7 160->160 @17", 50, 17, 17, 160, 160, 1, 7, 1, 0, 3},
                          {"6e 1x1 768->192 @17", 50, 17, 17, 768, 192, 1, 1, 1, 0, 0},
                          {"7c 3x3 p1 448->384 @8", 50, 8, 8, 448, 384, 3, 3, 1, 1, 1},
                          {"7c 1x1 2048->320 @8", 50, 8, 8, 2048, 320, 1, 1, 1, 0, 0}};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("%-26s %12s %12s   (us per launch, median [min, max] of 5 windows of 20 launches, windows alternating; outputs compared)\n", "shape", "LDS stages", "direct");
  for (const Shape& s : shapes) {
    rcdm_conv2d_desc d = {};
    d.n_img = s.n; d.h_in = s.h; d.w_in = s.w; d.c_in = s.ci; d.c_out = s.co; d.kh = s.kh; d.kw = s.kw;
    d.stride_h = d.stride_w = s.s; d.pad_h = s.ph; d.pad_w = s.pw; d.lda = s.ci; d.ldc = s.co;
    d.epilogue = RCDM_EPI_BIAS | RCDM_EPI_RELU;
    int ho = 0, wo = 0;
    if (conv2d_check(&d, ho, wo) != RCDM_OK) { printf("bad shape\n"); return 1; }
    const int M = s.n * ho * wo, K = s.kh * s.kw * s.ci;
    const size_t nx = (size_t)s.n * s.h * s.w * s.ci, nw = (size_t)s.co * K, no = (size_t)M * s.co;
    std::vector<f16> hx(nx), hw(nw); std::vector<float> hb(s.co);
    unsigned r = 12345u;
    auto rnd = [&]() { r = r * 1664525u + 1013904223u; return ((r >> 8) & 0xffff) / 32768.0f - 1.0f; };
    for (auto& v : hx) v = (f16)rnd();
    for (auto& v : hw) v = (f16)(rnd() * 0.05f);
    for (auto& v : hb) v = rnd();
    f16 *x, *w, *o1, *o2; float* b;
    CK(hipMalloc(&x, nx * 2)); CK(hipMalloc(&w, nw * 2)); CK(hipMalloc(&o1, no * 2)); CK(hipMalloc(&o2, no * 2)); CK(hipMalloc(&b, s.co * 4));
    CK(hipMemcpy(x, hx.data(), nx * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(w, hw.data(), nw * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(b, hb.data(), s.co * 4, hipMemcpyHostToDevice));
    CK(hipMemset(o1, 0xff, no * 2)); CK(hipMemset(o2, 0xff, no * 2));
    const dim3 grid((M + BM - 1) / BM, (s.co + BN - 1) / BN);
    auto run = [&](int which, f16* o) {
      if (which == 0) hipLaunchKernelGGL(conv2d_kernel, grid, dim3(NT), 0, 0, d, ho, wo, M, K, x, w, b, o);
      else hipLaunchKernelGGL(conv2d_direct, grid, dim3(NT), 0, 0, d, ho, wo, M, K, x, w, b, o);
    };
    run(0, o1); run(1, o2);
    CK(hipDeviceSynchronize()); CK(hipGetLastError());
    std::vector<unsigned short> g1(no), g2(no);
    CK(hipMemcpy(g1.data(), o1, no * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(g2.data(), o2, no * 2, hipMemcpyDeviceToHost));
    size_t diff = 0;
    for (size_t i = 0; i < no; ++i) diff += g1[i] != g2[i];
    std::vector<float> t[2];
    for (int round = 0; round < 5; ++round)
      for (int which = 0; which < 2; ++which) {
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < 20; ++i) run(which, which ? o2 : o1);
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        t[which].push_back(ms * 1000.0f / 20);
      }
    CK(hipGetLastError());
    for (auto& v : t) std::sort(v.begin(), v.end());
    const double fl = 2.0 * M * (double)K * s.co;
    printf("%-26s %6.1f [%5.1f, %5.1f] %6.1f [%5.1f, %5.1f]   %6.1f / %6.1f Tflop/s useful, %zu outputs differ\n", s.name, t[0][2], t[0][0], t[0][4],
           t[1][2], t[1][0], t[1][4], fl / t[0][2] / 1e6, fl / t[1][2] / 1e6, diff);
    (void)hipFree(x); (void)hipFree(w); (void)hipFree(o1); (void)hipFree(o2); (void)hipFree(b);
  }
  return 0;
}
