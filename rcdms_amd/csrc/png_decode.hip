// png_decode.hip — rcdm_png_decode (include/rcdm.h, "PNG, reading"): n PNG files in one device byte buffer -> n HWC uint8
// RGB / BGR images, one wavefront per file, two launches, no host readback.
//
//   png_inflate_kernel   a 64-thread workgroup per file.  The wave gathers the file's IDAT payloads into one contiguous zlib
//                        stream in the workspace (coalesced byte copies, the tail zero-filled to 16 bytes) and runs
//                        pngd::inflate (csrc/png_inflate.h) behind WaveIO:
//     input    1 KB of the stream at a time in LDS, loaded 16 bytes a lane; the bit reader takes aligned words from it.
//     control  the bit position is a serial dependency: every value the control flow sees goes through readfirstlane, so
//              the symbol loop is scalar code with broadcast LDS reads.
//     tables   canonical arrays built by lane 0 between two syncs, the first-level tables filled by all lanes (an entry is
//              independent).
//     window   the last 32 KB of output are a ring in LDS.  A literal is one lane's byte; a match of length L is written by
//              L lanes at once from ring[pos - D + i % D] — sources all lie in front of pos, so the rounds of one match do
//              not depend on each other — and a stored block is a wave-wide copy from the gathered stream.  LDS operations
//              of one wave execute in order, and sync() (a workgroup barrier, which for one wave is the fence alone)
//              stands between the lanes' writes and another lane's read.
//     flush    whenever 4096 bytes are complete they go from the ring to the workspace, coalesced, and into the Adler-32
//              (per-lane sum and weighted sum, one wave reduction per flush).  Nothing the kernel wrote to global memory
//              is read back by it except the gathered stream, behind a workgroup fence.
//     bounds   pngd::inflate checks every position before it asks WaveIO to move a byte (see png_inflate.h); the gather
//              clamps to the record's zlib_bytes.
//   png_unfilter_kernel  a wave per file with status 0, a lane per row of a 64-row band, row j running j pixels behind row
//                        j - 1: `b` arrives from the lane below by __shfl_up (its last result), `c` is the previous `b`,
//                        `a` the lane's own last result.  Lane 0 reads the finished row above the band from the workspace,
//                        where lane 63 left it.  Filter bytes are scanned first: one above 4 is EFILTER and nothing is
//                        written.  Output: grey replicated, alpha dropped, palette looked up (black beyond its end).
#include "common.h"
#include "png_inflate.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_SIDE = 8192;
constexpr uint32_t FLUSH = 4096, RING_MASK = pngd::WINDOW - 1, CHUNK_WORDS = 256;

static_assert(RCDM_PNG_EZLIB == pngd::EZLIB && RCDM_PNG_ETRUNC == pngd::ETRUNC && RCDM_PNG_EBLOCK == pngd::EBLOCK &&
                  RCDM_PNG_ESTORED == pngd::ESTORED && RCDM_PNG_ECODES == pngd::ECODES && RCDM_PNG_ESYMBOL == pngd::ESYMBOL &&
                  RCDM_PNG_EDISTANCE == pngd::EDISTANCE && RCDM_PNG_EOVERRUN == pngd::EOVERRUN &&
                  RCDM_PNG_EUNDERRUN == pngd::EUNDERRUN && RCDM_PNG_EADLER == pngd::EADLER && RCDM_PNG_EFILTER == pngd::EFILTER,
              "status codes of the header and of the core");

struct InflateLds {
  uint8_t ring[pngd::WINDOW];
  alignas(16) uint32_t in[CHUNK_WORDS];   // filled 16 bytes a lane
  pngd::Tables t;
};
static_assert(sizeof(InflateLds) <= 40 * 1024, "four inflate workgroups share a CU's 160 KB");

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, WAVE);
  return v;
}

struct WaveIO {
  static constexpr int LANES = WAVE;
  int lane;
  InflateLds& lds;
  const uint8_t* z;   // the gathered stream, zero-filled to a multiple of 16 bytes
  uint32_t zwords;    // words that hold stream bytes
  uint32_t zquads;    // 16-byte units of the padded stream
  uint8_t* out;       // expect bytes
  uint32_t chunk, flushed, s1, s2;

  __device__ __forceinline__ uint32_t uni(uint32_t v) const { return uniform(v); }
  __device__ __forceinline__ void sync() const { __syncthreads(); }

  __device__ __forceinline__ uint32_t word(uint32_t i) {
    if (i >= zwords) return 0;
    uint32_t c = i / CHUNK_WORDS;
    if (c != chunk) {
      chunk = c;
      uint32_t q = c * (CHUNK_WORDS / 4) + (uint32_t)lane;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (q < zquads) v = *reinterpret_cast<const uint4*>(z + (size_t)q * 16);
      __syncthreads();
      *reinterpret_cast<uint4*>(&lds.in[lane * 4]) = v;
      __syncthreads();
    }
    return uniform(lds.in[i % CHUNK_WORDS]);
  }

  // out[flushed, flushed + n) leave the ring, n <= FLUSH
  __device__ __forceinline__ void flush(uint32_t n) {
    __syncthreads();
    uint32_t sum = 0, weighted = 0;
    for (uint32_t p = (uint32_t)lane; p < n; p += WAVE) {
      uint32_t b = lds.ring[(flushed + p) & RING_MASK];
      out[flushed + p] = (uint8_t)b;
      sum += b;
      weighted += (n - p) * b;
    }
    pngd::adler_advance(s1, s2, n, uniform(wave_sum(sum)), uniform(wave_sum(weighted)));
    flushed += n;
  }
  __device__ __forceinline__ void advance(uint32_t pos) {
    while (pos - flushed >= FLUSH) flush(FLUSH);
  }

  __device__ __forceinline__ void literal(uint32_t pos, uint8_t b) {
    if (lane == 0) lds.ring[pos & RING_MASK] = b;
    advance(pos + 1);
  }
  __device__ __forceinline__ void match(uint32_t pos, uint32_t L, uint32_t D) {
    __syncthreads();
    uint32_t from = pos - D;
    if (D >= L) {
      for (uint32_t i = (uint32_t)lane; i < L; i += WAVE) lds.ring[(pos + i) & RING_MASK] = lds.ring[(from + i) & RING_MASK];
    } else {
      for (uint32_t i = (uint32_t)lane; i < L; i += WAVE) lds.ring[(pos + i) & RING_MASK] = lds.ring[(from + i % D) & RING_MASK];
    }
    advance(pos + L);
  }
  __device__ __forceinline__ void stored(uint64_t at, uint32_t pos, uint32_t n) {
    while (n) {
      uint32_t m = n < FLUSH ? n : FLUSH;
      for (uint32_t i = (uint32_t)lane; i < m; i += WAVE) lds.ring[(pos + i) & RING_MASK] = z[at + i];
      at += m;
      pos += m;
      n -= m;
      advance(pos);
    }
  }
  __device__ __forceinline__ uint32_t adler(uint32_t pos) {
    if (pos > flushed) flush(pos - flushed);
    return (s2 << 16) | s1;
  }
};

__device__ __forceinline__ uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

__global__ __launch_bounds__(WAVE) void png_inflate_kernel(const rcdm_png_file* files, const rcdm_png_idat* idats, int n_idat,
                                                            const uint8_t* src, uint8_t* ws, int32_t* status) {
  __shared__ InflateLds lds;
  const int lane = (int)threadIdx.x;
  const rcdm_png_file f = files[blockIdx.x];
  const int bpp = pngd::bytes_per_pixel(f.color_type);
  uint8_t* z = ws + f.ws_offset;
  const uint8_t* file = src + f.src_offset;
  // gather the IDAT payloads
  uint64_t zpos = 0;
  for (uint32_t k = 0; k < f.idat_count; ++k) {
    uint32_t idx = f.idat_first + k;
    if (idx >= (uint32_t)n_idat) break;
    uint64_t off = idats[idx].offset;
    uint64_t nb = idats[idx].bytes;
    if (off > f.src_bytes || nb > f.src_bytes - off) break;
    if (nb > f.zlib_bytes - zpos) nb = f.zlib_bytes - zpos;
    for (uint64_t i = (uint64_t)lane; i < nb; i += WAVE) z[zpos + i] = file[off + i];
    zpos += nb;
  }
  const uint64_t zpad = align16(f.zlib_bytes);
  for (uint64_t i = zpos + (uint64_t)lane; i < zpad; i += WAVE) z[i] = 0;   // a short gather reads as zeros: ETRUNC or the like
  __threadfence_block();
  __syncthreads();
  WaveIO io{lane, lds, z, (uint32_t)((f.zlib_bytes + 3) / 4), (uint32_t)(zpad / 16), ws + f.ws_offset + zpad, 0xffffffffu, 0, 1, 0};
  int st = bpp == 0 || f.w < 1 || f.h < 1 || f.w > (uint32_t)MAX_SIDE || f.h > (uint32_t)MAX_SIDE
               ? (int)pngd::EUNDERRUN
               : pngd::inflate(io, lds.t, f.zlib_bytes, f.h * (1u + (uint32_t)bpp * f.w));
  if (lane == 0) status[blockIdx.x] = st;
}

__global__ __launch_bounds__(WAVE) void png_unfilter_kernel(const rcdm_png_file* files, const uint8_t* src, uint8_t* ws, uint8_t* dst,
                                                             int32_t* status, int bgr) {
  const int lane = (int)threadIdx.x;
  if (status[blockIdx.x] != 0) return;
  const rcdm_png_file f = files[blockIdx.x];
  const uint32_t ct = f.color_type, w = f.w, h = f.h;
  const int bpp = pngd::bytes_per_pixel(ct);
  const size_t S = 1 + (size_t)bpp * w;
  uint8_t* raw = ws + f.ws_offset + align16(f.zlib_bytes);
  const uint8_t* plte = src + f.src_offset + f.plte_offset;
  uint8_t* img = dst + f.dst_offset;
  int bad = 0;
  for (uint32_t r = (uint32_t)lane; r < h; r += WAVE) bad |= raw[r * S] > 4;
  if (__any(bad)) {
    if (lane == 0) status[blockIdx.x] = (int)pngd::EFILTER;
    return;
  }
  for (uint32_t band = 0; band < h; band += WAVE) {
    const uint32_t row = band + (uint32_t)lane;
    const bool active = row < h;
    const uint32_t ft = active ? raw[row * S] : 0;
    uint8_t* in = raw + (active ? row : 0) * S + 1;
    const uint8_t* above = raw + (band ? (size_t)(band - 1) * S + 1 : 0);
    uint8_t* o = img + (size_t)(active ? row : 0) * f.dst_pitch;
    uint32_t mine = 0, c = 0;
    for (uint32_t t = 0; t < w + WAVE - 1; ++t) {
      uint32_t b = (uint32_t)__shfl_up((int)mine, 1, WAVE);
      const int x = (int)t - lane;
      if (lane == 0) {
        b = 0;
        if (band && t < w)
          for (int k = 0; k < bpp; ++k) b |= (uint32_t)above[(size_t)t * bpp + k] << (8 * k);
      }
      if (active && x >= 0 && x < (int)w) {
        uint32_t px = 0;
        for (int k = 0; k < bpp; ++k) {
          uint32_t v = in[(size_t)x * bpp + k];
          px |= pngd::unfilter_byte(ft, v, (mine >> (8 * k)) & 255u, (b >> (8 * k)) & 255u, (c >> (8 * k)) & 255u) << (8 * k);
        }
        mine = px;
        c = b;
        if (lane == WAVE - 1)   // the row the next band's lane 0 reads
          for (int k = 0; k < bpp; ++k) in[(size_t)x * bpp + k] = (uint8_t)(px >> (8 * k));
        uint32_t rgb = pngd::to_rgb(ct, px, plte, f.plte_entries);
        o[3 * x + (bgr ? 2 : 0)] = (uint8_t)rgb;
        o[3 * x + 1] = (uint8_t)(rgb >> 8);
        o[3 * x + (bgr ? 0 : 2)] = (uint8_t)(rgb >> 16);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

bool file_ok(const rcdm_png_file& f) {
  return pngd::bytes_per_pixel(f.color_type) && f.w >= 1 && f.h >= 1 && f.w <= (uint32_t)MAX_SIDE && f.h <= (uint32_t)MAX_SIDE &&
         f.dst_pitch >= 3 * f.w && !(f.ws_offset & 15);
}

}  // namespace

extern "C" {

size_t rcdm_png_decode_workspace_bytes(const rcdm_png_file* files, int n) {
  if (!files || n < 1 || n > 65535) return 0;
  uint64_t end = 0;
  for (int i = 0; i < n; ++i) {
    if (!file_ok(files[i])) return 0;
    uint64_t raw = (uint64_t)files[i].h * (1u + (uint64_t)pngd::bytes_per_pixel(files[i].color_type) * files[i].w);
    uint64_t e = files[i].ws_offset + RCDM_PNG_FILE_WORKSPACE(files[i].zlib_bytes, raw);
    end = e > end ? e : end;
  }
  return (size_t)end;
}

int rcdm_png_decode(const rcdm_png_file* files, const rcdm_png_idat* idats, int n, int n_idat, int order, const void* src,
                    void* workspace, void* dst, int32_t* status, void* stream) {
  if (!files || !idats || !src || !workspace || !dst || !status) return RCDM_EINVAL;
  if (n < 1 || n_idat < 1 || (order != RCDM_PNG_RGB && order != RCDM_PNG_BGR)) return RCDM_EINVAL;
  if (n > 65535) return RCDM_ESHAPE;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)status & 3) || ((uintptr_t)files & 7) || ((uintptr_t)idats & 7)) return RCDM_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(png_inflate_kernel, dim3(n), dim3(WAVE), 0, s, files, idats, n_idat, (const uint8_t*)src, (uint8_t*)workspace,
                     status);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3(n), dim3(WAVE), 0, s, files, (const uint8_t*)src, (uint8_t*)workspace, (uint8_t*)dst,
                     status, order == RCDM_PNG_BGR);
  return rcdm_check_launch();
}

}  // extern "C"
