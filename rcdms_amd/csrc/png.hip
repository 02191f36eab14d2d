// png.hip — PNG files of uint8 RGB frames, written on the device (include/rcdm.h, "PNG").
// The deflate stream holds literals only: per-row adaptive filters, then one dynamic-Huffman block per 32768 filtered bytes,
// each followed by an empty stored block that pads to a byte, so every block is a byte string of its own, every IDAT chunk
// holds one block and its CRC-32 covers nothing else.  Three launches on the caller's stream, ordered by nothing but the stream:
//   png_filter_kernel    a wave per scanline: five filter costs, the choice, the type byte + filtered row into the workspace
//   png_block_kernel     a workgroup per (image, 32768-byte block): histogram, Huffman code, bit packing into LDS, the chunk's
//                        bytes (type + data) into the block's slot, a record {bytes, CRC-32 register, Adler-32 partials}
//   png_assemble_kernel  a workgroup per (image, block): sums the chunk sizes in front of its own, copies its slot into the
//                        file, writes length / CRC; the first also signature + IHDR, the last Adler-32, IEND and sizes[i]
// The Huffman code (tests/png_oracle.py restates it): the symbols with a non-zero count — 256 literals and end-of-block,
// which counts 1 — ascending by (count, symbol index) form the leaf queue; internal nodes queue up in creation order; the
// next node is the front of the leaf queue unless the internal queue's front is STRICTLY lighter (the leaf queue wins a
// tie).  A leaf's code length is its depth.  Deeper than 15: every non-zero count c becomes (c + 1) >> 1 and the tree is
// rebuilt.  Codes are canonical (RFC 1951 3.2.2).  Sorting (a rank per symbol), depths (a walk per leaf) and canonical
// codes (a count per symbol) run on all 256 threads; only the two-queue merge, <= 256 steps, runs on one lane.
// CRC-32: the chunk, right-aligned in SLOT = 256 x 163 bytes, is cut into 256 pieces of 163 bytes, one table-driven CRC per
// thread with a zero register (leading zeros leave it zero; the initial 0xFFFFFFFF is the complement of the first four
// bytes, which are always "IDAT"), then 8 tree levels of crc(A|B) = crc(A) * x^(8|B|) + crc(B) with the eight fixed
// operators x^(8 * 163 * 2^j) mod P.
// Every store is a plain C++ store or an LDS atomic; nothing here reads a value back on the host.
// rcdm_png_encode_match puts png_match_block_kernel (further down, with its own description) in png_block_kernel's place:
// matches at a few fixed distances, and per block whichever of the two forms is smaller.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int BLOCK = RCDM_PNG_BLOCK;
constexpr int SLOT = RCDM_PNG_SLOT;          // bytes of one block's slot: chunk type + data, without the Adler-32 of the last
constexpr int SLOT_WORDS = SLOT / 4;
constexpr int PIECE = SLOT / NT;             // CRC piece of one thread
constexpr int PER_THREAD = BLOCK / NT;       // 128 filtered bytes a thread encodes
constexpr int NSYM = 257;
constexpr int HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4;
constexpr int MAX_SIDE = 8192;
constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ADLER = 65521u;
static_assert(SLOT % 16 == 0 && PIECE * NT == SLOT && PER_THREAD % 16 == 0, "slot / piece geometry");

struct Rec {
  uint32_t bytes;   // type + data in the slot
  uint32_t crc;     // CRC-32 register over those bytes (before the final complement)
  uint32_t a, b;    // sum of the block's filtered bytes, sum of (block length - position) * byte, both mod 65521
};

struct CrcOps {
  uint32_t k[8];    // x^(8 * PIECE * 2^j) mod P, reflected
};

struct Geo {
  int64_t total;          // filtered bytes of one image
  int64_t stream_stride;  // ... rounded up to 16
  int64_t slots_off, recs_off;
  int32_t nblk;
};

// worst-case data bytes of the IDAT of a block of nb filtered bytes: zlib header, the block, 00 00 FF FF, Adler-32.
// An optimal code costs <= 9 bits a symbol (the flat 9-bit code is a prefix code over 257 symbols); the limiter halves at
// most 4 times (a Huffman tree deeper than 15 needs a total count >= F(18) = 2584, and k halvings leave a total of
// <= 32769 / 2^k + 257), and a code that is optimal for the halved counts costs <= 9 (nb + 1 + 257 * 16) bits on the true ones.
__host__ __device__ constexpr int64_t block_cap(int64_t nb) { return 10 + (HEADER_BITS + 3 + 9 * (nb + 4113) + 7) / 8; }
static_assert(4 + block_cap(BLOCK) - 4 <= SLOT, "a full block's chunk fits its slot");

__host__ __device__ inline uint32_t mulmod(uint32_t a, uint32_t b) {   // a * b mod P, reflected bit order
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    if (a & (1u << i)) p ^= b;
    b = (b & 1) ? (b >> 1) ^ POLY : b >> 1;
  }
  return p;
}

__device__ __forceinline__ uint32_t crc_byte(uint32_t c, uint32_t byte) {
  c ^= byte;
  for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
  return c;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int filtered(int f, int x, int a, int b, int c) {
  const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : paeth(a, b, c);
  return (x - pred) & 255;
}

__device__ __forceinline__ unsigned cost_of(int v) { return v < 128 ? v : 256 - v; }

__global__ __launch_bounds__(NT) void png_filter_kernel(rcdm_png_desc d, const uint8_t* __restrict__ src, uint8_t* __restrict__ streams,
                                                        int64_t stream_stride) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), img = blockIdx.y;
  if (y >= d.h) return;                                  // the whole wave leaves; no barrier in this kernel
  const int rb = 3 * d.w;
  const uint8_t* row = src + (size_t)img * (size_t)d.src_stride + (size_t)y * (size_t)d.src_pitch;
  const uint8_t* up = row - d.src_pitch;                 // read only where y > 0
  const bool has_up = y > 0;
  int f = d.filter;
  if (f < 0) {
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int i = lane; i < rb; i += 64) {
      const int x = row[i], a = i >= 3 ? row[i - 3] : 0;
      const int b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
      c0 += cost_of(x);
      c1 += cost_of((x - a) & 255);
      c2 += cost_of((x - b) & 255);
      c3 += cost_of((x - ((a + b) >> 1)) & 255);
      c4 += cost_of((x - paeth(a, b, c)) & 255);
    }
    for (int m = 32; m >= 1; m >>= 1) {
      c0 += __shfl_xor(c0, m);
      c1 += __shfl_xor(c1, m);
      c2 += __shfl_xor(c2, m);
      c3 += __shfl_xor(c3, m);
      c4 += __shfl_xor(c4, m);
    }
    f = 0;
    unsigned best = c0;
    if (c1 < best) { best = c1; f = 1; }
    if (c2 < best) { best = c2; f = 2; }
    if (c3 < best) { best = c3; f = 3; }
    if (c4 < best) { best = c4; f = 4; }
  }
  uint8_t* o = streams + (size_t)img * (size_t)stream_stride + (size_t)y * (size_t)(rb + 1);
  if (lane == 0) o[0] = (uint8_t)f;
  for (int i = lane; i < rb; i += 64) {
    const int x = row[i], a = i >= 3 ? row[i - 3] : 0;
    const int b = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
    o[1 + i] = (uint8_t)filtered(f, x, a, b, c);
  }
}

// val's low n bits at bit `pos` of the LDS image (LSB first, as deflate packs); words past the slot are dropped
__device__ __forceinline__ void put_bits(uint32_t* out, uint32_t pos, uint32_t val, int n) {
  (void)n;
  const uint64_t v = (uint64_t)val << (pos & 31);
  const uint32_t w = pos >> 5;
  if (w < SLOT_WORDS) atomicOr(&out[w], (uint32_t)v);
  if ((uint32_t)(v >> 32) && w + 1 < SLOT_WORDS) atomicOr(&out[w + 1], (uint32_t)(v >> 32));
}

__global__ __launch_bounds__(NT) void png_block_kernel(Geo g, CrcOps ops, const uint8_t* __restrict__ streams, uint8_t* __restrict__ slots,
                                                       Rec* __restrict__ recs) {
  __shared__ uint32_t out[SLOT_WORDS];       // the chunk: type, (zlib header), deflate bytes
  __shared__ uint32_t hist[4][256];          // one histogram per wave
  __shared__ uint32_t cnt[NSYM];             // counts the code is built from (halved by the limiter)
  __shared__ uint32_t nw[2 * NSYM];          // node weights: leaves 0 .. n-1 in sorted order, internal nodes n .. 2n-2
  __shared__ uint16_t par[2 * NSYM];
  __shared__ uint16_t ssym[NSYM];            // symbol of sorted leaf r
  __shared__ uint32_t len[NSYM + 1];
  __shared__ uint32_t lut[NSYM];             // bit-reversed code | length << 16
  __shared__ uint32_t crct[256];
  __shared__ uint32_t scan[NT];
  __shared__ uint32_t blc[16], nextc[16];
  __shared__ uint32_t misc[4];               // 0: symbols in use, 1: deepest leaf, 2 / 3: Adler partial sums
  const int tid = threadIdx.x, blk = blockIdx.x, img = blockIdx.y;
  const int64_t off = (int64_t)blk * BLOCK;
  const int N = (int)(g.total - off < BLOCK ? g.total - off : BLOCK);
  const bool first = blk == 0, last = blk == g.nblk - 1;
  const uint4* d4 = (const uint4*)(streams + (size_t)img * (size_t)g.stream_stride + (size_t)off);

  for (int i = tid; i < SLOT_WORDS; i += NT) out[i] = 0;
  for (int i = tid; i < 4 * 256; i += NT) (&hist[0][0])[i] = 0;
  {
    uint32_t c = tid;
    for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
    crct[tid] = c;
  }
  if (tid < 4) misc[tid] = 0;
  __syncthreads();

  // histogram and Adler-32 partial sums of the block
  {
    uint32_t s1 = 0, s2 = 0;
    uint32_t* h = hist[tid >> 6];
    const int nvec = (N + 15) >> 4;
    for (int v = tid; v < nvec; v += NT) {
      const uint4 q = d4[v];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int p = v * 16 + j;
        if (p < N) {
          const uint32_t b = (w[j >> 2] >> (8 * (j & 3))) & 255;
          atomicAdd(&h[b], 1u);
          s1 += b;
          s2 += (uint32_t)(N - p) * b;           // <= 128 bytes a thread: < 2^31
        }
      }
    }
    atomicAdd(&misc[2], s1 % ADLER);
    atomicAdd(&misc[3], s2 % ADLER);
  }
  __syncthreads();
  for (int s = tid; s < NSYM; s += NT) cnt[s] = s < 256 ? hist[0][s] + hist[1][s] + hist[2][s] + hist[3][s] : 1u;

  // code lengths
  for (;;) {
    for (int s = tid; s <= NSYM; s += NT) len[s] = 0;
    if (tid == 0) misc[0] = misc[1] = 0;
    __syncthreads();
    for (int s = tid; s < NSYM; s += NT) {
      const uint32_t c = cnt[s];
      if (c) {
        int r = 0;
        for (int u = 0; u < NSYM; ++u) {
          const uint32_t cu = cnt[u];
          r += (cu && (cu < c || (cu == c && u < s))) ? 1 : 0;
        }
        nw[r] = c;
        ssym[r] = (uint16_t)s;
        atomicAdd(&misc[0], 1u);
      }
    }
    __syncthreads();
    const int n = (int)misc[0];                          // >= 2: a literal and end-of-block
    if (tid == 0) {
      int i = 0, j = n;
      for (int nxt = n; nxt < 2 * n - 1; ++nxt) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
          int pick;
          if (i < n && (j >= nxt || nw[i] <= nw[j])) pick = i++;
          else pick = j++;
          sum += nw[pick];
          par[pick] = (uint16_t)nxt;
        }
        nw[nxt] = sum;
      }
    }
    __syncthreads();
    for (int r = tid; r < n; r += NT) {
      uint32_t depth = 0;
      for (int node = r; node != 2 * n - 2 && depth < 2 * NSYM; node = par[node]) ++depth;
      len[ssym[r]] = depth;
      atomicMax(&misc[1], depth);
    }
    __syncthreads();
    const uint32_t deepest = misc[1];
    __syncthreads();
    if (deepest <= 15) break;
    for (int s = tid; s < NSYM; s += NT) {
      const uint32_t c = cnt[s];
      if (c) cnt[s] = (c + 1) >> 1;
    }
    __syncthreads();
  }

  // canonical codes
  if (tid < 16) blc[tid] = 0;
  __syncthreads();
  for (int s = tid; s < NSYM; s += NT)
    if (len[s]) atomicAdd(&blc[len[s]], 1u);
  __syncthreads();
  if (tid == 0) {
    uint32_t code = 0;
    nextc[0] = 0;
    for (int b = 1; b <= 15; ++b) {
      code = (code + (b == 1 ? 0u : blc[b - 1])) << 1;
      nextc[b] = code;
    }
  }
  __syncthreads();
  for (int s = tid; s < NSYM; s += NT) {
    const uint32_t l = len[s];
    uint32_t e = 0;
    if (l) {
      uint32_t k = 0;
      for (int u = 0; u < s; ++u) k += len[u] == l ? 1 : 0;
      e = (__brev(nextc[l] + k) >> (32 - l)) | (l << 16);
    }
    lut[s] = e;
  }
  __syncthreads();

  // bits of this thread's PER_THREAD bytes, scanned over the workgroup
  const int b0 = tid * PER_THREAD;
  const int mine = N - b0 < 0 ? 0 : (N - b0 < PER_THREAD ? N - b0 : PER_THREAD);
  const uint4* t4 = d4 + tid * (PER_THREAD / 16);
  uint32_t bits = 0;
  for (int v = 0; v * 16 < mine; ++v) {
    const uint4 q = t4[v];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (v * 16 + j < mine) bits += lut[(w[j >> 2] >> (8 * (j & 3))) & 255] >> 16;
  }
  scan[tid] = bits;
  __syncthreads();
  for (int s = 1; s < NT; s <<= 1) {
    const uint32_t add = tid >= s ? scan[tid - s] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const uint32_t base = 8u * (4 + (first ? 2 : 0));
  const uint32_t lit0 = base + HEADER_BITS;

  // header: block type, counts, the fixed code-length code, then 258 lengths of 4 bits each
  if (tid == 0) {
    out[0] |= 0x54414449u;                               // "IDAT"
    if (first) atomicOr(&out[1], 0x0178u);               // zlib header 78 01
    put_bits(out, base, 4, 3);                           // BFINAL 0, BTYPE 2
    put_bits(out, base + 13, 15, 4);                     // HLIT 257 and HDIST 1 are zeros; HCLEN 19
    for (int i = 3; i < 19; ++i) put_bits(out, base + 17 + 3 * i, 4, 3);   // 16, 17, 18 unused; 0..15 cost 4 bits
  }
  for (int s = tid; s < NSYM + 1; s += NT) put_bits(out, base + 74 + 4 * s, __brev(len[s]) >> 28, 4);   // len[257]: the distance length, 0

  // literals
  {
    uint32_t pos = lit0 + scan[tid] - bits;
    uint32_t w = pos >> 5;
    int nb = pos & 31;
    uint64_t acc = 0;
    for (int v = 0; v * 16 < mine; ++v) {
      const uint4 q = t4[v];
      const uint32_t ww[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (v * 16 + j < mine) {
          const uint32_t e = lut[(ww[j >> 2] >> (8 * (j & 3))) & 255];
          acc |= (uint64_t)(e & 0xffff) << nb;
          nb += e >> 16;
          if (nb >= 32) {
            if (w < SLOT_WORDS) atomicOr(&out[w], (uint32_t)acc);
            ++w;
            acc >>= 32;
            nb -= 32;
          }
        }
      }
    }
    if (nb > 0 && w < SLOT_WORDS) atomicOr(&out[w], (uint32_t)acc);
  }
  // end of block, the empty stored block
  uint32_t end = lit0 + scan[NT - 1];
  if (tid == 0) put_bits(out, end, lut[256] & 0xffff, 16);
  end += lut[256] >> 16;
  if (tid == 0) put_bits(out, end, last ? 1 : 0, 3);
  uint32_t bytes = (end + 3 + 7) >> 3;
  if (tid == 0) put_bits(out, bytes * 8, 0xFFFF0000u, 32);
  bytes += 4;
  if (bytes > SLOT) bytes = SLOT;                        // cannot happen (block_cap); never leave the slot
  __syncthreads();

  uint4* slot = (uint4*)(slots + ((size_t)img * g.nblk + blk) * SLOT);
  const uint4* o4 = (const uint4*)out;
  for (int i = tid; i * 16 < (int)bytes; i += NT) slot[i] = o4[i];

  // CRC-32 of type + data
  {
    const uint8_t* ob = (const uint8_t*)out;
    const int pad = SLOT - (int)bytes;
    uint32_t c = 0;
    for (int i = 0; i < PIECE; ++i) {
      const int di = tid * PIECE + i - pad;
      if (di >= 0) c = crct[(c ^ ob[di] ^ (di < 4 ? 0xFFu : 0u)) & 255] ^ (c >> 8);
    }
    scan[tid] = c;
    for (int j = 0; j < 8; ++j) {
      __syncthreads();
      const int s = 1 << j;
      if ((tid & (2 * s - 1)) == 0) scan[tid] = mulmod(ops.k[j], scan[tid]) ^ scan[tid + s];
    }
  }
  if (tid == 0) {
    Rec r;
    r.bytes = bytes;
    r.crc = scan[0];
    r.a = misc[2] % ADLER;
    r.b = misc[3] % ADLER;
    recs[(size_t)img * g.nblk + blk] = r;
  }
}

__global__ __launch_bounds__(NT) void png_assemble_kernel(rcdm_png_desc d, Geo g, const uint8_t* __restrict__ slots, const Rec* __restrict__ recs,
                                                          uint8_t* __restrict__ dst, uint64_t* __restrict__ sizes) {
  __shared__ unsigned long long red[3];
  const int tid = threadIdx.x, blk = blockIdx.x, img = blockIdx.y;
  const bool last = blk == g.nblk - 1;
  const Rec* rc = recs + (size_t)img * g.nblk;
  if (tid < 3) red[tid] = 0;
  __syncthreads();
  unsigned long long before = 0, sa = 0, sb = 0;
  for (int j = tid; j < blk; j += NT) before += rc[j].bytes + 8u;
  if (last) {
    for (int j = tid; j < g.nblk; j += NT) {
      const int64_t lenj = j == g.nblk - 1 ? g.total - (int64_t)j * BLOCK : BLOCK;
      const uint64_t after = (uint64_t)(g.total - (int64_t)j * BLOCK - lenj) % ADLER;
      sa += rc[j].a;
      sb += after * rc[j].a + rc[j].b;
    }
  }
  atomicAdd(&red[0], before);
  if (last) {
    atomicAdd(&red[1], sa % ADLER);
    atomicAdd(&red[2], sb % ADLER);
  }
  __syncthreads();
  uint8_t* file = dst + (size_t)img * (size_t)d.dst_stride;
  const size_t off = 33 + (size_t)red[0];
  const Rec me = rc[blk];
  const uint8_t* slot = slots + ((size_t)img * g.nblk + blk) * SLOT;
  uint8_t* o = file + off;
  for (uint32_t i = tid; i < me.bytes; i += NT) o[4 + i] = slot[i];
  if (tid == 0) {
    put_be32(o, me.bytes - 4 + (last ? 4u : 0u));
    uint32_t crc = me.crc;
    uint8_t* p = o + 4 + me.bytes;
    if (last) {
      const uint32_t a = (uint32_t)((1 + red[1]) % ADLER);
      const uint32_t b = (uint32_t)(((uint64_t)g.total % ADLER + red[2]) % ADLER);
      put_be32(p, (b << 16) | a);
      for (int i = 0; i < 4; ++i) crc = crc_byte(crc, p[i]);
      p += 4;
    }
    put_be32(p, ~crc);
    p += 4;
    if (last) {
      put_be32(p, 0);
      put_be32(p + 4, 0x49454E44u);                      // IEND
      put_be32(p + 8, 0xAE426082u);
      sizes[img] = (uint64_t)(p + 12 - file);
    }
  }
  if (blk == 0 && tid == 64) {
    put_be32(file, 0x89504E47u);
    put_be32(file + 4, 0x0D0A1A0Au);
    put_be32(file + 8, 13);
    put_be32(file + 12, 0x49484452u);                    // IHDR
    put_be32(file + 16, (uint32_t)d.w);
    put_be32(file + 20, (uint32_t)d.h);
    file[24] = 8;                                        // bit depth
    file[25] = 2;                                        // colour type: RGB
    file[26] = file[27] = file[28] = 0;                  // deflate, adaptive filtering, no interlace
    uint32_t crc = 0xFFFFFFFFu;
    for (int i = 12; i < 29; ++i) crc = crc_byte(crc, file[i]);
    put_be32(file + 29, ~crc);
  }
}

// ------------------------------------------------------------------------------------------------
// Match mode (include/rcdm.h, "PNG, match mode"; tests/png_match_oracle.py restates it): png_match_block_kernel takes
// png_block_kernel's place between the filter and the assemble kernel.  One workgroup of 1024 threads per (image, block),
// thread t owns the 32 stream positions 32 t .. 32 t + 31 of the block in every phase but the first:
//   masks     one equality bit per (candidate distance, position): s[i] == s[i - d], a wave per 64 positions and a ballot
//             per candidate; bytes in front of the block come from the image's stream in the workspace
//   lengths   per candidate the run of ones from each position: a find-first-zero scan over the words behind the thread's
//             own, then a sweep back through its 32 bits; the longest run wins, the earlier candidate on a tie
//   parse     the greedy parse is the chain b0 -> b0 + len -> ...: reachability by pointer doubling, ceil(log2 N) rounds
//   codes     literal-form and match-form histograms, three Huffman codes (huff_build: the construction of
//             png_block_kernel on any alphabet), both bit totals; the match form only if it is strictly smaller
//   bits      widths of the thread's own symbols, a scan over the workgroup, packing into LDS; then slot, CRC and record
//             exactly as png_block_kernel leaves them
// (length, candidate) of a thread's 32 positions stay in 16 of its registers from the lengths phase to the last bit.
// LDS: 76 KB for the block's bytes + 11 masks, reused for the 64 KB of jump pointers (read and written 16 bytes at a time by
// their owner) and then for the packed chunk; 4 KB reached bits; ~14 KB of code tables.  1024 threads: one workgroup per CU.
// huff_build and the kernel's tail (slot copy, 256-piece CRC, record) restate png_block_kernel's, which this mode may not
// touch: tie rules, the limiter and the CRC operators must stay in lockstep with it — the fallback's bytes are compared with
// png_block_kernel's by tests/test_hip_png_match.py (pngm_1x1, pngm_3x5, the batch's fifth image).
constexpr int MT = 1024;
constexpr int MW = BLOCK / 32;               // words of 32 positions
constexpr int NCAND = 11;
constexpr int NLL = 286, NDIST = 30;
constexpr int MHEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (NLL + NDIST) * 4;
constexpr int MIN_MATCH = 4, MAX_MATCH = 258;
static_assert(MT * 32 == BLOCK && MW == MT, "a thread per 32 positions");

struct alignas(16) MatchLds {
  union {
    struct {
      uint8_t sb[BLOCK];                     // the block's filtered bytes
      uint32_t mask[NCAND][MW];
    } a;
    uint16_t jump[BLOCK];                    // position after 2^k parse steps
    struct {
      uint32_t out[SLOT_WORDS];              // the chunk: type, (zlib header), deflate bytes
      uint32_t scan[MT];
      uint32_t crct[256];
    } c;
  } x;
  uint32_t reached[MW];
  uint32_t cntL[NLL], cntM[NLL], cntD[NDIST + 2];   // true counts: literal form, match form, distances
  uint32_t cnt[NLL];                         // counts a code is built from (halved by the limiter)
  uint32_t nw[2 * NLL];
  uint16_t par[2 * NLL];
  uint16_t ssym[NLL];
  uint32_t lenL[NLL], lenM[NLL], lenD[NDIST + 2];
  uint32_t lutL[NLL], lutM[NLL], lutD[NDIST + 2];   // bit-reversed code | length << 16
  uint32_t blc[16], nextc[16];
  uint32_t misc[8];                          // 0: symbols in use, 1: deepest leaf, 2 / 3: Adler sums, 4: extra bits, 5 / 6: bits L / M
  int32_t cand[NCAND];                       // distance, 0: dropped
  uint32_t dsym[NCAND], dbits[NCAND], dextra[NCAND];
};
static_assert(sizeof(MatchLds) <= 160 * 1024, "the match kernel's LDS");

// Huffman code of `count[0 .. nsym)` into len / lut, by every thread of the workgroup: png_block_kernel's construction,
// restated on any alphabet — keep the two in lockstep (leaf order, the leaf queue wins a tie, (c + 1) >> 1 limiter).
// Fewer than two used symbols: the used one gets length 1.
__device__ void huff_build(MatchLds& L, const uint32_t* count, int nsym, uint32_t* len, uint32_t* lut, int tid) {
  for (int s = tid; s < nsym; s += MT) L.cnt[s] = count[s];
  __syncthreads();
  for (;;) {
    for (int s = tid; s < nsym; s += MT) len[s] = 0;
    if (tid == 0) L.misc[0] = L.misc[1] = 0;
    __syncthreads();
    for (int s = tid; s < nsym; s += MT) {
      const uint32_t c = L.cnt[s];
      if (c) {
        int r = 0;
        for (int u = 0; u < nsym; ++u) {
          const uint32_t cu = L.cnt[u];
          r += (cu && (cu < c || (cu == c && u < s))) ? 1 : 0;
        }
        L.nw[r] = c;
        L.ssym[r] = (uint16_t)s;
        atomicAdd(&L.misc[0], 1u);
      }
    }
    __syncthreads();
    const int n = (int)L.misc[0];
    if (n < 2) {
      for (int s = tid; s < nsym; s += MT)
        if (L.cnt[s]) len[s] = 1;
      __syncthreads();
      break;
    }
    if (tid == 0) {
      int i = 0, j = n;
      for (int nxt = n; nxt < 2 * n - 1; ++nxt) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
          int pick;
          if (i < n && (j >= nxt || L.nw[i] <= L.nw[j])) pick = i++;
          else pick = j++;
          sum += L.nw[pick];
          L.par[pick] = (uint16_t)nxt;
        }
        L.nw[nxt] = sum;
      }
    }
    __syncthreads();
    for (int r = tid; r < n; r += MT) {
      uint32_t depth = 0;
      for (int node = r; node != 2 * n - 2 && depth < 2 * NLL; node = L.par[node]) ++depth;
      len[L.ssym[r]] = depth;
      atomicMax(&L.misc[1], depth);
    }
    __syncthreads();
    const uint32_t deepest = L.misc[1];
    __syncthreads();
    if (deepest <= 15) break;
    for (int s = tid; s < nsym; s += MT) {
      const uint32_t c = L.cnt[s];
      if (c) L.cnt[s] = (c + 1) >> 1;
    }
    __syncthreads();
  }
  if (tid < 16) L.blc[tid] = 0;
  __syncthreads();
  for (int s = tid; s < nsym; s += MT)
    if (len[s]) atomicAdd(&L.blc[len[s]], 1u);
  __syncthreads();
  if (tid == 0) {
    uint32_t code = 0;
    L.nextc[0] = 0;
    for (int b = 1; b <= 15; ++b) {
      code = (code + (b == 1 ? 0u : L.blc[b - 1])) << 1;
      L.nextc[b] = code;
    }
  }
  __syncthreads();
  for (int s = tid; s < nsym; s += MT) {
    const uint32_t l = len[s];
    uint32_t e = 0;
    if (l) {
      uint32_t k = 0;
      for (int u = 0; u < s; ++u) k += len[u] == l ? 1 : 0;
      e = (__brev(L.nextc[l] + k) >> (32 - l)) | (l << 16);
    }
    lut[s] = e;
  }
  __syncthreads();
}

// RFC 1951 3.2.5: match length 3..258 -> symbol, extra bits, extra value
__device__ __forceinline__ void length_code(int n, uint32_t& sym, uint32_t& eb, uint32_t& ev) {
  const uint32_t v = (uint32_t)n - 3;
  if (n == MAX_MATCH) {
    sym = 285; eb = 0; ev = 0;
  } else if (v < 8) {
    sym = 257 + v; eb = 0; ev = 0;
  } else {
    eb = 29 - __clz(v);                      // floor(log2 v) - 2
    sym = 261 + 4 * eb + ((v >> eb) & 3);
    ev = v & ((1u << eb) - 1);
  }
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[8], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 255; }
__device__ __forceinline__ uint32_t half_of(const uint32_t (&w)[16], int b) { return (w[b >> 1] >> (16 * (b & 1))) & 0xffff; }

__global__ __launch_bounds__(MT) void png_match_block_kernel(Geo g, CrcOps ops, int row, const uint8_t* __restrict__ streams,
                                                             uint8_t* __restrict__ slots, Rec* __restrict__ recs) {
  __shared__ MatchLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = blockIdx.x, img = blockIdx.y;
  const int64_t off = (int64_t)blk * BLOCK;
  const int N = (int)(g.total - off < BLOCK ? g.total - off : BLOCK);
  const bool first = blk == 0, last = blk == g.nblk - 1;
  const uint8_t* image = streams + (size_t)img * (size_t)g.stream_stride;   // the image's stream: history in front of the block
  const uint4* d4 = (const uint4*)(image + (size_t)off);
  const int nvec = (N + 15) >> 4;
  const int p0 = tid * 32;                   // this thread's positions

  L.reached[tid] = tid == 0 ? 1u : 0u;
  for (int s = tid; s < NLL; s += MT) {
    L.cntL[s] = s == 256 ? 1u : 0u;
    L.cntM[s] = s == 256 ? 1u : 0u;
    L.lenL[s] = 0;
  }
  if (tid < NDIST + 2) L.cntD[tid] = 0;
  if (tid < 8) L.misc[tid] = 0;
  if (tid < NCAND) {
    const int64_t S = row;
    const int64_t ds[NCAND] = {1, 2, 3, 4, 6, 9, 12, S - 3, S, S + 3, 2 * S};
    const int64_t dd = ds[tid];
    const bool ok = dd >= 1 && dd <= BLOCK;
    L.cand[tid] = ok ? (int32_t)dd : 0;
    uint32_t sym = 0, eb = 0, ev = 0;
    if (ok) {
      const uint32_t v = (uint32_t)dd - 1;
      if (v < 4) {
        sym = v;
      } else {
        const uint32_t n = 31 - __clz(v);
        eb = n - 1;
        sym = 2 * n + ((v >> (n - 1)) & 1);
        ev = v & ((1u << eb) - 1);
      }
    }
    L.dsym[tid] = sym;
    L.dbits[tid] = eb;
    L.dextra[tid] = ev;
  }
  __syncthreads();

  // the block's bytes into LDS; literal histogram (one atomic per run of equal bytes) and Adler-32 partial sums
  {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (2 * tid < nvec) {
      const uint4 q = d4[2 * tid];
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    }
    if (2 * tid + 1 < nvec) {
      const uint4 q = d4[2 * tid + 1];
      w[4] = q.x; w[5] = q.y; w[6] = q.z; w[7] = q.w;
    }
    uint4* sb4 = (uint4*)(L.x.a.sb + p0);
    sb4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    sb4[1] = make_uint4(w[4], w[5], w[6], w[7]);
    uint32_t s1 = 0, s2 = 0, prev = 0, run = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const int p = p0 + b;
      if (p < N) {
        const uint32_t v = byte_of(w, b);
        s1 += v;
        s2 += (uint32_t)(N - p) * v;         // 32 bytes a thread: < 2^31
        if (run && v != prev) {
          atomicAdd(&L.cntL[prev], run);
          run = 0;
        }
        prev = v;
        ++run;
      }
    }
    if (run) atomicAdd(&L.cntL[prev], run);
    if (p0 < N) {
      atomicAdd(&L.misc[2], s1 % ADLER);
      atomicAdd(&L.misc[3], s2 % ADLER);
    }
  }
  __syncthreads();

  // equality masks: a wave per 64 positions, a ballot per candidate
  for (int it = 0; it < BLOCK / MT; ++it) {
    const int base = (it * (MT / 64) + wave) * 64;
    const int i = base + lane;
    const int64_t gi = off + i;
    const uint32_t x = L.x.a.sb[i];
    for (int c = 0; c < NCAND; ++c) {
      const int dd = L.cand[c];
      bool e = false;
      if (dd > 0 && i < N && gi >= dd) {
        const uint32_t y = i >= dd ? L.x.a.sb[i - dd] : image[gi - dd];
        e = x == y;
      }
      const unsigned long long ball = __ballot(e);
      if (lane == 0) {
        L.x.a.mask[c][base >> 5] = (uint32_t)ball;
        L.x.a.mask[c][(base >> 5) + 1] = (uint32_t)(ball >> 32);
      }
    }
  }
  __syncthreads();

  // the longest candidate per position: length | candidate << 9 (length 0: none)
  uint32_t best[32];
#pragma unroll
  for (int b = 0; b < 32; ++b) best[b] = 0;
  for (int c = 0; c < NCAND; ++c) {
    const uint32_t mw = L.x.a.mask[c][tid];
    if (mw == 0) continue;
    uint32_t r = 0;                          // run of ones from the first position behind this word
    if (mw >> 31) {
      for (int w = tid + 1; w < MW && r < MAX_MATCH; ++w) {
        const uint32_t z = ~L.x.a.mask[c][w];
        if (z) {
          r += __ffs(z) - 1;
          break;
        }
        r += 32;
      }
    }
#pragma unroll
    for (int b = 31; b >= 0; --b) {
      r = ((mw >> b) & 1) ? r + 1 : 0;
      const uint32_t len = r < MAX_MATCH ? r : MAX_MATCH;
      if (len > (best[b] & 511)) best[b] = len | ((uint32_t)c << 9);
    }
  }
  uint32_t mw[16];                           // this thread's 32 positions, two a word: length (1: literal) | candidate << 9
#pragma unroll
  for (int b = 0; b < 32; b += 2) {
    if ((best[b] & 511) < MIN_MATCH) best[b] = 1;
    if ((best[b + 1] & 511) < MIN_MATCH) best[b + 1] = 1;
    mw[b >> 1] = best[b] | (best[b + 1] << 16);
  }
  __syncthreads();                           // the masks and the bytes are dead: jump takes their place
  {
    uint4* j4 = (uint4*)(L.x.jump + p0);
    uint32_t jw[16];
#pragma unroll
    for (int b = 0; b < 32; b += 2)
      jw[b >> 1] = (uint32_t)(p0 + b + (half_of(mw, b) & 511)) | ((uint32_t)(p0 + b + 1 + (half_of(mw, b + 1) & 511)) << 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) j4[q] = make_uint4(jw[4 * q], jw[4 * q + 1], jw[4 * q + 2], jw[4 * q + 3]);
  }
  __syncthreads();

  // greedy parse = the positions reachable from 0 under i -> i + length: after round k every position within 2^(k+1)
  // steps is marked and jump holds 2^(k+1) steps.  A mark seen early only marks another position of the chain.
  for (int k = 0; (1 << k) < N; ++k) {
    const uint32_t rw = L.reached[tid];
    uint4* j4 = (uint4*)(L.x.jump + p0);     // this thread's 32 pointers: four 16-byte reads, not 32 of two bytes
    uint32_t jw[16], nj[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint4 v = j4[q];
      jw[4 * q] = v.x; jw[4 * q + 1] = v.y; jw[4 * q + 2] = v.z; jw[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      const uint32_t j = half_of(jw, b);
      uint32_t j2 = j;
      if (j < (uint32_t)N) {
        j2 = L.x.jump[j];
        if ((rw >> b) & 1) atomicOr(&L.reached[j >> 5], 1u << (j & 31));
      }
      if (b & 1) nj[b >> 1] |= j2 << 16;
      else nj[b >> 1] = j2;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) j4[q] = make_uint4(nj[4 * q], nj[4 * q + 1], nj[4 * q + 2], nj[4 * q + 3]);
    __syncthreads();
  }

  // this thread's bytes again (for the literals of the parse), match-form histogram
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (2 * tid < nvec) {
    const uint4 q = d4[2 * tid];
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
  }
  if (2 * tid + 1 < nvec) {
    const uint4 q = d4[2 * tid + 1];
    w[4] = q.x; w[5] = q.y; w[6] = q.z; w[7] = q.w;
  }
  const uint32_t rw = L.reached[tid];
  {
    uint32_t xb = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      if ((rw >> b) & 1) {
        const uint32_t e = half_of(mw, b), len = e & 511, c = e >> 9;
        if (len >= MIN_MATCH) {
          uint32_t sym, eb, ev;
          length_code((int)len, sym, eb, ev);
          atomicAdd(&L.cntM[sym], 1u);
          atomicAdd(&L.cntD[L.dsym[c]], 1u);
          xb += eb + L.dbits[c];
        } else {
          atomicAdd(&L.cntM[byte_of(w, b)], 1u);
        }
      }
    }
    if (xb) atomicAdd(&L.misc[4], xb);
  }
  __syncthreads();

  // three codes, both bit totals, the choice
  huff_build(L, L.cntL, NSYM, L.lenL, L.lutL, tid);
  huff_build(L, L.cntM, NLL, L.lenM, L.lutM, tid);
  huff_build(L, L.cntD, NDIST, L.lenD, L.lutD, tid);
  {
    uint32_t bl = 0, bm = 0;
    for (int s = tid; s < NLL; s += MT) {
      if (s < NSYM) bl += L.cntL[s] * L.lenL[s];
      bm += L.cntM[s] * L.lenM[s];
      if (s < NDIST) bm += L.cntD[s] * L.lenD[s];
    }
    if (bl) atomicAdd(&L.misc[5], bl);
    if (bm) atomicAdd(&L.misc[6], bm);
  }
  __syncthreads();                           // also: nobody reads jump any more, the chunk takes its place
  const bool use_match = MHEADER_BITS + L.misc[6] + L.misc[4] < HEADER_BITS + L.misc[5];
  uint32_t* out = L.x.c.out;
  uint32_t* scan = L.x.c.scan;
  for (int i = tid; i < SLOT_WORDS; i += MT) out[i] = 0;
  if (tid < 256) {
    uint32_t c = tid;
    for (int i = 0; i < 8; ++i) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
    L.x.c.crct[tid] = c;
  }

  // bits of this thread's symbols, scanned over the workgroup
  uint32_t bits = 0;
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    if (p0 + b < N) {
      if (!use_match) {
        bits += L.lutL[byte_of(w, b)] >> 16;
      } else if ((rw >> b) & 1) {
        const uint32_t e = half_of(mw, b), len = e & 511, c = e >> 9;
        if (len >= MIN_MATCH) {
          uint32_t sym, eb, ev;
          length_code((int)len, sym, eb, ev);
          bits += (L.lutM[sym] >> 16) + eb + (L.lutD[L.dsym[c]] >> 16) + L.dbits[c];
        } else {
          bits += L.lutM[byte_of(w, b)] >> 16;
        }
      }
    }
  }
  scan[tid] = bits;
  __syncthreads();
  for (int s = 1; s < MT; s <<= 1) {
    const uint32_t add = tid >= s ? scan[tid - s] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const uint32_t base = 8u * (4 + (first ? 2 : 0));
  const uint32_t lit0 = base + (use_match ? MHEADER_BITS : HEADER_BITS);

  // header: block type, counts, the fixed code-length code, then the code lengths at 4 bits each
  if (tid == 0) {
    out[0] |= 0x54414449u;                               // "IDAT"
    if (first) atomicOr(&out[1], 0x0178u);               // zlib header 78 01
    put_bits(out, base, 4, 3);                           // BFINAL 0, BTYPE 2
    if (use_match) put_bits(out, base + 3, (NLL - 257) | ((NDIST - 1) << 5), 10);
    put_bits(out, base + 13, 15, 4);                     // HCLEN 19
    for (int i = 3; i < 19; ++i) put_bits(out, base + 17 + 3 * i, 4, 3);
  }
  if (use_match) {
    for (int s = tid; s < NLL + NDIST; s += MT)
      put_bits(out, base + 74 + 4 * s, __brev(s < NLL ? L.lenM[s] : L.lenD[s - NLL]) >> 28, 4);
  } else {
    for (int s = tid; s < NSYM + 1; s += MT) put_bits(out, base + 74 + 4 * s, __brev(L.lenL[s]) >> 28, 4);   // lenL[257]: the distance length, 0
  }

  // symbols
  {
    const uint32_t pos = lit0 + scan[tid] - bits;
    uint32_t ow = pos >> 5;
    int nb = pos & 31;
    uint64_t acc = 0;
#pragma unroll
    for (int b = 0; b < 32; ++b) {
      if (p0 + b < N && (!use_match || ((rw >> b) & 1))) {
        const uint32_t e = use_match ? half_of(mw, b) : 1u, len = e & 511, c = e >> 9;
        if (len >= MIN_MATCH) {
          uint32_t sym, eb, ev;
          length_code((int)len, sym, eb, ev);
          const uint32_t el = L.lutM[sym], ed = L.lutD[L.dsym[c]];
          acc |= (uint64_t)((el & 0xffff) | (ev << (el >> 16))) << nb;   // <= 15 + 5 bits
          nb += (el >> 16) + eb;
          if (nb >= 32) {
            if (ow < SLOT_WORDS) atomicOr(&out[ow], (uint32_t)acc);
            ++ow;
            acc >>= 32;
            nb -= 32;
          }
          acc |= (uint64_t)((ed & 0xffff) | (L.dextra[c] << (ed >> 16))) << nb;   // <= 15 + 13 bits
          nb += (ed >> 16) + L.dbits[c];
        } else {
          const uint32_t el = use_match ? L.lutM[byte_of(w, b)] : L.lutL[byte_of(w, b)];
          acc |= (uint64_t)(el & 0xffff) << nb;
          nb += el >> 16;
        }
        if (nb >= 32) {
          if (ow < SLOT_WORDS) atomicOr(&out[ow], (uint32_t)acc);
          ++ow;
          acc >>= 32;
          nb -= 32;
        }
      }
    }
    if (nb > 0 && ow < SLOT_WORDS) atomicOr(&out[ow], (uint32_t)acc);
  }
  // end of block, the empty stored block
  const uint32_t eob = use_match ? L.lutM[256] : L.lutL[256];
  uint32_t end = lit0 + scan[MT - 1];
  if (tid == 0) put_bits(out, end, eob & 0xffff, 16);
  end += eob >> 16;
  if (tid == 0) put_bits(out, end, last ? 1 : 0, 3);
  uint32_t bytes = (end + 3 + 7) >> 3;
  if (tid == 0) put_bits(out, bytes * 8, 0xFFFF0000u, 32);
  bytes += 4;
  if (bytes > SLOT) bytes = SLOT;                        // cannot happen (block_cap); never leave the slot
  __syncthreads();

  uint4* slot = (uint4*)(slots + ((size_t)img * g.nblk + blk) * SLOT);
  const uint4* o4 = (const uint4*)out;
  for (int i = tid; i * 16 < (int)bytes; i += MT) slot[i] = o4[i];

  // CRC-32 of type + data: 256 pieces, as png_block_kernel
  {
    const uint8_t* ob = (const uint8_t*)out;
    const int pad = SLOT - (int)bytes;
    uint32_t c = 0;
    if (tid < NT) {
      for (int i = 0; i < PIECE; ++i) {
        const int di = tid * PIECE + i - pad;
        if (di >= 0) c = L.x.c.crct[(c ^ ob[di] ^ (di < 4 ? 0xFFu : 0u)) & 255] ^ (c >> 8);
      }
    }
    __syncthreads();                                     // the scan's last reads (scan[MT - 1]) are done
    if (tid < NT) scan[tid] = c;
    for (int j = 0; j < 8; ++j) {
      __syncthreads();
      const int s = 1 << j;
      if (tid < NT && (tid & (2 * s - 1)) == 0) scan[tid] = mulmod(ops.k[j], scan[tid]) ^ scan[tid + s];
    }
  }
  if (tid == 0) {
    Rec r;
    r.bytes = bytes;
    r.crc = scan[0];
    r.a = L.misc[2] % ADLER;
    r.b = L.misc[3] % ADLER;
    recs[(size_t)img * g.nblk + blk] = r;
  }
}

int png_check(const rcdm_png_desc* d) {
  if (d->n <= 0 || d->channels != 3 || d->filter < RCDM_PNG_ADAPTIVE || d->filter > 4) return RCDM_EINVAL;
  if (d->h < 1 || d->w < 1 || d->h > MAX_SIDE || d->w > MAX_SIDE || d->n > 65535) return RCDM_ESHAPE;
  if (d->src_pitch < 3 * (int64_t)d->w || d->src_stride < 0) return RCDM_EINVAL;
  return RCDM_OK;
}

Geo png_geo(const rcdm_png_desc* d) {
  Geo g;
  g.total = (int64_t)d->h * (1 + 3 * (int64_t)d->w);
  g.stream_stride = (g.total + 15) & ~(int64_t)15;
  g.nblk = (int32_t)((g.total + BLOCK - 1) / BLOCK);
  g.slots_off = ((int64_t)d->n * g.stream_stride + 255) & ~(int64_t)255;
  g.recs_off = g.slots_off + (int64_t)d->n * g.nblk * SLOT;
  return g;
}

size_t png_bound(const Geo& g) {
  const int64_t tail = g.total - (int64_t)(g.nblk - 1) * BLOCK;
  return (size_t)(8 + 25 + 12 + (int64_t)(g.nblk - 1) * (12 + block_cap(BLOCK)) + 12 + block_cap(tail));
}

CrcOps png_crc_ops() {
  CrcOps ops;
  uint32_t p = 1u << 31, sq = 1u << 30;                  // x^0, x^1
  for (uint32_t e = 8u * PIECE; e; e >>= 1) {
    if (e & 1) p = mulmod(p, sq);
    sq = mulmod(sq, sq);
  }
  for (int j = 0; j < 8; ++j) {
    ops.k[j] = p;
    p = mulmod(p, p);
  }
  return ops;
}

}  // namespace

extern "C" {

size_t rcdm_png_bound(const rcdm_png_desc* d) {
  if (!d || png_check(d) != RCDM_OK) return 0;
  return png_bound(png_geo(d));
}

size_t rcdm_png_workspace_bytes(const rcdm_png_desc* d) {
  if (!d || png_check(d) != RCDM_OK) return 0;
  const Geo g = png_geo(d);
  return (size_t)(g.recs_off + (int64_t)d->n * g.nblk * (int64_t)sizeof(Rec));
}

int rcdm_png_encode(const rcdm_png_desc* d, const void* src, void* workspace, void* dst, uint64_t* sizes, void* stream) {
  if (!d || !src || !workspace || !dst || !sizes) return RCDM_EINVAL;
  const int rc = png_check(d);
  if (rc != RCDM_OK) return rc;
  const Geo g = png_geo(d);
  if (d->n > 1 && d->dst_stride < (int64_t)png_bound(g)) return RCDM_EINVAL;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)sizes & 7)) return RCDM_EINVAL;
  static const CrcOps ops = png_crc_ops();
  uint8_t* ws = (uint8_t*)workspace;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(png_filter_kernel, dim3((d->h + NT / 64 - 1) / (NT / 64), d->n), dim3(NT), 0, s, *d, (const uint8_t*)src, ws,
                     g.stream_stride);
  hipLaunchKernelGGL(png_block_kernel, dim3(g.nblk, d->n), dim3(NT), 0, s, g, ops, (const uint8_t*)ws, ws + g.slots_off,
                     (Rec*)(ws + g.recs_off));
  hipLaunchKernelGGL(png_assemble_kernel, dim3(g.nblk, d->n), dim3(NT), 0, s, *d, g, (const uint8_t*)(ws + g.slots_off),
                     (const Rec*)(ws + g.recs_off), (uint8_t*)dst, sizes);
  return rcdm_check_launch();
}

size_t rcdm_png_match_workspace_bytes(const rcdm_png_desc* d) { return rcdm_png_workspace_bytes(d); }

int rcdm_png_encode_match(const rcdm_png_desc* d, const void* src, void* workspace, void* dst, uint64_t* sizes, void* stream) {
  if (!d || !src || !workspace || !dst || !sizes) return RCDM_EINVAL;
  const int rc = png_check(d);
  if (rc != RCDM_OK) return rc;
  const Geo g = png_geo(d);
  if (d->n > 1 && d->dst_stride < (int64_t)png_bound(g)) return RCDM_EINVAL;
  if (((uintptr_t)workspace & 15) || ((uintptr_t)sizes & 7)) return RCDM_EINVAL;
  static const CrcOps ops = png_crc_ops();
  uint8_t* ws = (uint8_t*)workspace;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(png_filter_kernel, dim3((d->h + NT / 64 - 1) / (NT / 64), d->n), dim3(NT), 0, s, *d, (const uint8_t*)src, ws,
                     g.stream_stride);
  hipLaunchKernelGGL(png_match_block_kernel, dim3(g.nblk, d->n), dim3(MT), 0, s, g, ops, 1 + 3 * d->w, (const uint8_t*)ws,
                     ws + g.slots_off, (Rec*)(ws + g.recs_off));
  hipLaunchKernelGGL(png_assemble_kernel, dim3(g.nblk, d->n), dim3(NT), 0, s, *d, g, (const uint8_t*)(ws + g.slots_off),
                     (const Rec*)(ws + g.recs_off), (uint8_t*)dst, sizes);
  return rcdm_check_launch();
}

}  // extern "C"
