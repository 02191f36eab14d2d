// The lane-free core of the PNG reader (include/rcdm.h, "PNG, reading"): everything of inflate and of the PNG filters that
// is the same for one CPU thread and for one wavefront.  csrc/png_decode.hip runs it with a wave behind the `IO` policy
// (LDS window, wave-wide copies), tools/png_decode_host.cpp with plain loops — the same control flow, the same checks, the
// same status codes, so corrupt input is exercised on the CPU before any of it reaches a GPU.
//
//   codes      a Huffman code is kept canonically (RFC 1951 3.2.2): count[len] and the symbols sorted by (len, symbol).
//              canon_build validates the set as zlib does: over-subscribed -> ECODES; incomplete -> ECODES unless it is one
//              code of length 1 (the single distance code deflate allows); an empty set builds and decodes nothing.
//   tables     first level only: LIT_BITS / DIST_BITS peeked bits -> symbol << 4 | length, each entry computed on its own
//              by canon_decode (so a wave fills the table in parallel); 0 = the code is longer than the table — or
//              unassigned — and the step walks the canonical arrays bit by bit.  About 3.8 KB for all of it.
//   lanes      canon_build is a serial read-modify-write of the counters: ONE lane runs it (IO::lane == 0) between two
//              syncs and leaves its result in Tables::built; every other store of the block header (code lengths) is the
//              same value from every lane, and every value that steers control flow goes through IO::uni first.
//   bounds     every read position is checked against the stream's bits and every write against `expect` BEFORE the IO is
//              asked to move a byte: the IO policy never sees a position outside [0, expect) or a distance beyond pos.
//
// IO policy (device: one wavefront, all values uniform; host: one thread):
//   LANES, lane      the table fill strides by them
//   uni(v)           a value every lane holds -> provably uniform (readfirstlane); identity on the host
//   sync()           orders the lanes' table / window writes before later reads
//   word(i)          little-endian 32-bit word i of the zlib stream, 0 beyond its end
//   literal(pos, b)  out[pos] = b
//   match(pos, L, D) out[pos + i] = out[pos - D + i % D], i < L
//   stored(at, pos, n)  out[pos + i] = stream byte at + i, i < n
//   adler(pos)       Adler-32 of out[0, pos) (the device IO sums it as it flushes its window)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) && (defined(__HIP_DEVICE_COMPILE__) || defined(__HIP__))
#define PNGD_HD __host__ __device__ __forceinline__
#else
#define PNGD_HD inline
#endif

namespace pngd {

// the values of RCDM_PNG_E* in include/rcdm.h
enum Status {
  OK = 0,
  EZLIB = 1,      // zlib header: CM != 8, window > 32 K, preset dictionary, header checksum
  ETRUNC = 2,     // the stream ends inside a block or in front of the Adler-32
  EBLOCK = 3,     // block type 3
  ESTORED = 4,    // stored block: LEN != ~NLEN
  ECODES = 5,     // a code-length set that is over-subscribed, incomplete, too long, or lacks end-of-block
  ESYMBOL = 6,    // length symbol 286 / 287, distance symbol 30 / 31, or a bit pattern no code owns
  EDISTANCE = 7,  // a distance that reaches in front of the first output byte
  EOVERRUN = 8,   // the stream holds more than h * (1 + bpp * w) bytes
  EUNDERRUN = 9,  // the stream ends with fewer
  EADLER = 10,    // Adler-32 of the inflated bytes
  EFILTER = 11    // a filter byte above 4
};

constexpr int LIT_BITS = 10, DIST_BITS = 8, WINDOW = 32768;

struct CanonLit {
  uint16_t count[16], offs[16], sym[288];
};
struct CanonDist {  // the distance code, and the code-length code in front of it
  uint16_t count[16], offs[16], sym[32];
};
struct Tables {
  CanonLit lit;
  CanonDist dist;
  uint16_t lit1[1 << LIT_BITS];
  uint16_t dist1[1 << DIST_BITS];
  uint8_t lens[320];
  uint8_t cl[20];
  int32_t built;  // lane 0's canon_build result, read by every lane behind a sync
};

template <class C>
PNGD_HD int canon_build(C& c, const uint8_t* lens, int n, bool one_code_ok = true) {
  for (int l = 0; l < 16; ++l) c.count[l] = 0;
  for (int i = 0; i < n; ++i) c.count[lens[i]] = (uint16_t)(c.count[lens[i]] + 1);
  int left = 1, maxl = 0;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - (int)c.count[l];
    if (left < 0) return ECODES;
    if (c.count[l]) maxl = l;
  }
  if (maxl && left > 0 && !(one_code_ok && maxl == 1)) return ECODES;
  c.offs[1] = 0;
  for (int l = 1; l < 15; ++l) c.offs[l + 1] = (uint16_t)(c.offs[l] + c.count[l]);
  for (int i = 0; i < n; ++i) {
    int l = lens[i];
    if (l) {
      c.sym[c.offs[l]] = (uint16_t)i;
      c.offs[l] = (uint16_t)(c.offs[l] + 1);
    }
  }
  return OK;
}

// the code that starts at bit 0 of `bits`, at most maxlen long -> symbol << 4 | length, or 0
template <class C>
PNGD_HD uint32_t canon_decode(const C& c, uint32_t bits, int maxlen) {
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= maxlen; ++len) {
    code |= (int)(bits & 1);
    bits >>= 1;
    int cnt = c.count[len];
    if (code - cnt < first) return ((uint32_t)c.sym[index + (code - first)] << 4) | (uint32_t)len;
    index += cnt;
    first = (first + cnt) << 1;
    code <<= 1;
  }
  return 0;
}

PNGD_HD uint32_t length_base(int s) {
  static constexpr uint16_t t[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  return t[s];
}
PNGD_HD int length_extra(int s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
PNGD_HD uint32_t dist_base(int s) {
  static constexpr uint16_t t[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  return t[s];
}
PNGD_HD int dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }
PNGD_HD int cl_order(int i) {
  static constexpr uint8_t t[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return t[i];
}

template <class IO>
struct Reader {
  IO& io;
  uint64_t bb;
  int bc;
  uint32_t next;
  PNGD_HD explicit Reader(IO& io_) : io(io_), bb(0), bc(0), next(0) {}
  PNGD_HD void refill() {
    if (bc <= 32) {
      bb |= (uint64_t)io.word(next) << bc;
      ++next;
      bc += 32;
    }
  }
  PNGD_HD uint32_t peek() {  // >= 32 valid bits
    refill();
    return (uint32_t)bb;
  }
  PNGD_HD void skip(int n) {
    bb >>= n;
    bc -= n;
  }
  PNGD_HD uint32_t bits(int n) {  // n <= 16
    uint32_t v = peek() & ((1u << n) - 1u);
    skip(n);
    return v;
  }
  PNGD_HD uint64_t consumed() const { return (uint64_t)next * 32u - (uint64_t)bc; }
  PNGD_HD void seek(uint64_t byte) {
    next = (uint32_t)(byte >> 2);
    bb = 0;
    bc = 0;
    refill();
    skip((int)(byte & 3) * 8);
  }
};

template <class IO, class C>
PNGD_HD void fill_table(IO& io, const C& c, uint16_t* table, int bits) {
  for (int i = io.lane; i < (1 << bits); i += IO::LANES) table[i] = (uint16_t)canon_decode(c, (uint32_t)i, bits);
}

// zlib stream of `zbytes` bytes behind io.word -> exactly `expect` bytes through io; -> Status
template <class IO>
PNGD_HD int inflate(IO& io, Tables& T, uint64_t zbytes, uint32_t expect) {
  Reader<IO> r(io);
  const uint64_t zbits = zbytes * 8u;
  uint32_t cmf = r.bits(8), flg = r.bits(8);
  if (r.consumed() > zbits) return ETRUNC;
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || ((cmf << 8) | flg) % 31) return EZLIB;
  uint32_t pos = 0, final_block;
  do {
    final_block = r.bits(1);
    uint32_t type = r.bits(2);
    if (r.consumed() > zbits) return ETRUNC;
    if (type == 3) return EBLOCK;
    if (type == 0) {
      r.skip(r.bc & 7);
      uint32_t len = r.bits(16), nlen = r.bits(16);
      if (r.consumed() > zbits) return ETRUNC;
      if ((len ^ 0xffffu) != nlen) return ESTORED;
      uint64_t at = r.consumed() >> 3;
      if (at + len > zbytes) return ETRUNC;
      if (len > expect - pos) return EOVERRUN;
      io.stored(at, pos, len);
      pos += len;
      r.seek(at + len);
      continue;
    }
    int nlit, ndist;
    if (type == 1) {
      nlit = 288;
      ndist = 32;
      for (int i = 0; i < 288; ++i) T.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
      for (int i = 0; i < 32; ++i) T.lens[288 + i] = 5;
    } else {
      nlit = (int)r.bits(5) + 257;
      ndist = (int)r.bits(5) + 1;
      int ncl = (int)r.bits(4) + 4;
      if (nlit > 286 || ndist > 30) return ECODES;
      for (int i = 0; i < 19; ++i) T.cl[cl_order(i)] = (uint8_t)(i < ncl ? r.bits(3) : 0);
      if (r.consumed() > zbits) return ETRUNC;
      io.sync();
      if (io.lane == 0) T.built = canon_build(T.dist, T.cl, 19, false);
      io.sync();
      if (io.uni((uint32_t)T.built)) return ECODES;
      int i = 0;
      while (i < nlit + ndist) {
        uint32_t e = io.uni(canon_decode(T.dist, r.peek(), 7));
        if (!e) return ECODES;
        r.skip((int)(e & 15));
        int s = (int)(e >> 4), rep = 1;
        uint8_t v = (uint8_t)s;
        if (s >= 16) {
          if (s == 16) {
            if (i == 0) return ECODES;
            v = T.lens[i - 1];
            rep = 3 + (int)r.bits(2);
          } else {
            v = 0;
            rep = s == 17 ? 3 + (int)r.bits(3) : 11 + (int)r.bits(7);
          }
          v = (uint8_t)io.uni(v);
        }
        if (r.consumed() > zbits) return ETRUNC;
        if (i + rep > nlit + ndist) return ECODES;
        for (; rep > 0; --rep) T.lens[i++] = v;
      }
      io.sync();
      if (io.uni(T.lens[256]) == 0) return ECODES;
    }
    io.sync();
    if (io.lane == 0) T.built = canon_build(T.lit, T.lens, nlit) | canon_build(T.dist, T.lens + nlit, ndist);
    io.sync();
    if (io.uni((uint32_t)T.built)) return ECODES;
    fill_table(io, T.lit, T.lit1, LIT_BITS);
    fill_table(io, T.dist, T.dist1, DIST_BITS);
    io.sync();
    for (;;) {
      uint32_t v = r.peek();
      uint32_t e = io.uni(T.lit1[v & ((1u << LIT_BITS) - 1u)]);
      if (!e) e = io.uni(canon_decode(T.lit, v, 15));
      if (!e) return ESYMBOL;
      r.skip((int)(e & 15));
      int sym = (int)(e >> 4);
      if (sym < 256) {
        if (r.consumed() > zbits) return ETRUNC;
        if (pos >= expect) return EOVERRUN;
        io.literal(pos, (uint8_t)sym);
        ++pos;
        continue;
      }
      if (sym == 256) {
        if (r.consumed() > zbits) return ETRUNC;
        break;
      }
      if (sym >= 286) return ESYMBOL;
      sym -= 257;
      uint32_t L = length_base(sym) + r.bits(length_extra(sym));
      v = r.peek();
      e = io.uni(T.dist1[v & ((1u << DIST_BITS) - 1u)]);
      if (!e) e = io.uni(canon_decode(T.dist, v, 15));
      if (!e) return ESYMBOL;
      r.skip((int)(e & 15));
      int ds = (int)(e >> 4);
      if (ds >= 30) return ESYMBOL;
      uint32_t D = dist_base(ds) + r.bits(dist_extra(ds));
      if (r.consumed() > zbits) return ETRUNC;
      if (D > pos) return EDISTANCE;
      if (L > expect - pos) return EOVERRUN;
      io.match(pos, L, D);
      pos += L;
    }
  } while (!final_block);
  if (pos != expect) return EUNDERRUN;
  r.skip(r.bc & 7);
  uint32_t want = 0;
  for (int k = 0; k < 4; ++k) want = (want << 8) | r.bits(8);
  if (r.consumed() > zbits) return ETRUNC;
  return want == io.adler(pos) ? OK : EADLER;
}

// ---- PNG filters and colour types -------------------------------------------------------------
PNGD_HD int bytes_per_pixel(uint32_t color_type) {  // bit depth 8; 0 = not a colour type
  return color_type == 0 ? 1 : color_type == 2 ? 3 : color_type == 3 ? 1 : color_type == 4 ? 2 : color_type == 6 ? 4 : 0;
}

// one byte back through filter ft (0..4): x the filtered byte, a left, b above, c above-left (reconstructed, 0 outside)
PNGD_HD uint32_t unfilter_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  int p = (int)a + (int)b - (int)c;
  int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
  uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  uint32_t pred = ft == 0 ? 0u : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth;
  return (x + pred) & 255u;
}

// a pixel's reconstructed bytes, packed little-endian in px -> r | g << 8 | b << 16; palette indices >= plte_entries are black
PNGD_HD uint32_t to_rgb(uint32_t color_type, uint32_t px, const uint8_t* plte, uint32_t plte_entries) {
  if (color_type == 2 || color_type == 6) return px & 0xffffffu;
  if (color_type == 3) {
    uint32_t i = px & 255u;
    if (i >= plte_entries) return 0;
    return (uint32_t)plte[3 * i] | ((uint32_t)plte[3 * i + 1] << 8) | ((uint32_t)plte[3 * i + 2] << 16);
  }
  uint32_t g = px & 255u;
  return g | (g << 8) | (g << 16);
}

// Adler-32 state (s1, s2) advanced over n <= 4096 bytes given their plain sum and the sum of (n - i) * b[i]
PNGD_HD void adler_advance(uint32_t& s1, uint32_t& s2, uint32_t n, uint32_t sum, uint32_t weighted) {
  s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)n * s1 + weighted) % 65521u);
  s1 = (s1 + sum) % 65521u;
}

}  // namespace pngd
