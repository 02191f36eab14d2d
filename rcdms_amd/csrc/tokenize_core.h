// tokenize_core.h — the CLIP tokenizer's steps (include/rcdm.h, "CLIP tokenizer") as plain, lane-free C++: shared by the kernel
// (tokenize.hip) and by tools/tokenize_host.cpp, which runs the same functions on one CPU thread.  Nothing here knows about
// lanes, LDS or HIP beyond the TOK_HD marker; every function works on arrays its caller owns (Work), sized MAX_CAPTION.
//   special_at      step 1a, one position at a time: the longest special string that starts here on the raw bytes
//   resolve_specials  serial: keeps the leftmost non-overlapping of those matches and sets the stretch limits
//   match_added     step 1b, one position at a time (the kernel: a position per lane): the longest add_tokens string that
//                   starts here on the lower-cased bytes and ends inside the stretch
//   scan            steps 1c-3 + the symbols of step 4, serial: resolves the matches left to right, splits what lies between
//                   them into words and writes one symbol per byte (sym), its successor inside the word (nxt) and the word's
//                   first symbol (wst).  A match is a word of one symbol: it never merges
//   candidate / apply_merge   one round of step 4: the key (rank, position) of the live pair at a symbol, and the merge itself.
//                   A round takes the least key of every word (the kernel: an LDS minimum per word) and applies that ONE merge
//                   per word, the backend's order: lowest rank, leftmost first
//   frame           step 5: the value and mask of one output column
// Limits (checked by the callers before any of this runs): captions of at most MAX_CAPTION bytes, all below 0x80; at most
// MAX_ROWS table rows of at most MAX_ADDED_LEN bytes; ranks below 2^RANK_BITS.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TOK_HD __host__ __device__ inline
#else
#define TOK_HD inline
#endif

namespace tok {

constexpr int MAX_CAPTION = 1024;                 // bytes of one caption (RCDM_TOK_MAX_CAPTION)
constexpr int MAX_ADDED_LEN = 32;                 // bytes of one added or special token (RCDM_TOK_MAX_ADDED_LEN)
constexpr int MAX_ROWS = 66;                      // RCDM_TOK_MAX_ADDED tokens of add_tokens + the two special strings
constexpr int POS_BITS = 10;                      // a key is rank << POS_BITS | position: MAX_CAPTION == 1 << POS_BITS
constexpr int RANK_BITS = 32 - POS_BITS;
constexpr uint32_t NONE = 0xFFFFFFFFu;            // no key; an empty pair slot (a == NONE)
constexpr uint16_t END = 0xFFFFu;                 // nxt of a word's last symbol
static_assert(MAX_CAPTION == 1 << POS_BITS, "a position must fit the key");

struct Added {                                    // rcdm_tok_added
  uint8_t text[MAX_ADDED_LEN];                    // special: as written; else lower-cased
  int32_t len, id, special, reserved;
};
struct alignas(16) Pair {                         // rcdm_tok_pair: one slot of the open-addressing table, one 16-byte load
  uint32_t a, b, rank, merged;
};
static_assert(sizeof(Added) == 48 && sizeof(Pair) == 16, "the layouts of include/rcdm.h");

struct Work {
  uint8_t* txt;     // [L] the caption's bytes
  uint16_t* lim;    // [L] end of the stretch a byte lies in; 0 for the bytes of a special match
  uint8_t* mlen;    // [L] length of the match that starts here, 0: none
  uint8_t* mrow;    // [L] its table row
  int32_t* sym;     // [nsym] token id, -1 once merged into its left neighbour
  uint16_t* nxt;    // [nsym] next live symbol of the word, END at its last
  uint16_t* wst;    // [nsym] first symbol of the word
};

TOK_HD int lower(int c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }
// 0 whitespace (9-13, 32), 1 letter, 2 digit, 3 anything else; c already lower-cased
TOK_HD int cls(int c) { return (c >= 9 && c <= 13) || c == 32 ? 0 : c >= 'a' && c <= 'z' ? 1 : c >= '0' && c <= '9' ? 2 : 3; }

TOK_HD uint32_t pair_hash(uint32_t a, uint32_t b) {
  uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

// slots: a power of two, at most half full (the host builds it so); the probe count is bounded all the same
TOK_HD bool pair_lookup(const Pair* table, uint32_t slots, uint32_t a, uint32_t b, uint32_t& rank, uint32_t& merged) {
  uint32_t at = pair_hash(a, b) & (slots - 1);
  for (uint32_t probe = 0; probe < slots; ++probe) {
    const Pair e = table[at];
    if (e.a == NONE) return false;
    if (e.a == a && e.b == b) {
      rank = e.rank;
      merged = e.merged;
      return true;
    }
    at = (at + 1) & (slots - 1);
  }
  return false;
}

// the longest row of the wanted kind that matches at p and ends at or before `end`; -> its length, 0: none
TOK_HD int longest_at(const Work& w, int p, int end, const Added* rows, int n_rows, bool special, int& row) {
  int best = 0;
  for (int r = 0; r < n_rows; ++r) {
    const int len = rows[r].len;
    if ((rows[r].special != 0) != special || len <= best || p + len > end) continue;
    int k = 0;
    if (special)
      while (k < len && w.txt[p + k] == rows[r].text[k]) ++k;
    else
      while (k < len && lower(w.txt[p + k]) == rows[r].text[k]) ++k;
    if (k == len) {
      best = len;
      row = r;
    }
  }
  return best;
}

// step 1a, one position at a time: the longest special string that starts at p on the raw bytes
TOK_HD void special_at(const Work& w, int p, int L, const Added* rows, int n_rows) {
  int row = 0;
  w.mlen[p] = (uint8_t)longest_at(w, p, L, rows, n_rows, true, row);
  w.mrow[p] = (uint8_t)row;
}

// step 1a, serial, after special_at on every position: keeps the leftmost non-overlapping matches and sets the stretch limits
TOK_HD void resolve_specials(const Work& w, int L) {
  int start = 0;
  for (int p = 0; p < L;) {
    const int len = w.mlen[p];
    if (!len) {
      ++p;
      continue;
    }
    for (int q = start; q < p; ++q) w.lim[q] = (uint16_t)p;
    for (int q = p; q < p + len; ++q) {
      w.lim[q] = 0;
      if (q > p) w.mlen[q] = 0;
    }
    start = p += len;
  }
  for (int q = start; q < L; ++q) w.lim[q] = (uint16_t)L;
}

TOK_HD void match_added(const Work& w, int p, const Added* rows, int n_rows) {
  if (w.lim[p] <= p) return;                       // a byte of a special match
  int row = 0;
  const int len = longest_at(w, p, w.lim[p], rows, n_rows, false, row);
  w.mlen[p] = (uint8_t)len;
  w.mrow[p] = (uint8_t)row;
}

// -> nsym (<= L: a byte gives at most one symbol)
TOK_HD int scan(const Work& w, int L, const Added* rows, const int32_t* byte_plain, const int32_t* byte_end) {
  int n = 0;
  for (int p = 0; p < L;) {
    if (w.mlen[p]) {                               // reached by steps of matches and words only: a resolved match
      w.sym[n] = rows[w.mrow[p]].id;
      w.nxt[n] = END;
      w.wst[n] = (uint16_t)n;
      ++n;
      p += w.mlen[p];
      continue;
    }
    const int c = lower(w.txt[p]), k = cls(c);
    if (k == 0) {
      ++p;
      continue;
    }
    // a word never reaches into the next match: `free(q)` is "byte q exists and no match starts there"
    auto at = [&](int q) { return q < L && !w.mlen[q] ? lower(w.txt[q]) : -1; };
    int q = 0;
    if (c == '\'') {
      const int c1 = at(p + 1), c2 = c1 < 0 ? -1 : at(p + 2);
      if (c1 == 's' || c1 == 't') q = p + 2;                                                   // 's 't
      else if ((c1 == 'r' || c1 == 'v') && c2 == 'e') q = p + 3;                               // 're 've
      else if (c1 == 'm') q = p + 2;                                                           // 'm
      else if (c1 == 'l' && c2 == 'l') q = p + 3;                                              // 'll
      else if (c1 == 'd') q = p + 2;                                                           // 'd
    }
    if (!q) {
      q = p + 1;
      while (k != 2 && at(q) >= 0 && cls(at(q)) == k) ++q;      // a run of letters or of other bytes; a digit stands alone
    }
    const int first = n;
    for (int j = p; j < q; ++j, ++n) {
      const int b = lower(w.txt[j]);
      w.sym[n] = j == q - 1 ? byte_end[b] : byte_plain[b];
      w.nxt[n] = j == q - 1 ? END : (uint16_t)(n + 1);
      w.wst[n] = (uint16_t)first;
    }
    p = q;
  }
  return n;
}

// the key of the pair (symbol i, its successor) and what it merges to; NONE when i is dead, last in its word or the pair has
// no merge
TOK_HD uint32_t candidate(const Work& w, int i, const Pair* table, uint32_t slots, uint32_t& merged) {
  const int32_t a = w.sym[i];
  const uint16_t j = w.nxt[i];
  uint32_t rank = 0;
  if (a < 0 || j == END || !pair_lookup(table, slots, (uint32_t)a, (uint32_t)w.sym[j], rank, merged)) return NONE;
  return rank << POS_BITS | (uint32_t)i;
}

TOK_HD void apply_merge(const Work& w, int i, uint32_t merged) {
  const uint16_t j = w.nxt[i];
  w.sym[i] = (int32_t)merged;
  w.nxt[i] = w.nxt[j];
  w.sym[j] = -1;
}

// column `col` of a row that keeps `kept` tokens (tokens[0 .. kept)): bos, the tokens, eos, pad
TOK_HD int32_t frame(int col, int kept, const int32_t* tokens, int32_t bos, int32_t eos, int32_t pad, int& mask) {
  mask = col <= kept + 1;
  return col == 0 ? bos : col <= kept ? tokens[col - 1] : col == kept + 1 ? eos : pad;
}

}  // namespace tok
