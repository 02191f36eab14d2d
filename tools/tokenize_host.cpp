// The tokenizer's shared core (rcdms_amd/csrc/tokenize_core.h) on one CPU thread: the same functions in the same order as
// rcdm_clip_tokenize, with loops in place of the lanes and a plain minimum in place of the LDS one.  It is how the core meets
// every fixture before a GPU does, and it builds with sanitizers as it stands (host code with its own main):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I rcdms_amd/csrc tools/tokenize_host.cpp -o tokenize_host
//   tokenize_host call.bin
// call.bin is what rcdms_amd.tokenizer.ClipTokenizer.dump writes: 10 int32 (magic, n, max_length, truncation, bos, eos, pad,
// rows, slots, text bytes), offsets int32[n + 1], byte_ids int32[512], the added rows, the pair slots, the text, and optionally
// the expected input_ids int64[n][max_length].  Without them it prints one line per caption: length, largest-id position,
// first-eos position, the number of mask ones, then the ids.  With them it compares and prints `ok <n> rows` or the first row that differs (exit 1).
// Every per-caption array is allocated at the caption's exact size, so that a read or write one element outside it is seen.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tokenize_core.h"

namespace {

struct Call {
  int32_t n, max_length, truncation, bos, eos, pad, n_rows, text_bytes;
  uint32_t slots;
  std::vector<int32_t> offsets, byte_ids;
  std::vector<tok::Added> rows;
  std::vector<tok::Pair> pairs;
  std::vector<uint8_t> text;
  std::vector<int64_t> expect;
};

template <typename T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool load(const char* path, Call& c) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t h[10];
  bool ok = fread(h, 4, 10, f) == 10 && h[0] == 0x544F4B31;
  if (ok) {
    c.n = h[1], c.max_length = h[2], c.truncation = h[3], c.bos = h[4], c.eos = h[5], c.pad = h[6], c.n_rows = h[7];
    c.slots = (uint32_t)h[8], c.text_bytes = h[9];
    ok = c.n >= 1 && c.max_length >= 2 && c.n_rows >= 0 && c.n_rows <= tok::MAX_ROWS && c.slots >= 2 && !(c.slots & (c.slots - 1)) &&
         c.text_bytes >= 0;
  }
  ok = ok && read_vec(f, c.offsets, (size_t)c.n + 1) && read_vec(f, c.byte_ids, 512) && read_vec(f, c.rows, (size_t)c.n_rows) &&
       read_vec(f, c.pairs, c.slots) && read_vec(f, c.text, (size_t)c.text_bytes);
  if (ok && !read_vec(f, c.expect, (size_t)c.n * c.max_length)) c.expect.clear();
  fclose(f);
  return ok;
}

// one caption -> its row; returns the untruncated length, -1 for a caption the kernel refuses
int tokenize(const Call& c, int r, std::vector<int64_t>& ids, std::vector<int64_t>& mask, int& top_at, int& eos_at) {
  const int64_t o0 = c.offsets[r], o1 = c.offsets[r + 1];
  bool refused = !(o0 >= 0 && o1 >= o0 && o1 <= c.text_bytes && o1 - o0 <= tok::MAX_CAPTION);
  int L = refused ? 0 : (int)(o1 - o0);
  for (int i = 0; i < L; ++i) refused |= c.text[o0 + i] >= 0x80;
  if (refused) L = 0;
  std::vector<uint8_t> txt(c.text.begin() + (refused ? 0 : o0), c.text.begin() + (refused ? 0 : o0) + L), mlen(L), mrow(L);
  std::vector<uint16_t> lim(L), nxt(L), wst(L);
  std::vector<int32_t> sym(L), tokens;
  const tok::Work w = {txt.data(), lim.data(), mlen.data(), mrow.data(), sym.data(), nxt.data(), wst.data()};
  for (int p = 0; p < L; ++p) tok::special_at(w, p, L, c.rows.data(), c.n_rows);
  tok::resolve_specials(w, L);
  for (int p = 0; p < L; ++p) tok::match_added(w, p, c.rows.data(), c.n_rows);
  const int n = tok::scan(w, L, c.rows.data(), c.byte_ids.data(), c.byte_ids.data() + 256);
  std::vector<uint32_t> best(n, tok::NONE), mrg(n);
  for (int round = 0; round < n; ++round) {
    for (int i = 0; i < n; ++i) {
      uint32_t merged;
      const uint32_t key = tok::candidate(w, i, c.pairs.data(), c.slots, merged);
      if (key == tok::NONE) continue;
      mrg[i] = merged;
      if (key < best[wst[i]]) best[wst[i]] = key;
    }
    bool applied = false;
    for (int i = 0; i < n; ++i) {
      if (wst[i] != i || best[i] == tok::NONE) continue;
      const int at = (int)(best[i] & (tok::MAX_CAPTION - 1));
      tok::apply_merge(w, at, mrg[at]);
      best[i] = tok::NONE;
      applied = true;
    }
    if (!applied) break;
  }
  for (int i = 0; i < n; ++i)
    if (sym[i] >= 0) tokens.push_back(sym[i]);
  const int total = (int)tokens.size(), kept = total < c.max_length - 2 ? total : c.max_length - 2;
  tokens.resize(kept);                         // frame() reads tokens[0 .. kept) only
  ids.assign(c.max_length, 0);
  mask.assign(c.max_length, 0);
  int top = -1;
  top_at = eos_at = 0x7FFFFFFF;
  for (int col = 0; col < c.max_length; ++col) {
    int mk;
    const int32_t v = tok::frame(col, kept, tokens.data(), c.bos, c.eos, c.pad, mk);
    ids[col] = v;
    mask[col] = mk;
    if (v > top) top = v, top_at = col;
    if (v == c.eos && col < eos_at) eos_at = col;
  }
  return refused ? -1 : total + 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: tokenize_host call.bin\n");
    return 2;
  }
  Call c;
  if (!load(argv[1], c)) {
    fprintf(stderr, "%s: not a call written by ClipTokenizer.dump\n", argv[1]);
    return 2;
  }
  std::vector<int64_t> ids, mask;
  for (int r = 0; r < c.n; ++r) {
    int top_at, eos_at;
    const int len = tokenize(c, r, ids, mask, top_at, eos_at);
    if (c.expect.empty()) {
      int ones = 0;
      for (int col = 0; col < c.max_length; ++col) ones += (int)mask[col];
      printf("%d %d %d %d", len, top_at, eos_at, ones);
      for (int col = 0; col < c.max_length; ++col) printf(" %lld", (long long)ids[col]);
      printf("\n");
    } else if (memcmp(ids.data(), &c.expect[(size_t)r * c.max_length], sizeof(int64_t) * c.max_length)) {
      printf("row %d differs:\n  got ", r);
      for (int col = 0; col < c.max_length; ++col) printf(" %lld", (long long)ids[col]);
      printf("\n  want");
      for (int col = 0; col < c.max_length; ++col) printf(" %lld", (long long)c.expect[(size_t)r * c.max_length + col]);
      printf("\n");
      return 1;
    }
  }
  if (!c.expect.empty()) printf("ok %d rows\n", c.n);
  return 0;
}
