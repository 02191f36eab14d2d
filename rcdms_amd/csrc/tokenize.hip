// tokenize.hip — captions to CLIP token ids on the device (include/rcdm.h, "CLIP tokenizer").
//   rcdm_clip_tokenize   one launch, one 64-lane block (one wavefront) per caption.  The steps themselves are tokenize_core.h,
//                        shared with tools/tokenize_host.cpp; this file is their placement on the lanes:
//     load      the caption's bytes, the added-token rows and the two byte tables into LDS (a lane per byte / word)
//     specials  a position per lane: the longest special string starting there; lane 0 keeps the leftmost non-overlapping ones
//     added     a position per lane: the longest add_tokens row starting there, inside its stretch
//     scan      lane 0: resolve the matches, split into words, one symbol per byte.  Serial by nature (a regex scan whose
//               alternatives depend on where the last match ended) and short: a pass over LDS bytes
//     merge     all words of the caption advance together.  A round: every live symbol looks its pair up in the global hash
//               table and, if it has a merge, offers (rank << 10 | position) to an LDS minimum owned by its word (ds_min_u32 on
//               the slot of the word's first symbol: a minimum, so the result does not depend on the order of arrival) and
//               leaves the merged id beside it; then the lane that owns a word's first symbol applies the word's winner.  The number of rounds is the longest word's
//               merge count, not the caption's; a word may be longer than the wavefront (symbols are LDS entries, not lanes).
//     frame     ballot compaction of the live symbols, then a lane per output column: int64 ids and mask, row length, the
//               positions of the largest id and of the first eos by wave reductions.
// A wavefront per caption: a story's captions are ~100 bytes (two positions per lane), the rounds are latency-bound LDS /
// L2 round trips, and barriers inside one wave are free; a test set's 11 040 captions fill the 256 CUs with independent waves.
// LDS 26.4 KB per block.  Every global store is a plain C++ store to the caller's four outputs; nothing else is written.
#include "common.h"
#include "tokenize_core.h"

namespace {

constexpr int NT = 64;
constexpr int CAP = tok::MAX_CAPTION;
static_assert(sizeof(rcdm_tok_added) == sizeof(tok::Added) && sizeof(rcdm_tok_pair) == sizeof(tok::Pair), "rcdm.h and the core");
static_assert(RCDM_TOK_MAX_CAPTION == tok::MAX_CAPTION && RCDM_TOK_MAX_ROWS == tok::MAX_ROWS &&
              RCDM_TOK_MAX_ADDED_LEN == tok::MAX_ADDED_LEN && RCDM_TOK_MAX_RANK == 1 << tok::RANK_BITS, "rcdm.h and the core");

__global__ __launch_bounds__(NT) void tokenize_kernel(rcdm_tokenize_desc d, const uint8_t* __restrict__ text,
                                                      const int32_t* __restrict__ offsets, const int32_t* __restrict__ byte_ids,
                                                      const uint32_t* __restrict__ added, const tok::Pair* __restrict__ pairs,
                                                      int64_t* __restrict__ ids, int64_t* __restrict__ mask,
                                                      int32_t* __restrict__ lengths, int32_t* __restrict__ pool) {
  __shared__ uint8_t txt[CAP], mlen[CAP], mrow[CAP];
  __shared__ uint16_t lim[CAP], nxt[CAP], wst[CAP];
  __shared__ int32_t sym[CAP];
  __shared__ uint32_t best[CAP];                     // merge rounds: a word's least key, at its first symbol; then the tokens
  __shared__ uint32_t mrg[CAP];                      // merge rounds: what the pair at a symbol merges to
  __shared__ uint32_t rows_w[tok::MAX_ROWS * sizeof(tok::Added) / 4];
  __shared__ int32_t bytes[512];
  __shared__ int s_nsym;
  const int tid = threadIdx.x, r = blockIdx.x;
  const tok::Added* rows = (const tok::Added*)rows_w;
  const tok::Work w = {txt, lim, mlen, mrow, sym, nxt, wst};

  // ---- load: nothing outside text[0 .. text_bytes) is read, whatever the offsets say
  const int64_t o0 = offsets[r], o1 = offsets[r + 1];
  const bool bounds = o0 >= 0 && o1 >= o0 && o1 <= d.text_bytes && o1 - o0 <= CAP;
  int L = bounds ? (int)(o1 - o0) : 0;
  int high = 0;
  for (int i = tid; i < L; i += NT) {
    const uint8_t b = text[o0 + i];
    txt[i] = b;
    high |= b >> 7;
  }
  for (int i = tid; i < d.n_added * (int)(sizeof(tok::Added) / 4); i += NT) rows_w[i] = added[i];
  for (int i = tid; i < 512; i += NT) bytes[i] = byte_ids[i];
  for (int i = tid; i < CAP; i += NT) best[i] = tok::NONE;
  const int any_high = __syncthreads_or(high);
  const bool refused = !bounds || any_high;
  if (refused) L = 0;                                // block-uniform
  __syncthreads();

  // ---- steps 1-3
  for (int p = tid; p < L; p += NT) tok::special_at(w, p, L, rows, d.n_added);
  __syncthreads();
  if (tid == 0) tok::resolve_specials(w, L);
  __syncthreads();
  for (int p = tid; p < L; p += NT) tok::match_added(w, p, rows, d.n_added);
  __syncthreads();
  if (tid == 0) s_nsym = tok::scan(w, L, rows, bytes, bytes + 256);
  __syncthreads();
  const int n = s_nsym;

  // ---- step 4: at most n - 1 merges in all, so at most n rounds
  for (int round = 0; round < n; ++round) {
    for (int i = tid; i < n; i += NT) {
      uint32_t merged;
      const uint32_t key = tok::candidate(w, i, pairs, d.pair_slots, merged);
      if (key != tok::NONE) {
        mrg[i] = merged;
        atomicMin(&best[wst[i]], key);
      }
    }
    __syncthreads();
    int applied = 0;
    for (int i = tid; i < n; i += NT) {
      if (wst[i] != i || best[i] == tok::NONE) continue;          // a word's first symbol is never merged away
      const int at = (int)(best[i] & (CAP - 1));
      tok::apply_merge(w, at, mrg[at]);
      best[i] = tok::NONE;
      applied = 1;
    }
    if (!__syncthreads_or(applied)) break;
  }

  // ---- step 5
  int32_t* tokens = (int32_t*)best;
  int total = 0;
  for (int c = 0; c < n; c += NT) {
    const int i = c + tid;
    const bool live = i < n && sym[i] >= 0;
    const unsigned long long m = __ballot(live);
    if (live) tokens[total + __popcll(m & ((1ull << tid) - 1))] = sym[i];
    total += __popcll(m);
  }
  __syncthreads();
  const int kept = min(total, d.max_length - 2);
  int top = -1, top_at = 0x7FFFFFFF, eos_at = 0x7FFFFFFF;
  int64_t* idr = ids + (int64_t)r * d.ld;
  int64_t* mkr = mask + (int64_t)r * d.ld;
  for (int col = tid; col < d.max_length; col += NT) {            // ascending: the first of equal ids stays
    int mk;
    const int32_t v = tok::frame(col, kept, tokens, d.bos_id, d.eos_id, d.pad_id, mk);
    idr[col] = v;
    mkr[col] = mk;
    if (v > top) {
      top = v;
      top_at = col;
    }
    if (v == d.eos_id && col < eos_at) eos_at = col;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int v = __shfl_xor(top, o, 64), at = __shfl_xor(top_at, o, 64);
    if (v > top || (v == top && at < top_at)) {
      top = v;
      top_at = at;
    }
    eos_at = min(eos_at, __shfl_xor(eos_at, o, 64));
  }
  if (tid == 0) {
    lengths[r] = refused ? -1 : total + 2;
    pool[2 * r] = top_at;
    pool[2 * r + 1] = eos_at;
  }
}

}  // namespace

extern "C" {

uint32_t rcdm_tok_pair_hash(uint32_t a, uint32_t b) { return tok::pair_hash(a, b); }

static int tokenize_check(const rcdm_tokenize_desc* d) {
  if (d->n < 1 || d->max_length < 2 || d->ld < d->max_length || d->bos_id < 0 || d->eos_id < 0 || d->pad_id < 0 || d->n_added < 0 ||
      d->text_bytes < 0 || d->pair_slots < 2 || (d->pair_slots & (d->pair_slots - 1)))
    return RCDM_EINVAL;
  if (d->n > RCDM_TOK_MAX_CAPTIONS || d->max_length > RCDM_TOK_MAX_CAPTION + 2 || d->n_added > RCDM_TOK_MAX_ROWS ||
      d->text_bytes > 0x7FFFFFFFll || d->pair_slots > (1u << 26))
    return RCDM_ESHAPE;
  return RCDM_OK;
}

size_t rcdm_clip_tokenize_workspace_bytes(const rcdm_tokenize_desc* d) {
  (void)d;
  return 0;
}

int rcdm_clip_tokenize(const rcdm_tokenize_desc* d, const void* text, const int32_t* offsets, const int32_t* byte_ids,
                       const rcdm_tok_added* added, const rcdm_tok_pair* pairs, int64_t* input_ids, int64_t* attention_mask,
                       int32_t* lengths, int32_t* pool_index, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !text || !offsets || !byte_ids || !pairs || !input_ids || !attention_mask || !lengths || !pool_index) return RCDM_EINVAL;
  const int rc = tokenize_check(d);
  if (rc != RCDM_OK) return rc;
  if (d->n_added > 0 && !added) return RCDM_EINVAL;
  if ((((uintptr_t)input_ids | (uintptr_t)attention_mask) & 7) || ((uintptr_t)pairs & 15) ||
      (((uintptr_t)offsets | (uintptr_t)byte_ids | (uintptr_t)added | (uintptr_t)lengths | (uintptr_t)pool_index) & 3))
    return RCDM_EINVAL;
  const size_t need = rcdm_clip_tokenize_workspace_bytes(d);
  if (workspace_bytes < need || (need && !workspace)) return RCDM_EWORKSPACE;
  hipLaunchKernelGGL(tokenize_kernel, dim3(d->n), dim3(NT), 0, (hipStream_t)stream, *d, (const uint8_t*)text, offsets, byte_ids,
                     (const uint32_t*)added, (const tok::Pair*)pairs, input_ids, attention_mask, lengths, pool_index);
  return rcdm_check_launch();
}

}  // extern "C"
