// scores.hip — figures from classifier logits on the device (include/rcdm.h, "Scores from logits"; csrc/scores_core.h has every
// rule and the order of every sum).
//   rcdm_label_counts      the integer state behind Char-F1 / Frm-Acc, added into in place.
//     label_count_kernel   a block owns sc::LABEL_ROWS rows, a lane one row per pass.  The class loop is uniform over the wave:
//                          each class costs three ballots, and lane c keeps the wave's tp / fp / fn of class c in registers.  A
//                          row's key t (C + 1) + e goes to LDS; thread t then scans the pass's keys and alone increments the
//                          LDS bins = t mod 256 (broadcast reads, no atomics).  The block's int32 state goes to the workspace.
//     label_fold_kernel    a thread per state element: the blocks' partials in ascending order, added into the state.
//   rcdm_inception_score   kl_out[split], three launches:
//     isc_row_kernel       a wave per position: m, log s and h of its row (lane-strided partial sums, the xor butterfly, which
//                          gives sc::wave_tree's bits in every lane: the two addends of a level only swap sides).
//     isc_chunk_kernel     a thread per class walks chunks of 256 positions in ascending order and recomputes p from (m, log s);
//                          reads are coalesced over the classes, the row's m / log s / order entry are wave-uniform.  One
//                          thread of the first class block adds the chunk's h.
//     isc_split_kernel     a block per split: chunk sums in ascending order per class, g(P / n_k), fr's fixed sum, KL.
// All row offsets are formed in int64.  No atomics; no scratch (profiles/scores_kernel_resources.txt).
#include "common.h"
#include "scores_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = sc::THREADS;
constexpr int NO_KEY = 0xFFFF;            // above every key: 64 * 65 + 64 = 4224
static_assert(sc::LABEL_ROWS % NT == 0 && NT == fr::LANES, "whole passes of one row per lane; the split launch uses fr's tree");

struct label_args {
  const void* logits;
  const uint8_t* labels;
  const float* thresholds;         // or null: 0.0
  int64_t ldz, ldl, n, len;
  int C;
  int32_t* partials;               // [blocks][len]
  int64_t* state;
  int64_t blocks;
};

template <typename T>
__global__ __launch_bounds__(NT) void label_count_kernel(const label_args a) {
  __shared__ int32_t hist[(sc::MAX_LABEL_CLASSES + 1) * (sc::MAX_LABEL_CLASSES + 1)];
  __shared__ int32_t cls[NT / 64][3][64];
  __shared__ uint16_t keys[NT];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int C = a.C, bins = (C + 1) * (C + 1);
  const int64_t row0 = (int64_t)blockIdx.x * sc::LABEL_ROWS;
  const int rows = (int)(a.n - row0 < sc::LABEL_ROWS ? a.n - row0 : sc::LABEL_ROWS);
  for (int i = tid; i < bins; i += NT) hist[i] = 0;
  int tp = 0, fp = 0, fn = 0;               // lane c: class c over this wave's rows
  __syncthreads();
  for (int base = 0; base < rows; base += NT) {          // the whole block
    const bool live = base + tid < rows;
    const int64_t r = live ? row0 + base + tid : row0;
    const T* __restrict__ z = (const T*)a.logits + r * a.ldz;
    const uint8_t* __restrict__ y = a.labels + r * a.ldl;
    int t = 0, e = 0;
    for (int c = 0; c < C; ++c) {
      const float thr = a.thresholds ? a.thresholds[c] : 0.0f;
      const bool p = live && sc::predicts((float)z[c], thr);
      const bool l = live && sc::present(y[c]);
      const int ntp = __popcll(__ballot(p && l)), nfp = __popcll(__ballot(p && !l)), nfn = __popcll(__ballot(!p && l));
      if (lane == c) {
        tp += ntp;
        fp += nfp;
        fn += nfn;
      }
      t += p && l;
      e += p != l;
    }
    keys[tid] = (uint16_t)(live ? t * (C + 1) + e : NO_KEY);
    __syncthreads();
    const int held = rows - base < NT ? rows - base : NT;
    for (int i = 0; i < held; ++i) {
      const int k = keys[i];
      if ((k & (NT - 1)) == tid) hist[k] += 1;           // this thread owns the bin: no other touches it
    }
    __syncthreads();
  }
  cls[wave][sc::TP][lane] = tp;
  cls[wave][sc::FP][lane] = fp;
  cls[wave][sc::FN][lane] = fn;
  __syncthreads();
  int32_t* out = a.partials + (int64_t)blockIdx.x * a.len;
  if (tid == 0) out[0] = rows;
  if (tid < C) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      int s = 0;
#pragma unroll
      for (int v = 0; v < NT / 64; ++v) s += cls[v][w][tid];
      out[sc::class_at(tid, w)] = s;
    }
  }
  for (int i = tid; i < bins; i += NT) out[sc::hist_at(C, 0, 0) + i] = hist[i];
}

__global__ __launch_bounds__(NT) void label_fold_kernel(const label_args a) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= a.len) return;
  int64_t s = 0;
  for (int64_t b = 0; b < a.blocks; ++b) s += a.partials[b * a.len + i];
  a.state[i] += s;
}

struct isc_args {
  const void* logits;
  const int32_t* order;            // or null
  int64_t ld, n;
  int C, splits, cpb;
  int64_t slots;                   // chunk slots per split
  double *m, *logs, *h;            // [n], by position
  double* partial;                 // [splits][slots][C]
  double* hpart;                   // [splits][slots]
  double* row_h;                   // or null
  double* kl;
};

__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int s = sc::WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

template <typename T>
__global__ __launch_bounds__(NT) void isc_row_kernel(const isc_args a) {
  const int lane = threadIdx.x & 63;
  const int64_t pos = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (pos >= a.n) return;                    // the whole wave
  const int64_t row = a.order ? (int64_t)a.order[pos] : pos;
  const T* __restrict__ z = (const T*)a.logits + row * a.ld;
  const int C = a.C;
  double m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmax(m, (double)z[c]);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) m = fmax(m, __shfl_xor(m, s, 64));
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += sc::exp_shifted((double)z[c], m);
  const double logs = log(wave_tree_sum(s));
  double h = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double lp = sc::log_prob((double)z[c], m, logs);
    h += sc::plogp(exp(lp), lp);
  }
  h = wave_tree_sum(h);
  if (lane == 0) {
    a.m[pos] = m;
    a.logs[pos] = logs;
    a.h[pos] = h;
    if (a.row_h) a.row_h[pos] = h;
  }
}

// grid (class blocks, chunk blocks, splits)
template <typename T>
__global__ __launch_bounds__(NT) void isc_chunk_kernel(const isc_args a) {
  const int k = blockIdx.z, c = blockIdx.x * NT + threadIdx.x;
  const int64_t b0 = sc::split_begin(a.n, a.splits, k), b1 = sc::split_begin(a.n, a.splits, k + 1);
  const int64_t cps = sc::chunks(b1 - b0);
  for (int jj = 0; jj < a.cpb; ++jj) {
    const int64_t j = (int64_t)blockIdx.y * a.cpb + jj;
    if (j >= cps) break;                     // the whole block
    const int64_t p0 = b0 + j * sc::CHUNK;
    const int cnt = (int)(b1 - p0 < sc::CHUNK ? b1 - p0 : sc::CHUNK);
    const int64_t slot = (int64_t)k * a.slots + j;
    if (c < a.C) {
      double P = 0.0;
      for (int i = 0; i < cnt; ++i) {
        const int64_t pos = p0 + i, row = a.order ? (int64_t)a.order[pos] : pos;
        P += sc::prob((double)((const T*)a.logits)[row * a.ld + c], a.m[pos], a.logs[pos]);
      }
      a.partial[slot * a.C + c] = P;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      double H = 0.0;
      for (int i = 0; i < cnt; ++i) H += a.h[p0 + i];
      a.hpart[slot] = H;
    }
  }
}

__global__ __launch_bounds__(fr::LANES) void isc_split_kernel(const isc_args a) {
  __shared__ double red[fr::LANES];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = sc::split_begin(a.n, a.splits, k), b1 = sc::split_begin(a.n, a.splits, k + 1);
  const int64_t cps = sc::chunks(b1 - b0);
  const double nk = (double)(b1 - b0);
  const double* part = a.partial + (int64_t)k * a.slots * a.C;
  double g = 0.0;
  for (int c = tid; c < a.C; c += fr::LANES) {
    double P = 0.0;
    for (int64_t j = 0; j < cps; ++j) P += part[j * a.C + c];
    g += sc::mean_term(P, nk);
  }
  red[tid] = g;
  __syncthreads();
  for (int h = fr::LANES / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    double H = 0.0;
    for (int64_t j = 0; j < cps; ++j) H += a.hpart[(int64_t)k * a.slots + j];
    a.kl[k] = sc::kl(H, red[0], nk);
  }
}

int label_check(const rcdm_label_desc* d) {
  if (d->n < 1 || d->classes < 1 || d->ld_logits < d->classes || d->ld_labels < d->classes || d->flags != 0) return RCDM_EINVAL;
  if (d->dtype != RCDM_FSTATS_F32 && d->dtype != RCDM_FSTATS_F16) return RCDM_EINVAL;
  if (d->classes > sc::MAX_LABEL_CLASSES || d->n > sc::MAX_N) return RCDM_ESHAPE;
  return RCDM_OK;
}

int isc_check(const rcdm_isc_desc* d) {
  if (d->n < 1 || d->classes < 1 || d->splits < 1 || d->splits > d->n || d->ld < d->classes || d->flags != 0) return RCDM_EINVAL;
  if (d->dtype != RCDM_FSTATS_F32 && d->dtype != RCDM_FSTATS_F16) return RCDM_EINVAL;
  if (d->chunks_per_block < 0 || d->chunks_per_block > sc::MAX_CHUNKS_PER_BLOCK) return RCDM_EINVAL;
  if (d->classes < sc::MIN_CLASSES || d->classes > sc::MAX_CLASSES || d->n > sc::MAX_N || d->splits > sc::MAX_SPLITS) return RCDM_ESHAPE;
  return RCDM_OK;
}

size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

int64_t rcdm_label_state_len(int32_t classes) {
  return classes < 1 || classes > sc::MAX_LABEL_CLASSES ? 0 : sc::label_state_len(classes);
}

size_t rcdm_label_counts_workspace_bytes(const rcdm_label_desc* d) {
  if (!d || label_check(d) != RCDM_OK) return 0;
  return round8((size_t)sc::label_blocks(d->n) * (size_t)sc::label_state_len(d->classes) * sizeof(int32_t));
}

int rcdm_label_counts(const rcdm_label_desc* d, const void* logits, const uint8_t* labels, const float* thresholds, int64_t* state,
                      void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !logits || !labels || !state) return RCDM_EINVAL;
  const int rc = label_check(d);
  if (rc != RCDM_OK) return rc;
  const uintptr_t esz = d->dtype == RCDM_FSTATS_F16 ? 2 : 4;
  if (((uintptr_t)logits & (esz - 1)) || ((uintptr_t)thresholds & 3) || ((uintptr_t)state & 7) || ((uintptr_t)workspace & 7))
    return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_label_counts_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  label_args a;
  a.logits = logits;
  a.labels = labels;
  a.thresholds = thresholds;
  a.ldz = d->ld_logits;
  a.ldl = d->ld_labels;
  a.n = d->n;
  a.C = d->classes;
  a.len = sc::label_state_len(d->classes);
  a.partials = (int32_t*)workspace;
  a.state = state;
  a.blocks = sc::label_blocks(d->n);
  const dim3 grid((unsigned)a.blocks), threads(NT);
  if (d->dtype == RCDM_FSTATS_F16) hipLaunchKernelGGL(label_count_kernel<f16>, grid, threads, 0, st, a);
  else hipLaunchKernelGGL(label_count_kernel<float>, grid, threads, 0, st, a);
  if (rcdm_check_launch() != RCDM_OK) return RCDM_ELAUNCH;
  hipLaunchKernelGGL(label_fold_kernel, dim3((unsigned)((a.len + NT - 1) / NT)), threads, 0, st, a);
  return rcdm_check_launch();
}

size_t rcdm_inception_score_workspace_bytes(const rcdm_isc_desc* d) {
  if (!d || isc_check(d) != RCDM_OK) return 0;
  const size_t slots = (size_t)sc::split_slots(d->n, d->splits);
  return (3 * (size_t)d->n + (size_t)d->splits * slots * ((size_t)d->classes + 1)) * sizeof(double);
}

int rcdm_inception_score(const rcdm_isc_desc* d, const void* logits, const int32_t* order, double* kl_out, double* row_h,
                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !logits || !kl_out) return RCDM_EINVAL;
  const int rc = isc_check(d);
  if (rc != RCDM_OK) return rc;
  const uintptr_t esz = d->dtype == RCDM_FSTATS_F16 ? 2 : 4;
  if (((uintptr_t)logits & (esz - 1)) || ((uintptr_t)order & 3) || ((uintptr_t)kl_out & 7) || ((uintptr_t)row_h & 7) ||
      ((uintptr_t)workspace & 7))
    return RCDM_EINVAL;
  if (!workspace || workspace_bytes < rcdm_inception_score_workspace_bytes(d)) return RCDM_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  isc_args a;
  a.logits = logits;
  a.order = order;
  a.ld = d->ld;
  a.n = d->n;
  a.C = d->classes;
  a.splits = d->splits;
  a.slots = sc::split_slots(d->n, d->splits);
  // the library's choice: one chunk per block; either way no more than 65535 chunk blocks
  const int fit = (int)((a.slots + 65534) / 65535);
  a.cpb = d->chunks_per_block > fit ? d->chunks_per_block : fit;
  double* w = (double*)workspace;
  a.m = w;
  a.logs = w + a.n;
  a.h = w + 2 * a.n;
  a.partial = w + 3 * a.n;
  a.hpart = a.partial + (int64_t)a.splits * a.slots * a.C;
  a.row_h = row_h;
  a.kl = kl_out;
  const bool half = d->dtype == RCDM_FSTATS_F16;
  const dim3 threads(NT), rows((unsigned)((a.n + NT / 64 - 1) / (NT / 64)));
  if (half) hipLaunchKernelGGL(isc_row_kernel<f16>, rows, threads, 0, st, a);
  else hipLaunchKernelGGL(isc_row_kernel<float>, rows, threads, 0, st, a);
  if (rcdm_check_launch() != RCDM_OK) return RCDM_ELAUNCH;
  const dim3 grid((unsigned)((a.C + NT - 1) / NT), (unsigned)((a.slots + a.cpb - 1) / a.cpb), (unsigned)a.splits);
  if (half) hipLaunchKernelGGL(isc_chunk_kernel<f16>, grid, threads, 0, st, a);
  else hipLaunchKernelGGL(isc_chunk_kernel<float>, grid, threads, 0, st, a);
  if (rcdm_check_launch() != RCDM_OK) return RCDM_ELAUNCH;
  hipLaunchKernelGGL(isc_split_kernel, dim3((unsigned)a.splits), dim3(fr::LANES), 0, st, a);
  return rcdm_check_launch();
}

}  // extern "C"
