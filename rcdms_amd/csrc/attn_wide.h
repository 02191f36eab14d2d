// attn_wide.h — hand-over between the dispatcher in attn.hip and the wide-head flash kernel in attn_wide.hip.
#pragma once
#include "common.h"

struct AttnWideArgs {
  const f16* Q;
  const f16* K;
  const f16* V;
  f16* O;
  int batch, heads, Lq, Lk, d;
  int ldq, ldk, ldv, ldo;
  float c;          // scale * log2(e)
  int plain_order;  // RCDM_ATTN_XCD=0: blocks in plain (query block fastest) order
};

// unmasked flash attention for 160 < d <= 512, d % 64 == 0 (the caller has checked the shape and the 32-bit K/V offset range)
int rcdm_attn_wide_launch(const AttnWideArgs& a, hipStream_t stream);
