// lm_logit_epilogue.h — the lm_head's pick epilogue on one finished fp32 sum, shared by the
// decode head (wgemm_kernel, EPI_LOGITS / EPI_LOGITS_ROWS) and the tile head (head_tile_kernel,
// lm_pgemm.hip), so both process a logit with the same arithmetic in the same order.
#pragma once
#include "hip_common.h"
#include "lm_kernels.h"

namespace tts {

// Better (value, index): larger value wins, lower index on ties (torch.argmax semantics).
TTS_DEV void argmax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// Logit (row m, column n) from its fp32 sum: bf16 rounding, repetition penalty where the row's
// `seen` word `bits` (the word of column n) has the column's bit, frequency penalty from the
// counts, the EOS mask (eos = the row's masked id or -1), the optional fp32 store.  ROWS: the
// penalties of row m from a.row_par[m] (counts always set) instead of the launch's.
// Args: WgemmArgs or HeadTileArgs (the same field names).
template <bool ROWS, class Args>
TTS_DEV float logit_epilogue(const Args& a, float sum, uint32_t bits, int m, int n, int eos) {
  float v = rbf(sum);  // logits are materialised in bf16, then .float()
  if constexpr (ROWS) {
    // the row's own penalties (one 8-byte load beside the counts'); freq 0 subtracts an exact zero
    const float2 pf = *(const float2*)(a.row_par + m);
    if ((bits >> (n & 31)) & 1u) v = (v < 0.f) ? v * pf.x : v / pf.x;
    v -= pf.y * (float)a.counts[(size_t)m * a.seen_stride * 32 + n];
  } else {
    if ((bits >> (n & 31)) & 1u) v = (v < 0.f) ? v * a.penalty : v / a.penalty;
    if (a.counts) v -= a.freq_penalty * (float)a.counts[(size_t)m * a.seen_stride * 32 + n];
  }
  if (n == eos) v = -INFINITY;
  if (a.logits_out) a.logits_out[(size_t)m * a.ldl + n] = v;
  return v;
}

}  // namespace tts
