// lm_gemm_logits.hip — wgemm instantiations for the EPI_LOGITS epilogue and its per-row form
// EPI_LOGITS_ROWS (see lm_gemm_kernel.h).
#include "lm_gemm_kernel.h"

namespace tts {

void launch_wgemm_logits(const WgemmArgs& a, const WgemmPlan& p, bool norm, hipStream_t s) {
  if (!p.a_lds) launch_cfg<1, A_GLOBAL, false, EPI_LOGITS>(a, p.cfg, p.grid, s);
  else if (norm) launch_cfg<1, A_LDS, true, EPI_LOGITS>(a, p.cfg, p.grid, s);
  else launch_cfg<1, A_LDS, false, EPI_LOGITS>(a, p.cfg, p.grid, s);
}

// the penalties of row m from a.row_par[m] (the per-request slot batch's captured step)
void launch_wgemm_logits_rows(const WgemmArgs& a, const WgemmPlan& p, bool norm, hipStream_t s) {
  if (!dry_launches() && (!a.row_par || !a.counts))
    throw std::runtime_error("wgemm: the per-row lm_head epilogue needs row_par and counts");
  if (!p.a_lds) launch_cfg<1, A_GLOBAL, false, EPI_LOGITS_ROWS>(a, p.cfg, p.grid, s);
  else if (norm) launch_cfg<1, A_LDS, true, EPI_LOGITS_ROWS>(a, p.cfg, p.grid, s);
  else launch_cfg<1, A_LDS, false, EPI_LOGITS_ROWS>(a, p.cfg, p.grid, s);
}

}  // namespace tts
