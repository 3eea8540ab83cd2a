// lm_gemm_swiglu.hip — wgemm instantiations for the EPI_SWIGLU epilogue (see lm_gemm_kernel.h).
#include "lm_gemm_kernel.h"

namespace tts {

void launch_wgemm_swiglu(const WgemmArgs& a, const WgemmPlan& p, bool norm, hipStream_t s) {
  if (!p.a_lds) launch_cfg<2, A_GLOBAL, false, EPI_SWIGLU>(a, p.cfg, p.grid, s);
  else if (norm) launch_cfg<2, A_LDS, true, EPI_SWIGLU>(a, p.cfg, p.grid, s);
  else launch_cfg<2, A_LDS, false, EPI_SWIGLU>(a, p.cfg, p.grid, s);
}

// The fused launch's warm role as a launch of its own (scripts/warm_probe.py: what the gate/up
// launch behind it gains from the lines in L2, with nothing else running): warm.wgs workgroups of
// 16 waves, as the fused launch's
__global__ __launch_bounds__(DEC_NW * 64) void warm_probe_kernel(WgemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  warm_role(a, smem, (int)blockIdx.x);
}
void launch_warm_probe(const WarmArgs& warm, hipStream_t s) {
  if (warm.wgs <= 0) return;
  if (!warm.w || warm.stages <= 0 || warm.nblk <= 0) throw std::runtime_error("warm probe: empty plan");
  WgemmArgs a;
  a.warm = warm;
  hipLaunchKernelGGL(warm_probe_kernel, dim3(warm.wgs), dim3(DEC_NW * 64), 1024, s, a);
}

}  // namespace tts
