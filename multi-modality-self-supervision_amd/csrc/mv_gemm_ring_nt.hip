// 256-row LDS-DMA GEMM kernels, operand layout: y = x.W^T (both operands k-contiguous).  See mv_gemm_ring.h.
#include "mv_gemm_ring.h"

int mv_launch_ring_nt(const GemmArgs& p, bool f16, const MvGemmPlan& plan, hipStream_t stream) {
  switch (plan.kernel) {
    case MV_GEMM_RING14: return f16 ? mv_launch_ring_as<MV_GEMM_RING14, false, false, true>(p, plan, stream) : mv_launch_ring_as<MV_GEMM_RING14, false, false, false>(p, plan, stream);
    case MV_GEMM_RING320: return f16 ? mv_launch_ring_as<MV_GEMM_RING320, false, false, true>(p, plan, stream) : mv_launch_ring_as<MV_GEMM_RING320, false, false, false>(p, plan, stream);
    case MV_GEMM_RING256x128: return f16 ? mv_launch_ring_as<MV_GEMM_RING256x128, false, false, true>(p, plan, stream) : MV_E_ARG;
    case MV_GEMM_PRING: return f16 ? MV_E_ARG : mv_launch_ring_as<MV_GEMM_PRING, false, false, false>(p, plan, stream);
    default: return MV_E_ARG;
  }
}
