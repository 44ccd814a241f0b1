// 256-row LDS-DMA GEMM kernels, operand layout dW = dy^T.x, with 32-deep stages x4 (three stages = 96 KiB in flight instead of one
// 64-KiB stage): the weight-gradient GEMMs stream both operands from HBM once (no reuse across K), so what bounds a K-step is the
// fetch latency that the ring can cover.  See mv_gemm_ring.h.
#include "mv_gemm_ring.h"

int mv_launch_ring_tn4(const GemmArgs& p, bool f16, const MvGemmPlan& plan, hipStream_t stream) {
  switch (plan.kernel) {
    case MV_GEMM_RING_TN4: return f16 ? mv_launch_ring_as<MV_GEMM_RING_TN4, true, true, true>(p, plan, stream) : mv_launch_ring_as<MV_GEMM_RING_TN4, true, true, false>(p, plan, stream);
    default: return MV_E_ARG;
  }
}
