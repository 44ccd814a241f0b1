// 256-row LDS-DMA GEMM kernels, operand layout: A^T.B^T (bf16 only; not used by the training engine).  See mv_gemm_ring.h.
#include "mv_gemm_ring.h"

int mv_launch_ring_tnn(const GemmArgs& p, bool f16, const MvGemmPlan& plan, hipStream_t stream) {
  switch (plan.kernel) {
    case MV_GEMM_RING14: return f16 ? MV_E_ARG : mv_launch_ring_as<MV_GEMM_RING14, true, false, false>(p, plan, stream);
    case MV_GEMM_PRING: return f16 ? MV_E_ARG : mv_launch_ring_as<MV_GEMM_PRING, true, false, false>(p, plan, stream);
    default: return MV_E_ARG;
  }
}
