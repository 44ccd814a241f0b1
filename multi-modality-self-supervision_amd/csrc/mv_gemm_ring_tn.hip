// 256-row LDS-DMA GEMM kernels, operand layout: dW = dy^T.x (both operands contraction-major).  See mv_gemm_ring.h.
#include "mv_gemm_ring.h"

int mv_launch_ring_tn(const GemmArgs& p, bool f16, const MvGemmPlan& plan, hipStream_t stream) {
  switch (plan.kernel) {
    case MV_GEMM_RING14: return f16 ? mv_launch_ring_as<MV_GEMM_RING14, true, true, true>(p, plan, stream) : mv_launch_ring_as<MV_GEMM_RING14, true, true, false>(p, plan, stream);
    case MV_GEMM_RING256x128: return f16 ? mv_launch_ring_as<MV_GEMM_RING256x128, true, true, true>(p, plan, stream) : MV_E_ARG;
    case MV_GEMM_PRING: return f16 ? mv_launch_ring_as<MV_GEMM_PRING, true, true, true>(p, plan, stream) : mv_launch_ring_as<MV_GEMM_PRING, true, true, false>(p, plan, stream);
    default: return MV_E_ARG;
  }
}

// folds the slabs of the tail tiles of a grouped launch into C: block (tail tile, 16-row band), one 16-byte column group per thread
__global__ __launch_bounds__(256) void splitk_reduce_grouped_kernel(GroupArgs ga) {
  const MvGroupHeader h = group_header(ga.table);
  const group_tab_t tab = (group_tab_t)((uintptr_t)ga.table + sizeof(MvGroupHeader));
  const int tile = h.direct + blockIdx.x;
  const group_tab_t e = tab + mv_group_find(tab, h.count, tile);
  int m0, n0;
  mv_group_raster(tile - e->unit0, e->M, e->N, m0, n0);
  const int M = e->M, N = e->N, ldc = e->ldc;
  float* C = (float*)e->C;
  const int nsl = (e->K + e->kchunk - 1) / e->kchunk;        // slices past the contraction hold zeros: skip them
  const float* slab = ga.ws + (size_t)blockIdx.x * h.split * (MV_GROUP_TILE * MV_GROUP_TILE);
  const float al = ga.alpha ? *ga.alpha : 1.0f;
  const bool vec = ((ldc & 3) == 0) && ((((uintptr_t)C) & 15) == 0) && ((N & 3) == 0);
  const int c = (threadIdx.x & 63) * 4, n = n0 + c;
  for (int r = blockIdx.y * 16 + (threadIdx.x >> 6); r < blockIdx.y * 16 + 16; r += 4) {
    const int m = m0 + r;
    if (m >= M || n >= N) continue;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < nsl; ++k) s += *(const f32x4*)(slab + ((size_t)k * MV_GROUP_TILE + r) * MV_GROUP_TILE + c);
    s *= al;
    float* dst = C + (size_t)m * ldc + n;
    if (vec) {
      if (ga.accumulate) s += *(const f32x4*)dst;
      *(f32x4*)dst = s;
    } else {
      for (int j = 0; j < 4 && n + j < N; ++j) dst[j] = ga.accumulate ? dst[j] + s[j] : s[j];
    }
  }
}

// the grouped launch: `h` is the (validated) host copy of the table's header -- it decides the grid; the kernels read the device copy
int mv_launch_ring_tn_grouped(const MvGroupHeader& h, const GroupArgs& ga, bool f16, int n_blk, hipStream_t stream) {
  constexpr int shm = mv_ring_lds_bytes(MV_GEMM_PRING);
  const int units = h.direct + h.tail * h.split;
  const dim3 grid(units < n_blk ? units : n_blk), block(512);
  if (f16) mv_launch_lds<gemm_pring_grouped_kernel<4, 4, 2, true>>(grid, block, shm, stream, ga, units);
  else mv_launch_lds<gemm_pring_grouped_kernel<4, 4, 2, false>>(grid, block, shm, stream, ga, units);
  MV_CHECK_LAUNCH();
  if (h.tail > 0) {
    hipLaunchKernelGGL(splitk_reduce_grouped_kernel, dim3(h.tail, MV_GROUP_TILE / 16), dim3(256), 0, stream, ga);
    MV_CHECK_LAUNCH();
  }
  return MV_OK;
}
