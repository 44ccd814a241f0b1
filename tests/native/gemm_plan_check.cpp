// Stand-alone driver of mv_gemm's launch plan (csrc/mv_gemm_plan.h).  Reads calls from stdin, one per line of 25 integers
//   dtype ta tb M N K splitk ws_bytes has_ws epi c_dtype accumulate has_c3 has_colsum vec8_ok r8_ok has_alpha drop_on operands_ok
//   impl gemm_force gemm_nj gemm_rounds persistent_cus n_cu
// and prints the plan of each, one line of 17 integers
//   rc kernel variant rule tiles sk_auto splitk kchunk grid_x grid_y grid_z block lds_bytes units blocks reduce ring_lds_ok
// (ring_lds_ok: the LDS bytes of a ring kernel are stages x the stage size of the shape the launch units instantiate).  A malformed
// line is an error.  Plain C++17, for the host compiler alone and for the host sanitizers (tests/test_gemm_plan_cpu.py runs it):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/gemm_plan_check.cpp -o gemm_plan_check
//   ./gemm_plan_check < calls.txt
#include <cstdio>
#include <cstdlib>
#include "../../multi-modality-self-supervision_amd/csrc/mv_gemm_plan.h"

int main() {
  long long v[25];
  long lines = 0;
  for (;;) {
    int got = 0;
    while (got < 25 && std::scanf("%lld", &v[got]) == 1) ++got;
    if (got == 0) break;
    if (got != 25) { std::fprintf(stderr, "call %ld: %d of 25 integers\n", lines, got); return 1; }
    MvGemmCall c = {};
    c.dtype = (int)v[0]; c.ta = (int)v[1]; c.tb = (int)v[2]; c.M = (int)v[3]; c.N = (int)v[4]; c.K = (int)v[5]; c.splitk = (int)v[6];
    c.ws_bytes = (size_t)v[7]; c.has_ws = (int)v[8]; c.epi = (int)v[9]; c.c_dtype = (int)v[10]; c.accumulate = (int)v[11]; c.has_c3 = (int)v[12];
    c.has_colsum = (int)v[13]; c.vec8_ok = (int)v[14]; c.r8_ok = (int)v[15]; c.has_alpha = (int)v[16]; c.drop_on = (int)v[17]; c.operands_ok = (int)v[18];
    const MvGemmKnobs kn = {(int)v[19], (int)v[20], (int)v[21], (int)v[22], (int)v[23]};
    const MvGemmPlan p = mv_gemm_plan(c, kn, (int)v[24]);
    const bool ring = p.kernel >= MV_GEMM_RING14 && p.kernel < MV_GEMM_KERNELS;
    const MvRingShape s = mv_ring_shape(p.kernel);
    const int lds_ok = p.rc != MV_OK || !ring || (p.lds_bytes == s.nstage * mv_ring_stage_bytes(s) && p.block == 128 * s.wn);
    std::printf("%d %d %d %d %lld %lld %d %d %u %u %u %d %d %d %d %d %d\n", p.rc, p.kernel, p.variant, p.rule, p.tiles, p.sk_auto, p.splitk, p.kchunk,
                p.grid_x, p.grid_y, p.grid_z, p.block, p.lds_bytes, p.units, p.blocks, p.reduce, lds_ok);
    ++lines;
  }
  return 0;
}
