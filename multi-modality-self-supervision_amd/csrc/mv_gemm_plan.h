// The launch plan of mv_gemm: which kernel a call runs, with how many split-K slabs, which kchunk, which grid and how much LDS -- or
// which MV_E_* it is refused with.  ONE pure function, mv_gemm_plan(); plain C++17 host code like mv_gemm_group.h: no HIP, no knob or
// device query of its own (the caller passes the knob values and the CU count), so that mv_gemm (mv_gemm.hip), the workspace sizing
// (mv_gemm_workspace_bytes / mv_workspace_bytes), a CPU test (tests/test_gemm_plan_cpu.py) and the stand-alone program
// tests/native/gemm_plan_check.cpp all run the same code.  DESIGN.md, "The GEMM launch plan", has the tables.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/medvill.h"

// ---- tile shapes ---------------------------------------------------------------------------------------------------------------
constexpr int T128 = 128, T128_BK = 64;        // the 128x128 kernel (GT_BM / GT_BN / GT_BK of mv_gemm.hip)
constexpr int RING_ROWS = 256, RING_COLS = 256, RING_BK = 64;    // the ring kernels: 256-row tiles, slabs in multiples of a 64-deep stage
constexpr int RING_320_ROWS = 320;             // the 320 x 256 form (y = x.W^T and dx = dy.W)
constexpr int RING_V128_COLS = 128;            // the 256 x 128 form (f16 operands of y = x.W^T and dW = dy^T.x)
constexpr int VALU_TILE = 64, VALU_BK = 16;    // the plain VALU kernel
constexpr int VALU_MAX_GRID_Y = 65535;

// ---- big (a 256-row ring kernel) or small (the 128x128 kernel) -------------------------------------------------------------------
// measured on the model's shapes (profiles/r01_gemm_variants.txt): the ring kernels win for y = x.W^T with wide outputs and for
// dW = dy^T.x, the 128x128 register-staged kernel for dx = dy.W and for 768-column outputs (three blocks per CU), also for long contractions
constexpr int BIG_MIN_M = 256, BIG_MIN_N = 128;
constexpr int BIG_MIN_T128 = 128;              // at least this many 256 x 128 tiles ...
constexpr int BIG_LONG_K = 4096;               // ... or a contraction this long that may be split
constexpr int WIDE_NT_MIN_N = 1024;            // y = x.W^T counts as wide from here

// ---- WHOLE ROUNDS of tiles (round 5) ---------------------------------------------------------------------------------------------
// y = x.W^T and dx = dy.W with narrow outputs (768 columns: attention output projection, FFN-down and the three input gradients of a
// layer) over ~25,500 packed rows are 300 tiles of 256 x 256 -- 1.17 rounds of the 256 CUs, the second one 44 tiles on an idle chip --
// and 1,200 tiles of 128 x 128 = 1.56 rounds of that kernel's 768 slots; as 320 x 256 tiles they are 240 tiles: ONE round with 94 % of
// the CUs busy.  That is wave quantisation, not kernel quality (a tile takes the same time whether 44 or 256 CUs are busy), so the tile
// shape is chosen per call by (whole rounds) x (time of one round of that kernel).
// Measured at 25,483 rows (profiles/r05_notes.txt): FFN-down 151 -> 112 us, da 156 -> 113, dx(qkv) 117 -> 87, Wo 50 -> 42, dctx 44 -> 34.
constexpr int ROUNDS_MIN_M = 2048, ROUNDS_MIN_N = 256, ROUNDS_MIN_K = 256;
// whole rounds x the measured time of one round (any K: the three kernels' rounds scale alike): 128 x 128 tiles on 3 slots per CU,
// 256 x 256 ring tiles on one per CU, 320 x 256 ring tiles (FFN-down shape, us).  A partly filled round costs a full one.
constexpr int ROUND_COST_128 = 75, ROUND_COST_256 = 85, ROUND_COST_320 = 112;
constexpr int ROUND_SLOTS_PER_CU_128 = 3;
// Wide y = x.W^T outputs run several rounds of tiles; the last one is partly empty.  320-row tiles when they take strictly less
// (rounds x rows): the fused QKV projection at 25,483 rows is 900 tiles of 256 rows = 4 rounds (3.52 full) or 720 of 320 = 3 rounds.
constexpr int WIDE_COST_256 = 8, WIDE_COST_320 = 10;

// ---- split-K wanted at splitk = 0 (sk_auto) ---------------------------------------------------------------------------------------
// enough slabs to give every slot a unit, each at least SK_DEPTH deep, at most SK_CAP_*; only for contractions of SK_MIN_K and more
constexpr int SLOTS_128 = 512, SLOTS_128_SK = 768;        // the 128x128 kernel splits below 512 tiles, towards 768 units
constexpr int SLOTS_RING = 256, SLOTS_RING_V128 = 512;    // the ring kernels: one unit per CU (two for the 256 x 128 form)
constexpr int SK_MIN_K = 2048, SK_DEPTH = 1024, SK_CAP_128 = 16, SK_CAP_RING = 32;

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
enum MvGemmKernel {
  MV_GEMM_VALU = 0,            // gemm_simple_kernel: any dtype, exact f32
  MV_GEMM_MFMA128 = 1,         // gemm_mfma_kernel, one LDS stage, three blocks per CU
  MV_GEMM_MFMA128_2STAGE = 2,  // its two-stage form (knob gemm_nj = 32, bf16 operands)
  MV_GEMM_RING14 = 3,          // gemm_ring_kernel 256 x 256, 64-deep stages x2
  MV_GEMM_PRING = 4,           // gemm_pring_kernel: the persistent form of RING14
  MV_GEMM_RING320 = 5,         // gemm_ring_kernel 320 x 256
  MV_GEMM_RING256x128 = 6,     // gemm_ring_kernel 256 x 128, 32-deep stages x3, two blocks per CU
  MV_GEMM_RING_TN4 = 7,        // gemm_ring_kernel 256 x 256, 32-deep stages x4 (dW = dy^T.x)
  MV_GEMM_KERNELS = 8
};
enum MvGemmRule { MV_RULE_PLAIN = 0, MV_RULE_ROUNDS256, MV_RULE_ROUNDS320, MV_RULE_ROUNDS_BACK_TO_128, MV_RULE_WIDE320, MV_RULE_WIDE256 };

// template parameters of a ring kernel's instantiation (mv_gemm_ring.h): waves 2 x wn, each 16 * mi rows x 16 * nj columns, a ring of
// nstage stages 32 * ks deep.  The ONE table the launch units instantiate from and the plan sizes LDS from.
struct MvRingShape { int nj, wn, nstage, ks, mi; };
constexpr MvRingShape mv_ring_shape(int kernel) {
  return kernel == MV_GEMM_RING320       ? MvRingShape{4, 4, 2, 2, 10}
         : kernel == MV_GEMM_RING256x128 ? MvRingShape{4, 2, 3, 1, 8}
         : kernel == MV_GEMM_RING_TN4    ? MvRingShape{4, 4, 4, 1, 8}
                                         : MvRingShape{4, 4, 2, 2, 8};      // MV_GEMM_RING14, MV_GEMM_PRING
}
// bytes of one ring stage: the A image (32 * mi rows) and the B image (16 KiB per 32 k when wider than 128 columns, else 8 KiB)
constexpr int mv_ring_stage_bytes(MvRingShape s) { return 32 * s.mi * 64 * s.ks + (s.wn * 16 * s.nj > 128 ? 16384 : 8192) * s.ks; }
constexpr int mv_ring_lds_bytes(int kernel) { return mv_ring_shape(kernel).nstage * mv_ring_stage_bytes(mv_ring_shape(kernel)); }
constexpr int MFMA128_STAGE_BYTES = 32768;     // A tile 16 KiB + B tile 16 KiB

// ---- the call, the knobs, the plan -----------------------------------------------------------------------------------------------
struct MvGemmKnobs { int impl, gemm_force, gemm_nj, gemm_rounds, persistent_cus; };      // mv_knob() values (mv_common.h)
struct MvGemmCall {            // mv_gemm's arguments without the pointers
  int dtype, ta, tb, M, N, K;
  int splitk;                  // as requested: < 0 and 1 none, 0 the library chooses, > 1 that many slabs
  size_t ws_bytes;
  int has_ws;
  int epi, c_dtype, accumulate, has_c3, has_colsum;
  int vec8_ok, r8_ok;          // the alignment facts the column-sum condition needs (GemmArgs)
  int has_alpha;               // alpha_dev given
  int drop_on;                 // the dropout mask is on (MV_EPI_BIAS_RES with p_drop > 0)
  int operands_ok;             // MFMA kernels: lda / ldb multiples of 8, A / B 16-byte aligned, both operands below 2 GiB
};
struct MvGemmPlan {
  int rc;                      // MV_OK or the refusal; the routing fields below (kernel .. sk_auto) are filled either way
  int kernel;                  // MvGemmKernel: what launches
  int variant;                 // the ring variant as routed (14, 24, 10, 2 or whatever gemm_nj forces); 0 off the ring kernels
  int rule;                    // MvGemmRule: which rule of the route decided
  long long tiles;             // output tiles of the chosen kernel
  long long sk_auto;           // slabs wanted at splitk = 0 with an unlimited workspace (1 = none)
  int splitk, kchunk;          // the slabs that run and their depth
  unsigned grid_x, grid_y, grid_z;
  int block, lds_bytes;
  int units, blocks;           // persistent form: (tile, slab) units and the blocks that walk them (= grid_x); else 0
  int reduce;                  // splitk_reduce_kernel follows
};

// persistent kernels: at most persistent_cus blocks when the host partitions the chip (mv_set_persistent_cus)
inline int mv_persistent_blocks(int persistent_cus, int n_cu) { return (persistent_cus > 0 && persistent_cus < n_cu) ? persistent_cus : n_cu; }

inline long long mv_plan_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline long long mv_plan_sk_auto(long long slots, long long tiles, int K, int cap) {
  long long sk = slots / tiles;
  if (sk > K / SK_DEPTH) sk = K / SK_DEPTH;
  if (sk > cap) sk = cap;
  return sk < 1 ? 1 : sk;
}

// The ring kernel a routed variant runs on a layout and operand encoding.  A variant that has no kernel there runs the plain ring:
// the persistent form (24) exists for bf16 operands and for f16 dW = dy^T.x, the 320-row form (10) for y = x.W^T and dx = dy.W, the
// 256 x 128 form (2) for f16 y = x.W^T and dW = dy^T.x, the four-stage form (4) for dW = dy^T.x.
inline int mv_plan_ring_kernel(int ta, int tb, bool f16, int variant) {
  const bool nt = !ta && !tb, nn = !ta && tb, tn = ta && tb;
  if (variant == 4 && tn) return MV_GEMM_RING_TN4;
  if (variant == 2 && f16 && (nt || tn)) return MV_GEMM_RING256x128;
  if (variant == 10 && (nt || nn)) return MV_GEMM_RING320;
  if (variant == 24 && (!f16 || tn)) return MV_GEMM_PRING;
  return MV_GEMM_RING14;
}

// ---- the three split-K rules: (requested splitk, sk_auto) -> the slab count the kchunk is cut for --------------------------------
// ring kernels: the library's own wish, never more than an explicit request, clamped to what fits the workspace
inline long long mv_plan_slabs_ring(const MvGemmCall& c, int splitk, long long sk_auto, bool plain_f32) {
  if (splitk == 1) return 1;
  long long sk = sk_auto;
  if (splitk > 1 && sk > splitk) sk = splitk;
  if (sk > 1 && c.has_ws) {
    const long long fit = (long long)(c.ws_bytes / ((size_t)c.M * c.N * sizeof(float)));
    if (sk > fit) sk = fit < 1 ? 1 : fit;
  }
  if (sk > 1 && (!c.has_ws || !plain_f32)) sk = 1;
  return sk;
}
// 128x128 kernel: an explicit request as it is; its own wish all or nothing
inline long long mv_plan_slabs_128(const MvGemmCall& c, int splitk, long long sk_auto, bool plain_f32) {
  if (splitk != 0) return splitk;
  if (sk_auto > 1 && c.has_ws && plain_f32 && c.ws_bytes >= (size_t)sk_auto * c.M * c.N * sizeof(float)) return sk_auto;
  return 1;
}
// VALU kernel: an explicit request only (splitk = 0 has become 1 before)
inline long long mv_plan_slabs_valu(int splitk) { return splitk; }

inline MvGemmPlan mv_gemm_plan(const MvGemmCall& c, const MvGemmKnobs& kn, int n_cu) {
  MvGemmPlan pl = {};
  pl.rc = MV_OK; pl.kernel = MV_GEMM_VALU; pl.rule = MV_RULE_PLAIN; pl.sk_auto = 1; pl.splitk = 1;
  auto refuse = [&](int rc) { pl.rc = rc; return pl; };
  if (c.M <= 0 || c.N <= 0 || c.K <= 0 || n_cu <= 0) return refuse(MV_E_ARG);
  const int ta = c.ta, tb = c.tb, M = c.M, N = c.N, K = c.K;
  const bool is16 = c.dtype == MV_BF16 || c.dtype == MV_F16, c16 = c.c_dtype == MV_BF16 || c.c_dtype == MV_F16;
  const bool mfma = is16 && kn.impl == 0, f16 = c.dtype == MV_F16;
  const bool plain_f32 = c.epi == MV_EPI_NONE && c.c_dtype == MV_F32;
  int splitk = c.splitk < 0 ? 1 : c.splitk;

  // ---- route: big or small, ring variant, tiles, sk_auto (MFMA kernels only) ----------------------------------------------------
  bool big = false;
  if (mfma) {
    const bool rows256 = c.has_colsum != 0;                         // fused column sums need 256-row tiles
    const long long tm2 = mv_plan_cdiv(M, RING_ROWS), tn2 = mv_plan_cdiv(N, RING_COLS);
    const long long t256 = tm2 * tn2, t256x128 = tm2 * mv_plan_cdiv(N, RING_V128_COLS), t320 = mv_plan_cdiv(M, RING_320_ROWS) * tn2;
    const long long s128 = mv_plan_cdiv(M, T128) * mv_plan_cdiv(N, T128);
    const bool wide_nt = !ta && !tb && N >= WIDE_NT_MIN_N;
    big = (kn.gemm_force == 2) || (kn.gemm_force == 0 && M >= BIG_MIN_M && N >= BIG_MIN_N && ((K & 7) == 0 || (ta && tb)) && (wide_nt || ta) &&
                                   (t256x128 >= BIG_MIN_T128 || (K >= BIG_LONG_K && splitk != 1)));
    const bool rounds_on = kn.gemm_rounds != 0 && kn.gemm_force == 0 && kn.gemm_nj == 0;
    bool routed = false;
    if (rounds_on && !ta && !big && splitk <= 1 && M >= ROUNDS_MIN_M && N >= ROUNDS_MIN_N && (N & 7) == 0 && (K & 7) == 0 && K >= ROUNDS_MIN_K) {
      const long long c128 = mv_plan_cdiv(s128, (long long)ROUND_SLOTS_PER_CU_128 * n_cu) * ROUND_COST_128, c256 = mv_plan_cdiv(t256, n_cu) * ROUND_COST_256,
                      c320 = rows256 ? (1ll << 60) : mv_plan_cdiv(t320, n_cu) * ROUND_COST_320;
      if (c256 < c128 && c256 <= c320) { big = routed = true; pl.variant = 14; pl.tiles = t256; pl.rule = MV_RULE_ROUNDS256; }
      else if (c320 < c128 && c320 < c256) { big = routed = true; pl.variant = 10; pl.tiles = t320; pl.rule = MV_RULE_ROUNDS320; }
      else pl.rule = MV_RULE_ROUNDS_BACK_TO_128;
    }
    if (!routed && rounds_on && big && !ta && !tb && !rows256 && splitk <= 1 && (K & 7) == 0) {
      if (mv_plan_cdiv(t320, n_cu) * WIDE_COST_320 < mv_plan_cdiv(t256, n_cu) * WIDE_COST_256) { routed = true; pl.variant = 10; pl.tiles = t320; pl.rule = MV_RULE_WIDE320; }
      else pl.rule = MV_RULE_WIDE256;
    }
    if (!routed && big) {
      // 256x256 with 64-deep stages (whole 128-B lines per LDS-DMA row): best measured.  Weight gradients (split-K units, f32 partial
      // tiles) gain 5-8 % from the persistent form; y = x.W^T does not (profiles/r01_gemm_variants.txt)
      int v = kn.gemm_nj ? kn.gemm_nj : (ta ? 24 : 14);
      if (v == 10 && ta) v = 24;                                   // the 320-row form exists for y = x.W^T and dx = dy.W
      if (v == 2 && !(f16 && ta == tb)) v = ta ? 24 : 14;          // the 256x128 form exists for f16 operands of y = x.W^T and dW = dy^T.x
      pl.variant = v;
      pl.tiles = v == 2 ? t256x128 : (v == 10 ? t320 : t256);
      const long long slots = v == 2 ? SLOTS_RING_V128 : SLOTS_RING;
      if (v != 10 && pl.tiles < slots && K >= SK_MIN_K) pl.sk_auto = mv_plan_sk_auto(slots, pl.tiles, K, SK_CAP_RING);
    } else if (!big) {
      pl.tiles = s128;
      if (pl.tiles < SLOTS_128 && K >= SK_MIN_K) pl.sk_auto = mv_plan_sk_auto(SLOTS_128_SK, pl.tiles, K, SK_CAP_128);
    }
    // what launches: every variant number is resolved to a kernel HERE (the launch units have no fall-back of their own)
    pl.kernel = big ? mv_plan_ring_kernel(ta, tb, f16, pl.variant) : ((kn.gemm_nj == 32 && !f16) ? MV_GEMM_MFMA128_2STAGE : MV_GEMM_MFMA128);
  }

  // ---- refusals, in mv_gemm's order -----------------------------------------------------------------------------------------------
  if ((splitk > 1 || c.accumulate) && (!plain_f32 || c.has_c3)) return refuse(MV_E_SHAPE);
  if (splitk > 1 && (!c.has_ws || c.ws_bytes < (size_t)splitk * M * N * sizeof(float))) return refuse(MV_E_WORKSPACE);
  if (c.has_alpha && (!plain_f32 || c.has_c3)) return refuse(MV_E_ARG);
  if (splitk == 0 && !mfma) splitk = 1;                            // auto split-K only on the MFMA kernels
  if (c.drop_on && (N & 3)) return refuse(MV_E_SHAPE);             // the mask is keyed on groups of 4 consecutive columns
  if (mfma && f16 && ta && !tb) return refuse(MV_E_DTYPE);         // f16 operands: y = x.W^T, dx = dy.W and dW = dy^T.x
  if (mfma && !c.operands_ok) return refuse(MV_E_SHAPE);

  // ---- slabs, kchunk, grid ----------------------------------------------------------------------------------------------------------
  const long long sk = !mfma ? mv_plan_slabs_valu(splitk)
                       : big ? mv_plan_slabs_ring(c, splitk, pl.sk_auto, plain_f32)
                             : mv_plan_slabs_128(c, splitk, pl.sk_auto, plain_f32);
  const int bk = !mfma ? VALU_BK : big ? RING_BK : T128_BK;
  pl.kchunk = (int)(mv_plan_cdiv(mv_plan_cdiv(K, sk), bk) * bk);
  pl.splitk = (K + pl.kchunk - 1) / pl.kchunk;
  pl.reduce = pl.splitk > 1;
  pl.grid_y = pl.grid_z = 1;
  if (!mfma) {
    if (c.has_colsum) return refuse(MV_E_SHAPE);
    pl.grid_x = (unsigned)((N + VALU_TILE - 1) / VALU_TILE); pl.grid_y = (unsigned)((M + VALU_TILE - 1) / VALU_TILE); pl.grid_z = (unsigned)pl.splitk;
    pl.tiles = (long long)pl.grid_x * pl.grid_y;
    pl.block = 256;
    if (pl.grid_y > (unsigned)VALU_MAX_GRID_Y) return refuse(MV_E_SHAPE);
  } else if (!big) {
    if (c.has_colsum) return refuse(MV_E_SHAPE);                   // the 256x256 ring kernel only
    pl.grid_x = (unsigned)pl.tiles; pl.grid_y = (unsigned)pl.splitk;
    pl.block = 256;
    pl.lds_bytes = (pl.kernel == MV_GEMM_MFMA128_2STAGE ? 2 : 1) * MFMA128_STAGE_BYTES;
  } else {
    // fused column sums: only the path that owns whole 64-column strips per wave and stores 16-byte pieces computes them.  (Keyed on
    // the variant NUMBER, not on the kernel: a forced variant that falls back to the plain ring is refused all the same -- DESIGN.md)
    if (c.has_colsum && !(pl.variant == 14 && pl.splitk == 1 && !c.accumulate && c.vec8_ok && (N & 255) == 0 && c16 &&
                          (c.epi == MV_EPI_NONE || c.epi == MV_EPI_BIAS || c.epi == MV_EPI_BIAS_GELU_D || ((c.epi == MV_EPI_MUL || c.epi == MV_EPI_RES) && c.r8_ok))))
      return refuse(MV_E_SHAPE);
    const MvRingShape s = mv_ring_shape(pl.kernel);
    pl.block = 128 * s.wn;
    pl.lds_bytes = mv_ring_lds_bytes(pl.kernel);
    if (pl.kernel == MV_GEMM_PRING) {
      pl.units = (int)pl.tiles * pl.splitk;
      const int n_blk = mv_persistent_blocks(kn.persistent_cus, n_cu);
      pl.blocks = pl.units < n_blk ? pl.units : n_blk;
      pl.grid_x = (unsigned)pl.blocks;
    } else {
      pl.grid_x = (unsigned)(int)pl.tiles; pl.grid_y = (unsigned)pl.splitk;
    }
  }
  return pl;
}
