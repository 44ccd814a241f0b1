// The three MFMA attention kernels (forward, dQ, dK/dV) and their launchers.
#include "mv_attn.h"

// =========================================================================================
// MFMA kernels (bf16, dh = 64)
// =========================================================================================
#if ATT_PROF
__device__ unsigned long long g_att_prof[3][8];
__device__ unsigned long long g_att_tile[3][8];       // inside the tile body (forward: 0 score MFMAs, 1 row maximum + shuffle, 2 exponentials + sums, 3 dropout selects, 4 P.V)
#endif
// Where a ring iteration requests the next tile: after its own tile body, not right after the barrier (a switch, ATT_ISSUE_LATE, chose
// between the two until the late form was kept).  Inside a tile body
// the compiler may wait for one of ITS memory operations -- a scratch reload of a spilled register (dK/dV kernel), the mask words
// of a mixed-class tile (fwd, dQ) -- with vmcnt(0); vmcnt retires in order, so that wait also waits for every LDS-DMA issued
// before it.  Issued late, the youngest transfer in flight at that point is a whole tile old instead of a few instructions.

// ---- forward --------------------------------------------------------------------------------
// One 64-key tile of the forward for a wave's 32 queries.  PLAIN: every entry of the tile is visible and inside the sample (class 1, no
// ragged tail): no mask words, no bounds, the scale folded into the exponent's fma.  DROP: attention dropout on.  Compile-time, so each
// variant is straight-line code (the run-time form merged its paths through 32 register copies per tile).
template <bool PLAIN, bool DROP, bool F16>
__device__ __forceinline__ void fwd_tile(const AttnArgs& a, unsigned tk, unsigned tv, const bf16x8 (&qf)[4], f32x16 (&o)[2], float& m2,
                                         float& lsum, const uint32_t* myw, bool q_ok, int k0, int Lv, int cls, float c2, int h,
                                         const unsigned long long* mp PROF_TILE_ARGS) {
  PROF_T0;
  // The 64 select masks of the tile (two scalar loads of 128 bytes per 32-key half) are requested where they are used.  A scalar-cache miss
  // costs a round trip to L2 / HBM (measured: 3,500 shader cycles per tile), and requesting them FIRST, so that the score MFMAs and the softmax
  // hide it, was tried (a switch, ATT_EARLY_MASKS: the first half's masks at the top of the tile, or both): it was slower, 90.8 -> 95.8-96.6 /
  // 92.0 us -- scalar loads share lgkmcnt with the LDS reads, so every fragment wait behind them waited for the mask round trip too
  // (profiles/r04_notes.txt).
  f32x16 st[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
    for (int i = 0; i < 16; ++i) st[kk][i] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) st[kk] = mma32<F16>(frag_row_x(tk, 32 * kk, s), qf[s], st[kk]);
  }
  PROF_T(0, st[1][15]);
  float mx = -INFINITY;
  if (PLAIN) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[kk][r]);
    mx *= c2;
  } else {
    const bool tail = (k0 + 64 > Lv);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      uint32_t w = 0xffffffffu;
      if (cls != 1) { const int wi = (k0 >> 5) + kk; w = (q_ok && wi < a.W) ? myw[wi] : 0xffffffffu; }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kr = acc_row(r, h);
        float v = st[kk][r] * c2;
        if (cls != 1) v += ((w >> kr) & 1u) ? 0.f : MASK_ADD * LOG2E;
        if (tail && (k0 + 32 * kk + kr >= Lv)) v = -INFINITY;
        st[kk][r] = v;
        mx = fmaxf(mx, v);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mn = fmaxf(m2, mx);
  PROF_T(1, mn);
  const float alpha = fexp2(m2 - mn);
  m2 = mn;
  f32x2 ps2 = {0.f, 0.f};            // two partial sums: v_pk_add_f32, half the add instructions
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const float p0 = PLAIN ? fexp2(fmaf(st[kk][r], c2, -mn)) : fexp2(st[kk][r] - mn);
      const float p1 = PLAIN ? fexp2(fmaf(st[kk][r + 1], c2, -mn)) : fexp2(st[kk][r + 1] - mn);
      st[kk][r] = p0;
      st[kk][r + 1] = p1;
      ps2 += (f32x2){p0, p1};
    }
  const float ps = ps2[0] + ps2[1];
  lsum = lsum * alpha + ps;          // the normaliser sums the UNdropped probabilities
  PROF_T(2, lsum);
  if (DROP) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u64x8 m0, m1;
      sload_masks16(mp + 16 * kk, m0, m1);
#pragma unroll
      for (int r = 0; r < 8; ++r) {       // `ps` was computed from these values by compiler-scheduled adds: see sel_lane_after
        st[kk][r] = sel_lane_after(st[kk][r], ps, m0[r]);
        st[kk][8 + r] = sel_lane_after(st[kk][8 + r], ps, m1[r]);
      }
    }
  }
  PROF_T(3, st[1][15]);
  // Unconditional: 16 packed multiplies.  Skipping them while the running maximum does not move (almost every tile) costs MORE -- the two
  // paths leave the accumulators in different registers and hipcc pays the merge with 32-64 register copies on the skipping path.
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 pf = pack8t<F16>(st[kk], s2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) o[dt] = mma32<F16>(frag_tr_x(tv, dt, 32 * kk + 16 * s2), pf, o[dt]);
    }
  PROF_T(4, o[1][15]);
}

#define FWD_NS 3      // 48 KiB of LDS per block: three blocks per CU
template <bool F16>
__global__ __launch_bounds__(256, 3) void attn_fwd_mfma_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(128))) char smem[];   // (fragment addressing XORs bits 4-6 of tile base + lane word: bases are multiples of 128)   // FWD_NS stages x (K 8 KiB + V 8 KiB)
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, head, b;
  PROF_DECL;
  att_block(a, xb, head, b);
  const int L = a.L, H = a.H, ld = 3 * a.H, T = a.T;
  const int qb0 = xb * 128, q0 = qb0 + wid * 32, q = q0 + l31;
  // The tile classes depend on the block index alone: requested BEFORE the row plan (cu, qlim), not behind it -- a block's prologue is a chain
  // of dependent memory round trips (arguments -> row plan -> Q rows / tile classes -> first K / V tiles: 12,600 shader cycles, a fifth of
  // the block's life, profiles/r04_notes.txt), this takes one link out
  const TileMasks tmk = load_tile_masks<false>(a.info, b, T, qb0 >> 6, min(q0 >> 6, T - 1), lane);
  const int Lv = row_count(a, b);             // positions of this sample that exist as rows
  const int Lq = query_count(a, b, Lv);             // ... and those that are queries
  if (qb0 >= Lq) return;
  const bool wave_on = q0 < Lq, q_ok = q < Lq;
  const size_t rowbase = row_base(a, b);
  const size_t lrow = (size_t)b * L;                            // logical row base (mask words)
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.qkv, 0, a.bytes_qkv, 0x00020000);
  const dma_rsrc_t rsq = dma_rsrc(a.qkv, a.bytes_qkv);

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = load_rowfrag_global(rs, a.bytes_qkv, rowbase + q, q_ok, ld, head * 64 + 16 * s + 8 * h);

  const float c2 = a.scale * LOG2E;
  float m2 = -INFINITY, lsum = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }

  const int nkt = (Lv + 63) / 64;
  // K/V ring: the needed key tiles (set bits of tmk.need) are requested FWD_NS - 1 ahead of the one being computed on
  int cur = next_tile(tmk.need, -1, nkt);
  int iss = cur, issued = 0, done = 0;
  auto issue = [&]() {
    char* st_ = smem + (issued % FWD_NS) * 16384;
    tile_dma<4>(rsq, a.bytes_qkv, rowbase, iss * 64, Lv, ld, H + head * 64, st_, wid, lane);
    tile_dma<4>(rsq, a.bytes_qkv, rowbase, iss * 64, Lv, ld, 2 * H + head * 64, st_ + 8192, wid, lane);
    ++issued;
    iss = next_tile(tmk.need, iss, nkt);
  };
#pragma unroll
  for (int i = 0; i < FWD_NS - 1; ++i)
    if (iss < nkt) issue();
  const uint32_t* myw = a.bits + (lrow + (q_ok ? q : 0)) * a.W;
  const FragLane fl = frag_lane(lane);            // two registers held across the loop: the lane's part of every fragment address
  const unsigned smem_a = lds_addr(smem);
  PROF_MARK(0);
  while (cur < nkt) {
    att_wait_stage<4>(issued - done - 1);           // this wave's pieces of tile `cur` have landed ...
    PROF_MARK(1);
    __builtin_amdgcn_s_barrier();                   // ... and everybody's; everybody is done reading the slot refilled next
    PROF_MARK(2);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned tKa = smem_a + (unsigned)(done % FWD_NS) * 16384u;
    const int cls = !wave_on ? 0 : (((tmk.w_is1 >> cur) & 1) ? 1 : (((tmk.w_nz >> cur) & 1) ? 2 : 0));
    if (wave_on && cls != 0) {
      const int k0 = cur * 64;
      // (the two lane words are made opaque per tile: hipcc otherwise hoists every derived address out of the loop and spills them)
      unsigned rk_ = fl.rk, tr_ = fl.tr;
      int h_ = h;                   // (also the half-wave index: the masked variants' 32 per-register bit masks derive from it)
      asm volatile("" : "+v"(rk_), "+v"(tr_), "+v"(h_));
      const unsigned tk = tKa + rk_, tv = tKa + 8192u + tr_;
      const bool plain = (cls == 1) && (k0 + 64 <= Lv);
      const unsigned long long* mp = a.drop_on ? (const unsigned long long*)a.dropbits + dbits_block(a, (size_t)b * a.A + head, q0 >> 5, cur) : nullptr;
#define FWD_CALL(P_, D_) fwd_tile<P_, D_, F16>(a, tk, tv, qf, o, m2, lsum, myw, q_ok, k0, Lv, cls, c2, h_, mp PROF_TILE_PASS)
      switch ((plain ? 0 : 1) | (a.drop_on ? 2 : 0)) {       // one wave-uniform dispatch per tile
        case 0: FWD_CALL(true, false); break;
        case 1: FWD_CALL(false, false); break;
        case 2: FWD_CALL(true, true); break;
        default: FWD_CALL(false, true); break;
      }
#undef FWD_CALL
    }
#if ATT_PROF
    asm volatile("s_nop 0" ::"v"(o[0][0]), "v"(o[1][15]));      // the tile's last MFMAs have delivered
#endif
    PROF_MARK(3);
    if (iss < nkt) issue();
    cur = next_tile(tmk.need, cur, nkt);
    ++done;
    PROF_MARK(4);
  }
  // epilogue: whole rows through a per-wave LDS patch (every wave is past its last tile: the K / V stages are free)
  __builtin_amdgcn_s_barrier();
  const float ltot = lsum + __shfl_xor(lsum, 32, 64);
  const float inv = (a.drop_on ? a.inv_keep : 1.0f) / ltot;
  const int rows_ok = Lq - q0;                      // (<= 0 for a wave without queries: nothing is stored)
  char* patch = smem + wid * ATT_PATCH_BYTES;
  store_rows_tile<F16>(patch, o, inv, q_ok, a.out + (rowbase + q0) * (size_t)H + head * 64, (size_t)H, rows_ok, lane);
  if constexpr (F16) {
    if (a.out2) store_rows_tile<false>(patch, o, inv, q_ok, a.out2 + (rowbase + q0) * (size_t)H + head * 64, (size_t)H, rows_ok, lane);
  }
  if (q_ok && h == 0) a.lse[((size_t)b * a.A + head) * L + q] = (m2 + log2f(ltot)) * LN2;
#if ATT_PROF
  asm volatile("s_waitcnt vmcnt(0)");
#endif
  PROF_MARK(5);
  PROF_FLUSH(0);
}

// ---- backward: dQ ----------------------------------------------------------------------------
// One 64-key tile of the dQ pass for a wave's 32 queries.  MASKED: the tile needs its mask words (class 2; a ragged
// TAIL tile is always run as masked), DROP: attention dropout is on -- compile-time, so the per-element loops are
// straight-line code the scheduler can interleave with the MFMAs.
template <bool MASKED, bool DROP, bool TAIL, bool F16>
__device__ __forceinline__ void dq_tile(const AttnArgs& a, unsigned tk, unsigned tv, unsigned tkt, const bf16x8 (&qf)[4], const bf16x8 (&dof)[4],
                                        f32x16 (&dq)[2], const uint32_t* myw, bool q_ok, int q, int b, int head, int k0, int Lv,
                                        float lse2, float dlt, float c2, int h, const unsigned long long* mp) {
  // tk / tv: row-read bases of the K / V tiles (lds address + FragLane::rk), tkt: transposed-read base of the K tile (+ FragLane::tr)
  const float dlt_s = dlt * a.scale;                          // ds = p * (dp' - delta) * scale, with the scale folded in
  const float dscale = DROP ? a.inv_keep * a.scale : a.scale;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    f32x16 st, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      st = mma32<F16>(frag_row_x(tk, 32 * kk, s), qf[s], st);
      dp = mma32<F16>(frag_row_x(tv, 32 * kk, s), dof[s], dp);
    }
    uint32_t w = 0xffffffffu;
    if (MASKED) { const int wi = (k0 >> 5) + kk; w = (q_ok && wi < a.W) ? myw[wi] : 0xffffffffu; }
    u64x8 m0, m1;
    if (DROP) sload_masks16(mp + 16 * kk, m0, m1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kr = acc_row(r, h);
      float pv;
      if (!MASKED) {
        pv = fexp2(fmaf(st[r], c2, -lse2));
      } else {
        const float v = fmaf(st[r], c2, ((w >> kr) & 1u) ? 0.f : MASK_ADD * LOG2E);
        pv = fexp2(v - lse2);
      }
      if (TAIL) pv = (k0 + 32 * kk + kr >= Lv) ? 0.f : pv;
      // ds = p * (keep ? dp * inv_keep * scale - delta * scale : -delta * scale): the select takes the fma's result, never dp[r]
      // itself (an MFMA result feeding an asm statement would not get its wait states)
      float t = fmaf(dp[r], dscale, -dlt_s);
      if (DROP) t = sel_set_else(t, -dlt_s, r < 8 ? m0[r & 7] : m1[r & 7]);
      st[r] = pv * t;
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 dsf = pack8t<F16>(st, s2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        dq[dt] = mma32<F16>(frag_tr_x(tkt, dt, 32 * kk + 16 * s2), dsf, dq[dt]);
    }
  }
}

#define DQ_NS 4       // 64 KiB of LDS per block, two blocks per CU (register-limited)
template <bool F16>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_mfma_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(128))) char smem[];   // (fragment addressing XORs bits 4-6 of tile base + lane word: bases are multiples of 128)
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, head, b;
  att_block(a, xb, head, b);
  const int L = a.L, H = a.H, ld = 3 * a.H, T = a.T;
  const int qb0 = xb * 128, q0 = qb0 + wid * 32, q = q0 + l31;
  PROF_DECL;
  const TileMasks tmk = load_tile_masks<false>(a.info, b, T, qb0 >> 6, min(q0 >> 6, T - 1), lane);      // before the row plan: see the forward
  const int Lv = row_count(a, b);
  const int Lq = query_count(a, b, Lv);
  if (qb0 >= Lv) return;
  const size_t rowbase = row_base(a, b);
  if (qb0 >= Lq) {        // rows that are keys only: their dQ is zero (thread t: row t / 2, 32 of the head's 64 columns)
    const int r = qb0 + (tid >> 1);
    if (r < Lv) {
      bf16_t* z = a.dqkv + (rowbase + r) * (size_t)ld + head * 64 + 32 * (tid & 1);
#pragma unroll
      for (int c = 0; c < 32; c += 4) store4_16<F16>(z + c, 0.f, 0.f, 0.f, 0.f);
    }
    return;
  }
  const bool wave_on = q0 < Lq, q_ok = q < Lq;
  const size_t lrow = (size_t)b * L;
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.qkv, 0, a.bytes_qkv, 0x00020000);
  const dma_rsrc_t rsq = dma_rsrc(a.qkv, a.bytes_qkv);
  __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dctx, 0, a.bytes_ctx, 0x00020000);

  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    qf[s] = load_rowfrag_global(rs, a.bytes_qkv, rowbase + q, q_ok, ld, head * 64 + 16 * s + 8 * h);
    dof[s] = load_rowfrag_global(rsd, a.bytes_ctx, rowbase + q, q_ok, H, head * 64 + 16 * s + 8 * h);
  }
  const size_t sidx = ((size_t)b * a.A + head) * L + (q_ok ? q : 0);
  const float lse2 = q_ok ? a.lse_in[sidx] * LOG2E : INFINITY;
  // delta[q] = sum_d dO[q,d] * O[q,d], computed here (each lane holds 32 of the 64 d of its query) and published for
  // the dK/dV kernel that runs next
  float dlt = 0.f;
  {
    __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)a.ctx, 0, a.bytes_ctx, 0x00020000);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 of = load_rowfrag_global(rsc, a.bytes_ctx, rowbase + q, q_ok, H, head * 64 + 16 * s + 8 * h);
#pragma unroll
      for (int j = 0; j < 8; ++j) dlt = fmaf(frag_elem<F16>(of, j), frag_elem<F16>(dof[s], j), dlt);
    }
    dlt += __shfl_xor(dlt, 32, 64);
    if (q_ok && h == 0) a.delta_out[sidx] = dlt;
  }
  const float c2 = a.scale * LOG2E;
  f32x16 dq[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dq[0][i] = 0.f; dq[1][i] = 0.f; }

  const int nkt = (Lv + 63) / 64;
  int cur = next_tile(tmk.need, -1, nkt);
  int iss = cur, issued = 0, done = 0;
  auto issue = [&]() {
    char* st_ = smem + (issued % DQ_NS) * 16384;
    tile_dma<4>(rsq, a.bytes_qkv, rowbase, iss * 64, Lv, ld, H + head * 64, st_, wid, lane);
    tile_dma<4>(rsq, a.bytes_qkv, rowbase, iss * 64, Lv, ld, 2 * H + head * 64, st_ + 8192, wid, lane);
    ++issued;
    iss = next_tile(tmk.need, iss, nkt);
  };
#pragma unroll
  for (int i = 0; i < DQ_NS - 1; ++i)
    if (iss < nkt) issue();
  const uint32_t* myw = a.bits + (lrow + (q_ok ? q : 0)) * a.W;
  const FragLane fl = frag_lane(lane);
  const unsigned smem_a = lds_addr(smem);
  PROF_MARK(0);
  while (cur < nkt) {
    att_wait_stage<4>(issued - done - 1);
    PROF_MARK(1);
    __builtin_amdgcn_s_barrier();
    PROF_MARK(2);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned tKa = smem_a + (unsigned)(done % DQ_NS) * 16384u;
    const int cls = !wave_on ? 0 : (((tmk.w_is1 >> cur) & 1) ? 1 : (((tmk.w_nz >> cur) & 1) ? 2 : 0));
    if (wave_on && cls != 0) {
      const int k0 = cur * 64;
      const bool tail = (k0 + 64 > Lv);
      // fragment addresses: the lane's two words (opaque per tile: nothing derived from them is hoisted and spilled) + the tile's address
      unsigned rk_ = fl.rk, tr_ = fl.tr;
      int h_ = h;
      asm volatile("" : "+v"(rk_), "+v"(tr_), "+v"(h_));
      const unsigned tk = tKa + rk_, tv = tKa + 8192u + rk_, tkt = tKa + tr_;
      // one wave-uniform dispatch per tile: the element loops below contain no branches
      const unsigned long long* mp = a.drop_on ? (const unsigned long long*)a.dropbits + dbits_block(a, (size_t)b * a.A + head, q0 >> 5, cur) : nullptr;
      const int variant = (cls == 1 ? 0 : 1) | (tail ? 2 : 0) | (a.drop_on ? 4 : 0);
#define DQ_CALL(M_, D_, T_) dq_tile<M_, D_, T_, F16>(a, tk, tv, tkt, qf, dof, dq, myw, q_ok, q, b, head, k0, Lv, lse2, dlt, c2, h_, mp)
      switch (variant) {
        case 0: DQ_CALL(false, false, false); break;
        case 1: DQ_CALL(true, false, false); break;
        case 2: case 3: DQ_CALL(true, false, true); break;
        case 4: DQ_CALL(false, true, false); break;
        case 5: DQ_CALL(true, true, false); break;
        default: DQ_CALL(true, true, true); break;
      }
#undef DQ_CALL
    }
#if ATT_PROF
    asm volatile("s_nop 0" ::"v"(dq[0][0]), "v"(dq[1][15]));
#endif
    PROF_MARK(3);
    if (iss < nkt) issue();
    cur = next_tile(tmk.need, cur, nkt);
    ++done;
    PROF_MARK(4);
  }
  // epilogue: whole rows through a per-wave LDS patch; a key-only row inside a query tile (a.qlim) gets a zero dQ row
  __builtin_amdgcn_s_barrier();
  store_rows_tile<F16>(smem + wid * ATT_PATCH_BYTES, dq, 1.0f, q_ok, a.dqkv + (rowbase + q0) * (size_t)ld + head * 64, (size_t)ld, Lv - q0,
                       lane);
#if ATT_PROF
  asm volatile("s_waitcnt vmcnt(0)");
#endif
  PROF_MARK(5);
  PROF_FLUSH(1);
}

// ---- backward: dK, dV --------------------------------------------------------------------------
// LDS stage layout: Q tile 8 KiB | dO tile 8 KiB | lse2[64] f32 | delta[64] f32 | words[64][4] u32
#define KV_STAGE (8192 + 8192 + 256 + 256 + 1024 + 1024)     // ... | keep-bit dwords [4 waves][2 query halves][32 keys] u32
static_assert(KV_STAGE % 128 == 0 && ATT_PATCH_BYTES % 128 == 0, "frag_row_x / frag_tr_x XOR bits 4-6 of (tile base + lane word): every tile base must be a multiple of 128 bytes");
// One 64-query tile of the dK/dV pass for a wave's 32 keys (key on the lane).  MASKED: class-2 tile (mask words from LDS);
// DROP: attention dropout on -- compile-time, so the element loops are branch-free.
template <bool MASKED, bool DROP, bool F16>
__device__ __forceinline__ void dkv_tile(const AttnArgs& a, const char* tQ, const char* tD, const float* s_lse, const float* s_dl,
                                         const uint32_t* s_w, const bf16x8 (&kf)[4], const bf16x8 (&vf)[4], f32x16 (&dk)[2],
                                         f32x16 (&dv)[2], int b, int head, int cur, int key, int wid, float c2, int lane_in, const uint32_t* s_db,
                                         const FragLane& fl) {
  // The lane index is made opaque per tile: hipcc otherwise hoists every lane-dependent LDS offset of the 48 fragment reads out of the tile
  // loop (a dozen registers), runs out at the 256-register cap of two waves per SIMD and SPILLS them -- each reload inside a tile body was a
  // scratch load whose `s_waitcnt vmcnt(0)` also drained the LDS-DMA ring (8-11 per tile; SQ_WAIT_ANY 50 % of the wave cycles).  Recomputing
  // the offsets costs a few VALU instructions per tile.
  int lane = lane_in;
  unsigned rk_ = fl.rk, tr_ = fl.tr;       // the lane's part of every fragment address (FragLane): two registers across the tile loop
  asm volatile("" : "+v"(lane), "+v"(rk_), "+v"(tr_));
  const int l31 = lane & 31, h = lane >> 5;
  const unsigned tq = lds_addr(tQ) + rk_, td = lds_addr(tD) + rk_, tqt = lds_addr(tQ) + tr_, tdt = lds_addr(tD) + tr_;
  const float dscale = DROP ? a.inv_keep * a.scale : a.scale;
#pragma unroll
  for (int qq = 0; qq < 2; ++qq) {
    f32x16 sc, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { sc[i] = 0.f; dp[i] = 0.f; }
    {
      // the Q / dO fragments one step ahead of their MFMAs and no further: hipcc otherwise requests all eight up front (32 registers)
      // and spills elsewhere -- every reload of a spilled register is a scratch load whose `vmcnt(0)` also drains the LDS-DMA ring
      bf16x8 qc = frag_row_x(tq, 32 * qq, 0), dc = frag_row_x(td, 32 * qq, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8 qn = qc, dn = dc;
        if (s + 1 < 4) { qn = frag_row_x(tq, 32 * qq, s + 1); dn = frag_row_x(td, 32 * qq, s + 1); }
        __builtin_amdgcn_sched_barrier(0);
        sc = mma32<F16>(qc, kf[s], sc);
        dp = mma32<F16>(dc, vf[s], dp);
        __builtin_amdgcn_sched_barrier(0);
        qc = qn; dc = dn;
      }
    }
    f32x16& pv = dp;                          // P (dropped-out) overwrites dP element by element
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int qr0 = 32 * qq + 8 * g + 4 * h;      // 4 consecutive query rows of this register quad
      f32x4 l4 = *(const f32x4*)(s_lse + qr0);      // natural-log row statistics as the forward wrote them
      f32x4 d4 = *(const f32x4*)(s_dl + qr0);
      l4 *= LOG2E;
      d4 *= a.scale;
      // keep-bits: this key's dword holds the bits of the 32 queries of the half; element r is query acc_row(r, h) = (r&3) + 8*(r>>2) + 4*h
      int wsh = 0;
      if (DROP) wsh = (int)(s_db[wid * 64 + qq * 32 + l31] >> (4 * h));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        float p;                              // rows q >= Lv: dO row and delta are zero, so whatever p is, nothing is added
        if (!MASKED) {
          p = fexp2(fmaf(sc[r], c2, -l4[e]));
        } else {
          const uint32_t w = s_w[(qr0 + e) * 4 + wid];
          p = fexp2(fmaf(sc[r], c2, ((w >> l31) & 1u) ? 0.f : MASK_ADD * LOG2E) - l4[e]);
        }
        if (DROP) {
          const int t = __builtin_amdgcn_sbfe(wsh, e + 8 * g, 1);      // 0 or all ones
          sc[r] = p * fmaf(and_bits(dp[r], t), dscale, -d4[e]);
          pv[r] = and_bits(p * a.inv_keep, t);
        } else {
          sc[r] = p * fmaf(dp[r], dscale, -d4[e]);
          pv[r] = p;
        }
      }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 pf = pack8t<F16>(pv, s2);
      const bf16x8 dsf = pack8t<F16>(sc, s2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = mma32<F16>(frag_tr_x(tdt, dt, 32 * qq + 16 * s2), pf, dv[dt]);
        dk[dt] = mma32<F16>(frag_tr_x(tqt, dt, 32 * qq + 16 * s2), dsf, dk[dt]);
      }
    }
  }
}
#define DKV_NS 4      // 70 KiB of LDS per block, two blocks per CU (register-limited)
template <bool F16>
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_mfma_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(128))) char smem[];   // (fragment addressing XORs bits 4-6 of tile base + lane word: bases are multiples of 128)
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int xb, head, b;
  att_block(a, xb, head, b);
  const int L = a.L, H = a.H, ld = 3 * a.H, T = a.T;
  const int kb0 = xb * 128, k0w = kb0 + wid * 32, key = k0w + l31;
  PROF_DECL;
  const TileMasks tmk = load_tile_masks<true>(a.info, b, T, kb0 >> 6, min(k0w >> 6, T - 1), lane);      // before the row plan: see the forward
  const int Lv = row_count(a, b);
  if (kb0 >= Lv) return;
  const bool wave_on = k0w < Lv, k_ok = key < Lv;
  const size_t rowbase = row_base(a, b);
  const size_t lrow = (size_t)b * L;
  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.qkv, 0, a.bytes_qkv, 0x00020000);
  const dma_rsrc_t rsq = dma_rsrc(a.qkv, a.bytes_qkv);
  __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dctx, 0, a.bytes_ctx, 0x00020000);

  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    kf[s] = load_rowfrag_global(rs, a.bytes_qkv, rowbase + key, k_ok, ld, H + head * 64 + 16 * s + 8 * h);
    vf[s] = load_rowfrag_global(rs, a.bytes_qkv, rowbase + key, k_ok, ld, 2 * H + head * 64 + 16 * s + 8 * h);
  }
  const float c2 = a.scale * LOG2E;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { dk[0][i] = 0.f; dk[1][i] = 0.f; dv[0][i] = 0.f; dv[1][i] = 0.f; }

  const int Lq = query_count(a, b, Lv);        // rows that are queries: the others arrive as zero rows with zero statistics
  const int nqt = (Lq + 63) / 64;
  const int ka = kb0 >> 6;
  const int kw0 = kb0 >> 5;           // first of the block's 4 mask words
  const size_t sbase = ((size_t)b * a.A + head) * L;

  // Q / dO tiles, their softmax statistics and this key block's mask words all arrive by LDS-DMA into a ring of DKV_NS
  // stages (rows past Lv are zero-filled: a zero dO row and a zero delta make that row contribute nothing to dK or dV)
  const dma_rsrc_t rsdo = dma_rsrc(a.dctx, a.bytes_ctx);
  const dma_rsrc_t rsl = dma_rsrc(a.lse_in, a.bytes_stat), rsdl = dma_rsrc(a.delta, a.bytes_stat), rsw = dma_rsrc(a.bits, a.bytes_bits);
  const bool use_db = a.drop_on != 0;
  const dma_rsrc_t rsdb = dma_rsrc(a.dropbits, a.bytes_dbits);
  // this lane's keep-bit dword inside a (32-query x 64-key) block: key half kk, then the accumulator order of the key (2*r + h)
  const int kq32 = (lane & 31), kkw = (k0w >> 5) & 1;
  const unsigned db_in_block = (unsigned)(kkw * 32 + 2 * (((kq32 >> 3) << 2) | (kq32 & 3)) + ((kq32 >> 2) & 1));
  int cur = next_tile(tmk.need, -1, nqt);
  int iss = cur, issued = 0, done = 0;
  auto issue = [&]() {
    char* st_ = smem + (issued % DKV_NS) * KV_STAGE;
    tile_dma<4>(rsq, a.bytes_qkv, rowbase, iss * 64, Lq, ld, head * 64, st_, wid, lane);
    tile_dma<4>(rsdo, a.bytes_ctx, rowbase, iss * 64, Lq, H, head * 64, st_ + 8192, wid, lane);
    {   // 64 rows x 4 mask words: 256 dwords, 64 per wave
      const int idx = wid * 64 + lane, qq = iss * 64 + (idx >> 2), wi = kw0 + (idx & 3);
      const bool ok = qq < Lq && wi < a.W;
      const unsigned off = (unsigned)(((lrow + qq) * (size_t)a.W + wi) * 4);
      lds_dma4(rsw, (MV_LDS void*)(st_ + 16384 + 512 + wid * 256), ok ? off : a.bytes_bits);
    }
    {   // lse (even waves) / delta (odd waves) of the 64 query rows; issued by every wave so that the counted waits are uniform
      const int qi = iss * 64 + lane;
      const unsigned off = (unsigned)((sbase + qi) * 4);
      if (wid & 1) lds_dma4(rsdl, (MV_LDS void*)(st_ + 16384 + 256), qi < Lq ? off : a.bytes_stat);
      else lds_dma4(rsl, (MV_LDS void*)(st_ + 16384), qi < Lq ? off : a.bytes_stat);
    }
    if (use_db) {   // keep-bit dwords of this wave's 32 keys for the tile's two 32-query halves (lane >> 5)
      const size_t blk = dbits_block(a, (size_t)b * a.A + head, 2 * iss + (lane >> 5), k0w >> 6);
      const unsigned off = (unsigned)((blk * 2 + db_in_block) * 4);
      lds_dma4(rsdb, (MV_LDS void*)(st_ + 16384 + 512 + 1024 + wid * 256), (k0w < Lv && (2 * iss + (lane >> 5)) * 32 < Lq) ? off : a.bytes_dbits);
    }
    ++issued;
    iss = next_tile(tmk.need, iss, nqt);
  };
#pragma unroll
  for (int i = 0; i < DKV_NS - 1; ++i)
    if (iss < nqt) issue();
  const FragLane fl = frag_lane(lane);
  PROF_MARK(0);
  while (cur < nqt) {
    if (use_db) att_wait_stage<7>(issued - done - 1);
    else att_wait_stage<6>(issued - done - 1);
    PROF_MARK(1);
    __builtin_amdgcn_s_barrier();
    PROF_MARK(2);
    __builtin_amdgcn_sched_barrier(0);
    const char* st = smem + (done % DKV_NS) * KV_STAGE;
    const uint32_t* s_db = (const uint32_t*)(st + 16384 + 512 + 1024);
    const char* tQ = st;
    const char* tD = st + 8192;
    const float* s_lse = (const float*)(st + 16384);
    const float* s_dl = (const float*)(st + 16384 + 256);
    const uint32_t* s_w = (const uint32_t*)(st + 16384 + 512);
    const int cls = !wave_on ? 0 : (((tmk.w_is1 >> cur) & 1) ? 1 : (((tmk.w_nz >> cur) & 1) ? 2 : 0));
    if (wave_on && cls != 0) {
      const int variant = (cls == 1 ? 0 : 1) | (use_db ? 2 : 0);        // one wave-uniform dispatch per tile
#define DKV_CALL(M_, D_) dkv_tile<M_, D_, F16>(a, tQ, tD, s_lse, s_dl, s_w, kf, vf, dk, dv, b, head, cur, key, wid, c2, lane, s_db, fl)
      switch (variant) {
        case 0: DKV_CALL(false, false); break;
        case 1: DKV_CALL(true, false); break;
        case 2: DKV_CALL(false, true); break;
        default: DKV_CALL(true, true); break;
      }
#undef DKV_CALL
    }
#if ATT_PROF
    asm volatile("s_nop 0" ::"v"(dk[0][0]), "v"(dv[1][15]));
#endif
    PROF_MARK(3);
    if (iss < nqt) issue();
    cur = next_tile(tmk.need, cur, nqt);
    ++done;
    PROF_MARK(4);
  }
  // epilogue: whole rows through a per-wave LDS patch (dK, then dV through the same patch)
  __builtin_amdgcn_s_barrier();
  bf16_t* krow0 = a.dqkv + (rowbase + k0w) * (size_t)ld + H + head * 64;
  store_rows_tile<F16>(smem + wid * ATT_PATCH_BYTES, dk, 1.0f, k_ok, krow0, (size_t)ld, Lv - k0w, lane);
  store_rows_tile<F16>(smem + wid * ATT_PATCH_BYTES, dv, 1.0f, k_ok, krow0 + H, (size_t)ld, Lv - k0w, lane);
#if ATT_PROF
  asm volatile("s_waitcnt vmcnt(0)");
#endif
  PROF_MARK(5);
  PROF_FLUSH(2);
}
#if ATT_PROF
extern "C" int mv_debug_attn_prof(unsigned long long* out48) {       // variant libraries only: totals since the last call, then cleared
  unsigned long long z[24] = {0};
  hipError_t e = hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_att_prof), sizeof(z));
  if (e == hipSuccess) e = hipMemcpyFromSymbol(out48 + 24, HIP_SYMBOL(g_att_tile), sizeof(z));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_att_prof), z, sizeof(z));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_att_tile), z, sizeof(z));
  return (int)e;
}
#endif

// ---- launchers ---------------------------------------------------------------------------------
// The kernels take both 16-bit encodings as bf16_t pointers; <F16> picks the MFMA.  Every kernel asks for dynamic LDS (the dK/dV ring's
// 75,776 bytes are above the 64 KiB a launch gets without the attribute): mv_launch_lds.
static dim3 attn_grid(const AttnArgs& a) { return dim3((a.L + 127) / 128, a.A, a.B); }

int mv_attn_launch_fwd(const AttnArgs& a, bool f16, hipStream_t stream) {
  if (f16) mv_launch_lds<attn_fwd_mfma_kernel<true>>(attn_grid(a), dim3(256), FWD_NS * 16384, stream, a);
  else mv_launch_lds<attn_fwd_mfma_kernel<false>>(attn_grid(a), dim3(256), FWD_NS * 16384, stream, a);
  return (int)hipGetLastError();
}

int mv_attn_launch_bwd(const AttnArgs& a, bool f16, hipStream_t stream) {
  if (f16) mv_launch_lds<attn_bwd_dq_mfma_kernel<true>>(attn_grid(a), dim3(256), DQ_NS * 16384, stream, a);
  else mv_launch_lds<attn_bwd_dq_mfma_kernel<false>>(attn_grid(a), dim3(256), DQ_NS * 16384, stream, a);
  MV_CHECK_LAUNCH();
  if (f16) mv_launch_lds<attn_bwd_dkv_mfma_kernel<true>>(attn_grid(a), dim3(256), DKV_NS * KV_STAGE, stream, a);
  else mv_launch_lds<attn_bwd_dkv_mfma_kernel<false>>(attn_grid(a), dim3(256), DKV_NS * KV_STAGE, stream, a);
  return (int)hipGetLastError();
}
