// HOST-side helper of the C ABI (no device code).  The reference Dataset ships a materialised int64 [B,L,L] attention mask per batch
// (data/dataset_origin.py:138-176: 134 MB at B = 64, L = 512).  The trainer derives {family, n2, vl} descriptors from a few probe
// entries and runs on those (mv_mask_build); to hold the "mask indexing is bit-exact" contract on EVERY batch, every entry of the
// shipped matrix is compared here with what mv_mask_build makes of the descriptors -- the same predicates as mask_build_kernel
// (mv_attn_mask.hip), evaluated a 32-column word at a time -- in one pass over the matrix at memory speed, split over
// host threads by sample.  Nothing crosses PCIe; the trainer runs it on a worker thread one batch ahead of the step.
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <thread>
#include <vector>
#include "../../include/medvill.h"

namespace {

inline uint32_t pack32(const int64_t* p, int n) {
  uint32_t w = 0;
  if (n == 32) {
#pragma clang loop vectorize(enable) interleave(enable)
    for (int k = 0; k < 32; ++k) w |= (uint32_t)(p[k] != 0) << k;
  } else {
    for (int k = 0; k < n; ++k) w |= (uint32_t)(p[k] != 0) << k;
  }
  return w;
}

// bits of the columns [lo, hi) that fall into word w (columns 32 w .. 32 w + 31)
inline uint32_t span_bits(int lo, int hi, int w) {
  const int a = lo - 32 * w, b = hi - 32 * w;
  const int s = a < 0 ? 0 : a, e = b > 32 ? 32 : b;
  if (e <= s) return 0u;
  const uint32_t upto_e = (e == 32) ? 0xffffffffu : ((1u << e) - 1u);
  return upto_e & ~((1u << s) - 1u);          // s < 32 here
}

// row i of the closed form of (fam, n2, vl) as at most two column spans, clipped to [0, L)
inline void row_spans(int fam, int n2, int vl, int i, int L, int& lo0, int& hi0, int& lo1, int& hi1) {
  lo0 = hi0 = lo1 = hi1 = 0;
  switch (fam) {
    case 1: hi0 = n2; if (i >= n2) { lo1 = n2; hi1 = i + 1; } break;                        // seq2seq
    case 2: hi0 = (i < n2) ? L : (n2 > i + 1 ? n2 : i + 1); break;                          // BAR
    case 3: if (i < n2) hi0 = n2; else { lo0 = n2; hi0 = L; } break;                        // non-cross
    default: hi0 = vl; break;                                                               // bidirectional / 1-D
  }
  if (hi0 > L) hi0 = L;
  if (hi1 > L) hi1 = L;
  if (lo0 < 0) lo0 = 0;
  if (lo1 < 0) lo1 = 0;
}

template <int kDummy>
inline long long verify_range(const int64_t* mask, int ndim, const int32_t* desc, int L, int b0, int b1) {
  const int W = (L + 31) / 32;
  for (int b = b0; b < b1; ++b) {
    const int fam = desc[3 * b], n2 = desc[3 * b + 1], vl = desc[3 * b + 2];
    const int rows = (ndim == 3) ? L : 1;          // a [B,L] mask is one row per sample (broadcast over the queries)
    for (int i = 0; i < rows; ++i) {
      const int64_t* row = (ndim == 3) ? mask + ((size_t)b * L + i) * L : mask + (size_t)b * L;
      int lo0, hi0, lo1, hi1;
      row_spans(ndim == 3 ? fam : 0, n2, vl, i, L, lo0, hi0, lo1, hi1);
      for (int w = 0; w < W; ++w) {
        const int n = (L - 32 * w) >= 32 ? 32 : (L - 32 * w);
        const uint32_t got = pack32(row + 32 * w, n);
        const uint32_t want = span_bits(lo0, hi0, w) | span_bits(lo1, hi1, w);
        if (got != want) {
          const uint32_t diff = got ^ want;
          return ((long long)b * rows + i) * L + 32 * w + __builtin_ctz(diff);
        }
      }
    }
  }
  return -1;
}

__attribute__((target("avx2"))) long long verify_range_avx2(const int64_t* mask, int ndim, const int32_t* desc, int L, int b0, int b1) {
  return verify_range<1>(mask, ndim, desc, L, b0, b1);
}
long long verify_range_base(const int64_t* mask, int ndim, const int32_t* desc, int L, int b0, int b1) {
  return verify_range<0>(mask, ndim, desc, L, b0, b1);
}

}  // namespace

extern "C" int mv_mask_verify_host(const int64_t* mask, int mask_ndim, const int32_t* desc, int B, int L, int threads,
                                   long long* first_mismatch) {
  if (!mask || !desc || !first_mismatch || B <= 0 || L <= 0) return MV_E_ARG;
  if (mask_ndim != 2 && mask_ndim != 3) return MV_E_SHAPE;      // NotImplementedError in cxrbert_origin.py:80-81
  for (int b = 0; b < B; ++b)
    if (desc[3 * b] < 0 || desc[3 * b] > 4) return MV_E_ARG;
  static const bool avx2 = __builtin_cpu_supports("avx2");
  std::atomic<long long> bad(-1);
  auto run = [&](int b0, int b1) {
    const long long r = avx2 ? verify_range_avx2(mask, mask_ndim, desc, L, b0, b1) : verify_range_base(mask, mask_ndim, desc, L, b0, b1);
    if (r >= 0) {
      long long cur = bad.load();
      while ((cur < 0 || r < cur) && !bad.compare_exchange_weak(cur, r)) {}
    }
  };
  int nt = threads < 1 ? 1 : (threads > B ? B : threads);
  if (nt > 64) nt = 64;
  if (nt == 1) run(0, B);
  else {
    std::vector<std::thread> pool;
    pool.reserve(nt - 1);
    for (int t = 1; t < nt; ++t) pool.emplace_back(run, (int)((long long)B * t / nt), (int)((long long)B * (t + 1) / nt));
    run(0, B / nt);
    for (auto& th : pool) th.join();
  }
  *first_mismatch = bad.load();
  return MV_OK;
}
