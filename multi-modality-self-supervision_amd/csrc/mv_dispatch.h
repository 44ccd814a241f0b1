// Host-side choice of a kernel instantiation from the encoding codes of the C ABI (MV_F32 / MV_BF16 / MV_F16).
// An entry point states the encodings it takes as one `Accept` list at the top of its body (none: all three) and writes its launch once, in
// a generic lambda that is handed the element type(s) as tags.  Only listed combinations instantiate the lambda (`if constexpr`), so the
// kernels in the library are exactly the Accept lists; any other code or combination returns MV_E_DTYPE without a launch.  A lambda returns
// the int status of its launch, `(int)hipGetLastError()` (hipSuccess is MV_OK); MV_CHECK_LAUNCH() inside one returns from the lambda.
#pragma once
#include <type_traits>
#include "mv_common.h"

template <typename T> struct mv_tag {
  typedef T type;
  static constexpr int code = std::is_same_v<T, float> ? MV_F32 : std::is_same_v<T, bf16_t> ? MV_BF16 : MV_F16;
};
#define MV_T(tag) typename decltype(tag)::type      // the element type a lambda was handed

template <typename... T> struct mv_types {};        // accepted encodings of one argument
template <typename A, typename B> struct mv_pair {};
template <typename... P> struct mv_pairs {};        // accepted (first, second) encodings of two arguments
template <typename T, typename... A> constexpr bool mv_accepts(mv_types<A...>) { return (std::is_same_v<T, A> || ...); }
template <typename TA, typename TB, typename... P> constexpr bool mv_accepts(mv_pairs<P...>) { return (std::is_same_v<mv_pair<TA, TB>, P> || ...); }

template <typename Accept, typename F> inline int mv_with_type(int dt, Accept, F&& f) {
  if constexpr (mv_accepts<float>(Accept{})) if (dt == MV_F32) return f(mv_tag<float>{});
  if constexpr (mv_accepts<bf16_t>(Accept{})) if (dt == MV_BF16) return f(mv_tag<bf16_t>{});
  if constexpr (mv_accepts<f16_t>(Accept{})) if (dt == MV_F16) return f(mv_tag<f16_t>{});
  return MV_E_DTYPE;
}
template <typename F> inline int mv_with_type(int dt, F&& f) { return mv_with_type(dt, mv_types<float, bf16_t, f16_t>{}, f); }

template <typename Accept, typename F> inline int mv_with_types(int dt_a, int dt_b, Accept, F&& f) {
  return mv_with_type(dt_a, [&](auto ta) {
    return mv_with_type(dt_b, [&](auto tb) -> int {
      if constexpr (mv_accepts<MV_T(ta), MV_T(tb)>(Accept{})) return f(ta, tb);
      else return MV_E_DTYPE;
    });
  });
}

// the one-wave-per-row kernels hold a row in registers as NC chunks of 256 columns; NC is a template argument
template <typename F> inline int mv_with_row_chunks(int H, F&& f) {
  if (H <= 256) return f(std::integral_constant<int, 1>{});
  if (H <= 768) return f(std::integral_constant<int, 3>{});
  if (H <= 1024) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

// kernels that only move elements take the two 16-bit encodings as one: both run the bf16_t instantiation, as bits
template <typename T> using mv_bits_t = std::conditional_t<sizeof(T) == 2, bf16_t, T>;
