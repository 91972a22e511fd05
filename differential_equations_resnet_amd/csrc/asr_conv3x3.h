// Shared by the 3x3 conv translation units (asr_conv_f32.hip, asr_conv_bf16.hip,
// asr_stage_img.hip): the host entry points' (C, W) dispatch and the bf16 relu masking.
#pragma once
#include <type_traits>

#include "asr_common.h"

namespace asr {

// A kernel family's instantiation for a run-time (C, W): f(c, w) with the pair as integral constants, for the
// pairs of C in {16, 32, 64, 128, 256} x W in {32, 16, 8} that the constexpr predicate OK(C, W) accepts -- f is
// instantiated for those alone.  Every other pair: ASR_E_UNSUPPORTED, "<what>: C=.. W=..".
template <int V>
using int_c = std::integral_constant<int, V>;
template <bool (*OK)(int, int), typename F>
int dispatch_c_w(const char* what, int C, int W, F&& f) {
  int rc = ASR_OK;
  auto at = [&](auto c, auto w) -> bool {  // true: (C, W) is this pair, f ran
    if constexpr (OK(decltype(c)::value, decltype(w)::value)) {
      if (C != decltype(c)::value || W != decltype(w)::value) return false;
      rc = f(c, w);
      return true;
    }
    return false;
  };
  auto at_c = [&](auto c) -> bool { return at(c, int_c<32>{}) || at(c, int_c<16>{}) || at(c, int_c<8>{}); };
  if (at_c(int_c<16>{}) || at_c(int_c<32>{}) || at_c(int_c<64>{}) || at_c(int_c<128>{}) || at_c(int_c<256>{})) return rc;
  return fail(ASR_E_UNSUPPORTED, "%s: C=%d W=%d", what, C, W);
}

// 8 bf16 masked by 8 relu bits (bit j -> halfword j)
__device__ __forceinline__ uint4 mask8_bf16(uint4 v, unsigned bits) {
  auto h2 = [&](unsigned b) { return ((b & 1u) ? 0xffffu : 0u) | ((b & 2u) ? 0xffff0000u : 0u); };
  v.x &= h2(bits);
  v.y &= h2(bits >> 2);
  v.z &= h2(bits >> 4);
  v.w &= h2(bits >> 6);
  return v;
}

}  // namespace asr
