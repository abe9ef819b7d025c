// u8 cells <-> one bit per cell, four cells at a time (life_bits, life_rule_bits): per 4 cells one
// multiply-gather (v_mul + v_bfe) on load and one multiply-scatter (v_bfe + v_mul + v_and) on store.
#pragma once

#include <cstdint>

namespace mdfx {
namespace dev {

__device__ __forceinline__ uint32_t life_pack4(uint32_t d) {  // bytes 0/1 -> bits 0..3
  return __builtin_amdgcn_ubfe(d * 0x01020408u, 24, 4);
}
__device__ __forceinline__ uint32_t life_unpack4(uint32_t w, int k) {  // bits 4k..4k+3 -> bytes 0/1
  return (__builtin_amdgcn_ubfe(w, 4 * k, 4) * 0x00204081u) & 0x01010101u;
}

}  // namespace dev
}  // namespace mdfx
