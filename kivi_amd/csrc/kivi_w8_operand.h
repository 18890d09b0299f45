// Operand forming of the FP8 weight kernels (kivi_w8.hip, and the FP8 expert kernel of kivi_moe.hip; DESIGN.md sections 35 and 36):
// e4m3fn bytes of a row-major weight -> the packed 16-bit fragment of a v_mfma_f32_16x16x32 operand.  Device code only.
#pragma once
#include "kivi_common.h"

namespace {

// two e4m3fn bytes of `word` (the low two, or with HI the high two) -> the packed pair in the dtype, exactly
template <bool BF, bool HI>
__device__ __forceinline__ uint32_t cvt2(uint32_t word) {
    if constexpr (BF) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(word, 1.0f, HI));
    else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(word, 1.0f, HI));
}
// 8 consecutive bytes of a row -> the 8 elements of an operand fragment: register i holds elements 2 i (low half) and 2 i + 1
template <bool BF>
__device__ __forceinline__ u32x4 w8_operand(uint32_t lo, uint32_t hi) {
    return u32x4{cvt2<BF, false>(lo), cvt2<BF, true>(lo), cvt2<BF, false>(hi), cvt2<BF, true>(hi)};
}

}  // namespace
