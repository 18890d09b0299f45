// Per-request LoRA adapters: the batched low-rank side path of a linear layer.  Token n of a (B, Q, .) pass
// belongs to row n / Q, whose slot s = slots[n / Q] names the adapter; for s in [0, S)
//     t[n, j]  = sum_k float(A[s, j, k]) * float(x[n, k])            fp32, order a function of K alone
//     d[n, o]  = sum_j float(B[s, o, j]) * t[n, j]                   fp32, j ascending
//     y'[n, o] = round_dtype(fmaf(scale[s], d[n, o], float(y[n, o])))
// and a row whose slot lies outside [0, S) is not touched.  Every token carries its own weight operand, so this is a batched
// GEMV: memory- and latency-bound, on the VALU with 16-byte loads, no LDS, no barrier, no atomics.
//   shrink   grid (N, R / 4), four waves per block; wave w owns rank 4 blockIdx.y + w over the whole of K.  Lane l takes the
//            16-byte units l, l + 64, ... of the A row and of x, eight fused multiply-adds per unit into one fp32 accumulator,
//            elements ascending; the wave is reduced by the xor tree 32, 16, 8, 4, 2, 1; lane 0 writes t[n, j].
//   expand   grid (N, ceil(O / 512)), one thread per two adjacent outputs: the two B rows by 16-byte loads, t[n, :] through the
//            uniform path (its address is the block's), one 32-bit read-modify-write of y.
// Both stop at ranks[s] rounded up to 8 (an adapter of rank r occupies [0, r) of its slot, the rest are zeros), so a token's bits
// depend on its x, its slot and that slot's tables alone: not on its batch, the other rows' slots, R or S.  The guards are
// block-uniform (a block holds one token).  Every offset comes from kivi_lora_plan.h, which tests/lora_plan_main.cpp walks.
#include <hip/hip_fp16.h>

#include "kivi_common.h"
#include "kivi_lora_plan.h"

namespace {

// fp32 -> the 16 bits of the dtype, round to nearest even, once
template <bool BF>
__device__ __forceinline__ uint16_t to_bits(float f) {
    if constexpr (BF) {
        const uint32_t u = __float_as_uint(f);
        if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);     // NaN stays NaN
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    } else {
        return f2h_bits(f);
    }
}
template <bool BF>
__device__ __forceinline__ float from_bits(uint16_t h) {
    if constexpr (BF) return (float)bf16{h};
    else return h2f_bits(h);
}

template <bool BF>
__global__ __launch_bounds__(KIVI_LORA_SHRINK_WAVES* KIVI_LORA_WAVE) void lora_shrink_kernel(
    const uint16_t* __restrict__ x, int64_t x_stride, int64_t Q, int64_t K, const int* __restrict__ slots, int S, int R,
    const int* __restrict__ ranks, const uint16_t* __restrict__ A, float* __restrict__ t) {
    const int64_t n = blockIdx.x;
    const int s = slots[n / Q];
    if (!kivi_lora_plan_slot_ok(s, S)) return;                                        // block-uniform: the row stays untouched
    if (kivi_lora_plan_shrink_rank(blockIdx.y, 0) >= kivi_lora_plan_active_ranks(ranks[s], R)) return;
    const int lane = threadIdx.x & 63;
    const int j = kivi_lora_plan_shrink_rank(blockIdx.y, threadIdx.x >> 6);
    const int64_t units = kivi_lora_plan_units(K);
    float acc = 0.0f;
#pragma unroll 4
    for (int64_t i = 0; kivi_lora_plan_lane_unit(lane, i) < units; i++) {
        const int64_t u = kivi_lora_plan_lane_unit(lane, i);
        const u16x8 a = *(const u16x8*)(A + kivi_lora_plan_a_unit(s, R, K, j, u));
        const u16x8 v = *(const u16x8*)(x + kivi_lora_plan_x_unit(n, x_stride, u));
#pragma unroll
        for (int e = 0; e < 8; e++) acc = __builtin_fmaf(from_bits<BF>(a[e]), from_bits<BF>(v[e]), acc);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) t[kivi_lora_plan_t_at(n, R, j)] = acc;
}

template <bool BF>
__global__ __launch_bounds__(KIVI_LORA_EXPAND_THREADS) void lora_expand_kernel(
    const float* __restrict__ t, const int* __restrict__ slots, int S, int R, const int* __restrict__ ranks,
    const float* __restrict__ scale, const uint16_t* __restrict__ Bm, uint16_t* __restrict__ y, int64_t y_stride, int64_t Q,
    int64_t O) {
    const int64_t n = blockIdx.x;
    const int s = slots[n / Q];
    if (!kivi_lora_plan_slot_ok(s, S)) return;                                        // block-uniform
    const int rr = kivi_lora_plan_active_ranks(ranks[s], R);
    const int64_t o = kivi_lora_plan_expand_out(blockIdx.y, threadIdx.x);
    if (rr == 0 || o >= O) return;                                                    // (O is even: o + 1 < O with o)
    const float sc = scale[s];
    const float* __restrict__ tn = t + kivi_lora_plan_t_at(n, R, 0);
    float d0 = 0.0f, d1 = 0.0f;
    for (int j8 = 0; j8 * KIVI_LORA_UNIT < rr; j8++) {
        const u16x8 b0 = *(const u16x8*)(Bm + kivi_lora_plan_b_unit(s, O, R, o, j8));
        const u16x8 b1 = *(const u16x8*)(Bm + kivi_lora_plan_b_unit(s, O, R, o + 1, j8));
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float tj = tn[j8 * KIVI_LORA_UNIT + e];
            d0 = __builtin_fmaf(from_bits<BF>(b0[e]), tj, d0);
            d1 = __builtin_fmaf(from_bits<BF>(b1[e]), tj, d1);
        }
    }
    uint32_t* word = (uint32_t*)(y + kivi_lora_plan_y_at(n, y_stride, o));
    const uint32_t w = *word;
    const uint16_t r0 = to_bits<BF>(__builtin_fmaf(sc, d0, from_bits<BF>((uint16_t)(w & 0xFFFFu))));
    const uint16_t r1 = to_bits<BF>(__builtin_fmaf(sc, d1, from_bits<BF>((uint16_t)(w >> 16))));
    *word = (uint32_t)r0 | ((uint32_t)r1 << 16);
}

int check_common(const char* what, int dtype, int64_t N, int64_t Q, int S, int R) {
    KIVI_REQUIRE(kivi_lora_plan_dtype_ok(dtype), KIVI_EINVAL, "%s: dtype=%d (16: fp16, 0x110: bf16)", what, dtype);
    KIVI_REQUIRE(kivi_lora_plan_tokens_ok(N, Q), KIVI_EINVAL, "%s: N=%lld Q=%lld (N >= 1 tokens in whole rows of Q >= 1, N < 2^31)", what,
                 (long long)N, (long long)Q);
    KIVI_REQUIRE(kivi_lora_plan_slots_ok(S), KIVI_EINVAL, "%s: S=%d (at least one slot)", what, S);
    KIVI_REQUIRE(kivi_lora_plan_rank_ok(R), KIVI_EINVAL, "%s: R=%d (the table rank is 8, 16, 32 or 64)", what, R);
    return 0;
}

}  // namespace

extern "C" int kivi_lora_shrink(const void* x, int64_t x_stride, int dtype, int64_t N, int64_t Q, int K, const void* slots, int S, int R,
                                const void* ranks, const void* A, void* t, kivi_stream_t stream) {
    const char* what = "kivi_lora_shrink";
    if (int rc = check_common(what, dtype, N, Q, S, R)) return rc;
    KIVI_REQUIRE(kivi_lora_plan_dim_ok(K), KIVI_EINVAL, "%s: K=%d (a positive multiple of 8)", what, K);
    KIVI_REQUIRE(x_stride >= K, KIVI_EINVAL, "%s: x_stride=%lld < K=%d", what, (long long)x_stride, K);
    KIVI_REQUIRE(x && slots && ranks && A && t, KIVI_EINVAL, "%s: null x, slots, ranks, A or t", what);
    KIVI_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)A % 16 == 0 && x_stride % 8 == 0, KIVI_EALIGN,
                 "%s: x or A off 16 bytes, or x_stride=%lld not a multiple of 8", what, (long long)x_stride);
    KIVI_REQUIRE((uintptr_t)slots % 4 == 0 && (uintptr_t)ranks % 4 == 0 && (uintptr_t)t % 4 == 0, KIVI_EALIGN,
                 "%s: slots, ranks or t off 4 bytes", what);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)N, (unsigned)kivi_lora_plan_shrink_grid_y(R)), block(KIVI_LORA_SHRINK_WAVES * KIVI_LORA_WAVE);
    if (dtype == KIVI_LORA_BF16)
        KIVI_LAUNCH(lora_shrink_kernel<true>, grid, block, s, (const uint16_t*)x, x_stride, Q, (int64_t)K, (const int*)slots, S, R,
                    (const int*)ranks, (const uint16_t*)A, (float*)t);
    else
        KIVI_LAUNCH(lora_shrink_kernel<false>, grid, block, s, (const uint16_t*)x, x_stride, Q, (int64_t)K, (const int*)slots, S, R,
                    (const int*)ranks, (const uint16_t*)A, (float*)t);
    return kivi_launch_status(what);
}

extern "C" int kivi_lora_expand(const void* t, const void* slots, int S, int R, const void* ranks, const void* scale, const void* B,
                                void* y, int64_t y_stride, int dtype, int64_t N, int64_t Q, int O, kivi_stream_t stream) {
    const char* what = "kivi_lora_expand";
    if (int rc = check_common(what, dtype, N, Q, S, R)) return rc;
    KIVI_REQUIRE(kivi_lora_plan_dim_ok(O) && kivi_lora_plan_expand_grid_ok(O), KIVI_EINVAL,
                 "%s: O=%d (a positive multiple of 8, at most 512 * 65535)", what, O);
    KIVI_REQUIRE(y_stride >= O, KIVI_EINVAL, "%s: y_stride=%lld < O=%d", what, (long long)y_stride, O);
    KIVI_REQUIRE(t && slots && ranks && scale && B && y, KIVI_EINVAL, "%s: null t, slots, ranks, scale, B or y", what);
    KIVI_REQUIRE((uintptr_t)B % 16 == 0, KIVI_EALIGN, "%s: B off 16 bytes", what);
    KIVI_REQUIRE((uintptr_t)y % 4 == 0 && y_stride % 2 == 0, KIVI_EALIGN, "%s: y off 4 bytes, or y_stride=%lld odd", what,
                 (long long)y_stride);
    KIVI_REQUIRE((uintptr_t)slots % 4 == 0 && (uintptr_t)ranks % 4 == 0 && (uintptr_t)t % 4 == 0 && (uintptr_t)scale % 4 == 0, KIVI_EALIGN,
                 "%s: slots, ranks, scale or t off 4 bytes", what);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)N, (unsigned)kivi_lora_plan_expand_grid_y(O)), block(KIVI_LORA_EXPAND_THREADS);
    if (dtype == KIVI_LORA_BF16)
        KIVI_LAUNCH(lora_expand_kernel<true>, grid, block, s, (const float*)t, (const int*)slots, S, R, (const int*)ranks,
                    (const float*)scale, (const uint16_t*)B, (uint16_t*)y, y_stride, Q, (int64_t)O);
    else
        KIVI_LAUNCH(lora_expand_kernel<false>, grid, block, s, (const float*)t, (const int*)slots, S, R, (const int*)ranks,
                    (const float*)scale, (const uint16_t*)B, (uint16_t*)y, y_stride, Q, (int64_t)O);
    return kivi_launch_status(what);
}
