// kivi_qk_rope (include/kivi_hip.h): what a layer does to its q and k projections before the attention, in ONE
// launch -- the optional per-head RMSNorm of Qwen3, the rotary embedding from the caller's cos / sin tables, and the placement into
// the (B, heads, Q, D) layout the attention reads, with the query heads of a kv head padded from R to Rp by zero heads.
//
// One wave per (batch row, token, head slot): D = 128 is two elements per lane, and lane l holds channels l and l + 64 -- the very pair
// the rotation exchanges, so RoPE needs no cross-lane traffic, and the norm is one wave reduction.  Every load and store of a wave is
// one contiguous 128-byte row segment.  The traffic is a few hundred KB per decode step: what the kernel saves is launches.
//
// Arithmetic: every product and the sum of the rotation is rounded to fp16 on its own, as torch evaluates `x * cos + rot(x) * sin` on
// fp16 tensors (a product of two fp16 values is exact in fp32, so one rounding of it is torch's; the sum is torch's fp32 add of two
// fp16 values, rounded).  Contraction is switched off for this file: left on, the compiler narrows the fp32 operations between the
// conversions to fp16 ones and fuses a product with the sum into one v_fma_f16 -- one rounding where torch has two.
#include <hip/hip_fp16.h>

#include "kivi_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / KIVI_WAVE;
constexpr int kD = 128;

__device__ __forceinline__ float round16(float x) { return __half2float(__float2half_rn(x)); }

// double -> the fp32 value that rounds to the same fp16 as the double does: truncated, with a sticky last bit (round to odd), so the
// fp16 rounding that follows is the only one
__device__ __forceinline__ float to_odd(double d) {
    float f = __double2float_rz(d);
    if ((double)f != d) f = __uint_as_float(__float_as_uint(f) | 1u);
    return f;
}

// HF's Qwen3RMSNorm on one head: mean of squares, fp16(x * rsqrt(var + eps)), fp16(weight * that).  HF evaluates the first two in
// fp32, which leaves about one element in a thousand an fp16 ulp away from the formula's own value, WHICH elements depending on the
// order of the sum.  Here the 128 squares (exact in fp64), their sum, the root and the product are fp64, so the result is the
// formula's correctly rounded value whatever the reduction order -- 256 fp64 operations per head, nothing beside the launch.
__device__ __forceinline__ void head_norm(float& a, float& b, const __half* __restrict__ w, float eps, int lane) {
    double ss = (double)a * a + (double)b * b;
#pragma unroll
    for (int m = 1; m < KIVI_WAVE; m <<= 1) ss += __shfl_xor(ss, m);
    const double r = 1.0 / sqrt(ss * (1.0 / kD) + (double)eps);
    a = round16(__half2float(w[lane]) * round16(to_odd(a * r)));
    b = round16(__half2float(w[lane + 64]) * round16(to_odd(b * r)));
}

__global__ __launch_bounds__(kThreads) void qk_rope_kernel(const __half* __restrict__ q_in, int64_t q_sb, int64_t q_st, int64_t q_sh,
                                                           const __half* __restrict__ k_in, int64_t k_sb, int64_t k_st, int64_t k_sh,
                                                           const __half* __restrict__ cos_t, const __half* __restrict__ sin_t,
                                                           int64_t cs_sb, int64_t cs_st, const __half* __restrict__ q_w,
                                                           const __half* __restrict__ k_w, float eps, __half* __restrict__ q_out,
                                                           __half* __restrict__ k_out, int64_t units, int Q, int nh_kv, int R, int Rp) {
    const int lane = threadIdx.x & (KIVI_WAVE - 1);
    const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / KIVI_WAVE;       // wave-uniform, as everything derived from it
    if (unit >= units) return;
    const int slots = nh_kv * (Rp + 1);                     // per (b, t): nh_kv * Rp query slots, then nh_kv key heads
    const int s = (int)(unit % slots);
    const int64_t bt = unit / slots;
    const int t = (int)(bt % Q);
    const int64_t b = bt / Q;
    const bool is_k = s >= nh_kv * Rp;
    const int kv = is_k ? s - nh_kv * Rp : s / Rp, r = is_k ? 0 : s % Rp;
    __half* dst = is_k ? k_out + ((b * nh_kv + kv) * Q + t) * kD : q_out + ((b * nh_kv * Rp + s) * Q + t) * kD;
    if (!is_k && r >= R) {                                  // a pad head: zeros on every call (the buffer may be torch.empty)
        dst[lane] = __float2half_rn(0.0f);
        dst[lane + 64] = __float2half_rn(0.0f);
        return;
    }
    const __half* src = is_k ? k_in + b * k_sb + t * k_st + kv * k_sh : q_in + b * q_sb + t * q_st + (int64_t)(kv * R + r) * q_sh;
    float a = __half2float(src[lane]), c = __half2float(src[lane + 64]);
    const __half* w = is_k ? k_w : q_w;
    if (w) head_norm(a, c, w, eps, lane);
    const int64_t cs = b * cs_sb + t * cs_st;
    const float c0 = __half2float(cos_t[cs + lane]), c1 = __half2float(cos_t[cs + lane + 64]);
    const float s0 = __half2float(sin_t[cs + lane]), s1 = __half2float(sin_t[cs + lane + 64]);
    // rot(x)[i] = -x[i + 64], rot(x)[i + 64] = x[i]
    dst[lane] = __float2half_rn(round16(a * c0) + round16(-c * s0));
    dst[lane + 64] = __float2half_rn(round16(c * c1) + round16(a * s1));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kivi_qkv_rope_bf16 (include/kivi_hip.h): the same walk over bf16 projections and fp32 tables, fp16 out, with
// nh_kv value slots per (row, token) behind the key slots.  Nothing here imitates a bf16 torch chain: every input is the exact
// number it holds, the formula is evaluated in fp64 -- products of two inputs are exact there, and so is the sum of the 128 squares
// for any head whose values lie within 2^15 of each other -- and the result is rounded once, through to_odd.  With contraction off
// (above) each fp64 operation below is one IEEE operation: the order written here is the contract's.
__device__ __forceinline__ double bf16_in(const uint16_t* __restrict__ p, int i) { return (double)(float)bf16{p[i]}; }

// one rounding to fp16; a finite value that would round to an infinity is stored as the largest fp16 of its sign
__device__ __forceinline__ __half out16(double d) {
    float f = to_odd(d);
    if (__builtin_isfinite(d)) f = fminf(fmaxf(f, -65504.0f), 65504.0f);
    return __float2half_rn(f);
}

__global__ __launch_bounds__(kThreads) void qkv_rope_bf16_kernel(
    const uint16_t* __restrict__ q_in, int64_t q_sb, int64_t q_st, int64_t q_sh, const uint16_t* __restrict__ k_in, int64_t k_sb,
    int64_t k_st, int64_t k_sh, const uint16_t* __restrict__ v_in, int64_t v_sb, int64_t v_st, int64_t v_sh,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int64_t cs_sb, int64_t cs_st, const uint16_t* __restrict__ q_w,
    const uint16_t* __restrict__ k_w, float eps, __half* __restrict__ q_out, __half* __restrict__ k_out, __half* __restrict__ v_out,
    int64_t units, int Q, int nh_kv, int R, int Rp) {
    const int lane = threadIdx.x & (KIVI_WAVE - 1);
    const int64_t unit = (int64_t)blockIdx.x * kWaves + threadIdx.x / KIVI_WAVE;       // wave-uniform, as everything derived from it
    if (unit >= units) return;
    const int nq = nh_kv * Rp, slots = nq + 2 * nh_kv;      // per (b, t): nh_kv * Rp query slots, nh_kv key heads, nh_kv value heads
    const int s = (int)(unit % slots);
    const int64_t bt = unit / slots;
    const int t = (int)(bt % Q);
    const int64_t b = bt / Q;
    if (s >= nq + nh_kv) {                                  // a value head: the conversion alone
        const int kv = s - nq - nh_kv;
        const uint16_t* src = v_in + b * v_sb + t * v_st + kv * v_sh;
        __half* dst = v_out + ((b * nh_kv + kv) * Q + t) * kD;
        dst[lane] = out16(bf16_in(src, lane));
        dst[lane + 64] = out16(bf16_in(src, lane + 64));
        return;
    }
    const bool is_k = s >= nq;
    const int kv = is_k ? s - nq : s / Rp, r = is_k ? 0 : s % Rp;
    __half* dst = is_k ? k_out + ((b * nh_kv + kv) * Q + t) * kD : q_out + ((b * nq + s) * Q + t) * kD;
    if (!is_k && r >= R) {                                  // a pad head: zeros on every call (the buffer may be torch.empty)
        dst[lane] = __float2half_rn(0.0f);
        dst[lane + 64] = __float2half_rn(0.0f);
        return;
    }
    const uint16_t* src = is_k ? k_in + b * k_sb + t * k_st + kv * k_sh : q_in + b * q_sb + t * q_st + (int64_t)(kv * R + r) * q_sh;
    double a = bf16_in(src, lane), c = bf16_in(src, lane + 64);
    const uint16_t* w = is_k ? k_w : q_w;
    if (w) {
        double ss = a * a + c * c;
#pragma unroll
        for (int m = 1; m < KIVI_WAVE; m <<= 1) ss += __shfl_xor(ss, m);
        const double rs = 1.0 / sqrt(ss * (1.0 / kD) + (double)eps);
        a = (bf16_in(w, lane) * a) * rs;
        c = (bf16_in(w, lane + 64) * c) * rs;
    }
    const int64_t cs = b * cs_sb + t * cs_st;
    const double c0 = cos_t[cs + lane], c1 = cos_t[cs + lane + 64], s0 = sin_t[cs + lane], s1 = sin_t[cs + lane + 64];
    // rot(y)[i] = -y[i + 64], rot(y)[i + 64] = y[i]
    dst[lane] = out16(a * c0 + (-c) * s0);
    dst[lane + 64] = out16(c * c1 + a * s1);
}

}  // namespace

extern "C" int kivi_qkv_rope_bf16(const void* q_in, int64_t q_sb, int64_t q_st, int64_t q_sh, const void* k_in, int64_t k_sb,
                                  int64_t k_st, int64_t k_sh, const void* v_in, int64_t v_sb, int64_t v_st, int64_t v_sh,
                                  const void* cos, const void* sin, int64_t cs_sb, int64_t cs_st, const void* q_weight,
                                  const void* k_weight, float eps, void* q_out, void* k_out, void* v_out, int B, int Q, int nh,
                                  int nh_kv, int Rp, int D, kivi_stream_t stream) {
    KIVI_REQUIRE(D == kD, KIVI_EINVAL, "kivi_qkv_rope_bf16: D=%d (the matrix-pipe layout's head size, 128, only)", D);
    KIVI_REQUIRE(B >= 1 && Q >= 1 && nh >= 1 && nh_kv >= 1 && nh % nh_kv == 0, KIVI_EINVAL,
                 "kivi_qkv_rope_bf16: B=%d Q=%d nh=%d nh_kv=%d (all >= 1, nh a multiple of nh_kv)", B, Q, nh, nh_kv);
    const int R = nh / nh_kv;
    KIVI_REQUIRE(Rp >= R && Rp <= 64, KIVI_EINVAL, "kivi_qkv_rope_bf16: Rp=%d (nh / nh_kv = %d <= Rp <= 64)", Rp, R);
    KIVI_REQUIRE(q_in && k_in && v_in && cos && sin && q_out && k_out && v_out, KIVI_EINVAL,
                 "kivi_qkv_rope_bf16: null q_in, k_in, v_in, cos, sin, q_out, k_out or v_out");
    KIVI_REQUIRE(eps >= 0.0f && eps < INFINITY, KIVI_EINVAL, "kivi_qkv_rope_bf16: eps=%g (finite, >= 0)", (double)eps);
    KIVI_REQUIRE(q_sb >= 0 && q_st >= 0 && q_sh >= 0 && k_sb >= 0 && k_st >= 0 && k_sh >= 0 && v_sb >= 0 && v_st >= 0 && v_sh >= 0 &&
                     cs_sb >= 0 && cs_st >= 0,
                 KIVI_EINVAL, "kivi_qkv_rope_bf16: negative stride");
    const int64_t units = (int64_t)B * Q * nh_kv * (Rp + 2);
    const int64_t blocks = (units + kWaves - 1) / kWaves;
    KIVI_REQUIRE(blocks < (1LL << 31), KIVI_EINVAL, "kivi_qkv_rope_bf16: %lld blocks (B * Q * nh_kv * (Rp + 2) / 4 < 2^31)",
                 (long long)blocks);
    for (const void* p : {q_in, k_in, v_in, q_weight, k_weight, (const void*)q_out, (const void*)k_out, (const void*)v_out})
        KIVI_REQUIRE((uintptr_t)p % 2 == 0, KIVI_EALIGN, "kivi_qkv_rope_bf16: a 2-byte pointer off 2 bytes");
    KIVI_REQUIRE((uintptr_t)cos % 4 == 0 && (uintptr_t)sin % 4 == 0, KIVI_EALIGN, "kivi_qkv_rope_bf16: cos or sin off 4 bytes");
    KIVI_LAUNCH(qkv_rope_bf16_kernel, dim3((unsigned)blocks), dim3(kThreads), (hipStream_t)stream, (const uint16_t*)q_in, q_sb, q_st,
                q_sh, (const uint16_t*)k_in, k_sb, k_st, k_sh, (const uint16_t*)v_in, v_sb, v_st, v_sh, (const float*)cos,
                (const float*)sin, cs_sb, cs_st, (const uint16_t*)q_weight, (const uint16_t*)k_weight, eps, (__half*)q_out,
                (__half*)k_out, (__half*)v_out, units, Q, nh_kv, R, Rp);
    return kivi_launch_status("kivi_qkv_rope_bf16");
}

extern "C" int kivi_qk_rope(const void* q_in, int64_t q_sb, int64_t q_st, int64_t q_sh, const void* k_in, int64_t k_sb, int64_t k_st,
                            int64_t k_sh, const void* cos, const void* sin, int64_t cs_sb, int64_t cs_st, const void* q_weight,
                            const void* k_weight, float eps, void* q_out, void* k_out, int B, int Q, int nh, int nh_kv, int Rp, int D,
                            kivi_stream_t stream) {
    KIVI_REQUIRE(D == kD, KIVI_EINVAL, "kivi_qk_rope: D=%d (the matrix-pipe layout's head size, 128, only)", D);
    KIVI_REQUIRE(B >= 1 && Q >= 1 && nh >= 1 && nh_kv >= 1 && nh % nh_kv == 0, KIVI_EINVAL,
                 "kivi_qk_rope: B=%d Q=%d nh=%d nh_kv=%d (all >= 1, nh a multiple of nh_kv)", B, Q, nh, nh_kv);
    const int R = nh / nh_kv;
    KIVI_REQUIRE(Rp >= R && Rp <= 64, KIVI_EINVAL, "kivi_qk_rope: Rp=%d (nh / nh_kv = %d <= Rp <= 64)", Rp, R);
    KIVI_REQUIRE(q_in && k_in && cos && sin && q_out && k_out, KIVI_EINVAL, "kivi_qk_rope: null q_in, k_in, cos, sin, q_out or k_out");
    KIVI_REQUIRE(eps >= 0.0f && eps < INFINITY, KIVI_EINVAL, "kivi_qk_rope: eps=%g (finite, >= 0)", (double)eps);
    KIVI_REQUIRE(q_sb >= 0 && q_st >= 0 && q_sh >= 0 && k_sb >= 0 && k_st >= 0 && k_sh >= 0 && cs_sb >= 0 && cs_st >= 0, KIVI_EINVAL,
                 "kivi_qk_rope: negative stride");
    const int64_t units = (int64_t)B * Q * nh_kv * (Rp + 1);
    const int64_t blocks = (units + kWaves - 1) / kWaves;
    KIVI_REQUIRE(blocks < (1LL << 31), KIVI_EINVAL, "kivi_qk_rope: %lld blocks (B * Q * nh_kv * (Rp + 1) / 4 < 2^31)", (long long)blocks);
    for (const void* p : {q_in, k_in, cos, sin, q_weight, k_weight, (const void*)q_out, (const void*)k_out})
        KIVI_REQUIRE((uintptr_t)p % 2 == 0, KIVI_EALIGN, "kivi_qk_rope: a pointer off 2 bytes");
    KIVI_LAUNCH(qk_rope_kernel, dim3((unsigned)blocks), dim3(kThreads), (hipStream_t)stream, (const __half*)q_in, q_sb, q_st, q_sh,
                (const __half*)k_in, k_sb, k_st, k_sh, (const __half*)cos, (const __half*)sin, cs_sb, cs_st, (const __half*)q_weight,
                (const __half*)k_weight, eps, (__half*)q_out, (__half*)k_out, units, Q, nh_kv, R, Rp);
    return kivi_launch_status("kivi_qk_rope");
}
