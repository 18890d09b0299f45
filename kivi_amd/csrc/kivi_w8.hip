// kivi_w8_dequant / kivi_w8_linear / kivi_w8_gate_up (include/kivi_hip.h): FP8 weights under 16-bit
// activations (W8A16).  The buffers are the checkpoint's own: `weight` (O, K) row-major, one OCP e4m3fn byte per element -- gfx950's
// native FP8 encoding --, and `weight_scale_inv` (ceil(O / 128), K / 128) fp32, the factor one multiplies by.  The represented weight
// is the real number e4m3(weight[o, k]) * weight_scale_inv[o / 128, k / 128].
//
//   dequant   one lane per 8 consecutive bytes of a row: round_to_dtype(fp32(e4m3) * scale), the product rounded to fp32 first;
//             one 16-byte store
//   linear    one block of 8 waves per stripe of 16 output rows, orientation and determinism of w4_linear_kernel (kivi_w4.hip): the
//             weight rows are the A operand of v_mfma_f32_16x16x32, the tokens the B operand, straight from L2; the result has the
//             token on lane & 15 and rows 4 (lane >> 4) + i in the registers.  The waves take contiguous runs of the stripe's tiles
//             (kivi_w8_plan.h) and their partial tiles meet in LDS as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).
//   gate_up   the same kernel holding the gate and the up stripe of the same rows: silu(g) * u, rounded once
//
// Operand forming on a row-major weight: a lane's 16-byte load is 16 consecutive k of ONE row, where an MFMA step wants 8 per lane.
// The order in which a step sums k is free as long as both operands agree, so lane (r, kb) reads, for half h of a tile, bytes
// k = 128 tile + 64 h + 16 kb .. + 16: the low 8 are its A fragment of one step against x[k .. k + 8), the high 8 that of the next
// against x[k + 8 .. k + 16) (kivi_w8_plan_step_k).  Two bytes become a packed 16-bit pair in one v_cvt_scalef32_pk_{f16,bf16}_fp8
// at scale 1: every e4m3 value is exact in fp16 and in bf16.  A tile lies inside one 128 x 128 scale block, so the scale is one
// fp32 per (stripe >> 3, tile): yacc = fma(acc_tile, s, yacc) in fp32.
// A token's bits depend on K only: which elements a wave adds, the order, and the tree do not know N, the token's column or the
// other columns.  No atomics.
#include <hip/hip_fp16.h>

#include "kivi_common.h"
#include "kivi_quant.h"
#include "kivi_w8_operand.h"
#include "kivi_w8_plan.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kWaves = KIVI_W8_WAVES;
constexpr int kThreads = kWaves * KIVI_WAVE;

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

// cvt2 / w8_operand (bytes -> an operand fragment in the dtype): kivi_w8_operand.h, shared with the FP8 expert kernel

// ------------------------------------------------------------------------------------------------------------------- dequant
template <bool BF>
__global__ __launch_bounds__(256) void w8_dequant_kernel(const uint8_t* __restrict__ w, const float* __restrict__ scale,
                                                         uint16_t* __restrict__ out, int64_t out_stride, int64_t O, int64_t K) {
    const int64_t cpr = K >> 3;                                        // 8-byte chunks per row
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= O * cpr) return;
    const int64_t o = u / cpr, c = u % cpr;
    const u32x2 b = *reinterpret_cast<const u32x2*>(w + o * K + c * 8);
    const float s = scale[(o >> 7) * (K >> 7) + (c >> 4)];                // kivi_w8_plan_scale_index(o, 8 c, K)
    const u32x4 v = w8_operand<BF>(b[0], b[1]);
    u16x8 r;
#pragma unroll
    for (int e = 0; e < 8; e++) r[e] = to_bits<BF>(from_bits<BF>((uint16_t)(v[e >> 1] >> (16 * (e & 1)))) * s);
    *reinterpret_cast<u16x8*>(out + o * out_stride + c * 8) = r;
}

// --------------------------------------------------------------------------------------------------------------------- linear
template <bool BF>
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ u32x4 ld16(const void* p) { return *reinterpret_cast<const u32x4*>(p); }

// What one wave needs of one tile: per matrix the 2 x 16 bytes of its lane's row and the tile's scale, and 16 bytes per step of
// each of its NT x 16 token rows (x[t][s]: step s, kivi_w8_plan_step_k).
template <int NM, int NT>
struct W8Stage {
    u32x4 w[NM][2];
    float s[NM];
    u32x4 x[NT][4];
    __device__ __forceinline__ void load(bool in, int tile, const uint8_t* const* wr, const float* const* sp, const uint16_t* const* xr,
                                         const bool* live) {
        if (!in) return;                                               // wave-uniform: the tile is past the wave's run
#pragma unroll
        for (int m = 0; m < NM; m++) {
            w[m][0] = ld16(wr[m] + (int64_t)tile * KIVI_W8_K_TILE);
            w[m][1] = ld16(wr[m] + (int64_t)tile * KIVI_W8_K_TILE + 64);
            s[m] = sp[m][tile];
        }
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                x[t][j] = live[t] ? ld16(xr[t] + (int64_t)tile * KIVI_W8_K_TILE + 64 * (j >> 1) + 8 * (j & 1)) : u32x4{0u, 0u, 0u, 0u};
    }
};

// One stripe of 16 output rows over all N tokens, in chunks of 16 NT tokens.
//   x      (N, K) by x_stride;   y (N, O) by y_stride -- GATEUP: O = I, y = silu(gate) * up
//   w / sc     bytes (O, K) and scales (ceil(O / 128), K / 128);  *2: the up matrix (GATEUP only);  bias (O) in the dtype or null
template <bool BF, int NT, bool GATEUP>
__global__ __launch_bounds__(kThreads) void w8_linear_kernel(const uint16_t* __restrict__ x, int64_t x_stride,
                                                             const uint8_t* __restrict__ w, const float* __restrict__ sc,
                                                             const uint8_t* __restrict__ w2, const float* __restrict__ sc2,
                                                             const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                                             int64_t y_stride, int N, int O, int K) {
    constexpr int NM = GATEUP ? 2 : 1;
    constexpr int kRing = NM * NT >= 4 ? 1 : NM * NT == 2 ? 2 : 4;    // tiles requested ahead: what the register file holds
    __shared__ f32x4 red[kWaves - 1][NM * NT][KIVI_WAVE];
    const int lane = threadIdx.x & (KIVI_WAVE - 1), wave = threadIdx.x / KIVI_WAVE;
    const int r = lane & 15, kb = lane >> 4;
    const int tiles = K >> 7;
    const int t0 = (int)((int64_t)tiles * wave / kWaves), t1 = (int)((int64_t)tiles * (wave + 1) / kWaves);
    const int64_t stripe = blockIdx.x;
    const int64_t row = stripe * KIVI_W8_ROW_TILE + r;                 // < O: O is a multiple of 16 and the grid is O / 16
    const int64_t srow = (stripe >> 3) * tiles;                          // kivi_w8_plan_stripe_scale_row: 8 stripes per block-row
    const uint8_t* wr[NM];
    const float* sp[NM];
    wr[0] = w + row * K + 16 * kb;
    sp[0] = sc + srow;
    if constexpr (GATEUP) {
        wr[1] = w2 + row * K + 16 * kb;
        sp[1] = sc2 + srow;
    }
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    for (int n0 = 0; n0 < N; n0 += 16 * NT) {                          // block-uniform
        const uint16_t* xr[NT];
        bool live[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int n = n0 + 16 * t + r;
            live[t] = n < N;
            xr[t] = x + (int64_t)(live[t] ? n : 0) * x_stride + 16 * kb;
        }
        f32x4 yacc[NM][NT];
#pragma unroll
        for (int m = 0; m < NM; m++)
#pragma unroll
            for (int t = 0; t < NT; t++) yacc[m][t] = zero;

        // Everything a tile needs -- its bytes, its scale, the token rows -- is requested kRing tiles ahead, in one order: the memory
        // counter retires loads in order, so a load issued just before its use would make the wave wait for every request before
        // it, the bytes fetched ahead included.
        W8Stage<NM, NT> ring[kRing];
#pragma unroll
        for (int d = 0; d < kRing; d++) ring[d].load(t0 + d < t1, t0 + d, wr, sp, xr, live);

        for (int base = t0; base < t1; base += kRing) {                // wave-uniform
#pragma unroll
            for (int d = 0; d < kRing; d++) {
                const int tile = base + d;
                if (tile >= t1) break;
                W8Stage<NM, NT>& cur = ring[d];
                f32x4 acc[NM][NT];
#pragma unroll
                for (int m = 0; m < NM; m++)
#pragma unroll
                    for (int t = 0; t < NT; t++) acc[m][t] = zero;
#pragma unroll
                for (int j = 0; j < 4; j++) {                          // four steps of 32 reduction elements
                    u32x4 a[NM];
#pragma unroll
                    for (int m = 0; m < NM; m++) a[m] = w8_operand<BF>(cur.w[m][j >> 1][2 * (j & 1)], cur.w[m][j >> 1][2 * (j & 1) + 1]);
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int m = 0; m < NM; m++) acc[m][t] = mfma<BF>(a[m], cur.x[t][j], acc[m][t]);
                }
#pragma unroll
                for (int m = 0; m < NM; m++)
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int i = 0; i < 4; i++) yacc[m][t][i] = __builtin_fmaf(acc[m][t][i], cur.s[m], yacc[m][t][i]);
                cur.load(tile + kRing < t1, tile + kRing, wr, sp, xr, live);
            }
        }

        if (wave > 0) {
#pragma unroll
            for (int m = 0; m < NM; m++)
#pragma unroll
                for (int t = 0; t < NT; t++) red[wave - 1][m * NT + t][lane] = yacc[m][t];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < NT; t++) {
                f32x4 v[NM];
#pragma unroll
                for (int m = 0; m < NM; m++) {
                    const int q = m * NT + t;
                    v[m] = ((yacc[m][t] + red[0][q][lane]) + (red[1][q][lane] + red[2][q][lane])) +
                           ((red[3][q][lane] + red[4][q][lane]) + (red[5][q][lane] + red[6][q][lane]));
                }
                const int n = n0 + 16 * t + r;
                if (n < N) {
                    const int o0 = (int)stripe * KIVI_W8_ROW_TILE + 4 * kb;      // lane: token n, rows o0 .. o0 + 3
                    uint16_t h[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        if constexpr (GATEUP) {
                            const float g = v[0][i];
                            h[i] = to_bits<BF>(g / (1.0f + expf(-g)) * v[1][i]);
                        } else {
                            h[i] = to_bits<BF>(bias ? v[0][i] + from_bits<BF>(bias[o0 + i]) : v[0][i]);
                        }
                    }
                    const u32x2 out = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
                    *reinterpret_cast<u32x2*>(y + (int64_t)n * y_stride + o0) = out;
                }
            }
        }
        __syncthreads();                                               // the next chunk writes `red` again
    }
}

template <bool BF, bool GATEUP>
void w8_launch(int nt, dim3 grid, hipStream_t s, const uint16_t* x, int64_t x_stride, const uint8_t* w, const float* sc, const uint8_t* w2,
               const float* sc2, const uint16_t* bias, uint16_t* y, int64_t y_stride, int N, int O, int K) {
    if (nt == 1)
        KIVI_LAUNCH((w8_linear_kernel<BF, 1, GATEUP>), grid, dim3(kThreads), s, x, x_stride, w, sc, w2, sc2, bias, y, y_stride, N, O, K);
    else if (nt == 2)
        KIVI_LAUNCH((w8_linear_kernel<BF, 2, GATEUP>), grid, dim3(kThreads), s, x, x_stride, w, sc, w2, sc2, bias, y, y_stride, N, O, K);
    else if constexpr (!GATEUP)                                        // (gate_up carries two matrices: at most two token tiles)
        KIVI_LAUNCH((w8_linear_kernel<BF, 4, GATEUP>), grid, dim3(kThreads), s, x, x_stride, w, sc, w2, sc2, bias, y, y_stride, N, O, K);
}

int w8_check_matrix(const char* what, int dtype, int O, int K) {
    KIVI_REQUIRE(kivi_w8_plan_dtype_ok(dtype), KIVI_EINVAL, "%s: dtype=%d (16: fp16, 0x110: bf16)", what, dtype);
    KIVI_REQUIRE(kivi_w8_plan_shape_ok(O, K), KIVI_EINVAL, "%s: O=%d K=%d (O a positive multiple of 16, K of 128, O * K < 2^40)", what, O,
                 K);
    return 0;
}

int w8_run(const char* what, bool gate_up, const void* x, int64_t x_stride, int dtype, int N, int O, int K, const void* w1, const void* s1,
           const void* w2, const void* s2, const void* bias, void* y, int64_t y_stride, kivi_stream_t stream) {
    if (const int rc = w8_check_matrix(what, dtype, O, K)) return rc;
    KIVI_REQUIRE(kivi_w8_plan_tokens_ok(N, O), KIVI_EINVAL, "%s: N=%d O=%d (N >= 1, N * O < 2^31)", what, N, O);
    KIVI_REQUIRE(x_stride >= K && y_stride >= O, KIVI_EINVAL, "%s: x_stride=%lld < K=%d or y_stride=%lld < O=%d", what,
                 (long long)x_stride, K, (long long)y_stride, O);
    KIVI_REQUIRE(x && w1 && s1 && y && (!gate_up || (w2 && s2)), KIVI_EINVAL, "%s: null x, weight, scales or y", what);
    for (const void* p : {x, w1, w2})
        KIVI_REQUIRE((uintptr_t)p % 16 == 0, KIVI_EALIGN, "%s: x or weight off 16 bytes", what);
    KIVI_REQUIRE((uintptr_t)s1 % 4 == 0 && (uintptr_t)s2 % 4 == 0 && (uintptr_t)y % 8 == 0, KIVI_EALIGN,
                 "%s: scales off 4 bytes or y off 8", what);
    KIVI_REQUIRE((uintptr_t)bias % 2 == 0 && x_stride % 8 == 0 && y_stride % 4 == 0, KIVI_EALIGN,
                 "%s: bias off 2 bytes, x_stride=%lld not a multiple of 8 or y_stride=%lld not of 4", what, (long long)x_stride,
                 (long long)y_stride);
    const dim3 grid((unsigned)kivi_w8_plan_stripes(O));
    const int nt = kivi_w8_plan_token_tiles(N, gate_up);
    hipStream_t s = (hipStream_t)stream;
#define KIVI_W8_ARGS                                                                                                                  \
    nt, grid, s, (const uint16_t*)x, x_stride, (const uint8_t*)w1, (const float*)s1, (const uint8_t*)w2, (const float*)s2,            \
        (const uint16_t*)bias, (uint16_t*)y, y_stride, N, O, K
    if (dtype == KIVI_W8_BF16) {
        if (gate_up) w8_launch<true, true>(KIVI_W8_ARGS);
        else w8_launch<true, false>(KIVI_W8_ARGS);
    } else {
        if (gate_up) w8_launch<false, true>(KIVI_W8_ARGS);
        else w8_launch<false, false>(KIVI_W8_ARGS);
    }
#undef KIVI_W8_ARGS
    return kivi_launch_status(what);
}

}  // namespace

extern "C" int64_t kivi_w8_bytes(int O, int K) {
    const int64_t b = kivi_w8_plan_bytes(O, K);
    KIVI_REQUIRE(b >= 0, KIVI_EINVAL, "kivi_w8_bytes: O=%d K=%d (O a positive multiple of 16, K of 128)", O, K);
    return b;
}

extern "C" int kivi_w8_dequant(const void* weight, const void* scale_inv, int O, int K, int dtype, void* out, int64_t out_stride,
                               kivi_stream_t stream) {
    if (const int rc = w8_check_matrix("kivi_w8_dequant", dtype, O, K)) return rc;
    KIVI_REQUIRE(out_stride >= K, KIVI_EINVAL, "kivi_w8_dequant: out_stride=%lld < K=%d", (long long)out_stride, K);
    KIVI_REQUIRE(out && weight && scale_inv, KIVI_EINVAL, "kivi_w8_dequant: null weight, scale_inv or out");
    KIVI_REQUIRE((uintptr_t)out % 16 == 0 && out_stride % 8 == 0 && (uintptr_t)weight % 16 == 0 && (uintptr_t)scale_inv % 4 == 0,
                 KIVI_EALIGN, "kivi_w8_dequant: out or weight off 16 bytes, out_stride=%lld not a multiple of 8 or scale_inv off 4 bytes",
                 (long long)out_stride);
    const dim3 grid((unsigned)kivi_w8_plan_elem_blocks(O, K));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KIVI_W8_BF16)
        KIVI_LAUNCH(w8_dequant_kernel<true>, grid, dim3(256), s, (const uint8_t*)weight, (const float*)scale_inv, (uint16_t*)out,
                    out_stride, (int64_t)O, (int64_t)K);
    else
        KIVI_LAUNCH(w8_dequant_kernel<false>, grid, dim3(256), s, (const uint8_t*)weight, (const float*)scale_inv, (uint16_t*)out,
                    out_stride, (int64_t)O, (int64_t)K);
    return kivi_launch_status("kivi_w8_dequant");
}

extern "C" int kivi_w8_linear(const void* x, int64_t x_stride, int dtype, int N, int O, int K, const void* weight, const void* scale_inv,
                              const void* bias, void* y, int64_t y_stride, kivi_stream_t stream) {
    return w8_run("kivi_w8_linear", false, x, x_stride, dtype, N, O, K, weight, scale_inv, nullptr, nullptr, bias, y, y_stride, stream);
}

extern "C" int kivi_w8_gate_up(const void* x, int64_t x_stride, int dtype, int N, int I, int K, const void* gate_weight,
                               const void* gate_scale_inv, const void* up_weight, const void* up_scale_inv, void* y, int64_t y_stride,
                               kivi_stream_t stream) {
    return w8_run("kivi_w8_gate_up", true, x, x_stride, dtype, N, I, K, gate_weight, gate_scale_inv, up_weight, up_scale_inv, nullptr, y,
                  y_stride, stream);
}
