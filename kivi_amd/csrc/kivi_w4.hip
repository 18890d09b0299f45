// kivi_w4_pack / kivi_w4_dequant / kivi_w4_linear / kivi_w4_gate_up (include/kivi_hip.h): weight-only 4-bit,
// group-wise asymmetric dense layers.  The codes, scales and zero points are the reference's last-dim quantiser's (kivi_quant.h) for
// the fp16 image of the weight; the layout ("WT4", kivi_mfma_layout.h) makes a wave's 16-byte load per lane the A operands of four
// v_mfma_f32_16x16x32 after one shift and one mask per register.
//
//   pack      one lane per 8 consecutive elements of a row; the G / 8 lanes of a group meet through shuffles; W is read once
//   dequant   one lane per code word: 8 elements round(fmaf(code, scale, mn)) of a dense row, one 16-byte store
//   linear    one block of 8 waves per stripe of 16 output rows.  Orientation of moe_gemm_kernel: the weight
//             rows are the A operand, the tokens the B operand, straight from L2; the result has the token on lane & 15 and rows
//             4 (lane >> 4) + i in the registers.  The waves take contiguous runs of the stripe's tiles (kivi_w4_plan.h) and their
//             partial tiles meet in LDS as ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).
//   gate_up   the same kernel holding the gate and the up stripe of the same rows: silu(g) * u, rounded once
//
// The codes stay INTEGERS in the operand (the factored form): per 64 reduction elements (a group, or half of one at G = 128)
//     y += s * sum_k c'(k) x(k)  +  z * sum_k x(k)
// with both sums on the matrix pipe in fp32 (the second against an A operand of ones: it lands in the result layout, so no lane
// exchange and no workspace) and two fused multiply-adds per output in fp32:
//   fp16   c' = code * 2^-18, an fp16 subnormal with the code at the top of the mantissa (docs/4bit_matrix_pipe.md): s = scale * 2^18,
//          z = mn
//   bf16   c' = 128 + code, exact in bf16's 8 significant bits (0x4300 | code):   s = scale, z = mn - 128 scale
// A token's bits depend on K and G only: which elements a wave adds, the order, and the tree do not know N, the token's column or
// the other columns.  No atomics.
#include <hip/hip_fp16.h>

#include "kivi_common.h"
#include "kivi_mfma_layout.h"
#include "kivi_quant.h"
#include "kivi_w4_plan.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kWaves = KIVI_W4_WAVES;
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

// -------------------------------------------------------------------------------------------------------------- pack / dequant
// chunk c = 8 consecutive elements of row o: tile c / 16, and inside the tile's 128 elements 32 j + 8 kb + e with j = (c % 16) / 4,
// kb = c % 4.  The field of element e sits at bits 4 (e >> 1) + 16 (e & 1).
__device__ __forceinline__ int64_t wt4_word(int64_t o, int64_t c, int64_t tiles) {
    return ((o >> 4) * tiles + (c >> 4)) * KIVI_W4_TILE_WORDS + ((o & 15) + 16 * (c & 3)) * 4 + ((c >> 2) & 3);
}

template <bool BF>
__global__ __launch_bounds__(256) void w4_pack_kernel(const uint16_t* __restrict__ w, int64_t w_stride, uint32_t* __restrict__ code,
                                                      uint16_t* __restrict__ scale, uint16_t* __restrict__ mn, int64_t O, int64_t K,
                                                      int gshift) {
    const int64_t cpr = K >> 3;                                        // chunks per row (a multiple of 16)
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = u < O * cpr;                                    // whole groups fall out together (cpr % 16 == 0)
    const int64_t o = valid ? u / cpr : 0, c = valid ? u % cpr : 0;
    u16x8 v = *reinterpret_cast<const u16x8*>(w + o * w_stride + c * 8);
    if constexpr (BF) {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = f2h_bits((float)bf16{v[i]});          // the fp16 image: one rounding, to nearest even
    }
    uint32_t kmin = 0xFFFFu, kmax = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t k = h_key(v[i]);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
    }
    const int lpg = 1 << (gshift - 3);                                 // lanes per group: 8 or 16
    for (int m = 1; m < lpg; m <<= 1) {
        const uint32_t omin = __shfl_xor(kmin, m), omax = __shfl_xor(kmax, m);
        kmin = omin < kmin ? omin : kmin;
        kmax = omax > kmax ? omax : kmax;
    }
    const GroupQ g = make_group(kmin, kmax, 15);
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) word |= quant_one<4>(v[e], g) << (4 * (e >> 1) + 16 * (e & 1));
    if (!valid) return;
    code[wt4_word(o, c, K >> 7)] = word;
    if ((c & (lpg - 1)) == 0) {
        const int64_t h = ((o >> 4) * (K >> gshift) + (c >> (gshift - 3))) * 16 + (o & 15);
        scale[h] = g.scale;
        mn[h] = g.mn;
    }
}

template <bool BF>
__global__ __launch_bounds__(256) void w4_dequant_kernel(const uint32_t* __restrict__ code, const uint16_t* __restrict__ scale,
                                                         const uint16_t* __restrict__ mn, uint16_t* __restrict__ out,
                                                         int64_t out_stride, int64_t O, int64_t K, int gshift) {
    const int64_t cpr = K >> 3;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= O * cpr) return;
    const int64_t o = u / cpr, c = u % cpr;
    const uint32_t word = code[wt4_word(o, c, K >> 7)];
    const int64_t h = ((o >> 4) * (K >> gshift) + (c >> (gshift - 3))) * 16 + (o & 15);
    const float s = h2f_bits(scale[h]), z = h2f_bits(mn[h]);
    u16x8 r;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const float q = (float)((word >> (4 * (e >> 1) + 16 * (e & 1))) & 15u);
        r[e] = to_bits<BF>(__builtin_fmaf(q, s, z));
    }
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

// the A operand of one 32-element step from its code word: register i holds elements 2 i (low half) and 2 i + 1
template <bool BF>
__device__ __forceinline__ u32x4 w4_views(uint32_t w) {
    if constexpr (BF)
        return u32x4{(w & 0x000F000Fu) | 0x43004300u, ((w >> 4) & 0x000F000Fu) | 0x43004300u, ((w >> 8) & 0x000F000Fu) | 0x43004300u,
                     ((w >> 12) & 0x000F000Fu) | 0x43004300u};
    else
        return u32x4{(w << 6) & 0x03C003C0u, (w << 2) & 0x03C003C0u, (w >> 2) & 0x03C003C0u, (w >> 6) & 0x03C003C0u};
}

// the factors (s, z) of the four output rows of a lane from the 4 + 4 halves of its group
template <bool BF>
__device__ __forceinline__ void w4_factors(u32x2 sb, u32x2 mb, float* s, float* z) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float sc = h2f_bits((uint16_t)(sb[i >> 1] >> (16 * (i & 1)))), m = h2f_bits((uint16_t)(mb[i >> 1] >> (16 * (i & 1))));
        if constexpr (BF) {
            s[i] = sc;
            z[i] = __builtin_fmaf(-128.0f, sc, m);
        } else {
            s[i] = sc * 262144.0f;
            z[i] = m;
        }
    }
}

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// What one wave needs of one tile: the code words of its NM matrices, the scales and zero points of the groups of the tile's two
// halves (the same group at G = 128), 16 bytes per step of each of its NT x 16 token rows.
template <int NM, int NT>
struct W4Stage {
    u32x4 w[NM];
    u32x2 sb[NM][2], mb[NM][2];
    u32x4 x[NT][4];
    __device__ __forceinline__ void load(bool in, int tile, int gpt, const u32x4* const* wq, const uint16_t* const* sp,
                                         const uint16_t* const* mp, const uint16_t* const* xr, const bool* live) {
        if (!in) return;                                               // wave-uniform: the tile is past the wave's run
#pragma unroll
        for (int m = 0; m < NM; m++) {
            w[m] = wq[m][(int64_t)tile * KIVI_WAVE];
            sb[m][0] = *reinterpret_cast<const u32x2*>(sp[m] + (int64_t)(tile * gpt) * 16);
            mb[m][0] = *reinterpret_cast<const u32x2*>(mp[m] + (int64_t)(tile * gpt) * 16);
            sb[m][1] = *reinterpret_cast<const u32x2*>(sp[m] + (int64_t)(tile * gpt + gpt - 1) * 16);
            mb[m][1] = *reinterpret_cast<const u32x2*>(mp[m] + (int64_t)(tile * gpt + gpt - 1) * 16);
        }
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int j = 0; j < 4; j++) x[t][j] = live[t] ? ld16(xr[t] + (int64_t)tile * 128 + 32 * j) : u32x4{0u, 0u, 0u, 0u};
    }
};

// One stripe of 16 output rows over all N tokens, in chunks of 16 NT tokens.
//   x      (N, K) by x_stride;   y (N, O) by y_stride -- GATEUP: O = I, y = silu(gate) * up
//   qw / sc / mz    codes, scales, zero points (WT4);  *2: the up matrix (GATEUP only);  bias (O) in the dtype or null
template <bool BF, int NT, bool GATEUP>
__global__ __launch_bounds__(kThreads) void w4_linear_kernel(const uint16_t* __restrict__ x, int64_t x_stride,
                                                             const uint32_t* __restrict__ qw, const uint16_t* __restrict__ sc,
                                                             const uint16_t* __restrict__ mz, const uint32_t* __restrict__ qw2,
                                                             const uint16_t* __restrict__ sc2, const uint16_t* __restrict__ mz2,
                                                             const uint16_t* __restrict__ bias, uint16_t* __restrict__ y,
                                                             int64_t y_stride, int N, int O, int K, int gshift) {
    constexpr int NM = GATEUP ? 2 : 1;
    constexpr int kRing = NM * NT >= 4 ? 1 : NM * NT == 2 ? 2 : 4;    // tiles requested ahead: what the register file holds
    __shared__ f32x4 red[kWaves - 1][NM * NT][KIVI_WAVE];
    const int lane = threadIdx.x & (KIVI_WAVE - 1), wave = threadIdx.x / KIVI_WAVE;
    const int r = lane & 15, kb = lane >> 4;
    const int tiles = K >> 7, gpt = 128 >> gshift;                     // groups per tile: 1 or 2
    const int t0 = (int)((int64_t)tiles * wave / kWaves), t1 = (int)((int64_t)tiles * (wave + 1) / kWaves);
    const int64_t stripe = blockIdx.x;
    const u32x4* wq[NM];
    const uint16_t* sp[NM];
    const uint16_t* mp[NM];
    wq[0] = reinterpret_cast<const u32x4*>(qw) + stripe * tiles * KIVI_WAVE + lane;
    sp[0] = sc + stripe * (K >> gshift) * 16 + 4 * kb;
    mp[0] = mz + stripe * (K >> gshift) * 16 + 4 * kb;
    if constexpr (GATEUP) {
        wq[1] = reinterpret_cast<const u32x4*>(qw2) + stripe * tiles * KIVI_WAVE + lane;
        sp[1] = sc2 + stripe * (K >> gshift) * 16 + 4 * kb;
        mp[1] = mz2 + stripe * (K >> gshift) * 16 + 4 * kb;
    }
    const u32x4 ones = BF ? u32x4{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u}
                          : u32x4{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u};
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

    for (int n0 = 0; n0 < N; n0 += 16 * NT) {                          // block-uniform
        const uint16_t* xr[NT];
        bool live[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int n = n0 + 16 * t + r;
            live[t] = n < N;
            xr[t] = x + (int64_t)(live[t] ? n : 0) * x_stride + 8 * kb;
        }
        f32x4 yacc[NM][NT];
#pragma unroll
        for (int m = 0; m < NM; m++)
#pragma unroll
            for (int t = 0; t < NT; t++) yacc[m][t] = zero;

        // Everything a tile needs -- its code words, the scales and zero points of its two halves, the token rows -- is requested
        // kRing tiles ahead, in one order: the memory counter retires loads in order, so a load issued just before its use would
        // make the wave wait for every request before it, the codes fetched ahead included.
        W4Stage<NM, NT> ring[kRing];
#pragma unroll
        for (int d = 0; d < kRing; d++) ring[d].load(t0 + d < t1, t0 + d, gpt, wq, sp, mp, xr, live);

        for (int base = t0; base < t1; base += kRing) {                // wave-uniform
#pragma unroll
            for (int d = 0; d < kRing; d++) {
                const int tile = base + d;
                if (tile >= t1) break;
                W4Stage<NM, NT>& cur = ring[d];
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {                       // 64 reduction elements: two steps of 32
                    f32x4 acc[NM][NT], sx[NT];
#pragma unroll
                    for (int t = 0; t < NT; t++) {
                        sx[t] = zero;
#pragma unroll
                        for (int m = 0; m < NM; m++) acc[m][t] = zero;
                    }
#pragma unroll
                    for (int jj = 0; jj < 2; jj++) {
                        const int j = 2 * hf + jj;
                        u32x4 a[NM];
#pragma unroll
                        for (int m = 0; m < NM; m++) a[m] = w4_views<BF>(cur.w[m][j]);
#pragma unroll
                        for (int t = 0; t < NT; t++) {
#pragma unroll
                            for (int m = 0; m < NM; m++) acc[m][t] = mfma<BF>(a[m], cur.x[t][j], acc[m][t]);
                            sx[t] = mfma<BF>(ones, cur.x[t][j], sx[t]);
                        }
                    }
#pragma unroll
                    for (int m = 0; m < NM; m++) {
                        float s[4], z[4];
                        w4_factors<BF>(cur.sb[m][hf], cur.mb[m][hf], s, z);
#pragma unroll
                        for (int t = 0; t < NT; t++)
#pragma unroll
                            for (int i = 0; i < 4; i++)
                                yacc[m][t][i] = __builtin_fmaf(sx[t][i], z[i], __builtin_fmaf(acc[m][t][i], s[i], yacc[m][t][i]));
                    }
                }
                cur.load(tile + kRing < t1, tile + kRing, gpt, wq, sp, mp, xr, live);
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
                    const int o0 = (int)stripe * KIVI_W4_ROW_TILE + 4 * kb;      // lane: token n, rows o0 .. o0 + 3
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
void w4_launch(int nt, dim3 grid, hipStream_t s, const uint16_t* x, int64_t x_stride, const uint32_t* qw, const uint16_t* sc,
               const uint16_t* mz, const uint32_t* qw2, const uint16_t* sc2, const uint16_t* mz2, const uint16_t* bias, uint16_t* y,
               int64_t y_stride, int N, int O, int K, int gshift) {
    if (nt == 1)
        KIVI_LAUNCH((w4_linear_kernel<BF, 1, GATEUP>), grid, dim3(kThreads), s, x, x_stride, qw, sc, mz, qw2, sc2, mz2, bias, y, y_stride,
                    N, O, K, gshift);
    else if (nt == 2)
        KIVI_LAUNCH((w4_linear_kernel<BF, 2, GATEUP>), grid, dim3(kThreads), s, x, x_stride, qw, sc, mz, qw2, sc2, mz2, bias, y, y_stride,
                    N, O, K, gshift);
    else if constexpr (!GATEUP)                                        // (gate_up carries two matrices: at most two token tiles)
        KIVI_LAUNCH((w4_linear_kernel<BF, 4, GATEUP>), grid, dim3(kThreads), s, x, x_stride, qw, sc, mz, qw2, sc2, mz2, bias, y, y_stride,
                    N, O, K, gshift);
}

int w4_check_matrix(const char* what, int dtype, int O, int K, int group) {
    KIVI_REQUIRE(kivi_w4_plan_dtype_ok(dtype), KIVI_EINVAL, "%s: dtype=%d (16: fp16, 0x110: bf16)", what, dtype);
    KIVI_REQUIRE(kivi_w4_plan_shape_ok(O, K, group), KIVI_EINVAL, "%s: O=%d K=%d group=%d (O a positive multiple of 16, K of 128, group 64 "
                 "or 128, O * K < 2^40)", what, O, K, group);
    return 0;
}

int w4_run(const char* what, bool gate_up, const void* x, int64_t x_stride, int dtype, int N, int O, int K, int group, const void* q1,
           const void* s1, const void* m1, const void* q2, const void* s2, const void* m2, const void* bias, void* y, int64_t y_stride,
           kivi_stream_t stream) {
    if (const int rc = w4_check_matrix(what, dtype, O, K, group)) return rc;
    KIVI_REQUIRE(kivi_w4_plan_tokens_ok(N, O), KIVI_EINVAL, "%s: N=%d O=%d (N >= 1, N * O < 2^31)", what, N, O);
    KIVI_REQUIRE(x_stride >= K && y_stride >= O, KIVI_EINVAL, "%s: x_stride=%lld < K=%d or y_stride=%lld < O=%d", what,
                 (long long)x_stride, K, (long long)y_stride, O);
    KIVI_REQUIRE(x && q1 && s1 && m1 && y && (!gate_up || (q2 && s2 && m2)), KIVI_EINVAL, "%s: null x, codes, scales, mins or y", what);
    for (const void* p : {x, q1, q2})
        KIVI_REQUIRE((uintptr_t)p % 16 == 0, KIVI_EALIGN, "%s: x or codes off 16 bytes", what);
    for (const void* p : {s1, m1, s2, m2, (const void*)y})
        KIVI_REQUIRE((uintptr_t)p % 8 == 0, KIVI_EALIGN, "%s: scales, mins or y off 8 bytes", what);
    KIVI_REQUIRE((uintptr_t)bias % 2 == 0 && x_stride % 8 == 0 && y_stride % 4 == 0, KIVI_EALIGN,
                 "%s: bias off 2 bytes, x_stride=%lld not a multiple of 8 or y_stride=%lld not of 4", what, (long long)x_stride,
                 (long long)y_stride);
    const dim3 grid((unsigned)kivi_w4_plan_stripes(O));
    const int nt = kivi_w4_plan_token_tiles(N, gate_up), gshift = group == 64 ? 6 : 7;
    hipStream_t s = (hipStream_t)stream;
#define KIVI_W4_ARGS                                                                                                                  \
    nt, grid, s, (const uint16_t*)x, x_stride, (const uint32_t*)q1, (const uint16_t*)s1, (const uint16_t*)m1, (const uint32_t*)q2,    \
        (const uint16_t*)s2, (const uint16_t*)m2, (const uint16_t*)bias, (uint16_t*)y, y_stride, N, O, K, gshift
    if (dtype == KIVI_W4_BF16) {
        if (gate_up) w4_launch<true, true>(KIVI_W4_ARGS);
        else w4_launch<true, false>(KIVI_W4_ARGS);
    } else {
        if (gate_up) w4_launch<false, true>(KIVI_W4_ARGS);
        else w4_launch<false, false>(KIVI_W4_ARGS);
    }
#undef KIVI_W4_ARGS
    return kivi_launch_status(what);
}

}  // namespace

extern "C" int64_t kivi_w4_bytes(int O, int K, int group) {
    const int64_t b = kivi_w4_plan_bytes(O, K, group);
    KIVI_REQUIRE(b >= 0, KIVI_EINVAL, "kivi_w4_bytes: O=%d K=%d group=%d (O a positive multiple of 16, K of 128, group 64 or 128)", O, K,
                 group);
    return b;
}

extern "C" int kivi_w4_pack(const void* w, int64_t w_stride, int dtype, int O, int K, int group, void* qweight, void* scales, void* mins,
                            kivi_stream_t stream) {
    if (const int rc = w4_check_matrix("kivi_w4_pack", dtype, O, K, group)) return rc;
    KIVI_REQUIRE(w_stride >= K, KIVI_EINVAL, "kivi_w4_pack: w_stride=%lld < K=%d", (long long)w_stride, K);
    KIVI_REQUIRE(w && qweight && scales && mins, KIVI_EINVAL, "kivi_w4_pack: null w, qweight, scales or mins");
    KIVI_REQUIRE((uintptr_t)w % 16 == 0 && w_stride % 8 == 0 && (uintptr_t)qweight % 16 == 0 && (uintptr_t)scales % 8 == 0 &&
                 (uintptr_t)mins % 8 == 0, KIVI_EALIGN, "kivi_w4_pack: w or qweight off 16 bytes, w_stride=%lld not a multiple of 8, "
                 "scales or mins off 8 bytes", (long long)w_stride);
    const dim3 grid((unsigned)kivi_w4_plan_elem_blocks(O, K));
    hipStream_t s = (hipStream_t)stream;
    const int gshift = group == 64 ? 6 : 7;
    if (dtype == KIVI_W4_BF16)
        KIVI_LAUNCH(w4_pack_kernel<true>, grid, dim3(256), s, (const uint16_t*)w, w_stride, (uint32_t*)qweight, (uint16_t*)scales,
                    (uint16_t*)mins, (int64_t)O, (int64_t)K, gshift);
    else
        KIVI_LAUNCH(w4_pack_kernel<false>, grid, dim3(256), s, (const uint16_t*)w, w_stride, (uint32_t*)qweight, (uint16_t*)scales,
                    (uint16_t*)mins, (int64_t)O, (int64_t)K, gshift);
    return kivi_launch_status("kivi_w4_pack");
}

extern "C" int kivi_w4_dequant(const void* qweight, const void* scales, const void* mins, int O, int K, int group, int dtype, void* out,
                               int64_t out_stride, kivi_stream_t stream) {
    if (const int rc = w4_check_matrix("kivi_w4_dequant", dtype, O, K, group)) return rc;
    KIVI_REQUIRE(out_stride >= K, KIVI_EINVAL, "kivi_w4_dequant: out_stride=%lld < K=%d", (long long)out_stride, K);
    KIVI_REQUIRE(out && qweight && scales && mins, KIVI_EINVAL, "kivi_w4_dequant: null qweight, scales, mins or out");
    KIVI_REQUIRE((uintptr_t)out % 16 == 0 && out_stride % 8 == 0 && (uintptr_t)qweight % 16 == 0 && (uintptr_t)scales % 8 == 0 &&
                 (uintptr_t)mins % 8 == 0, KIVI_EALIGN, "kivi_w4_dequant: out or qweight off 16 bytes, out_stride=%lld not a multiple "
                 "of 8, scales or mins off 8 bytes", (long long)out_stride);
    const dim3 grid((unsigned)kivi_w4_plan_elem_blocks(O, K));
    hipStream_t s = (hipStream_t)stream;
    const int gshift = group == 64 ? 6 : 7;
    if (dtype == KIVI_W4_BF16)
        KIVI_LAUNCH(w4_dequant_kernel<true>, grid, dim3(256), s, (const uint32_t*)qweight, (const uint16_t*)scales, (const uint16_t*)mins,
                    (uint16_t*)out, out_stride, (int64_t)O, (int64_t)K, gshift);
    else
        KIVI_LAUNCH(w4_dequant_kernel<false>, grid, dim3(256), s, (const uint32_t*)qweight, (const uint16_t*)scales, (const uint16_t*)mins,
                    (uint16_t*)out, out_stride, (int64_t)O, (int64_t)K, gshift);
    return kivi_launch_status("kivi_w4_dequant");
}

extern "C" int kivi_w4_linear(const void* x, int64_t x_stride, int dtype, int N, int O, int K, int group, const void* qweight,
                              const void* scales, const void* mins, const void* bias, void* y, int64_t y_stride, kivi_stream_t stream) {
    return w4_run("kivi_w4_linear", false, x, x_stride, dtype, N, O, K, group, qweight, scales, mins, nullptr, nullptr, nullptr, bias, y,
                  y_stride, stream);
}

extern "C" int kivi_w4_gate_up(const void* x, int64_t x_stride, int dtype, int N, int I, int K, int group, const void* gate_qweight,
                               const void* gate_scales, const void* gate_mins, const void* up_qweight, const void* up_scales,
                               const void* up_mins, void* y, int64_t y_stride, kivi_stream_t stream) {
    return w4_run("kivi_w4_gate_up", true, x, x_stride, dtype, N, I, K, group, gate_qweight, gate_scales, gate_mins, up_qweight,
                  up_scales, up_mins, nullptr, y, y_stride, stream);
}
