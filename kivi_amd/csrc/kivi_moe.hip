// kivi_moe_route / kivi_moe_experts (include/kivi_hip.h): the sparse mixture-of-experts feed-forward block of
// Mixtral / Qwen3-MoE as launches that never report to the host, so that a decode step holding one can be captured.
// kivi_moe_experts_w8 (section 36): the same three launches over experts held as block-scaled e4m3fn bytes (moe_gemm_w8_kernel).
//
//   route     one wave per token: the K largest logits (ties to the lower expert), their softmax weights, a count per expert;
//             then one block: the prefix sums, the tile list and the grouping of the pairs by expert
//   gate/up   one block per (tile of <= 16 pairs of one expert, 16 rows of I): a = silu(x Wg^T) * (x Wu^T) on the matrix pipe
//   down      one block per (tile, 16 rows of H): y_pair = a Wd^T in fp32
//   combine   out[n] = sum_k w[n, k] * y_pair[pos[n, k]] in slot order, rounded once
//
// Matrix-pipe orientation (v_mfma_f32_16x16x32_f16 / _bf16): the 16 weight rows are the A operand, the tile's 16 token rows the B
// operand.  Lane (r = lane & 15, kb = lane >> 4) feeds elements 8 kb .. 8 kb + 7 of a 32-element step of row r: 16 contiguous bytes
// of a weight row (A) or of a token row (B), so both operands are one 16-byte load per lane straight from memory.  The result has
// the token on the lane (lane & 15) and four consecutive weight rows in the registers (4 (lane >> 4) + j).
//
// The four waves of a block SPLIT THE REDUCTION AXIS: wave w takes the 128-element stretches w, w + 4, w + 8, ... of the rows, and
// the four partial tiles are added as (w0 + w1) + (w2 + w3) through LDS.  A one-token Mixtral step is then 2 x 896 + 2 x 256 blocks
// and a Qwen3-30B-A3B one 8 x 48 + 8 x 128: the weight stream is spread over every CU.  No two waves read the same element of x, so
// an LDS stage of the token rows would be written and read by one wave only: they go from L2 into the B operand directly (columns
// past the tile's rows are not loaded at all: a one-token step reads one row).  What a pair's sum looks like -- which elements a
// wave adds, in which order, and how the four partials meet -- is a function of H and I alone: not of the pair's column in its
// tile, of N, or of the other tokens.  A token has the same bits whatever else is in the batch.
#include <hip/hip_fp16.h>

#include "kivi_common.h"
#include "kivi_moe_plan.h"
#include "kivi_moe_w8_plan.h"
#include "kivi_w8_operand.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / KIVI_WAVE;
constexpr int kTile = KIVI_MOE_TOKEN_TILE;

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

// ------------------------------------------------------------------------------------------------------------------- route
// A float as an unsigned key of the same order (-0 has been made +0 by the caller: equal logits have equal keys), and back.
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

template <bool BF>
__global__ __launch_bounds__(kThreads) void moe_route_kernel(const uint16_t* __restrict__ logits, int64_t row_stride, int N, int E, int K,
                                                             int flags, int* __restrict__ idx, float* __restrict__ w,
                                                             int* __restrict__ counts, int* __restrict__ pos) {
    const int lane = threadIdx.x & (KIVI_WAVE - 1);
    const int64_t n = (int64_t)blockIdx.x * kWaves + threadIdx.x / KIVI_WAVE;          // wave-uniform
    if (n >= N) return;
    const uint16_t* row = logits + n * row_stride;
    // lane l holds experts l, l + 64, l + 128, l + 192: key << 32 | ~expert, so that the maximum is the largest logit at the lowest
    // expert; a slot past E or already taken is 0, below every live one
    uint64_t cand[4];
    float v[4], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e = lane + 64 * j;
        v[j] = e < E ? from_bits<BF>(row[e]) + 0.0f : -INFINITY;
        cand[j] = e < E ? ((uint64_t)key_of(v[j]) << 32) | (uint32_t)(0xFFFFFFFFu - e) : 0ull;
        mx = __builtin_fmaxf(mx, v[j]);
    }
#pragma unroll
    for (int m = 1; m < KIVI_WAVE; m <<= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, m));
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) sum += lane + 64 * j < E ? expf(v[j] - mx) : 0.0f;
#pragma unroll
    for (int m = 1; m < KIVI_WAVE; m <<= 1) sum += __shfl_xor(sum, m);
    int my_e = 0;
    float my_p = 0.0f;
    for (int k = 0; k < K; k++) {                           // K <= E: every round finds a live slot
        uint64_t best = cand[0];
#pragma unroll
        for (int j = 1; j < 4; j++) best = cand[j] > best ? cand[j] : best;
#pragma unroll
        for (int m = 1; m < KIVI_WAVE; m <<= 1) {
            const uint64_t o = __shfl_xor(best, m);
            best = o > best ? o : best;
        }
        int e = (int)(0xFFFFFFFFu - (uint32_t)best);
        e = e < E ? e : E - 1;                              // (cannot happen; keeps every index the later kernels use inside E)
        const float p = expf(value_of((uint32_t)(best >> 32)) - mx) / sum;
        if (lane == k) my_e = e, my_p = p;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (lane + 64 * j == e) cand[j] = 0ull;
    }
    if (flags & KIVI_MOE_NORM_TOPK) {
        float s = 0.0f;
        for (int k = 0; k < K; k++) s += __shfl(my_p, k);   // slot order
        my_p = my_p / s;
    }
    if (flags & KIVI_MOE_ROUND_WEIGHTS) my_p = from_bits<BF>(to_bits<BF>(my_p));
    if (lane < K) {
        idx[n * K + lane] = my_e;
        w[n * K + lane] = my_p;
        pos[n * K + lane] = atomicAdd(&counts[my_e], 1);    // the pair's rank inside its expert; moe_plan_kernel adds the offset
    }
}

// exclusive prefix sum of one value per thread over the block (256 threads), and the total
__device__ __forceinline__ int block_scan(int v, int* lds, int* total) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    *total = lds[kThreads - 1];
    return lds[t] - v;
}

__global__ __launch_bounds__(kThreads) void moe_plan_kernel(const int* __restrict__ idx, const int* __restrict__ counts, int E, int NK,
                                                            int max_tiles, int* __restrict__ offsets, int* __restrict__ pairs,
                                                            int* __restrict__ pos, int* __restrict__ tiles, int* __restrict__ n_tiles) {
    __shared__ int scan[kThreads];
    __shared__ int off[KIVI_MOE_MAX_E];
    const int t = threadIdx.x;
    const int c = t < E ? counts[t] : 0;
    int total, total_tiles;
    const int o = block_scan(c, scan, &total);
    const int nt = (c + kTile - 1) / kTile;
    const int tb = block_scan(nt, scan, &total_tiles);
    if (t < E) {
        off[t] = o;
        offsets[t] = o;
        for (int j = 0; j < nt && tb + j < max_tiles; j++) {
            int* tl = tiles + (int64_t)(tb + j) * KIVI_MOE_TILE_WORDS;
            tl[0] = t;
            tl[1] = o + j * kTile;
            tl[2] = c - j * kTile < kTile ? c - j * kTile : kTile;
        }
    }
    if (t == 0) {
        offsets[E] = total;
        *n_tiles = total_tiles < max_tiles ? total_tiles : max_tiles;
    }
    __syncthreads();
    for (int p = t; p < NK; p += kThreads) {
        const int q = off[idx[p]] + pos[p];
        if ((unsigned)q < (unsigned)NK) {                   // (always: the counts are those of idx)
            pos[p] = q;
            pairs[q] = p;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- experts
template <bool BF>
__device__ __forceinline__ f32x4 mfma(u32x4 a, u32x4 b, f32x4 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// One tile x 16 weight rows.  GATEUP: rows i0 .. i0 + 15 of the expert's gate AND up matrices over x (reduction over H), the
// activation out; else rows h0 .. h0 + 15 of its down matrix over the activations (reduction over I), fp32 out.
//   src     GATEUP: x (N, H) by src_stride, the row of a pair found through `pairs`; else act (NK, I), row = position in `pairs`
//   wmat    GATEUP: gate_up (E, 2 I, H); else down (E, H, I)
//   R       rows of the matrix this launch walks (I / H), C its columns = the reduction length (H / I)
template <bool BF, bool GATEUP>
__global__ __launch_bounds__(kThreads) void moe_gemm_kernel(const uint16_t* __restrict__ src, int64_t src_stride,
                                                            const uint16_t* __restrict__ wmat, const int* __restrict__ pairs,
                                                            const int* __restrict__ tiles, const int* __restrict__ n_tiles,
                                                            int max_tiles, void* __restrict__ dst, int NK, int R, int C, int E, int K) {
    __shared__ f32x4 red[kWaves - 1][GATEUP ? 2 : 1][KIVI_WAVE];
    const int tile = blockIdx.x;
    const int live_tiles = *n_tiles;
    if (tile >= live_tiles || tile >= max_tiles) return;    // block-uniform: the grid is the host's bound
    const int* tl = tiles + (int64_t)tile * KIVI_MOE_TILE_WORDS;
    const int e = tl[0], first = tl[1], rows = tl[2];
    if ((unsigned)e >= (unsigned)E || rows < 1 || rows > kTile || first < 0 || first > NK - rows) return;   // not a plan of route's
    const int lane = threadIdx.x & (KIVI_WAVE - 1), wave = threadIdx.x / KIVI_WAVE;
    const int r = lane & 15, kb = lane >> 4;
    const int r0 = blockIdx.y * KIVI_MOE_ROW_TILE;
    const uint16_t* wa = wmat + ((int64_t)e * (GATEUP ? 2 : 1) * R + r0 + r) * C + 8 * kb;
    const uint16_t* wb = wa + (int64_t)R * C;               // the up rows (GATEUP only)
    bool live = r < rows;
    const uint16_t* xr = src;
    if (live) {
        if constexpr (GATEUP) {
            const int pair = pairs[first + r];
            live = (unsigned)pair < (unsigned)NK;
            xr = src + (int64_t)(live ? pair / K : 0) * src_stride + 8 * kb;
        } else {
            xr = src + (int64_t)(first + r) * src_stride + 8 * kb;
        }
    }
    f32x4 acc_a = {0.0f, 0.0f, 0.0f, 0.0f}, acc_b = {0.0f, 0.0f, 0.0f, 0.0f};
    const int steps = C / 32;
    for (int s0 = 4 * wave; s0 < steps; s0 += 4 * kWaves) {
        u32x4 a[4], b[4], x[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 32 * (s0 + j);
            const bool in = s0 + j < steps;                 // wave-uniform
            a[j] = in ? ld16(wa + k) : u32x4{0u, 0u, 0u, 0u};
            if constexpr (GATEUP) b[j] = in ? ld16(wb + k) : u32x4{0u, 0u, 0u, 0u};
            x[j] = in && live ? ld16(xr + k) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (s0 + j < steps) {
                acc_a = mfma<BF>(a[j], x[j], acc_a);
                if constexpr (GATEUP) acc_b = mfma<BF>(b[j], x[j], acc_b);
            }
        }
    }
    if (wave > 0) {
        red[wave - 1][0][lane] = acc_a;
        if constexpr (GATEUP) red[wave - 1][1][lane] = acc_b;
    }
    __syncthreads();
    if (wave > 0) return;
    acc_a = (acc_a + red[0][0][lane]) + (red[1][0][lane] + red[2][0][lane]);
    if constexpr (GATEUP) acc_b = (acc_b + red[0][1][lane]) + (red[1][1][lane] + red[2][1][lane]);
    if (r >= rows) return;
    // lane: token column r, weight rows r0 + 4 kb + j
    if constexpr (GATEUP) {
        uint16_t h[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float g = acc_a[j];
            h[j] = to_bits<BF>(g / (1.0f + expf(-g)) * acc_b[j]);
        }
        u32x2 out = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        *reinterpret_cast<u32x2*>((uint16_t*)dst + (int64_t)(first + r) * R + r0 + 4 * kb) = out;
    } else {
        *reinterpret_cast<f32x4*>((float*)dst + (int64_t)(first + r) * R + r0 + 4 * kb) = acc_a;
    }
}

// ------------------------------------------------------------------------------------------------------- experts, FP8 weights
// moe_gemm_kernel over e4m3fn bytes with one fp32 scale per 128 x 128 block.  The block, the guards, the
// split of the reduction axis, the tree and the epilogues are moe_gemm_kernel's; inside a 128-element stretch the operands are
// formed as kivi_w8.hip forms them (kivi_w8_operand.h, kivi_w8_plan_step_k): lane (r, kb) reads, for half h, the 16 bytes of its
// row at k = 128 stretch + 64 h + 16 kb -- the low 8 its A fragment of one step against x[k .. k + 8), the high 8 that of the
// next against x[k + 8 .. k + 16).  The stretch's four MFMAs go into a zeroed tile, then yacc = fma(tile, s, yacc) with the ONE
// scale of (stripe, stretch).  Every address is kivi_moe_w8_plan.h's.
//   What one wave needs of one stretch: per matrix 2 x 16 bytes of its lane's row and the scale, and 16 bytes per step of its token row.
template <int NM>
struct MoeW8Stage {
    u32x4 w[NM][2];
    float s[NM];
    u32x4 x[4];
    __device__ __forceinline__ void load(bool in, int64_t st, const uint8_t* const* wr, const float* const* sp, const uint16_t* xr,
                                         int kb, bool live) {
        if (!in) return;                                    // wave-uniform: past the wave's last stretch
#pragma unroll
        for (int m = 0; m < NM; m++) {
            w[m][0] = *reinterpret_cast<const u32x4*>(wr[m] + kivi_moe_w8_plan_weight_byte(0, 0, 0, 0, st, 0, 0));
            w[m][1] = *reinterpret_cast<const u32x4*>(wr[m] + kivi_moe_w8_plan_weight_byte(0, 0, 0, 0, st, 1, 0));
            s[m] = sp[m][st];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = live ? ld16(xr + kivi_moe_w8_plan_src_elem(0, 0, st, j, kb)) : u32x4{0u, 0u, 0u, 0u};
    }
};

//   src     GATEUP: x (N, H) by src_stride, the row of a pair found through `pairs`; else act (NK, I), row = position in `pairs`
//   wmat / scale   GATEUP: gate_up (E, 2 I, H) bytes and (E, 2 I / 128, H / 128) fp32; else down (E, H, I) and (E, H / 128, I / 128)
//   R       rows of the matrix this launch walks (I / H), C its columns = the reduction length (H / I): multiples of 128
template <bool BF, bool GATEUP>
__global__ __launch_bounds__(kThreads) void moe_gemm_w8_kernel(const uint16_t* __restrict__ src, int64_t src_stride,
                                                               const uint8_t* __restrict__ wmat, const float* __restrict__ scale,
                                                               const int* __restrict__ pairs, const int* __restrict__ tiles,
                                                               const int* __restrict__ n_tiles, int max_tiles, void* __restrict__ dst,
                                                               int NK, int R, int C, int E, int K) {
    constexpr int NM = GATEUP ? 2 : 1;
    __shared__ f32x4 red[kWaves - 1][NM][KIVI_WAVE];
    const int tile = blockIdx.x;
    const int live_tiles = *n_tiles;
    if (tile >= live_tiles || tile >= max_tiles) return;    // block-uniform: the grid is the host's bound
    const int* tl = tiles + (int64_t)tile * KIVI_MOE_TILE_WORDS;
    const int e = tl[0], first = tl[1], rows = tl[2];
    if ((unsigned)e >= (unsigned)E || rows < 1 || rows > kTile || first < 0 || first > NK - rows) return;   // not a plan of route's
    const int lane = threadIdx.x & (KIVI_WAVE - 1), wave = threadIdx.x / KIVI_WAVE;
    const int r = lane & 15, kb = lane >> 4;
    const int r0 = blockIdx.y * KIVI_MOE_ROW_TILE;
    const int64_t slab = (int64_t)NM * R;                   // rows of an expert's matrix: 2 I (gate rows, then up rows) or H
    const uint8_t* wr[NM];
    const float* sp[NM];
    wr[0] = wmat + kivi_moe_w8_plan_weight_byte(e, slab, r0 + r, C, 0, 0, kb);
    sp[0] = scale + kivi_moe_w8_plan_scale_word(e, slab, r0, C, 0);
    if constexpr (GATEUP) {
        wr[1] = wmat + kivi_moe_w8_plan_weight_byte(e, slab, (int64_t)R + r0 + r, C, 0, 0, kb);
        sp[1] = scale + kivi_moe_w8_plan_scale_word(e, slab, (int64_t)R + r0, C, 0);
    }
    bool live = r < rows;
    const uint16_t* xr = src;
    if (live) {
        if constexpr (GATEUP) {
            const int pair = pairs[first + r];
            live = (unsigned)pair < (unsigned)NK;
            xr = src + kivi_moe_w8_plan_src_elem(live ? pair / K : 0, src_stride, 0, 0, 0);
        } else {
            xr = src + kivi_moe_w8_plan_src_elem(first + r, src_stride, 0, 0, 0);
        }
    }
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 yacc[NM];
#pragma unroll
    for (int m = 0; m < NM; m++) yacc[m] = zero;
    const int64_t stretches = kivi_moe_w8_plan_stretches(C);
    // a stretch's bytes, scales and token row are requested one stretch of the wave ahead of their use
    MoeW8Stage<NM> cur, nxt;
    cur.load(wave < stretches, wave, wr, sp, xr, kb, live);
    for (int64_t st = wave; st < stretches; st += kWaves) { // wave-uniform
        nxt.load(st + kWaves < stretches, st + kWaves, wr, sp, xr, kb, live);
        f32x4 acc[NM];
#pragma unroll
        for (int m = 0; m < NM; m++) acc[m] = zero;
#pragma unroll
        for (int j = 0; j < 4; j++)                         // four steps of 32 reduction elements
#pragma unroll
            for (int m = 0; m < NM; m++)
                acc[m] = mfma<BF>(w8_operand<BF>(cur.w[m][j >> 1][2 * (j & 1)], cur.w[m][j >> 1][2 * (j & 1) + 1]), cur.x[j], acc[m]);
#pragma unroll
        for (int m = 0; m < NM; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) yacc[m][i] = __builtin_fmaf(acc[m][i], cur.s[m], yacc[m][i]);
        cur = nxt;
    }
    if (wave > 0) {
#pragma unroll
        for (int m = 0; m < NM; m++) red[wave - 1][m][lane] = yacc[m];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int m = 0; m < NM; m++) yacc[m] = (yacc[m] + red[0][m][lane]) + (red[1][m][lane] + red[2][m][lane]);
    if (r >= rows) return;
    // lane: token column r, weight rows r0 + 4 kb + j
    const int64_t at = kivi_moe_w8_plan_dst_elem(first + r, R, r0, kb);
    if constexpr (GATEUP) {
        uint16_t h[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float g = yacc[0][j];
            h[j] = to_bits<BF>(g / (1.0f + expf(-g)) * yacc[NM - 1][j]);
        }
        u32x2 out = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        *reinterpret_cast<u32x2*>((uint16_t*)dst + at) = out;
    } else {
        *reinterpret_cast<f32x4*>((float*)dst + at) = yacc[0];
    }
}

template <bool BF>
__global__ __launch_bounds__(kThreads) void moe_combine_kernel(const float* __restrict__ y, const float* __restrict__ w,
                                                               const int* __restrict__ pos, uint16_t* __restrict__ out,
                                                               int64_t out_stride, int N, int H, int K, int NK) {
    const int64_t unit = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int per_row = H / 4;
    if (unit >= (int64_t)N * per_row) return;
    const int64_t n = unit / per_row;
    const int h = (int)(unit % per_row) * 4;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < K; k++) {                           // slot order
        const int q = pos[n * K + k];
        if ((unsigned)q >= (unsigned)NK) continue;          // not a plan of route's
        const float wk = w[n * K + k];
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + (int64_t)q * H + h);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_fmaf(wk, v[j], acc[j]);
    }
    u32x2 o = {(uint32_t)to_bits<BF>(acc[0]) | ((uint32_t)to_bits<BF>(acc[1]) << 16),
               (uint32_t)to_bits<BF>(acc[2]) | ((uint32_t)to_bits<BF>(acc[3]) << 16)};
    *reinterpret_cast<u32x2*>(out + n * out_stride + h) = o;
}

}  // namespace

extern "C" int kivi_moe_max_tiles(int N, int E, int top_k) {
    const int64_t t = kivi_moe_plan_max_tiles((int64_t)N, E, top_k);
    KIVI_REQUIRE(t >= 0, KIVI_EINVAL, "kivi_moe_max_tiles: N=%d E=%d top_k=%d (N >= 1, E in [1, 256], top_k in [1, min(E, 16)], "
                 "N * top_k < 2^31)", N, E, top_k);
    return (int)t;
}

extern "C" int64_t kivi_moe_workspace_bytes(int N, int H, int I, int E, int top_k) {
    const int64_t b = kivi_moe_plan_workspace_bytes((int64_t)N, H, I, E, top_k);
    KIVI_REQUIRE(b >= 0 && kivi_moe_plan_grids_ok(N, H, I), KIVI_EINVAL, "kivi_moe_workspace_bytes: N=%d H=%d I=%d E=%d top_k=%d (H, I "
                 "multiples of 32 up to 16 * 65535; N >= 1, E in [1, 256], top_k in [1, min(E, 16)], N * top_k < 2^31)", N, H, I, E, top_k);
    return b;
}

extern "C" int kivi_moe_route(const void* logits, int64_t row_stride, int dtype, int N, int E, int top_k, int flags, void* idx, void* w,
                              void* counts, void* offsets, void* pairs, void* pos, void* tiles, void* n_tiles, kivi_stream_t stream) {
    KIVI_REQUIRE(kivi_moe_plan_dtype_ok(dtype), KIVI_EINVAL, "kivi_moe_route: dtype=%d (16: fp16, 0x110: bf16)", dtype);
    const int64_t nk = kivi_moe_plan_pairs(N, E, top_k);
    KIVI_REQUIRE(nk >= 0, KIVI_EINVAL, "kivi_moe_route: N=%d E=%d top_k=%d (N >= 1, E in [1, 256], top_k in [1, min(E, 16)], "
                 "N * top_k < 2^31)", N, E, top_k);
    KIVI_REQUIRE((flags & ~(KIVI_MOE_NORM_TOPK | KIVI_MOE_ROUND_WEIGHTS)) == 0, KIVI_EINVAL, "kivi_moe_route: flags=0x%x", flags);
    KIVI_REQUIRE(row_stride >= E, KIVI_EINVAL, "kivi_moe_route: row_stride=%lld < E=%d", (long long)row_stride, E);
    KIVI_REQUIRE(logits && idx && w && counts && offsets && pairs && pos && tiles && n_tiles, KIVI_EINVAL,
                 "kivi_moe_route: null logits, idx, w, counts, offsets, pairs, pos, tiles or n_tiles");
    KIVI_REQUIRE((uintptr_t)logits % 2 == 0, KIVI_EALIGN, "kivi_moe_route: logits off 2 bytes");
    for (const void* p : {(const void*)idx, (const void*)w, (const void*)counts, (const void*)offsets, (const void*)pairs,
                          (const void*)pos, (const void*)tiles, (const void*)n_tiles})
        KIVI_REQUIRE((uintptr_t)p % 4 == 0, KIVI_EALIGN, "kivi_moe_route: a 4-byte output off 4 bytes");
    const int max_tiles = (int)kivi_moe_plan_max_tiles((int64_t)N, E, top_k);
    hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipMemsetAsync(counts, 0, (size_t)E * sizeof(int), s);
    if (err != hipSuccess) {
        kivi_set_error("kivi_moe_route: clearing the counts failed: %s", hipGetErrorString(err));
        return (int)err;
    }
    const dim3 grid((unsigned)kivi_moe_plan_route_blocks(N));
    if (dtype == KIVI_MOE_BF16)
        KIVI_LAUNCH(moe_route_kernel<true>, grid, dim3(kThreads), s, (const uint16_t*)logits, row_stride, N, E, top_k, flags, (int*)idx,
                    (float*)w, (int*)counts, (int*)pos);
    else
        KIVI_LAUNCH(moe_route_kernel<false>, grid, dim3(kThreads), s, (const uint16_t*)logits, row_stride, N, E, top_k, flags, (int*)idx,
                    (float*)w, (int*)counts, (int*)pos);
    KIVI_LAUNCH(moe_plan_kernel, dim3(1), dim3(kThreads), s, (const int*)idx, (const int*)counts, E, (int)nk, max_tiles, (int*)offsets,
                (int*)pairs, (int*)pos, (int*)tiles, (int*)n_tiles);
    return kivi_launch_status("kivi_moe_route");
}

extern "C" int kivi_moe_experts(const void* x, int64_t x_stride, int dtype, int N, int H, int I, int E, int top_k, const void* w,
                                const void* pairs, const void* pos, const void* tiles, const void* n_tiles, const void* gate_up,
                                const void* down, void* out, int64_t out_stride, void* workspace, int64_t workspace_bytes,
                                kivi_stream_t stream) {
    KIVI_REQUIRE(kivi_moe_plan_dtype_ok(dtype), KIVI_EINVAL, "kivi_moe_experts: dtype=%d (16: fp16, 0x110: bf16)", dtype);
    const int64_t nk = kivi_moe_plan_pairs(N, E, top_k);
    KIVI_REQUIRE(nk >= 0, KIVI_EINVAL, "kivi_moe_experts: N=%d E=%d top_k=%d (N >= 1, E in [1, 256], top_k in [1, min(E, 16)], "
                 "N * top_k < 2^31)", N, E, top_k);
    KIVI_REQUIRE(kivi_moe_plan_dims_ok(H, I) && kivi_moe_plan_grids_ok(N, H, I), KIVI_EINVAL,
                 "kivi_moe_experts: H=%d I=%d (multiples of 32, at most 16 * 65535; N * H / 1024 < 2^31)", H, I);
    KIVI_REQUIRE(x_stride >= H && out_stride >= H, KIVI_EINVAL, "kivi_moe_experts: x_stride=%lld or out_stride=%lld < H=%d",
                 (long long)x_stride, (long long)out_stride, H);
    KIVI_REQUIRE(x && w && pairs && pos && tiles && n_tiles && gate_up && down && out && workspace, KIVI_EINVAL,
                 "kivi_moe_experts: null x, w, pairs, pos, tiles, n_tiles, gate_up, down, out or workspace");
    const int64_t need = kivi_moe_plan_workspace_bytes((int64_t)N, H, I, E, top_k);
    KIVI_REQUIRE(need >= 0 && workspace_bytes >= need, KIVI_EINVAL, "kivi_moe_experts: workspace_bytes=%lld < %lld",
                 (long long)workspace_bytes, (long long)need);
    for (const void* p : {x, gate_up, down, (const void*)workspace})
        KIVI_REQUIRE((uintptr_t)p % 16 == 0, KIVI_EALIGN, "kivi_moe_experts: x, gate_up, down or workspace off 16 bytes");
    KIVI_REQUIRE((uintptr_t)out % 8 == 0 && x_stride % 8 == 0 && out_stride % 4 == 0, KIVI_EALIGN,
                 "kivi_moe_experts: out off 8 bytes, x_stride=%lld not a multiple of 8 or out_stride=%lld not of 4", (long long)x_stride,
                 (long long)out_stride);
    for (const void* p : {w, pairs, pos, tiles, n_tiles})
        KIVI_REQUIRE((uintptr_t)p % 4 == 0, KIVI_EALIGN, "kivi_moe_experts: a 4-byte plan member off 4 bytes");
    const int max_tiles = (int)kivi_moe_plan_max_tiles((int64_t)N, E, top_k);
    hipStream_t s = (hipStream_t)stream;
    uint16_t* act = (uint16_t*)workspace;
    float* y = (float*)((char*)workspace + kivi_moe_plan_act_bytes(nk, I));
    const dim3 g1((unsigned)max_tiles, (unsigned)kivi_moe_plan_row_blocks(I)), g2((unsigned)max_tiles, (unsigned)kivi_moe_plan_row_blocks(H));
    const dim3 g3((unsigned)kivi_moe_plan_combine_blocks(N, H));
    if (dtype == KIVI_MOE_BF16) {
        KIVI_LAUNCH((moe_gemm_kernel<true, true>), g1, dim3(kThreads), s, (const uint16_t*)x, x_stride, (const uint16_t*)gate_up,
                    (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)act, (int)nk, I, H, E, top_k);
        KIVI_LAUNCH((moe_gemm_kernel<true, false>), g2, dim3(kThreads), s, (const uint16_t*)act, (int64_t)I, (const uint16_t*)down,
                    (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)y, (int)nk, H, I, E, top_k);
        KIVI_LAUNCH(moe_combine_kernel<true>, g3, dim3(kThreads), s, (const float*)y, (const float*)w, (const int*)pos, (uint16_t*)out,
                    out_stride, N, H, top_k, (int)nk);
    } else {
        KIVI_LAUNCH((moe_gemm_kernel<false, true>), g1, dim3(kThreads), s, (const uint16_t*)x, x_stride, (const uint16_t*)gate_up,
                    (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)act, (int)nk, I, H, E, top_k);
        KIVI_LAUNCH((moe_gemm_kernel<false, false>), g2, dim3(kThreads), s, (const uint16_t*)act, (int64_t)I, (const uint16_t*)down,
                    (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)y, (int)nk, H, I, E, top_k);
        KIVI_LAUNCH(moe_combine_kernel<false>, g3, dim3(kThreads), s, (const float*)y, (const float*)w, (const int*)pos, (uint16_t*)out,
                    out_stride, N, H, top_k, (int)nk);
    }
    return kivi_launch_status("kivi_moe_experts");
}

extern "C" int kivi_moe_experts_w8(const void* x, int64_t x_stride, int dtype, int N, int H, int I, int E, int top_k, const void* w,
                                   const void* pairs, const void* pos, const void* tiles, const void* n_tiles, const void* gate_up,
                                   const void* gate_up_scale, const void* down, const void* down_scale, void* out, int64_t out_stride,
                                   void* workspace, int64_t workspace_bytes, kivi_stream_t stream) {
    static_assert(kWaves == KIVI_MOE_W8_WAVES, "the stretches of kivi_moe_w8_plan.h are dealt over the block's waves");
    KIVI_REQUIRE(kivi_moe_plan_dtype_ok(dtype), KIVI_EINVAL, "kivi_moe_experts_w8: dtype=%d (16: fp16, 0x110: bf16)", dtype);
    const int64_t nk = kivi_moe_plan_pairs(N, E, top_k);
    KIVI_REQUIRE(nk >= 0, KIVI_EINVAL, "kivi_moe_experts_w8: N=%d E=%d top_k=%d (N >= 1, E in [1, 256], top_k in [1, min(E, 16)], "
                 "N * top_k < 2^31)", N, E, top_k);
    KIVI_REQUIRE(kivi_moe_w8_plan_dims_ok(H, I) && kivi_moe_plan_grids_ok(N, H, I), KIVI_EINVAL,
                 "kivi_moe_experts_w8: H=%d I=%d (positive multiples of 128, at most 16 * 65535; N * H / 1024 < 2^31)", H, I);
    KIVI_REQUIRE(x_stride >= H && out_stride >= H, KIVI_EINVAL, "kivi_moe_experts_w8: x_stride=%lld or out_stride=%lld < H=%d",
                 (long long)x_stride, (long long)out_stride, H);
    KIVI_REQUIRE(x && w && pairs && pos && tiles && n_tiles && gate_up && gate_up_scale && down && down_scale && out && workspace,
                 KIVI_EINVAL, "kivi_moe_experts_w8: null x, w, pairs, pos, tiles, n_tiles, gate_up, gate_up_scale, down, down_scale, out "
                 "or workspace");
    const int64_t need = kivi_moe_plan_workspace_bytes((int64_t)N, H, I, E, top_k);
    KIVI_REQUIRE(need >= 0 && workspace_bytes >= need, KIVI_EINVAL, "kivi_moe_experts_w8: workspace_bytes=%lld < %lld",
                 (long long)workspace_bytes, (long long)need);
    for (const void* p : {x, gate_up, down, (const void*)workspace})
        KIVI_REQUIRE((uintptr_t)p % 16 == 0, KIVI_EALIGN, "kivi_moe_experts_w8: x, gate_up, down or workspace off 16 bytes");
    KIVI_REQUIRE((uintptr_t)out % 8 == 0 && x_stride % 8 == 0 && out_stride % 4 == 0, KIVI_EALIGN,
                 "kivi_moe_experts_w8: out off 8 bytes, x_stride=%lld not a multiple of 8 or out_stride=%lld not of 4", (long long)x_stride,
                 (long long)out_stride);
    for (const void* p : {w, pairs, pos, tiles, n_tiles, gate_up_scale, down_scale})
        KIVI_REQUIRE((uintptr_t)p % 4 == 0, KIVI_EALIGN, "kivi_moe_experts_w8: a 4-byte plan member or a scale grid off 4 bytes");
    const int max_tiles = (int)kivi_moe_plan_max_tiles((int64_t)N, E, top_k);
    hipStream_t s = (hipStream_t)stream;
    uint16_t* act = (uint16_t*)workspace;
    float* y = (float*)((char*)workspace + kivi_moe_w8_plan_y_offset(nk, I));
    const dim3 g1((unsigned)max_tiles, (unsigned)kivi_moe_plan_row_blocks(I)), g2((unsigned)max_tiles, (unsigned)kivi_moe_plan_row_blocks(H));
    const dim3 g3((unsigned)kivi_moe_plan_combine_blocks(N, H));
    if (dtype == KIVI_MOE_BF16) {
        KIVI_LAUNCH((moe_gemm_w8_kernel<true, true>), g1, dim3(kThreads), s, (const uint16_t*)x, x_stride, (const uint8_t*)gate_up,
                    (const float*)gate_up_scale, (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)act, (int)nk,
                    I, H, E, top_k);
        KIVI_LAUNCH((moe_gemm_w8_kernel<true, false>), g2, dim3(kThreads), s, (const uint16_t*)act, (int64_t)I, (const uint8_t*)down,
                    (const float*)down_scale, (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)y, (int)nk, H,
                    I, E, top_k);
        KIVI_LAUNCH(moe_combine_kernel<true>, g3, dim3(kThreads), s, (const float*)y, (const float*)w, (const int*)pos, (uint16_t*)out,
                    out_stride, N, H, top_k, (int)nk);
    } else {
        KIVI_LAUNCH((moe_gemm_w8_kernel<false, true>), g1, dim3(kThreads), s, (const uint16_t*)x, x_stride, (const uint8_t*)gate_up,
                    (const float*)gate_up_scale, (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)act, (int)nk,
                    I, H, E, top_k);
        KIVI_LAUNCH((moe_gemm_w8_kernel<false, false>), g2, dim3(kThreads), s, (const uint16_t*)act, (int64_t)I, (const uint8_t*)down,
                    (const float*)down_scale, (const int*)pairs, (const int*)tiles, (const int*)n_tiles, max_tiles, (void*)y, (int)nk, H,
                    I, E, top_k);
        KIVI_LAUNCH(moe_combine_kernel<false>, g3, dim3(kThreads), s, (const float*)y, (const float*)w, (const int*)pos, (uint16_t*)out,
                    out_stride, N, H, top_k, (int)nk);
    }
    return kivi_launch_status("kivi_moe_experts_w8");
}
