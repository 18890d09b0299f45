// kivi_prefill_attention (include/kivi_hip.h): the prompt pass's attention -- causal, grouped-query, aware
// of leading pads -- over fp16 q / k / v read by strides, without a copy of K / V per query head and without a T x T mask.
//
// One block of four waves per (batch row, query head, 128 query rows); a wave owns 32 query rows, two 16-column matrix tiles.
// The products are transposed as in mf_extend_kernel (kivi_extend.hip): S^T = K Q^T and O^T = V^T P^T, so a lane holds ONE query
// row (lane & 15) in both accumulators, the softmax of a row needs two cross-lane steps (the four lane groups that share a row),
// and the fp16 probabilities of S^T's accumulator ARE the B operand of the second product: element j of lane group g is the key
// 16 (j >> 2) + 4 g + (j & 3) of the 32-key tile, and the A operand (V^T) takes its tokens in that same order.
//
// K and V tiles of 32 keys x 128 channels go global -> registers -> LDS, two buffers: the loads of tile t + 1 are issued before the
// products of tile t and stored after them, one barrier per tile.  Both tiles use ONE image, 256-byte rows whose 16-byte chunk c of
// row r sits at chunk c ^ (((r & 3) << 2) | ((r >> 2) & 3)): the K rows are read with ds_read_b128 (a lane: 8 channels of a key), V
// with ds_read_b64_tr_b16 (a lane: 4 keys of a channel, the transposition V^T needs), both without the bank conflicts of plain rows.
// The transposed read gathers across lanes and needs every lane active: the products run under wave-uniform conditions only, and a
// tile is always 32 whole rows in LDS (keys past T are stored as zeros, rows past T carry a zero q and are never written out).
//
// Which tiles a block stages and a wave multiplies is the plan of kivi_prefill_plan.h: tiles wholly under the lead or wholly above
// the diagonal are skipped, and only a tile that mixes live and dead pairs compares its scores against (lead, row).  The online
// softmax keeps a running maximum m and a per-lane partial sum in fp32, in the exp2 domain (scores * scale * log2 e).  A dead
// score is -inf, and every difference is taken against max(m, tile) with -inf replaced by 0, so -inf - -inf never reaches the
// exponential: a row without a live key so far keeps m = -inf, its sum and accumulators 0, and its first live tile sets m.
// Query rows under the lead are pads: exact zeros are written for them.  Every output element is written by one lane, 8 bytes at
// a time (4 consecutive channels); there is no workspace, no atomic and no exchange between blocks.
#include "kivi_common.h"
#include "kivi_prefill_plan.h"

#include <math.h>

namespace {

typedef _Float16 pf_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 pf_h8 __attribute__((ext_vector_type(8)));
typedef float pf_f4 __attribute__((ext_vector_type(4)));
typedef __fp16 pf_t4 __attribute__((__vector_size__(4 * sizeof(__fp16))));        // the transposed read's own result type
typedef __attribute__((address_space(3))) pf_t4 pf_lds_t4;

struct PfArgs {
    const uint16_t* q; int64_t q_sb, q_sh, q_st;
    const uint16_t* k; int64_t k_sb, k_sh, k_st;
    const uint16_t* v; int64_t v_sb, v_sh, v_st;
    uint16_t* out; int64_t o_sb, o_sh, o_st;
    const int32_t* lead;
    int B, nh, G, T;
    float scale_log2;                                      // scale * log2(e)
};

constexpr int kTileBytes = kPrefillKTile * 256;            // 32 keys x 128 fp16 channels

// byte offset of 16-byte chunk ch (0..15) of row `row` of a staged tile
__device__ __forceinline__ int tile_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

__device__ __forceinline__ pf_f4 mfma(pf_h8 a, pf_h8 b, pf_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(kPrefillThreads) void prefill_attn_kernel(const PfArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][2][kTileBytes];      // [buffer][K, V]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n = lane & 15, qd = lane >> 4;
    const KiviPrefillBlock blk = kivi_prefill_block(a.B, a.nh, a.T, blockIdx.x);
    const int b = blk.b, h = blk.h, hk = h / a.G;
    const int lead = a.lead ? kivi_prefill_clamp_lead(a.lead[b], a.T) : 0;
    const KiviPrefillTiles bt = kivi_prefill_tiles(blk.q0, blk.q1, lead);            // what the block stages
    const int wq0 = blk.q0 + wave * kPrefillWaveRows, wq1 = min(wq0 + kPrefillWaveRows, blk.q1);
    KiviPrefillTiles wt = {0, 0};                                                   // what this wave multiplies
    if (wq0 < wq1) wt = kivi_prefill_tiles(wq0, wq1, lead);

    pf_h8 qf[2][4];                                       // B operand of S^T = K Q^T: q[row 16 u + n][32 c + 8 qd + j]
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int row = wq0 + 16 * u + n;
        const uint16_t* qp = a.q + b * a.q_sb + (int64_t)h * a.q_sh + (int64_t)row * a.q_st + 8 * qd;
#pragma unroll
        for (int c = 0; c < 4; c++) qf[u][c] = row < wq1 ? __builtin_bit_cast(pf_h8, *(const u32x4*)(qp + 32 * c)) : pf_h8{};
    }

    // staging: thread -> chunk (tid & 15) of the tile rows (tid >> 4) and (tid >> 4) + 16 (the same swizzle for both)
    const int srow = tid >> 4, sch = tid & 15;
    const uint16_t* kg = a.k + b * a.k_sb + (int64_t)hk * a.k_sh + 8 * sch;
    const uint16_t* vg = a.v + b * a.v_sb + (int64_t)hk * a.v_sh + 8 * sch;
    const int soff = tile_off(srow, sch);
    u32x4 kr[2], vr[2];
    auto gload = [&](int kt) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int key = kt * kPrefillKTile + srow + 16 * r;
            const bool ok = key < a.T;
            kr[r] = ok ? *(const u32x4*)(kg + (int64_t)key * a.k_st) : u32x4{0u, 0u, 0u, 0u};
            vr[r] = ok ? *(const u32x4*)(vg + (int64_t)key * a.v_st) : u32x4{0u, 0u, 0u, 0u};
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int r = 0; r < 2; r++) {
            *(u32x4*)(lds[buf][0] + soff + 4096 * r) = kr[r];
            *(u32x4*)(lds[buf][1] + soff + 4096 * r) = vr[r];
        }
    };
    // this lane's read addresses: K row n of a 16-key half, chunk 4 c + qd;  V: lane 4 q + p of group qd supplies keys 4 qd + q,
    // channels 16 ct + 4 p .. + 3 of the transposed read's 4 x 16 block
    const int ksw = ((n & 3) << 2) | ((n >> 2) & 3);
    const int tq = n >> 2, tp = n & 3, vsw = (tq << 2) | qd;
    const int vrow_off = 256 * (4 * qd + tq) + 8 * (tp & 1);

    pf_f4 acc[2][8];                                      // O^T: channels 16 ct + 4 qd + reg of row 16 u + n
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
        for (int ct = 0; ct < 8; ct++) acc[u][ct] = pf_f4{0.f, 0.f, 0.f, 0.f};
    float m[2] = {-__builtin_inff(), -__builtin_inff()}, l[2] = {0.f, 0.f};

    if (bt.kt0 < bt.kt1) {
        gload(bt.kt0);
        lstore(0);
    }
    __syncthreads();
    for (int kt = bt.kt0; kt < bt.kt1; kt++) {
        const int buf = (kt - bt.kt0) & 1;
        const bool more = kt + 1 < bt.kt1;
        if (more) gload(kt + 1);
        if (kt < wt.kt1) {                                // wave-uniform (wt.kt0 == bt.kt0 whenever wt is not empty)
            const uint8_t* kT = lds[buf][0];
            const uint8_t* vT = lds[buf][1];
            // ------------------------------------------------------------ S^T tile: 32 keys x 32 rows
            pf_f4 s[2][2];
#pragma unroll
            for (int u = 0; u < 2; u++) s[u][0] = s[u][1] = pf_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tile = 0; tile < 2; tile++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const pf_h8 ka = *(const pf_h8*)(kT + 256 * (16 * tile + n) + 16 * ((4 * c + qd) ^ ksw));
#pragma unroll
                    for (int u = 0; u < 2; u++) s[u][tile] = mfma(ka, qf[u][c], s[u][tile]);
                }
            // ------------------------------------------------------------ online softmax, fp16 probabilities
            const bool partial = kivi_prefill_partial(wq0, wq1, lead, kt);
            const int k0 = kt * kPrefillKTile;
            pf_h8 pb[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int i = wq0 + 16 * u + n;
                float x[8], tmax = -__builtin_inff();
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int key = k0 + 16 * (j >> 2) + 4 * qd + (j & 3);
                    float xv = s[u][j >> 2][j & 3] * a.scale_log2;
                    if (partial && !(key >= lead && key <= i)) xv = -__builtin_inff();
                    x[j] = xv;
                    tmax = fmaxf(tmax, xv);
                }
                tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
                const float mnew = fmaxf(m[u], tmax);
                const float msafe = mnew == -__builtin_inff() ? 0.f : mnew;
                const float alpha = __builtin_amdgcn_exp2f(m[u] - msafe);
                float psum = 0.f;
                pf_h8 p;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float e = __builtin_amdgcn_exp2f(x[j] - msafe);
                    psum += e;
                    p[j] = (_Float16)e;
                }
                pb[u] = p;
                l[u] = l[u] * alpha + psum;
                m[u] = mnew;
#pragma unroll
                for (int ct = 0; ct < 8; ct++) acc[u][ct] *= alpha;
            }
            // ------------------------------------------------------------ O^T += V^T P^T
#pragma unroll
            for (int ct = 0; ct < 8; ct++) {
                const int voff = vrow_off + 16 * ((2 * ct + (tp >> 1)) ^ vsw);
                const pf_h4 lo = __builtin_bit_cast(pf_h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((pf_lds_t4*)(vT + voff)));
                const pf_h4 hi = __builtin_bit_cast(pf_h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((pf_lds_t4*)(vT + voff + 16 * 256)));
                const pf_h8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int u = 0; u < 2; u++) acc[u][ct] = mfma(va, pb[u], acc[u][ct]);
            }
        }
        if (more) lstore(buf ^ 1);
        __syncthreads();
    }
    // ---------------------------------------------------------------- one division by the fp32 sum, one rounding to fp16
#pragma unroll
    for (int u = 0; u < 2; u++) {
        float sum = l[u];
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const int i = wq0 + 16 * u + n;
        if (i >= wq1) continue;
        const bool live = i >= lead;                      // a live row holds its own key: sum >= 1
        const float inv = live ? 1.0f / sum : 0.f;
        uint16_t* op = a.out + b * a.o_sb + (int64_t)h * a.o_sh + (int64_t)i * a.o_st + 4 * qd;
#pragma unroll
        for (int ct = 0; ct < 8; ct++) {
            uint32_t w[2] = {0u, 0u};
            if (live) {
#pragma unroll
                for (int r = 0; r < 4; r++) w[r >> 1] |= (uint32_t)f2h_bits(acc[u][ct][r] * inv) << (16 * (r & 1));
            }
            *(u32x2*)(op + 16 * ct) = u32x2{w[0], w[1]};
        }
    }
}

bool rows16(const void* p, int64_t sb, int64_t sh, int64_t st) {
    return (uintptr_t)p % 16 == 0 && sb % 8 == 0 && sh % 8 == 0 && st % 8 == 0;
}

}  // namespace

extern "C" int kivi_prefill_attention(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_st, const void* k, int64_t k_sb,
                                      int64_t k_sh, int64_t k_st, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_st, void* out,
                                      int64_t o_sb, int64_t o_sh, int64_t o_st, const int32_t* lead, int B, int nh, int nh_kv, int T,
                                      int D, float scale, kivi_stream_t stream) {
    KIVI_REQUIRE(D == 128, KIVI_EINVAL, "kivi_prefill_attention: D=%d (head_dim 128 only)", D);
    KIVI_REQUIRE(B >= 1 && nh >= 1 && nh_kv >= 1 && T >= 1, KIVI_EINVAL, "kivi_prefill_attention: bad shape (B=%d nh=%d nh_kv=%d T=%d)", B,
                 nh, nh_kv, T);
    KIVI_REQUIRE(nh % nh_kv == 0, KIVI_EINVAL, "kivi_prefill_attention: nh=%d is not a multiple of nh_kv=%d", nh, nh_kv);
    const int G = nh / nh_kv;
    KIVI_REQUIRE(G == 1 || G == 2 || G == 4 || G == 8, KIVI_EINVAL, "kivi_prefill_attention: nh / nh_kv = %d (1, 2, 4 or 8)", G);
    KIVI_REQUIRE(q && k && v && out, KIVI_EINVAL, "kivi_prefill_attention: null q / k / v / out");
    KIVI_REQUIRE(isfinite(scale) && scale > 0.f, KIVI_EINVAL, "kivi_prefill_attention: scale=%g (finite and positive)", (double)scale);
    const int64_t blocks = T <= (1 << 30) ? kivi_prefill_blocks(B, nh, T) : (1LL << 31);
    KIVI_REQUIRE(blocks < (1LL << 31), KIVI_EINVAL, "kivi_prefill_attention: B=%d nh=%d T=%d: grid too large (2^31 blocks or more)", B, nh, T);
    KIVI_REQUIRE(rows16(q, q_sb, q_sh, q_st) && rows16(k, k_sb, k_sh, k_st) && rows16(v, v_sb, v_sh, v_st) && rows16(out, o_sb, o_sh, o_st),
                 KIVI_EALIGN, "kivi_prefill_attention: q / k / v / out and their strides must be multiples of 16 bytes");
    KIVI_REQUIRE((uintptr_t)lead % 4 == 0, KIVI_EALIGN, "kivi_prefill_attention: lead must be 4-byte aligned");
    PfArgs a;
    a.q = (const uint16_t*)q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_st = q_st;
    a.k = (const uint16_t*)k; a.k_sb = k_sb; a.k_sh = k_sh; a.k_st = k_st;
    a.v = (const uint16_t*)v; a.v_sb = v_sb; a.v_sh = v_sh; a.v_st = v_st;
    a.out = (uint16_t*)out; a.o_sb = o_sb; a.o_sh = o_sh; a.o_st = o_st;
    a.lead = lead;
    a.B = B; a.nh = nh; a.G = G; a.T = T;
    a.scale_log2 = (float)((double)scale * 1.4426950408889634074);
    KIVI_LAUNCH(prefill_attn_kernel, dim3((unsigned)blocks), dim3(kPrefillThreads), (hipStream_t)stream, a);
    return kivi_launch_status("kivi_prefill_attention");
}
