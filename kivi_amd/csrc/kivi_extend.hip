// Multi-token extend of a matrix-pipe cache (kivi_mfma_layout.h): attention of a chunk of Q new tokens over the cache as it stood
// before the call plus the chunk itself (causal), then the cache update that Q decode steps would have made.
//
// Attention (mf_extend_kernel): one block per (batch row, kv head, 16-row tile), four waves that take the 32-token key tiles in
// turn, two passes (the softmax statistics of every row, then the fp16 probabilities and the sV sums), merged through LDS.  MFMA rows are (chunk position, query head of the kv group):
// row r of the unit = i * G + h.  The products are transposed -- S^T = K Q^T, O^T = V^T P^T -- so that every lane holds ONE query
// row (lane & 15) in both accumulators, and the probabilities of S^T's accumulator are the B operand of the sV product without any
// lane movement (the token order inside the 32-wide k step is permuted the same way on the V side).
// Dequantisation is plain fp32: v = fmaf(code, scale, mn) (the reference's scale * code + zero, quant/csrc/gemv_cuda.cu:407-413),
// split into an exact-as-possible fp16 pair hi = fp16(v), lo = fp16(v - hi) fed to two chained MFMAs (~22 bits of v); the other
// operand is q or the fp16 probabilities, exactly.  No range-word placement: the store's range words are not read here.
#include "kivi_common.h"
#include "kivi_gqa_dev.h"
#include "kivi_quant.h"

namespace {

struct ExtArgs {
    MfStore kt, vt;
    const uint16_t* kres; int64_t kr_sb, kr_sh, kr_st;
    const uint16_t* vres; int64_t vr_sb, vr_sh, vr_st;
    const uint16_t* q; int64_t q_sb, q_sh, q_st;
    const uint16_t* kn; int64_t kn_sb, kn_sh, kn_st;
    const uint16_t* vn; int64_t vn_sb, vn_sh, vn_st;
    const uint16_t* mask; int64_t mask_sb, mask_sq;
    uint16_t* out; int64_t out_sb, out_sh, out_st;
    uint16_t* dump; int64_t d_sb, d_sh, d_sq;             // KIVI_GQA_DUMP_SCORES (tests): null in production
    int64_t Tq, Tv, P0;
    int Q, G, nh_kv, win_start, win_rows, ntile_rows;
};

__device__ __forceinline__ float h2f(uint16_t h) { return h2f_bits(h); }
__device__ __forceinline__ uint16_t f2h(float f) { return f2h_bits(f); }

// fp32 value -> (hi, lo) fp16 bit patterns, hi + lo = v to ~22 bits
__device__ __forceinline__ void split(float v, uint16_t& hi, uint16_t& lo) {
    hi = f2h(v);
    lo = f2h(v - h2f(hi));
}

__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *(const u32x4*)p; }

__device__ __forceinline__ f4 mfma(h8 a, h8 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

__device__ __forceinline__ h8 pack8(const uint16_t* x) {
    return as_h8(x[0] | ((uint32_t)x[1] << 16), x[2] | ((uint32_t)x[3] << 16), x[4] | ((uint32_t)x[5] << 16), x[6] | ((uint32_t)x[7] << 16));
}

// one packed V element (token t < Tv, channel d) in fp32
template <int BITS>
__device__ __forceinline__ float v_packed(const ExtArgs& a, int b, int hk, int64_t t, int d) {
    const uint32_t* sb = mf_sb(a.vt, b, hk, t >> 9);
    const int blk = (int)((t >> 5) & 15), tt = (int)(t & 31);
    uint32_t code;
    if constexpr (BITS == 2) code = (sb[blk * KIVI_MF_BLOCK_WORDS + vt_word(tt, d)] >> vt_bit(tt, d)) & 3u;
    else code = (sb[blk * KIVI_MF4_BLOCK_WORDS + vt4_word(tt, d)] >> vt4_bit(tt)) & 15u;
    const int hidx = blk * 128 + vt_half(tt, d >> 5);
    const float s = h2f(((const uint16_t*)(sb + MfL<BITS>::SCALE_WORD0))[hidx]);
    const float m = h2f(((const uint16_t*)(sb + MfL<BITS>::MN_WORD0))[hidx]);
    return fmaf((float)code, s, m);
}

// fp16 V element of a token at or past Tv: the ring window before the chunk, the chunk after it
__device__ __forceinline__ float v_fp16(const ExtArgs& a, int b, int hk, int64_t t, int d) {
    if (t < a.P0) {
        int64_t row = a.win_start + (t - a.Tv);
        if (row >= a.win_rows) row -= a.win_rows;
        return h2f(a.vres[b * a.vr_sb + hk * a.vr_sh + row * a.vr_st + d]);
    }
    return h2f(a.vn[b * a.vn_sb + hk * a.vn_sh + (t - a.P0) * a.vn_st + d]);
}

template <int BITS>
__global__ __launch_bounds__(256) void mf_extend_kernel(ExtArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 15, qd = lane >> 4;
    const int unit = blockIdx.y, b = unit / a.nh_kv, hk = unit - b * a.nh_kv;
    const int rt = blockIdx.x;
    const int rows = a.Q * a.G;
    // this lane's query row
    const int r = rt * 16 + n;
    const bool live = r < rows;
    const int ci = live ? r / a.G : a.Q - 1, hq = hk * a.G + (live ? r - (r / a.G) * a.G : 0);
    // last chunk position of the tile: keys past P0 + ilast are masked for every row of the tile
    const int ilast = min(rows - 1, rt * 16 + 15) / a.G;
    const int64_t nkeys = a.P0 + ilast + 1;
    const int ntiles = (int)((nkeys + 31) >> 5);

    h8 qf[4];                                             // B operand of S^T = K Q^T: q[row n][32 c + 8 qd + j]
    {
        const uint16_t* qp = a.q + b * a.q_sb + (int64_t)hq * a.q_sh + (int64_t)ci * a.q_st + 8 * qd;
#pragma unroll
        for (int c = 0; c < 4; c++) qf[c] = live ? __builtin_bit_cast(h8, ld16(qp + 32 * c)) : h8{};
    }
    const uint16_t* mrow = a.mask ? a.mask + b * a.mask_sb + (int64_t)ci * a.mask_sq : nullptr;

    f4 acc[8], accw[8];                                   // O^T: channels 16 ct + 4 qd + reg of row n; packed / fp16 values
#pragma unroll
    for (int ct = 0; ct < 8; ct++) acc[ct] = accw[ct] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -__builtin_inff(), l = 0.f;               // pass 0: running max / sum of this wave's tiles
    float M = 0.f, L = 1.f;                               // pass 1: the row's max and sum (all waves)
    __shared__ float sm_m[4][16], sm_l[4][16];

    // Two passes over the keys: the statistics of the row first, then the probabilities exactly as the hook rounds them,
    // fp16(exp(w - max) / sum), as the B operand of the sV products.  (An online softmax that rounds exp(w - running max)
    // instead lands as far from the reference again as the reference's own probability rounding: measured 1.2-2.1x the
    // 3e-3 bar on outlier / x30 inputs; the second qK^T pass costs the K half of the traffic once more.)
    for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (qd == 0) { sm_m[wave][n] = m; sm_l[wave][n] = l; }
        __syncthreads();
        M = -__builtin_inff();
#pragma unroll
        for (int wv = 0; wv < 4; wv++) M = fmaxf(M, sm_m[wv][n]);
        L = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; wv++) L += sm_m[wv][n] == -__builtin_inff() ? 0.f : expf(sm_m[wv][n] - M) * sm_l[wv][n];
    }
    for (int kt = wave; kt < ntiles; kt += 4) {
        const int64_t t0 = (int64_t)kt * 32;
        // ---------------------------------------------------------------- S^T tile: 32 tokens x 16 rows
        f4 s[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
        if (t0 + 32 <= a.Tq) {
            const uint32_t* sb = mf_sb(a.kt, b, hk, t0 >> 9);
            const int g = (int)((t0 >> 5) & 15);
            u32x4 w[2];
            if constexpr (BITS == 2) {
                w[0] = *(const u32x4*)(sb + g * KIVI_MF_BLOCK_WORDS + lane * 4);
                w[1] = w[0];
            } else {
                w[0] = *(const u32x4*)(sb + g * KIVI_MF4_BLOCK_WORDS + lane * 4);
                w[1] = *(const u32x4*)(sb + g * KIVI_MF4_BLOCK_WORDS + 256 + lane * 4);
            }
            const uint16_t* sc = (const uint16_t*)(sb + MfL<BITS>::SCALE_WORD0);
            const uint16_t* mn = (const uint16_t*)(sb + MfL<BITS>::MN_WORD0);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int d0 = 32 * c + 8 * qd;
                const u32x4 sv = ld16(sc + kt_sm_half(g, d0)), mv = ld16(mn + kt_sm_half(g, d0));
                const uint16_t* s16 = (const uint16_t*)&sv;
                const uint16_t* m16 = (const uint16_t*)&mv;
#pragma unroll
                for (int tile = 0; tile < 2; tile++) {
                    uint16_t hi[8], lo[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int pos = BITS == 2 ? mf_pos(tile, j >> 1) + 16 * (j & 1) : 4 * (j >> 1) + 16 * (j & 1);
                        const uint32_t code = (w[tile][c] >> pos) & ((1u << BITS) - 1);
                        split(fmaf((float)code, h2f(s16[j]), h2f(m16[j])), hi[j], lo[j]);
                    }
                    s[tile] = mfma(pack8(hi), qf[c], s[tile]);
                    s[tile] = mfma(pack8(lo), qf[c], s[tile]);
                }
            }
        } else {
            // fp16 keys (Tq is a multiple of 32: a tile is packed or not as a whole): the K residual, then the chunk
#pragma unroll
            for (int tile = 0; tile < 2; tile++) {
                const int64_t t = t0 + 16 * tile + n;
                const uint16_t* kp = nullptr;
                if (t < a.P0) kp = a.kres + b * a.kr_sb + hk * a.kr_sh + (t - a.Tq) * a.kr_st;
                else if (t < a.P0 + a.Q) kp = a.kn + b * a.kn_sb + hk * a.kn_sh + (t - a.P0) * a.kn_st;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const h8 kf = kp ? __builtin_bit_cast(h8, ld16(kp + 32 * c + 8 * qd)) : h8{};
                    s[tile] = mfma(kf, qf[c], s[tile]);
                }
            }
        }
        // ---------------------------------------------------------------- scores as the hook rounds them; online softmax
        float w[8];
        float tmax = -__builtin_inff();
#pragma unroll
        for (int tile = 0; tile < 2; tile++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int64_t t = t0 + 16 * tile + 4 * qd + reg;
                float x = h2f(f2h(h2f(f2h(s[tile][reg])) / 11.313708498984761f));   // fp16(fp16(q.k) / sqrt(128))
                if (mrow && t < a.P0 + a.Q) x = fmaxf(h2f(f2h(x + h2f(mrow[t]))), -65504.f);
                const bool ok = t < a.P0 || (t < a.P0 + a.Q && t - a.P0 <= ci);
                if (a.dump && pass == 1 && live && ok)      // the row the softmax consumes, key t (every visible key, once)
                    a.dump[b * a.d_sb + (int64_t)hq * a.d_sh + (int64_t)ci * a.d_sq + t] = f2h(x);
                x = ok ? x : -__builtin_inff();
                w[4 * tile + reg] = x;
                tmax = fmaxf(tmax, x);
            }
        if (pass == 0) {
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float mnew = fmaxf(m, tmax);
            if (mnew == -__builtin_inff()) continue;      // nothing of this row in the tile, nor before it
            float psum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) psum += expf(w[j] - mnew);
            l = l * expf(m - mnew) + psum;
            m = mnew;
            continue;
        }
        uint16_t p16[8];
#pragma unroll
        for (int j = 0; j < 8; j++) p16[j] = f2h(expf(w[j] - M) / L);     // llama_kivi.py:375: fp32 softmax, fp16 probabilities
        const h8 pb = pack8(p16);                        // B operand of O^T = V^T P^T: k = 8 qd + j <-> token 16 (j >> 2) + 4 qd + (j & 3)
        // ---------------------------------------------------------------- O^T += V^T P^T
        if (t0 + 32 <= a.Tv) {
            const uint32_t* sb = mf_sb(a.vt, b, hk, t0 >> 9);
            const int g = (int)((t0 >> 5) & 15);
            const uint16_t* sc = (const uint16_t*)(sb + MfL<BITS>::SCALE_WORD0) + g * 128;
            const uint16_t* mn = (const uint16_t*)(sb + MfL<BITS>::MN_WORD0) + g * 128;
            u32x4 wv[2][2];                               // [token half jj][channel tile parity] (2-bit: one word holds both)
            uint64_t svv[2][4], mvv[2][4];
#pragma unroll
            for (int jj = 0; jj < 2; jj++) {
                const int kbv = 2 * jj + (qd >> 1);
                if constexpr (BITS == 2) {
                    wv[jj][0] = *(const u32x4*)(sb + g * KIVI_MF_BLOCK_WORDS + (n + 16 * kbv) * 4);
                    wv[jj][1] = wv[jj][0];
                } else {
                    wv[jj][0] = *(const u32x4*)(sb + g * KIVI_MF4_BLOCK_WORDS + (n + 16 * kbv) * 4);
                    wv[jj][1] = *(const u32x4*)(sb + g * KIVI_MF4_BLOCK_WORDS + 256 + (n + 16 * kbv) * 4);
                }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int h0 = kbv * 32 + c * 8 + 4 * (qd & 1);
                    svv[jj][c] = *(const uint64_t*)(sc + h0);
                    mvv[jj][c] = *(const uint64_t*)(mn + h0);
                }
            }
#pragma unroll
            for (int ct = 0; ct < 8; ct++) {
                const int c = ct >> 1, tile = ct & 1;
                uint16_t hi[8], lo[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int jj = j >> 2, e = 4 * (qd & 1) + (j & 3);
                    const int pos = BITS == 2 ? mf_pos(tile, e >> 1) + 16 * (e & 1) : 4 * (e >> 1) + 16 * (e & 1);
                    const uint32_t code = (wv[jj][tile][c] >> pos) & ((1u << BITS) - 1);
                    const uint16_t sh = (uint16_t)(svv[jj][c] >> (16 * (j & 3))), mh = (uint16_t)(mvv[jj][c] >> (16 * (j & 3)));
                    split(fmaf((float)code, h2f(sh), h2f(mh)), hi[j], lo[j]);
                }
                acc[ct] = mfma(pack8(hi), pb, acc[ct]);
                acc[ct] = mfma(pack8(lo), pb, acc[ct]);
            }
        } else {
            // the tail: a tile that straddles Tv, the window, the chunk (element loads; at most (R + Q) / 32 + 1 tiles of a row).
            // The packed and the fp16 values go to separate sums: the hook rounds the two parts of the output separately.
            uint16_t pp[8], pw[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const bool packed = t0 + 16 * (j >> 2) + 4 * qd + (j & 3) < a.Tv;
                pp[j] = packed ? p16[j] : (uint16_t)0;
                pw[j] = packed ? (uint16_t)0 : p16[j];
            }
            const h8 pbp = pack8(pp), pbw = pack8(pw);
#pragma unroll
            for (int ct = 0; ct < 8; ct++) {
                const int d = 16 * ct + n;
                uint16_t hi[8], lo[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int64_t t = t0 + 16 * (j >> 2) + 4 * qd + (j & 3);
                    float v = 0.f;
                    if (t < a.Tv) v = v_packed<BITS>(a, b, hk, t, d);
                    else if (t < a.P0 + a.Q) v = v_fp16(a, b, hk, t, d);
                    split(v, hi[j], lo[j]);
                }
                const h8 vh = pack8(hi);
                acc[ct] = mfma(vh, pbp, acc[ct]);
                acc[ct] = mfma(pack8(lo), pbp, acc[ct]);
                accw[ct] = mfma(vh, pbw, accw[ct]);            // fp16 values: lo = 0
            }
        }
    }
    }
    // ---------------------------------------------------------------- sum the four waves
    __shared__ float sm_o[2][4][16][129];
#pragma unroll
    for (int ct = 0; ct < 8; ct++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            sm_o[0][wave][n][16 * ct + 4 * qd + reg] = acc[ct][reg];
            sm_o[1][wave][n][16 * ct + 4 * qd + reg] = accw[ct][reg];
        }
    __syncthreads();
    // thread -> (row, 8 channels)
    const int row = threadIdx.x >> 4, d0 = (threadIdx.x & 15) * 8;
    const int rr = rt * 16 + row;
    if (rr >= rows) return;
    const int oi = rr / a.G, oh = hk * a.G + (rr - oi * a.G);
    uint16_t o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        float x = 0.f, y = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; wv++) {
            x += sm_o[0][wv][row][d0 + k];
            y += sm_o[1][wv][row][d0 + k];
        }
        o[k] = f2h(h2f(f2h(x)) + h2f(f2h(y)));    // fp16(fp16(packed sV) + fp16(fp16 sV)), llama_kivi.py:382-384
    }
    *(u32x4*)(a.out + b * a.out_sb + (int64_t)oh * a.out_sh + (int64_t)oi * a.out_st + d0) =
        u32x4{o[0] | ((uint32_t)o[1] << 16), o[2] | ((uint32_t)o[3] << 16), o[4] | ((uint32_t)o[5] << 16), o[6] | ((uint32_t)o[7] << 16)};
}

// Per-token V quantisation of tokens [0, T) of `v` into the VT layout at token offset `off` (any offset): one block per
// (unit, 32-token block touched).  Threads 0..127 quantise (token, channel group) pairs exactly as the decode step's V flush does
// (make_group over the 32 channels, quant_one) and write the group's scale / zero point and range marks; then every code word of
// the block is rewritten by one thread: fields of the new tokens cleared and set, the others kept (read-modify-write).
template <int BITS>
__global__ __launch_bounds__(256) void vt_pack_at_kernel(const uint16_t* v, int64_t v_sb, int64_t v_sh, int64_t v_st, MfStore st,
                                                         int* range, int64_t off, int64_t T, int nh_kv, int nblk) {
    const int unit = blockIdx.y, b = unit / nh_kv, hk = unit - b * nh_kv;
    const int64_t bi = (off >> 5) + blockIdx.x;
    const int64_t lo = off - bi * 32, hi = off + T - bi * 32;     // block tokens tt in [lo, hi) are new
    __shared__ uint8_t codes[32][128];
    const int tid = threadIdx.x;
    uint32_t* sb = mf_sb(st, b, hk, bi >> 4);
    const int blk = (int)(bi & 15);
    if (tid < 128) {
        const int tt = tid >> 2, c = tid & 3;
        if (tt >= lo && tt < hi) {
            const uint16_t* src = v + b * v_sb + hk * v_sh + (bi * 32 + tt - off) * v_st + 32 * c;
            uint16_t x[32];
#pragma unroll
            for (int k = 0; k < 4; k++) *(u32x4*)(x + 8 * k) = ld16(src + 8 * k);
            uint32_t kmin = h_key(x[0]), kmax = kmin;
#pragma unroll
            for (int k = 1; k < 32; k++) {
                const uint32_t key = h_key(x[k]);
                kmin = key < kmin ? key : kmin;
                kmax = key > kmax ? key : kmax;
            }
            const GroupQ gq = make_group(kmin, kmax, (1 << BITS) - 1);
#pragma unroll
            for (int k = 0; k < 32; k++) codes[tt][32 * c + k] = (uint8_t)quant_one<BITS>(x[k], gq);
            const int hidx = blk * 128 + vt_half(tt, c);
            ((uint16_t*)(sb + MfL<BITS>::SCALE_WORD0))[hidx] = gq.scale;
            ((uint16_t*)(sb + MfL<BITS>::MN_WORD0))[hidx] = gq.mn;
            mf_range_mark(range + unit, gq.scale);
        }
    }
    __syncthreads();
    constexpr int WORDS = BITS == 2 ? KIVI_MF_BLOCK_WORDS : KIVI_MF4_BLOCK_WORDS;
    for (int w = tid; w < WORDS; w += 256) {
        const int tile4 = BITS == 4 ? w >> 8 : 0, wl = w & 255;
        const int nn = (wl >> 2) & 15, kbv = wl >> 6, c = wl & 3;
        uint32_t word = sb[blk * WORDS + w];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int tt = 8 * kbv + e;
            if (tt < lo || tt >= hi) continue;
            if constexpr (BITS == 2) {
#pragma unroll
                for (int tile = 0; tile < 2; tile++) {
                    const int pos = mf_pos(tile, e >> 1) + 16 * (e & 1);
                    word = (word & ~(3u << pos)) | ((uint32_t)codes[tt][32 * c + 16 * tile + nn] << pos);
                }
            } else {
                const int pos = 4 * (e >> 1) + 16 * (e & 1);
                word = (word & ~(15u << pos)) | ((uint32_t)codes[tt][32 * c + 16 * tile4 + nn] << pos);
            }
        }
        sb[blk * WORDS + w] = word;
    }
}

// dst row (row0 + t) mod rows <- src row t, t in [0, T), of every unit (128 fp16 channels, 16 bytes per thread)
__global__ __launch_bounds__(256) void rows_copy_kernel(const uint16_t* src, int64_t s_sb, int64_t s_sh, int64_t s_st, uint16_t* dst,
                                                        int64_t d_sb, int64_t d_sh, int64_t d_st, int64_t row0, int64_t rows, int64_t T,
                                                        int nh_kv, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (unit, t, 16-byte piece)
    if (i >= total) return;
    const int piece = (int)(i & 15);
    const int64_t rest = i >> 4, t = rest % T, unit = rest / T;
    const int b = (int)(unit / nh_kv), hk = (int)(unit - (int64_t)b * nh_kv);
    int64_t row = row0 + t;
    row %= rows;
    *(u32x4*)(dst + b * d_sb + hk * d_sh + row * d_st + 8 * piece) = ld16(src + b * s_sb + hk * s_sh + t * s_st + 8 * piece);
}

int rows_copy(const void* src, int64_t s_sb, int64_t s_sh, int64_t s_st, void* dst, int64_t d_sb, int64_t d_sh, int64_t d_st, int64_t row0,
              int64_t rows, int64_t T, int B, int nh_kv, hipStream_t s) {
    if (T <= 0) return 0;
    const int64_t total = (int64_t)B * nh_kv * T * 16;
    hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint16_t*)src, s_sb, s_sh, s_st,
                       (uint16_t*)dst, d_sb, d_sh, d_st, row0, rows, T, nh_kv, total);
    return kivi_launch_status("rows_copy");
}

bool rows16(const void* p, int64_t sb, int64_t sh, int64_t st) {
    return p && (uintptr_t)p % 16 == 0 && sb % 8 == 0 && sh % 8 == 0 && st % 8 == 0;
}

}  // namespace

extern "C" int kivi_vt_pack_at(const void* v, int64_t v_sb, int64_t v_sh, int64_t v_st, void* vt, int64_t vt_sb, int64_t vt_sh,
                               int64_t vt_ss, void* vt_range, int64_t token_offset, int B, int nh_kv, int64_t T, int D, int group_size,
                               int bits, kivi_stream_t stream) {
    KIVI_REQUIRE((bits == 2 || bits == 4) && group_size == 32 && D == 128, KIVI_EUNSUPPORTED,
                 "kivi_vt_pack_at: the MFMA cache layout covers 2- and 4-bit codes, group_size 32, head_dim 128 (got %d / %d / %d)", bits,
                 group_size, D);
    KIVI_REQUIRE(B > 0 && nh_kv > 0 && T >= 0 && token_offset >= 0, KIVI_EINVAL, "kivi_vt_pack_at: bad shape (B=%d nh_kv=%d T=%lld offset=%lld)",
                 B, nh_kv, (long long)T, (long long)token_offset);
    KIVI_REQUIRE(vt_range && (uintptr_t)vt_range % 4 == 0, KIVI_EINVAL, "kivi_vt_pack_at: null / misaligned range flags");
    KIVI_REQUIRE(vt && (uintptr_t)vt % 16 == 0 && vt_sb % 4 == 0 && vt_sh % 4 == 0 && vt_ss % 4 == 0 &&
                     vt_ss >= (bits == 4 ? KIVI_MF4_SB_WORDS : KIVI_MF_SB_WORDS),
                 KIVI_EALIGN, "kivi_vt_pack_at: cache storage must be 16-byte aligned super-blocks");
    KIVI_REQUIRE(rows16(v, v_sb, v_sh, v_st), KIVI_EALIGN, "kivi_vt_pack_at: value rows must be 16-byte aligned");
    const int64_t nblk = T ? (token_offset + T - 1) / 32 - token_offset / 32 + 1 : 0;
    KIVI_REQUIRE(nblk < 65536 && (int64_t)B * nh_kv < 65536, KIVI_EINVAL, "kivi_vt_pack_at: grid too large");
    if (T == 0) return 0;
    const MfStore st = {(uint32_t*)vt, vt_sb, vt_sh, vt_ss};
    if (bits == 4)
        hipLaunchKernelGGL(vt_pack_at_kernel<4>, dim3((unsigned)nblk, (unsigned)(B * nh_kv)), dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t*)v, v_sb, v_sh, v_st, st, (int*)vt_range, token_offset, T, nh_kv, (int)nblk);
    else
        hipLaunchKernelGGL(vt_pack_at_kernel<2>, dim3((unsigned)nblk, (unsigned)(B * nh_kv)), dim3(256), 0, (hipStream_t)stream,
                           (const uint16_t*)v, v_sb, v_sh, v_st, st, (int*)vt_range, token_offset, T, nh_kv, (int)nblk);
    return kivi_launch_status("vt_pack_at");
}

extern "C" int kivi_mf_extend_layer(const kivi_mf_layer_desc* L, int64_t* st, int Q, const void* q, int64_t q_sb, int64_t q_sh,
                                    int64_t q_st, int nh, const void* knew, int64_t kn_sb, int64_t kn_sh, int64_t kn_st, const void* vnew,
                                    int64_t vn_sb, int64_t vn_sh, int64_t vn_st, const void* mask, int64_t mask_sb, int64_t mask_sq,
                                    void* out, int64_t out_sb, int64_t out_sh, int64_t out_st, kivi_stream_t stream) {
    KIVI_REQUIRE(L && st && q && knew && vnew && out, KIVI_EINVAL, "kivi_mf_extend_layer: null argument");
    int64_t Tq = st[0], kres = st[1], Tv = st[2], wstart = st[3], vres = st[4], kv = st[5];
    const int R = L->residual_length;
    KIVI_REQUIRE(Q >= 1, KIVI_EINVAL, "kivi_mf_extend_layer: Q=%d, at least one new token", Q);
    KIVI_REQUIRE(R > 0 && R % 32 == 0 && R <= 128 && Tq >= 0 && Tq % 32 == 0 && kres >= 0 && kres < R && Tv >= 0 && wstart >= 0 &&
                     vres >= 0 && vres <= R && kv == Tq + kres && kv == Tv + vres && kv > 0,
                 KIVI_EINVAL, "kivi_mf_extend_layer: inconsistent lengths (Tq=%lld kres=%lld Tv=%lld vres=%lld kv=%lld R=%d)",
                 (long long)Tq, (long long)kres, (long long)Tv, (long long)vres, (long long)kv, R);
    KIVI_REQUIRE((L->bits == 2 || L->bits == 4) && L->group_size == 32 && L->D == 128, KIVI_EUNSUPPORTED,
                 "kivi_mf_extend_layer: the MFMA cache layout covers 2- and 4-bit codes, group_size 32, head_dim 128 (got %d / %d / %d)",
                 L->bits, L->group_size, L->D);
    KIVI_REQUIRE(L->B > 0 && L->nh_kv > 0 && nh > 0 && nh % L->nh_kv == 0 && nh / L->nh_kv <= 8, KIVI_EINVAL,
                 "kivi_mf_extend_layer: bad shape (B=%d nh=%d nh_kv=%d)", L->B, nh, L->nh_kv);
    KIVI_REQUIRE(L->B < 65536 && L->nh_kv < 65536 && (int64_t)L->B * L->nh_kv < 65536, KIVI_EINVAL, "kivi_mf_extend_layer: grid too large");
    KIVI_REQUIRE(L->kt && L->vt && L->k_res && L->v_res && L->kt_range && L->vt_range, KIVI_EINVAL,
                 "kivi_mf_extend_layer: null cache buffer in the descriptor");
    KIVI_REQUIRE(L->cap % 512 == 0 && kv + Q <= L->cap, KIVI_EINVAL, "kivi_mf_extend_layer: cache capacity %lld exceeded (%lld + %d)",
                 (long long)L->cap, (long long)kv, Q);
    KIVI_REQUIRE((L->flags & KIVI_GQA_WINDOW_RING) != 0 && L->v_window_rows >= R + 1 && wstart < L->v_window_rows, KIVI_EINVAL,
                 "kivi_mf_extend_layer: needs the ring window of >= R + 1 rows");
    // mask_sq == 0: one key row per batch row, shared by all Q chunk rows (a padding mask; causality is applied below regardless)
    KIVI_REQUIRE(mask == nullptr || (mask_sq == 0 ? mask_sb >= kv + Q : mask_sq >= kv + Q && mask_sb >= (int64_t)Q * mask_sq), KIVI_EINVAL,
                 "kivi_mf_extend_layer: mask rows of %lld halves cannot hold %lld keys", (long long)(mask_sq ? mask_sq : mask_sb),
                 (long long)(kv + Q));
    const int sbw = L->bits == 4 ? KIVI_MF4_SB_WORDS : KIVI_MF_SB_WORDS;
    KIVI_REQUIRE((uintptr_t)L->kt % 16 == 0 && (uintptr_t)L->vt % 16 == 0 && L->kt_sb % 4 == 0 && L->kt_sh % 4 == 0 && L->kt_ss % 4 == 0 &&
                     L->vt_sb % 4 == 0 && L->vt_sh % 4 == 0 && L->vt_ss % 4 == 0 && L->kt_ss >= sbw && L->vt_ss >= sbw &&
                     (uintptr_t)L->kt_range % 4 == 0 && (uintptr_t)L->vt_range % 4 == 0,
                 KIVI_EALIGN, "kivi_mf_extend_layer: cache storage must be 16-byte aligned super-blocks");
    KIVI_REQUIRE(rows16(L->k_res, L->kr_sb, L->kr_sh, L->kr_st) && rows16(L->v_res, L->vr_sb, L->vr_sh, L->vr_st) &&
                     rows16(q, q_sb, q_sh, q_st) && rows16(knew, kn_sb, kn_sh, kn_st) && rows16(vnew, vn_sb, vn_sh, vn_st) &&
                     rows16(out, out_sb, out_sh, out_st),
                 KIVI_EALIGN, "kivi_mf_extend_layer: fp16 rows must be 16-byte aligned");
    const bool dump = (L->flags & KIVI_GQA_DUMP_SCORES) != 0;
    KIVI_REQUIRE(!dump || (L->scores && (uintptr_t)L->scores % 2 == 0 && L->s_pitch >= kv + Q && L->s_sh >= (int64_t)Q * L->s_pitch &&
                           L->s_sb >= (int64_t)nh * L->s_sh),
                 KIVI_EINVAL, "kivi_mf_extend_layer: the score dump needs rows of >= %lld halves, Q rows per head, nh heads per batch row "
                 "(s_pitch=%lld s_sh=%lld s_sb=%lld)", (long long)(kv + Q), (long long)L->s_pitch, (long long)L->s_sh, (long long)L->s_sb);
    const int G = nh / L->nh_kv;
    const int64_t ntile_rows = ((int64_t)Q * G + 15) / 16;
    KIVI_REQUIRE(ntile_rows < (1 << 30), KIVI_EINVAL, "kivi_mf_extend_layer: chunk too long");
    hipStream_t s = (hipStream_t)stream;

    // 1. attention over the cache as it stands + the chunk
    ExtArgs a;
    a.kt = {(uint32_t*)L->kt, L->kt_sb, L->kt_sh, L->kt_ss};
    a.vt = {(uint32_t*)L->vt, L->vt_sb, L->vt_sh, L->vt_ss};
    a.kres = (const uint16_t*)L->k_res; a.kr_sb = L->kr_sb; a.kr_sh = L->kr_sh; a.kr_st = L->kr_st;
    a.vres = (const uint16_t*)L->v_res; a.vr_sb = L->vr_sb; a.vr_sh = L->vr_sh; a.vr_st = L->vr_st;
    a.q = (const uint16_t*)q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_st = q_st;
    a.kn = (const uint16_t*)knew; a.kn_sb = kn_sb; a.kn_sh = kn_sh; a.kn_st = kn_st;
    a.vn = (const uint16_t*)vnew; a.vn_sb = vn_sb; a.vn_sh = vn_sh; a.vn_st = vn_st;
    a.mask = (const uint16_t*)mask; a.mask_sb = mask_sb; a.mask_sq = mask_sq;
    a.out = (uint16_t*)out; a.out_sb = out_sb; a.out_sh = out_sh; a.out_st = out_st;
    a.dump = dump ? (uint16_t*)L->scores : nullptr; a.d_sb = L->s_sb; a.d_sh = L->s_sh; a.d_sq = L->s_pitch;
    a.Tq = Tq; a.Tv = Tv; a.P0 = kv;
    a.Q = Q; a.G = G; a.nh_kv = L->nh_kv; a.win_start = (int)wstart; a.win_rows = (int)L->v_window_rows; a.ntile_rows = (int)ntile_rows;
    const dim3 grid((unsigned)ntile_rows, (unsigned)(L->B * L->nh_kv));
    if (L->bits == 4) hipLaunchKernelGGL(mf_extend_kernel<4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(mf_extend_kernel<2>, grid, dim3(256), 0, s, a);
    int rc = kivi_launch_status("mf_extend");
    if (rc) return rc;             // nothing committed

    // 2. K: fill the residual to R, flush it, flush whole R-runs straight from the chunk, keep the rest
    const int B = L->B, nk = L->nh_kv;
    int64_t done = 0;                                     // chunk tokens consumed on the K side
    if (kres + Q >= R) {
        rc = rows_copy(knew, kn_sb, kn_sh, kn_st, L->k_res, L->kr_sb, L->kr_sh, L->kr_st, kres, R, R - kres, B, nk, s);
        if (!rc) rc = kivi_kt_pack(L->k_res, L->kr_sb, L->kr_sh, L->kr_st, L->kt, L->kt_sb, L->kt_sh, L->kt_ss, L->kt_range, Tq, B, nk, R,
                                   L->D, L->group_size, L->bits, stream);
        if (rc) return rc;
        done = R - kres;
        Tq += R;
        const int64_t runs = (Q - done) / R * R;
        if (runs) {
            rc = kivi_kt_pack((const uint16_t*)knew + done * kn_st, kn_sb, kn_sh, kn_st, L->kt, L->kt_sb, L->kt_sh, L->kt_ss, L->kt_range, Tq,
                              B, nk, runs, L->D, L->group_size, L->bits, stream);
            if (rc) return rc;
            Tq += runs;
            done += runs;
        }
        kres = 0;
    }
    rc = rows_copy((const uint16_t*)knew + done * kn_st, kn_sb, kn_sh, kn_st, L->k_res, L->kr_sb, L->kr_sh, L->kr_st, kres, R, Q - done, B, nk, s);
    if (rc) return rc;
    kres += Q - done;

    // 3. V: the tokens that leave the window (the oldest of window + chunk), quantised at Tv
    const int64_t rows = L->v_window_rows;
    const int64_t nout = vres + Q > R ? vres + Q - R : 0;
    const int64_t from_win = nout < vres ? nout : vres;
    if (from_win) {
        const int64_t seg1 = wstart + from_win <= rows ? from_win : rows - wstart;
        rc = kivi_vt_pack_at((const uint16_t*)L->v_res + wstart * L->vr_st, L->vr_sb, L->vr_sh, L->vr_st, L->vt, L->vt_sb, L->vt_sh, L->vt_ss,
                             L->vt_range, Tv, B, nk, seg1, L->D, L->group_size, L->bits, stream);
        if (!rc && from_win > seg1)
            rc = kivi_vt_pack_at(L->v_res, L->vr_sb, L->vr_sh, L->vr_st, L->vt, L->vt_sb, L->vt_sh, L->vt_ss, L->vt_range, Tv + seg1, B, nk,
                                 from_win - seg1, L->D, L->group_size, L->bits, stream);
        if (rc) return rc;
    }
    if (nout > from_win) {
        rc = kivi_vt_pack_at(vnew, vn_sb, vn_sh, vn_st, L->vt, L->vt_sb, L->vt_sh, L->vt_ss, L->vt_range, Tv + from_win, B, nk, nout - from_win,
                             L->D, L->group_size, L->bits, stream);
        if (rc) return rc;
    }
    // 4. the chunk tokens that stay in the window, at the rows Q decode steps would have used: token i at (wstart + vres + i) mod rows
    const int64_t first = nout > vres ? nout - vres : 0;
    rc = rows_copy((const uint16_t*)vnew + first * vn_st, vn_sb, vn_sh, vn_st, L->v_res, L->vr_sb, L->vr_sh, L->vr_st,
                   (wstart + vres + first) % rows, rows, Q - first, B, nk, s);
    if (rc) return rc;
    Tv += nout;
    wstart = (wstart + nout) % rows;
    vres = vres + Q - nout;
    st[0] = Tq; st[1] = kres; st[2] = Tv; st[3] = wstart; st[4] = vres; st[5] = kv + Q;
    return 0;
}
