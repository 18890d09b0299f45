// Fused temperature / top-k / top-p / min-p sampler (include/kivi_hip.h, kivi_sample).
//
// One workgroup of 1024 threads per row.  Every filter of the contract keeps the tokens whose score s = float(logit) / temperature
// is >= some threshold (whole tie classes), so the kernel never sorts: it finds each threshold as an exact key of the
// order-preserving uint32 image of s by radix select (11 + 11 + 10-bit digits, LDS histograms), then draws by inverse CDF in
// vocabulary order.  Probabilities are carried as integer weights w = floor(exp(s - max) * 2^40): every sum is an integer sum, so
// histograms may use LDS integer atomics and the result does not depend on the order of the additions -- the same row, seed and
// draw index give the same token on every run, eager or replayed from a graph.
//
//   pass 0        max key (block reduction)
//   top-k         3 passes: count histograms, the k-th largest key t_k (ties: keep s >= that value)
//   top-p         3 passes over the top-k survivors: weight histograms; the first pass's total is Z_k; t_p = the lowest key whose
//                 strictly-higher mass is < top_p * Z_k
//   draw          1 pass: per bucket (BS consecutive tokens, one wave each) the kept weight; a block scan over the <= 1024 buckets
//                 finds the bucket where the running sum crosses u * S; wave 0 scans that bucket's tokens.
// The row is read from memory in every pass (an L2 hit after the first); nothing is staged, so any V up to KIVI_SAMPLE_MAX_V works.
// kivi_sample: a second, one-thread launch advances the draw counter n of the RNG state after the sampler has read it.
// kivi_sample_rows: the same row body with parameters, seed, stream and draw index read per row from device
// memory; a greedy flag per row; each block advances its own row's draw index.  kivi_sample_rows_pen (section 22) and
// kivi_sample_rows_con (section 25) launch the same kernel, sample_rows_kernel, with more of its optional state: a per-row history
// table and penalty record -- repetition / presence / frequency penalties applied where the logit is read (PenRow), the token counted
// in the table where it is written; kivi_seen_mark fills the table -- and a constraint record per row -- an allow mask, a sorted list
// of biased or suppressed tokens -- applied by the reader ConRow; kivi_allow_mark writes mask rows from id lists.
#include "kivi_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / KIVI_WAVE;
constexpr int kBins = 2048;
constexpr float kWScale = 1099511627776.0f;            // 2^40

__device__ __forceinline__ uint32_t key_of(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ uint64_t weight_of(float e) { return e > 0.0f ? (uint64_t)(e * kWScale) : 0; }

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, int d) {
    const uint32_t lo = __shfl_down((uint32_t)v, d), hi = __shfl_down((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int l) {
    const uint32_t lo = __shfl((uint32_t)v, l), hi = __shfl((uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < KIVI_WAVE; d <<= 1) {
        const uint64_t o = shfl_up64(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), first output word.
__device__ __forceinline__ uint32_t philox_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
    return c0;
}

struct Shared {
    uint64_t hist[kBins];       // radix histograms; the draw's bucket sums reuse the first 1024
    uint64_t wsum[kWaves];
    uint64_t sel_above, sel_base, sel_rem;
    uint32_t wmax[kWaves];
    uint32_t sel_bin, sel_bucket, token;
};

template <typename T>
struct Row {
    const T* p;
    float temp;
    bool div;
    __device__ __forceinline__ float s(int e) const {
        const float x = (float)p[e];
        return (div ? x / temp : x) + 0.0f;          // + 0: -0 and +0 are one tie class (one key)
    }
};

// The reader of a penalised row: the penalised logit of include/kivi_hip.h from the row's history word (bit 15: in the prompt;
// bits 0-14: times emitted), then Row's score.  Every operation is one correctly rounded fp32 operation, none contracted into an
// fma, so a torch fp32 restatement gives the same bits (kivi_amd/sampling.py: reference_penalise).
template <typename T>
struct PenRow {
    const T* p;
    float temp;
    bool div;
    const uint16_t* seen;
    float theta, pres, freq;
    const uint8_t* marks;                            // LDS, mark_chunks(): bit c of the row = some word of tokens [64 c, 64 c + 64) is set
    __device__ __forceinline__ float penalised(float x, uint32_t w) const {
#pragma clang fp contract(off)                       // (HIP's __fmul_rn / __fsub_rn are plain * and -: they would contract)
        const uint32_t c = w & 0x7FFFu;
        if (w) x = x > 0.0f ? x / theta : x * theta; // (the build divides correctly rounded, as x / temp below)
        const float t = freq * (float)c;
        x = x - t;
        if (c) x = x - pres;
        return x;
    }
    __device__ __forceinline__ float s(int e) const {
        float x = (float)p[e];
        // Every pass walks the row in aligned runs of 64 tokens per wave, so this branch is wave-uniform: a wave whose run holds no
        // marked token -- most of them -- loads no table word and skips the arithmetic.  For a zero word the rule only subtracts
        // a zero, which can at most turn -0 into +0, as the + 0 below does anyway.
        if ((marks[e >> 9] >> ((e >> 6) & 7)) & 1) x = penalised(x, seen[e]);
        return (div ? x / temp : x) + 0.0f;
    }
};

// The chunk bitmap of PenRow, by the whole block, once per launch: a wave step reads 512 words of the row's history with one 16-byte
// load per lane (rows are 16-byte aligned and a multiple of 8 words long, so a load that starts below V ends inside the row; what
// lies between V and the row's end can only set a bit too many) and stores the byte of its 8 chunks.  The caller's barrier follows.
__device__ __forceinline__ void mark_chunks(uint8_t* marks, const uint16_t* hist, int V) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint4* q = reinterpret_cast<const uint4*>(hist);
    for (int g = wave; g * 512 < V; g += kWaves) {
        const int e = g * 512 + lane * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (e < V) v = q[e >> 3];
        const uint64_t any = __builtin_amdgcn_ballot_w64((v.x | v.y | v.z | v.w) != 0);
        const uint64_t bits = __builtin_amdgcn_ballot_w64(lane < 8 && ((any >> (8 * (lane & 7))) & 0xFFu) != 0);
        if (lane == 0) marks[g] = (uint8_t)bits;
    }
}

// One radix digit over the tokens of this wave's segment: histogram (counts, or weights when MASS) of the keys >= lo whose bits
// above `shift + nbits` equal those of `prefix`, then wave 0 picks the lowest non-empty bin whose strictly-higher total is < the
// remaining target (for counts: the bin that holds the k-th largest; for weights: the bin that holds the top-p boundary class).
template <bool MASS, class Reader>
__device__ void radix_digit(Shared& sh, const Reader& row, int e0, int e1, float m, uint32_t lo, uint32_t& prefix, int shift,
                            int nbits, uint64_t& rem, double frac) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nb = 1 << nbits;
    for (int i = tid; i < nb; i += kThreads) sh.hist[i] = 0;
    __syncthreads();
    const int hs = shift + nbits;
    for (int e = e0 + lane; e < e1; e += KIVI_WAVE) {
        const float s = row.s(e);
        const uint32_t k = key_of(s);
        if (k < lo || (hs < 32 && (k >> hs) != (prefix >> hs))) continue;
        const uint64_t v = MASS ? weight_of(expf(s - m)) : 1;
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&sh.hist[(k >> shift) & (nb - 1)]), (unsigned long long)v);
    }
    __syncthreads();
    if (tid < KIVI_WAVE) {
        const int per = nb / KIVI_WAVE;
        uint64_t tot = 0;
        for (int i = 0; i < per; ++i) tot += sh.hist[lane * per + i];
        uint64_t suf = tot;
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) {
            const uint64_t o = shfl_down64(suf, d);
            if (lane + d < KIVI_WAVE) suf += o;
        }
        const uint64_t total = shfl64(suf, 0);
        uint64_t R = rem;
        if (frac >= 0.0) {                            // first top-p digit: the total is Z_k, the target ceil(top_p * Z_k)
            const double x = frac * (double)total;
            R = (uint64_t)x;
            if ((double)R < x) ++R;
        }
        uint64_t above = suf - tot, best_above = 0;
        int best = 1 << 30;
        for (int i = per - 1; i >= 0; --i) {
            const uint64_t h = sh.hist[lane * per + i];
            if (h && above < R) {
                best = lane * per + i;
                best_above = above;
            }
            above += h;
        }
        int lowest = best;
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) lowest = min(lowest, __shfl_xor(lowest, d));
        if (lowest == (1 << 30)) {                    // nothing of positive weight (a row outside the contract): any bin
            if (lane == 0) {
                sh.sel_bin = 0;
                sh.sel_above = 0;
                sh.sel_rem = R;
            }
        } else if (best == lowest) {
            sh.sel_bin = (uint32_t)best;
            sh.sel_above = best_above;
            sh.sel_rem = R;
        }
    }
    __syncthreads();
    prefix |= sh.sel_bin << shift;
    rem = sh.sel_rem - sh.sel_above;
    __syncthreads();
}

template <bool MASS, class Reader>
__device__ uint32_t radix_select(Shared& sh, const Reader& row, int e0, int e1, float m, uint32_t lo, uint64_t rem, double frac) {
    uint32_t prefix = 0;
    radix_digit<MASS>(sh, row, e0, e1, m, lo, prefix, 21, 11, rem, frac);
    radix_digit<MASS>(sh, row, e0, e1, m, lo, prefix, 10, 11, rem, -1.0);
    radix_digit<MASS>(sh, row, e0, e1, m, lo, prefix, 0, 10, rem, -1.0);
    return prefix;
}

// One row, by the whole workgroup: the body of both kernels.  Every branch below is on values that are the same for all threads of
// the block (the row's parameters, V, BS), so every __syncthreads() is reached by all 1024 threads on every path.
// Counter word 0 of the draw is `c0`, the key `seed`, the draw index `n`.  `row`: the reader of the row's scores (Row, PenRow or
// ConRow).  Returns the token (every thread).
template <class R>
__device__ __forceinline__ int sample_row(Shared& sh, const R& row, int V, int BS, int top_k, float top_p, float min_p, uint32_t c0,
                                          uint64_t seed, int64_t n, int64_t* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbk = (V + BS - 1) / BS, bpw = (nbk + kWaves - 1) / kWaves;
    const int bk0 = min(nbk, wave * bpw), bk1 = min(nbk, (wave + 1) * bpw);
    const int e0 = min(V, bk0 * BS), e1 = min(V, bk1 * BS);

    // max key
    uint32_t mk = 0;
    for (int e = e0 + lane; e < e1; e += KIVI_WAVE) mk = max(mk, key_of(row.s(e)));
#pragma unroll
    for (int d = 1; d < KIVI_WAVE; d <<= 1) mk = max(mk, (uint32_t)__shfl_xor(mk, d));
    if (lane == 0) sh.wmax[wave] = mk;
    __syncthreads();
    mk = 0;
    for (int w = 0; w < kWaves; ++w) mk = max(mk, sh.wmax[w]);
    const float m = float_of(mk);

    // thresholds (keys): top-k, then top-p over the top-k survivors
    uint32_t tk = 0, tp = 0;
    const int k = min(top_k, V);
    if (k > 0 && k < V) tk = radix_select<false>(sh, row, e0, e1, m, 0, (uint64_t)k, -1.0);
    if (top_p < 1.0f) tp = radix_select<true>(sh, row, e0, e1, m, tk, 0, (double)top_p);
    const uint32_t thr = max(tk, tp);
    auto kept_weight = [&](int e) -> uint64_t {
        const float s = row.s(e);
        const float p = expf(s - m);
        return (key_of(s) >= thr && p >= min_p) ? weight_of(p) : 0;
    };

    // draw: bucket sums (bucket b = tokens [b * BS, (b + 1) * BS), owned by one wave), block scan, crossing bucket, crossing token
    for (int b = bk0; b < bk1; ++b) {
        uint64_t acc = 0;
        for (int e = b * BS + lane; e < min(V, (b + 1) * BS); e += KIVI_WAVE) acc += kept_weight(e);
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) acc += shfl_down64(acc, d);
        if (lane == 0) sh.hist[b] = acc;
    }
    if (tid == 0) sh.token = 0;                       // a row with no positive weight (outside the contract) gets token 0
    __syncthreads();
    const uint64_t v = tid < nbk ? sh.hist[tid] : 0;
    uint64_t incl = wave_incl_scan64(v, lane);
    if (lane == 63) sh.wsum[wave] = incl;
    __syncthreads();
    uint64_t S = 0;
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) incl += sh.wsum[w];
        S += sh.wsum[w];
    }
    const uint32_t u24 = philox_x0(c0, 0, (uint32_t)n, (uint32_t)((uint64_t)n >> 32), (uint32_t)seed, (uint32_t)(seed >> 32)) >> 8;
    // floor(S * u24 / 2^24), exactly (S < 2^61)
    const uint64_t target = (S >> 24) * u24 + (((S & 0xFFFFFFu) * u24) >> 24);
    if (S > 0 && tid < nbk && incl - v <= target && target < incl) {
        sh.sel_bucket = (uint32_t)tid;
        sh.sel_base = incl - v;
    }
    __syncthreads();
    if (S > 0 && tid < KIVI_WAVE) {
        const int b = (int)sh.sel_bucket;
        uint64_t base = sh.sel_base;
        for (int j = b * BS; j < min(V, (b + 1) * BS); j += KIVI_WAVE) {
            const int e = j + lane;
            const uint64_t w = e < V ? kept_weight(e) : 0;
            const uint64_t c = wave_incl_scan64(w, lane);
            if (base + c - w <= target && target < base + c) sh.token = (uint32_t)e;
            base += shfl64(c, 63);
        }
    }
    __syncthreads();
    if (tid == 0) *out = (int64_t)sh.token;
    return (int)sh.token;
}

// A greedy row: the lowest index that maximises float(logit) (-0 and +0 tie), the tie rule of kivi_token_logprob's rank.  The key
// image orders -inf below every finite value, so a -inf logit wins only when the whole row is -inf; NaN / +inf rows get some index.
// Returns the token on thread 0 (0 on the others).
template <class R>
__device__ __forceinline__ int greedy_row(Shared& sh, const R& row, int V, int64_t* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t best = 0;                                // (key << 32) | ~index: the maximum is the largest key at the lowest index
    for (int e = tid; e < V; e += kThreads) best = max(best, ((uint64_t)key_of(row.s(e)) << 32) | (uint32_t)~(uint32_t)e);
#pragma unroll
    for (int d = 1; d < KIVI_WAVE; d <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)best, d), hi = __shfl_xor((uint32_t)(best >> 32), d);
        best = max(best, ((uint64_t)hi << 32) | lo);
    }
    if (lane == 0) sh.wsum[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < kWaves; ++w) best = max(best, sh.wsum[w]);
        const uint32_t j = ~(uint32_t)best;
        const uint32_t tok = j < (uint32_t)V ? j : 0;  // (V >= 1: thread 0 always has an entry, so j < V; the guard is for form)
        *out = (int64_t)tok;
        return (int)tok;
    }
    return 0;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_kernel(const T* __restrict__ logits, int64_t row_stride, int V, int BS, float temp,
                                                          int top_k, float top_p, float min_p, const int64_t* __restrict__ state,
                                                          int64_t* __restrict__ out, int64_t out_stride) {
    __shared__ Shared sh;
    sample_row(sh, Row<T>{logits + (int64_t)blockIdx.x * row_stride, temp, temp != 1.0f}, V, BS, top_k, top_p, min_p, blockIdx.x,
               (uint64_t)state[0], state[1], out + (int64_t)blockIdx.x * out_stride);
}

// The row body of sample_rows_kernel over any reader: the greedy or the sampling path -- a block-uniform choice -- over `row`, whose
// temp / div this sets, with the clamps of a record outside the contract (include/kivi_hip.h): it never loops and never indexes
// outside the row.  Returns the token on thread 0.
template <class R>
__device__ __forceinline__ int rows_token(Shared& sh, R row, const kivi_sample_row& r, int V, int BS, int64_t n,
                                          int64_t* __restrict__ dst) {
    const bool greedy = (r.flags & KIVI_SAMPLE_ROW_GREEDY) || !(r.temperature > 0.0f) || !__builtin_isfinite(r.temperature);
    if (greedy) return greedy_row(sh, row, V, dst);                     // (temp 1, no division)
    row.temp = r.temperature;
    row.div = r.temperature != 1.0f;
    const int top_k = max(r.top_k, 0);
    float top_p = r.top_p <= 1.0f ? r.top_p : 1.0f;                     // NaN and > 1: off
    if (!(top_p > 0.0f)) top_p = 1.17549435e-38f;                       // <= 0: the smallest (0, 1] value, the top class alone
    float min_p = r.min_p >= 0.0f ? r.min_p : 0.0f;                     // NaN and < 0: off
    if (min_p >= 1.0f) min_p = 0.99999994f;                             // the largest value below 1: the maximum stays
    return sample_row(sh, row, V, BS, top_k, top_p, min_p, r.stream, (uint64_t)r.seed, n, dst);
}

// The reader of a constrained row: the rule of include/kivi_hip.h -- the list entry's bias or suppression,
// PenRow's penalised logit, the allow mask -- then Row's score.  MASK: the row's allow mask is in force; its word is loaded from
// global memory beside the logit, before anything depends on either (the 64 tokens of a wave's run are two words, which every later
// pass finds in the cache).  LIST: the row has a list or a penalty.  `marks` is then the chunk bitmap of PenRow as 32-bit words with
// the chunks of the listed tokens folded in, and `first[c]` the number of list entries below token 64 c: in a wave whose run of 64
// tokens holds a listed or seen token -- a wave-uniform branch -- the run's entries are list[first[c] .. first[c + 1]), usually one or
// two, compared one by one (three dependent LDS reads under the logit's load, where a binary search per token was ten).  The scan is
// bounded by n_list whatever the list holds.  A token of such a chunk without an entry and with a zero history word only has a
// zero subtracted, as in PenRow.
struct ListEnt {
    uint32_t word, bits;                             // kivi_sample_list_entry with the value as its bits
};
template <typename T, bool MASK, bool LIST>
struct ConRow {
    const T* p;
    float temp;
    bool div;
    PenRow<T> pen;                                   // (its p / temp / div / marks are not used)
    bool penalised;
    const uint32_t* marks;                           // LDS
    const uint16_t* first;                           // LDS
    const ListEnt* list;                             // LDS; NaN values already 0
    bool suppress;                                   // draw_index < suppress_until
    const uint32_t* allow;                           // the row's mask (MASK)
    __device__ __forceinline__ float s(int e) const {
#pragma clang fp contract(off)
        float x = (float)p[e];
        uint32_t aw = 0xFFFFFFFFu;
        if (MASK) aw = allow[e >> 5];
        bool masked = false;
        if (LIST && ((marks[e >> 11] >> ((e >> 6) & 31)) & 1)) {
            const int lo = first[e >> 6], hi = first[(e >> 6) + 1];
            int at = -1;
            for (int j = lo; j < hi; ++j)
                if (at < 0 && (int)(list[j].word & KIVI_LIST_TOKEN) == e) at = j;
            if (at >= 0) {
                const ListEnt ent = list[at];
                if ((ent.word & KIVI_LIST_SUPPRESS) && suppress) masked = true;
                else x = x + __builtin_bit_cast(float, ent.bits);
            }
            if (penalised) x = pen.penalised(x, pen.seen[e]);
        }
        if (!((aw >> (e & 31)) & 1)) masked = true;
        if (masked) x = -__builtin_inff();
        return (div ? x / temp : x) + 0.0f;
    }
};

// The row kernel of kivi_sample_rows, kivi_sample_rows_pen and kivi_sample_rows_con: block b reads rows[b] and draw_index[b], takes
// the greedy or the sampling path and then stores draw_index[b] + 1 itself (one lane, a plain vector store): no second launch.  Every
// thread has read n before the first barrier of either path, and the store comes after the last one.
// The state beyond the records is optional, and every choice below is block-uniform.  `seen` (with `pen`): the
// row's penalty record, clamped as the header says, and its row of the history table; null reads as the neutral record.  `con`
// (section 25): the row's constraint record, with `allow` and `lists`; null reads as the neutral record (flags 0, n_list 0).
// STATE = false is the instantiation for a launch with none of it (kivi_sample_rows): the first line of the table alone, without the
// LDS arrays and record loads of the others, which cost a 32-row launch about 1 % when it carried them.
//   neutral record, not penalised   Row: nothing is loaded from table, masks or lists
//   neutral record, penalised       PenRow, after the row's history is folded into a bitmap of 64-token chunks in LDS (mark_chunks),
//                                   so that the passes touch the table only where something is marked
//   a mask alone                    ConRow<MASK>
//   any other                       ConRow<., LIST>: the list is copied into LDS (n_list clamped, NaN values zeroed), the chunk bitmap
//                                   built -- zeroed, then mark_chunks over the history if the row is penalised, then an LDS atomic OR
//                                   per listed token below V -- and the table first[] (one binary search of the list per chunk)
// With a table thread 0 then counts the token it has just written: one 16-bit load, one plain 16-bit vector store, after the last
// barrier of the row body, so after every read of the table by this block; no other block reads or writes this row of the table.
template <typename T, bool STATE>
__global__ __launch_bounds__(kThreads) void sample_rows_kernel(const T* __restrict__ logits, int64_t row_stride, int V, int BS,
                                                               const kivi_sample_row* __restrict__ rows, int64_t* draw_index,
                                                               const kivi_sample_penalty* __restrict__ pen, uint16_t* seen,
                                                               int64_t seen_stride, const kivi_sample_constraint* __restrict__ con,
                                                               const uint32_t* __restrict__ allow, int64_t allow_stride,
                                                               const kivi_sample_list_entry* __restrict__ lists, int64_t list_stride,
                                                               int64_t* __restrict__ out, int64_t out_stride) {
    __shared__ Shared sh;
    const int b = blockIdx.x;
    const kivi_sample_row r = rows[b];
    const int64_t n = draw_index[b];
    const T* row = logits + (int64_t)b * row_stride;
    uint16_t* hist = (STATE && seen) ? seen + (int64_t)b * seen_stride : nullptr;
    int64_t* dst = out + (int64_t)b * out_stride;
    int tok;
    if constexpr (!STATE) {
        tok = rows_token(sh, Row<T>{row, 1.0f, false}, r, V, BS, n, dst);
    } else {
        __shared__ uint32_t marks[KIVI_SAMPLE_MAX_V / 2048];
        __shared__ ListEnt lst[KIVI_SAMPLE_MAX_LIST];
        __shared__ uint16_t first[KIVI_SAMPLE_MAX_V / 64 + 2];
        float theta = 1.0f, pres = 0.0f, freq = 0.0f;
        if (seen) {
            theta = pen[b].repetition, pres = pen[b].presence, freq = pen[b].frequency;
            if (!(theta > 0.0f) || !__builtin_isfinite(theta)) theta = 1.0f;
            if (!__builtin_isfinite(pres)) pres = 0.0f;
            if (!__builtin_isfinite(freq)) freq = 0.0f;
        }
        const bool penalised = !(theta == 1.0f && pres == 0.0f && freq == 0.0f);
        kivi_sample_constraint c = {};
        if (con) c = con[b];
        const int n_list = lists ? min(max(c.n_list, 0), min(KIVI_SAMPLE_MAX_LIST, (int)list_stride)) : 0;
        const uint32_t* mask = (allow && (c.flags & KIVI_CONSTRAINT_MASK)) ? allow + (int64_t)b * allow_stride : nullptr;
        const PenRow<T> pr{row, 1.0f, false, hist, theta, pres, freq, reinterpret_cast<const uint8_t*>(marks)};
        if (!mask && n_list == 0) {
            if (!penalised) {
                tok = rows_token(sh, Row<T>{row, 1.0f, false}, r, V, BS, n, dst);
            } else {
                mark_chunks(reinterpret_cast<uint8_t*>(marks), hist, V);
                __syncthreads();
                tok = rows_token(sh, pr, r, V, BS, n, dst);
            }
        } else if (n_list == 0 && !penalised) {
            const ConRow<T, true, false> cr{row, 1.0f, false, pr, false, marks, first, lst, false, mask};
            tok = rows_token(sh, cr, r, V, BS, n, dst);
        } else {
            const int tid = threadIdx.x;
            if (tid < KIVI_SAMPLE_MAX_V / 2048) marks[tid] = 0;
            const kivi_sample_list_entry* src = lists + (int64_t)b * list_stride;
            for (int i = tid; i < n_list; i += kThreads) {
                const kivi_sample_list_entry ent = src[i];
                lst[i] = ListEnt{ent.word, __builtin_isnan(ent.value) ? 0u : __builtin_bit_cast(uint32_t, ent.value)};
            }
            __syncthreads();
            if (penalised) {
                mark_chunks(reinterpret_cast<uint8_t*>(marks), hist, V);
                __syncthreads();
            }
            for (int i = tid; i < n_list; i += kThreads) {
                const uint32_t id = lst[i].word & KIVI_LIST_TOKEN;
                if (id < (uint32_t)V) atomicOr(&marks[id >> 11], 1u << ((id >> 6) & 31));
            }
            for (int ch = tid; ch <= (V + 63) / 64; ch += kThreads) {       // first[ch]: the entries below token 64 ch (in [0, n_list])
                int lo = 0, hi = n_list;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((int)(lst[mid].word & KIVI_LIST_TOKEN) < ch * 64) lo = mid + 1;
                    else hi = mid;
                }
                first[ch] = (uint16_t)lo;
            }
            __syncthreads();
            const bool sup = n < c.suppress_until;
            if (mask)
                tok = rows_token(sh, ConRow<T, true, true>{row, 1.0f, false, pr, penalised, marks, first, lst, sup, mask}, r, V, BS, n,
                                 dst);
            else
                tok = rows_token(sh, ConRow<T, false, true>{row, 1.0f, false, pr, penalised, marks, first, lst, sup, mask}, r, V, BS, n,
                                 dst);
        }
    }
    if (threadIdx.x == 0) {
        draw_index[b] = n + 1;
        if (hist) {
            const uint16_t w = hist[tok];                               // tok in [0, V), V <= seen_stride
            if ((w & 0x7FFFu) != 0x7FFFu) hist[tok] = (uint16_t)(w + 1);
        }
    }
}

// kivi_allow_mark: block i serves mask row rows[i] (null: i).  NONE / ALL store the row's ceil(V / 32) words; a fence and a barrier
// put the marks of the same block after them.  A mark is an atomic OR (SET) or AND (UNSET) on the token's 32-bit word.
__global__ __launch_bounds__(256) void allow_mark_kernel(uint32_t* allow, int64_t allow_stride, int V, const int32_t* __restrict__ rows,
                                                         const int64_t* __restrict__ tokens, int64_t tok_row_stride, int T,
                                                         const int32_t* __restrict__ len, int flags) {
    const int i = blockIdx.x;
    const int64_t d = rows ? (int64_t)rows[i] : (int64_t)i;
    if (d < 0) return;                                                  // (block-uniform)
    uint32_t* row = allow + d * allow_stride;
    if (flags & (KIVI_ALLOW_NONE | KIVI_ALLOW_ALL)) {
        const uint32_t fill = (flags & KIVI_ALLOW_ALL) ? 0xFFFFFFFFu : 0u;
        for (int j = threadIdx.x; j < (V + 31) / 32; j += blockDim.x) row[j] = fill;
        __threadfence();
        __syncthreads();
    }
    if (!(flags & (KIVI_ALLOW_SET | KIVI_ALLOW_UNSET))) return;
    const int t1 = len ? min(max(len[i], 0), T) : T;
    const int64_t* tk = tokens + (int64_t)i * tok_row_stride;
    for (int t = threadIdx.x; t < t1; t += blockDim.x) {
        const int64_t id = tk[t];
        if (id < 0 || id >= V) continue;
        if (flags & KIVI_ALLOW_SET) atomicOr(row + (id >> 5), 1u << (id & 31));
        else atomicAnd(row + (id >> 5), ~(1u << (id & 31)));
    }
}

// kivi_seen_mark: block i serves destination row rows[i] (null: i).  CLEAR zeroes the row's seen_stride words with 16-byte stores;
// a fence and a barrier put the marks of the same block after them.  Two tokens share a 32-bit word of the table, so a mark is an
// atomic on that word: an OR of bit 15 (PROMPT), or a compare-and-swap that adds 1 to the 15-bit count unless it is 32767 (OUTPUT;
// a plain add would carry into bit 15).  Each failed swap is another thread's success, so the loop ends.
__global__ __launch_bounds__(256) void seen_mark_kernel(uint16_t* seen, int64_t seen_stride, int V, const int32_t* __restrict__ rows,
                                                        const int64_t* __restrict__ tokens, int64_t tok_row_stride, int T,
                                                        const int32_t* __restrict__ lead, int flags) {
    const int i = blockIdx.x;
    const int64_t d = rows ? (int64_t)rows[i] : (int64_t)i;
    if (d < 0) return;                                                  // (block-uniform)
    uint16_t* hist = seen + d * seen_stride;
    if (flags & KIVI_SEEN_CLEAR) {
        uint4* q = reinterpret_cast<uint4*>(hist);
        for (int64_t j = threadIdx.x; j < seen_stride / 8; j += blockDim.x) q[j] = make_uint4(0, 0, 0, 0);
        __threadfence();
        __syncthreads();
    }
    if (!(flags & (KIVI_SEEN_PROMPT | KIVI_SEEN_OUTPUT))) return;
    const int t0 = lead ? min(max(lead[i], 0), T) : 0;
    unsigned int* words = reinterpret_cast<unsigned int*>(hist);
    const int64_t* tk = tokens + (int64_t)i * tok_row_stride;
    for (int t = t0 + (int)threadIdx.x; t < T; t += blockDim.x) {
        const int64_t id = tk[t];
        if (id < 0 || id >= V) continue;
        unsigned int* w = words + (id >> 1);
        const int sft = (int)(id & 1) * 16;
        if (flags & KIVI_SEEN_PROMPT) {
            atomicOr(w, 0x8000u << sft);
        } else {
            unsigned int old = __atomic_load_n(w, __ATOMIC_RELAXED);
            while (((old >> sft) & 0x7FFFu) != 0x7FFFu) {
                const unsigned int got = atomicCAS(w, old, old + (1u << sft));
                if (got == old) break;
                old = got;
            }
        }
    }
}

__global__ void advance_kernel(int64_t* state) { state[1] += 1; }

}  // namespace

// The bucket of the draw: a power of two, at most 1024 buckets per row.
static int bucket_size(int V) {
    int BS = KIVI_WAVE;
    while ((int64_t)BS * 1024 < V) BS <<= 1;
    return BS;
}

extern "C" int kivi_sample(const void* logits, int logits_bits, int64_t row_stride, int B, int V, float temperature, int top_k,
                           float top_p, float min_p, int64_t* rng_state, int64_t* out_tokens, int64_t out_stride,
                           kivi_stream_t stream) {
    const int esz = kivi_logits_esz(logits_bits);
    KIVI_REQUIRE(esz, KIVI_EINVAL, "kivi_sample: logits_bits=%d (16: fp16, 32: fp32, KIVI_LOGITS_BF16: bf16)", logits_bits);
    KIVI_REQUIRE(B >= 1 && B <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "kivi_sample: B=%d (1 <= B <= %d)", B, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_sample: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(row_stride >= V || B == 1, KIVI_EINVAL, "kivi_sample: row_stride=%lld below V=%d", (long long)row_stride, V);
    KIVI_REQUIRE(out_stride >= 1 || B == 1, KIVI_EINVAL, "kivi_sample: out_stride=%lld", (long long)out_stride);
    KIVI_REQUIRE(temperature > 0.0f && __builtin_isfinite(temperature), KIVI_EINVAL, "kivi_sample: temperature=%g (finite, > 0)",
                 (double)temperature);
    KIVI_REQUIRE(top_k >= 0, KIVI_EINVAL, "kivi_sample: top_k=%d (0 = off)", top_k);
    KIVI_REQUIRE(top_p > 0.0f && top_p <= 1.0f, KIVI_EINVAL, "kivi_sample: top_p=%g (0 < top_p <= 1; 1 = off)", (double)top_p);
    KIVI_REQUIRE(min_p >= 0.0f && min_p < 1.0f, KIVI_EINVAL, "kivi_sample: min_p=%g (0 <= min_p < 1; 0 = off)", (double)min_p);
    KIVI_REQUIRE(logits && rng_state && out_tokens, KIVI_EINVAL, "kivi_sample: null pointer");
    KIVI_REQUIRE((uintptr_t)logits % esz == 0 && (uintptr_t)rng_state % 8 == 0 && (uintptr_t)out_tokens % 8 == 0, KIVI_EALIGN,
                 "kivi_sample: misaligned logits (%d-byte elements), rng_state or out_tokens (8 bytes)", esz);
    const int BS = bucket_size(V);
    const hipStream_t s = (hipStream_t)stream;
    if (logits_bits == 16)
        KIVI_LAUNCH(sample_kernel<f16>, dim3(B), dim3(kThreads), s, (const f16*)logits, row_stride, V, BS, temperature, top_k, top_p,
                    min_p, (const int64_t*)rng_state, out_tokens, out_stride);
    else if (logits_bits == KIVI_LOGITS_BF16)
        KIVI_LAUNCH(sample_kernel<bf16>, dim3(B), dim3(kThreads), s, (const bf16*)logits, row_stride, V, BS, temperature, top_k,
                    top_p, min_p, (const int64_t*)rng_state, out_tokens, out_stride);
    else
        KIVI_LAUNCH(sample_kernel<float>, dim3(B), dim3(kThreads), s, (const float*)logits, row_stride, V, BS, temperature, top_k,
                    top_p, min_p, (const int64_t*)rng_state, out_tokens, out_stride);
    int rc = kivi_launch_status("kivi_sample");
    if (rc) return rc;
    KIVI_LAUNCH(advance_kernel, dim3(1), dim3(1), s, rng_state);
    return kivi_launch_status("kivi_sample (advance)");
}

// The checks and the launch of the three row entries.  `name`: the entry, in front of every message; `required`: whether the
// pointers this entry cannot do without -- beyond logits, rows, draw_index and out_tokens -- are there.  An entry without a table
// or without constraint state passes null pointers and zero strides, which every check from the fourth on lets through.
static int launch_rows(const char* name, bool required, const void* logits, int logits_bits, int64_t row_stride, int B, int V,
                       const kivi_sample_row* rows, int64_t* draw_index, const kivi_sample_penalty* pen, uint16_t* seen,
                       int64_t seen_stride, const kivi_sample_constraint* con, const uint32_t* allow, int64_t allow_stride,
                       const kivi_sample_list_entry* list, int64_t list_stride, int64_t* out_tokens, int64_t out_stride,
                       kivi_stream_t stream) {
    const int esz = kivi_logits_esz(logits_bits);
    KIVI_REQUIRE(esz, KIVI_EINVAL, "%s: logits_bits=%d (16: fp16, 32: fp32, KIVI_LOGITS_BF16: bf16)", name, logits_bits);
    KIVI_REQUIRE(B >= 1 && B <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "%s: B=%d (1 <= B <= %d)", name, B, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "%s: V=%d (1 <= V <= %d)", name, V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(row_stride >= V || B == 1, KIVI_EINVAL, "%s: row_stride=%lld below V=%d", name, (long long)row_stride, V);
    KIVI_REQUIRE(out_stride >= 1 || B == 1, KIVI_EINVAL, "%s: out_stride=%lld", name, (long long)out_stride);
    KIVI_REQUIRE(logits && rows && draw_index && out_tokens && required, KIVI_EINVAL, "%s: null pointer", name);
    KIVI_REQUIRE(!pen == !seen, KIVI_EINVAL, "%s: pen and seen have to be both given or both null", name);
    KIVI_REQUIRE(!seen || seen_stride >= V, KIVI_EINVAL, "%s: seen_stride=%lld below V=%d", name, (long long)seen_stride, V);
    KIVI_REQUIRE(!allow || allow_stride >= (V + 31) / 32, KIVI_EINVAL, "%s: allow_stride=%lld below ceil(V / 32)=%d", name,
                 (long long)allow_stride, (V + 31) / 32);
    KIVI_REQUIRE(list_stride >= 0 && list_stride <= KIVI_SAMPLE_MAX_LIST, KIVI_EINVAL, "%s: list_stride=%lld (0 <= list_stride <= %d)",
                 name, (long long)list_stride, KIVI_SAMPLE_MAX_LIST);
    KIVI_REQUIRE((uintptr_t)logits % esz == 0 && (uintptr_t)rows % 8 == 0 && (uintptr_t)draw_index % 8 == 0 &&
                     (uintptr_t)out_tokens % 8 == 0,
                 KIVI_EALIGN, "%s: misaligned logits (%d-byte elements), rows, draw_index or out_tokens (8 bytes)", name, esz);
    KIVI_REQUIRE((uintptr_t)pen % 4 == 0 && (uintptr_t)seen % 16 == 0 && (!seen || seen_stride % 8 == 0), KIVI_EALIGN,
                 "%s: misaligned pen (4 bytes) or seen (16 bytes), or seen_stride=%lld not a multiple of 8", name, (long long)seen_stride);
    KIVI_REQUIRE((uintptr_t)con % 8 == 0 && (uintptr_t)allow % 16 == 0 && (!allow || allow_stride % 4 == 0) && (uintptr_t)list % 8 == 0,
                 KIVI_EALIGN, "%s: misaligned con or list (8 bytes) or allow (16 bytes), or allow_stride=%lld not a multiple of 4", name,
                 (long long)allow_stride);
    const int BS = bucket_size(V);
    const hipStream_t s = (hipStream_t)stream;
    const bool state = seen || con;                  // neither: the instantiation without their LDS arrays and record loads
#define ROWS_LAUNCH(T, STATE)                                                                                                 \
    KIVI_LAUNCH((sample_rows_kernel<T, STATE>), dim3(B), dim3(kThreads), s, (const T*)logits, row_stride, V, BS, rows, draw_index, pen, \
                seen, seen_stride, con, allow, allow_stride, list, list_stride, out_tokens, out_stride)
    if (logits_bits == 16) {
        if (state) ROWS_LAUNCH(f16, true);
        else ROWS_LAUNCH(f16, false);
    } else if (logits_bits == KIVI_LOGITS_BF16) {
        if (state) ROWS_LAUNCH(bf16, true);
        else ROWS_LAUNCH(bf16, false);
    } else {
        if (state) ROWS_LAUNCH(float, true);
        else ROWS_LAUNCH(float, false);
    }
#undef ROWS_LAUNCH
    return kivi_launch_status(name);
}

extern "C" int kivi_sample_rows(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                                int64_t* draw_index, int64_t* out_tokens, int64_t out_stride, kivi_stream_t stream) {
    return launch_rows("kivi_sample_rows", true, logits, logits_bits, row_stride, B, V, rows, draw_index, nullptr, nullptr, 0, nullptr,
                       nullptr, 0, nullptr, 0, out_tokens, out_stride, stream);
}

extern "C" int kivi_sample_rows_pen(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                                    int64_t* draw_index, const kivi_sample_penalty* pen, uint16_t* seen, int64_t seen_stride,
                                    int64_t* out_tokens, int64_t out_stride, kivi_stream_t stream) {
    return launch_rows("kivi_sample_rows_pen", pen && seen, logits, logits_bits, row_stride, B, V, rows, draw_index, pen, seen,
                       seen_stride, nullptr, nullptr, 0, nullptr, 0, out_tokens, out_stride, stream);
}

extern "C" int kivi_sample_rows_con(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                                    int64_t* draw_index, const kivi_sample_penalty* pen, uint16_t* seen, int64_t seen_stride,
                                    const kivi_sample_constraint* con, const uint32_t* allow, int64_t allow_stride,
                                    const kivi_sample_list_entry* list, int64_t list_stride, int64_t* out_tokens, int64_t out_stride,
                                    kivi_stream_t stream) {
    return launch_rows("kivi_sample_rows_con", con != nullptr, logits, logits_bits, row_stride, B, V, rows, draw_index, pen, seen,
                       seen_stride, con, allow, allow_stride, list, list_stride, out_tokens, out_stride, stream);
}

extern "C" int kivi_seen_mark(uint16_t* seen, int64_t seen_stride, int V, const int32_t* rows, int n, const int64_t* tokens,
                              int64_t tok_row_stride, int T, const int32_t* lead, int flags, kivi_stream_t stream) {
    const int marks = flags & (KIVI_SEEN_PROMPT | KIVI_SEEN_OUTPUT);
    KIVI_REQUIRE(flags != 0 && !(flags & ~(KIVI_SEEN_CLEAR | KIVI_SEEN_PROMPT | KIVI_SEEN_OUTPUT)) &&
                     marks != (KIVI_SEEN_PROMPT | KIVI_SEEN_OUTPUT),
                 KIVI_EINVAL, "kivi_seen_mark: flags=%d (KIVI_SEEN_CLEAR, and at most one of KIVI_SEEN_PROMPT / KIVI_SEEN_OUTPUT)", flags);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_seen_mark: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(n >= 1 && n <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "kivi_seen_mark: n=%d (1 <= n <= %d)", n, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(T >= 0, KIVI_EINVAL, "kivi_seen_mark: T=%d", T);
    KIVI_REQUIRE(seen, KIVI_EINVAL, "kivi_seen_mark: null seen");
    KIVI_REQUIRE(seen_stride >= V, KIVI_EINVAL, "kivi_seen_mark: seen_stride=%lld below V=%d", (long long)seen_stride, V);
    KIVI_REQUIRE(tokens || T == 0 || !marks, KIVI_EINVAL, "kivi_seen_mark: null tokens with T=%d", T);
    KIVI_REQUIRE(tok_row_stride >= T || n == 1, KIVI_EINVAL, "kivi_seen_mark: tok_row_stride=%lld below T=%d",
                 (long long)tok_row_stride, T);
    KIVI_REQUIRE((uintptr_t)seen % 16 == 0 && seen_stride % 8 == 0, KIVI_EALIGN,
                 "kivi_seen_mark: misaligned seen (16 bytes), or seen_stride=%lld not a multiple of 8", (long long)seen_stride);
    KIVI_REQUIRE((uintptr_t)rows % 4 == 0 && (uintptr_t)lead % 4 == 0 && (uintptr_t)tokens % 8 == 0, KIVI_EALIGN,
                 "kivi_seen_mark: misaligned rows or lead (4 bytes) or tokens (8 bytes)");
    const bool mark = marks && T > 0;
    if (!mark && !(flags & KIVI_SEEN_CLEAR)) return 0;                  // nothing to do, nothing enqueued
    KIVI_LAUNCH(seen_mark_kernel, dim3(n), dim3(256), (hipStream_t)stream, seen, seen_stride, V, rows, tokens, tok_row_stride,
                mark ? T : 0, lead, mark ? flags : KIVI_SEEN_CLEAR);
    return kivi_launch_status("kivi_seen_mark");
}

extern "C" int kivi_allow_mark(uint32_t* allow, int64_t allow_stride, int V, const int32_t* rows, int n, const int64_t* tokens,
                               int64_t tok_row_stride, int T, const int32_t* len, int flags, kivi_stream_t stream) {
    const int fill = flags & (KIVI_ALLOW_NONE | KIVI_ALLOW_ALL), marks = flags & (KIVI_ALLOW_SET | KIVI_ALLOW_UNSET);
    KIVI_REQUIRE(flags != 0 && !(flags & ~(KIVI_ALLOW_NONE | KIVI_ALLOW_ALL | KIVI_ALLOW_SET | KIVI_ALLOW_UNSET)) &&
                     fill != (KIVI_ALLOW_NONE | KIVI_ALLOW_ALL) && marks != (KIVI_ALLOW_SET | KIVI_ALLOW_UNSET),
                 KIVI_EINVAL,
                 "kivi_allow_mark: flags=%d (at most one of KIVI_ALLOW_NONE / KIVI_ALLOW_ALL and one of KIVI_ALLOW_SET / KIVI_ALLOW_UNSET)",
                 flags);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_allow_mark: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(n >= 1 && n <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "kivi_allow_mark: n=%d (1 <= n <= %d)", n, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(T >= 0, KIVI_EINVAL, "kivi_allow_mark: T=%d", T);
    KIVI_REQUIRE(allow, KIVI_EINVAL, "kivi_allow_mark: null allow");
    KIVI_REQUIRE(allow_stride >= (V + 31) / 32, KIVI_EINVAL, "kivi_allow_mark: allow_stride=%lld below ceil(V / 32)=%d",
                 (long long)allow_stride, (V + 31) / 32);
    KIVI_REQUIRE(tokens || T == 0 || !marks, KIVI_EINVAL, "kivi_allow_mark: null tokens with T=%d", T);
    KIVI_REQUIRE(tok_row_stride >= T || n == 1, KIVI_EINVAL, "kivi_allow_mark: tok_row_stride=%lld below T=%d",
                 (long long)tok_row_stride, T);
    KIVI_REQUIRE((uintptr_t)allow % 16 == 0 && allow_stride % 4 == 0, KIVI_EALIGN,
                 "kivi_allow_mark: misaligned allow (16 bytes), or allow_stride=%lld not a multiple of 4", (long long)allow_stride);
    KIVI_REQUIRE((uintptr_t)rows % 4 == 0 && (uintptr_t)len % 4 == 0 && (uintptr_t)tokens % 8 == 0, KIVI_EALIGN,
                 "kivi_allow_mark: misaligned rows or len (4 bytes) or tokens (8 bytes)");
    const bool mark = marks && T > 0;
    if (!mark && !fill) return 0;                                       // nothing to do, nothing enqueued
    KIVI_LAUNCH(allow_mark_kernel, dim3(n), dim3(256), (hipStream_t)stream, allow, allow_stride, V, rows, tokens, tok_row_stride,
                mark ? T : 0, len, mark ? flags : fill);
    return kivi_launch_status("kivi_allow_mark");
}
