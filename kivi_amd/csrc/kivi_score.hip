// Fused log-softmax + gather: the log-probability (and rank) of one given token per row (include/kivi_hip.h, kivi_token_logprob;
// DESIGN.md section 14).
//
// One workgroup of 1024 threads per row, rows taken grid-stride (N = B * T rows of a prefill exceed 65535).  Two sweeps of the row:
//   sweep 1       m = max_j x_j and the rank of the target, #{j : x_j > x_t, or x_j == x_t and j < t} (argmax's tie rule)
//   sweep 2       S = sum_j floor(exp(x_j - m) * 2^40), a 64-bit INTEGER sum of the weights kivi_sample draws from
// then lse = m + log(S * 2^-40) and logprob = x_t - lse.  A maximum, a count and an integer sum do not depend on the order of their
// operands, so a row gives the same bits however it is cut: aligned or not, strided or contiguous, eager or replayed from a graph.
// The row is read from memory in both sweeps (the second hits the caches); nothing is staged, no (N, V) fp32 tensor exists, and any
// V up to KIVI_SAMPLE_MAX_V works.  Loads are 16 bytes per lane from the first 16-byte boundary of the row on, with a scalar head
// and tail of fewer than 16 bytes each.  No atomics.
//
// Further down: kivi_token_top_logprobs, the same values plus the k most likely tokens of every row.
#include "kivi_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / KIVI_WAVE;
constexpr float kWScale = 1099511627776.0f;            // 2^40

__device__ __forceinline__ uint64_t weight_of(float e) { return e > 0.0f ? (uint64_t)(e * kWScale) : 0; }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int d) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// What a vector load of T carries per element: T itself, or for bf16 (a struct: no vector of it exists) its 16 bits.
template <typename T>
struct Lane {
    using type = T;
    static __device__ __forceinline__ float value(T v) { return (float)v; }
};
template <>
struct Lane<bf16> {
    using type = uint16_t;
    static __device__ __forceinline__ float value(uint16_t v) { return (float)bf16{v}; }
};

template <typename T>
using vec16 = typename Lane<T>::type __attribute__((ext_vector_type(16 / sizeof(T))));

// f(j, x_j) for every j in [0, V) exactly once over the block: elements [0, head) and the tail one per thread, the rest as
// 16-byte vectors (p + head is 16-byte aligned; head and the tail are shorter than a vector, so shorter than the block).
template <int UNROLL = 2, typename T, typename F>
__device__ __forceinline__ void sweep(const T* __restrict__ p, int V, int head, int nvec, F&& f) {
    constexpr int VEC = 16 / sizeof(T);
    const int tid = threadIdx.x;
    if (tid < head) f(tid, (float)p[tid]);
    const vec16<T>* pv = reinterpret_cast<const vec16<T>*>(p + head);
#pragma unroll UNROLL
    for (int i = tid; i < nvec; i += kThreads) {
        const vec16<T> v = pv[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) f(head + i * VEC + j, Lane<T>::value(v[j]));
    }
    const int e = head + nvec * VEC + tid;
    if (e < V) f(e, (float)p[e]);
}

struct Shared {
    uint64_t wsum[kWaves];
    float wmax[kWaves];
    int wcnt[kWaves];
};

template <typename T>
__global__ __launch_bounds__(kThreads) void token_logprob_kernel(const T* __restrict__ logits, int64_t row_stride, int64_t N, int V,
                                                                 const int64_t* __restrict__ targets, int64_t target_stride,
                                                                 int64_t ignore_index, float* __restrict__ out_logprob,
                                                                 float* __restrict__ out_lse, int32_t* __restrict__ out_rank) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ Shared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t r = blockIdx.x; r < N; r += gridDim.x) {
        const T* p = logits + r * row_stride;
        const int head = min(V, (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) / sizeof(T)));
        const int nvec = (V - head) / VEC;
        const int64_t t = targets[r * target_stride];
        const bool ignored = t == ignore_index;
        const bool scored = !ignored && t >= 0 && t < V;
        const int ti = scored ? (int)t : 0;
        const float xt = (float)p[ti];

        // sweep 1: max, rank
        float m = -__builtin_inff();
        int cnt = 0;
        sweep(p, V, head, nvec, [&](int j, float x) {
            m = __builtin_fmaxf(m, x);
            cnt += (x > xt || (x == xt && j < ti)) ? 1 : 0;
        });
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) {
            m = __builtin_fmaxf(m, __shfl_xor(m, d));
            cnt += __shfl_xor(cnt, d);
        }
        if (lane == 0) {
            sh.wmax[wave] = m;
            sh.wcnt[wave] = cnt;
        }
        __syncthreads();
        m = sh.wmax[0];
        cnt = sh.wcnt[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            m = __builtin_fmaxf(m, sh.wmax[w]);
            cnt += sh.wcnt[w];
        }

        // sweep 2: the integer sum of the weights
        uint64_t S = 0;
        sweep(p, V, head, nvec, [&](int, float x) { S += weight_of(expf(x - m)); });
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) S += shfl_xor64(S, d);
        if (lane == 0) sh.wsum[wave] = S;
        __syncthreads();
        if (tid == 0) {
            S = 0;
            for (int w = 0; w < kWaves; ++w) S += sh.wsum[w];
            const float lse = m + logf((float)S * (1.0f / kWScale));
            out_logprob[r] = ignored ? 0.0f : scored ? xt - lse : __builtin_nanf("");
            if (out_lse) out_lse[r] = lse;
            if (out_rank) out_rank[r] = scored ? cnt : -1;
        }
        __syncthreads();                              // sh is reused by the block's next row
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kivi_token_top_logprobs: the k most likely tokens of a row with their log-probabilities, beside what
// token_logprob_kernel gives.  The order is on the key of x + 0.0f (kivi_sample's order-preserving uint32 image; -0 and +0 one class),
// ties by ascending index.  Per row:
//   sweep 1       m, the target's rank, and the count histogram of the key's top 11 bits
//   digit sweeps  the k-th largest key by radix select (11 + 11 + 10 bits; an fp16 logit's key has constant low 10 bits, so fp16
//                 rows skip the third), then -- only when the class at the threshold holds more tokens than remain to be taken --
//                 the highest index to take, two 10-bit digits over the 20-bit index
//   last sweep    S as above; the exactly k selected (key, index) pairs drop into LDS slots handed out by an integer counter
//   wave 0        orders the pairs by counting and writes ids and x - lse
// Counts, a maximum and an integer sum do not depend on the order of their operands; the slot a pair lands in does, the place it is
// written to does not.  LDS atomics are on integers only.
constexpr int kTopBins = 2048;

__device__ __forceinline__ uint32_t key_of(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct TopShared {
    uint32_t hist[kTopBins];
    uint64_t wsum[kWaves];
    float wmax[kWaves];
    int wcnt[kWaves];
    uint32_t sel_bin, sel_above, sel_cnt, nsel;
    uint32_t pkey[KIVI_TOP_LOGPROBS_MAX];
    int pidx[KIVI_TOP_LOGPROBS_MAX];
};

__device__ __forceinline__ void clear_hist(TopShared& sh, int nb) {
    for (int i = threadIdx.x; i < nb; i += kThreads) sh.hist[i] = 0;
    __syncthreads();
}

// After a digit's histogram is complete: wave 0 finds the one bin b with  #(bins above b) < rem <= #(bins above b) + hist[b]  (the
// bin of the rem-th largest), every thread then takes the digit into `prefix` and the bins above off `rem`.  Returns hist[b].
__device__ __forceinline__ uint32_t pick_bin(TopShared& sh, int nbits, int shift, uint32_t& prefix, uint32_t& rem) {
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < KIVI_WAVE) {
        const int per = (1 << nbits) / KIVI_WAVE;
        uint32_t tot = 0;
#pragma unroll 4
        for (int i = 0; i < per; ++i) tot += sh.hist[lane * per + i];
        uint32_t suf = tot;
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) {
            const uint32_t o = __shfl_down(suf, d);
            if (lane + d < KIVI_WAVE) suf += o;
        }
        uint32_t above = suf - tot, bin = 0, bin_above = 0, bin_cnt = 0;
        bool found = false;
#pragma unroll 4
        for (int i = per - 1; i >= 0; --i) {
            const uint32_t h = sh.hist[lane * per + i];
            if (above < rem && rem <= above + h) {
                bin = (uint32_t)(lane * per + i);
                bin_above = above;
                bin_cnt = h;
                found = true;
            }
            above += h;
        }
        const bool none = __builtin_amdgcn_ballot_w64(found) == 0;   // fewer than rem counted (never inside the contract): any bin
        if (found || (none && lane == 0)) {
            sh.sel_bin = bin;
            sh.sel_above = bin_above;
            sh.sel_cnt = found ? bin_cnt : rem;
        }
    }
    __syncthreads();
    prefix |= __builtin_amdgcn_readfirstlane(sh.sel_bin) << shift;   // block-uniform: keep them scalar
    rem -= __builtin_amdgcn_readfirstlane(sh.sel_above);
    const uint32_t cnt = __builtin_amdgcn_readfirstlane(sh.sel_cnt);
    __syncthreads();                                  // hist and sel_* are rewritten by the next digit
    return cnt;
}

// Every branch around a barrier below is on values that are the same for all threads of the block (arguments, and what pick_bin
// broadcasts through LDS), so every __syncthreads() is reached by all 1024 threads.
template <typename T>
__global__ __launch_bounds__(kThreads) void token_top_logprobs_kernel(const T* __restrict__ logits, int64_t row_stride, int64_t N, int V,
                                                                      int k, const int64_t* __restrict__ targets,
                                                                      int64_t target_stride, int64_t ignore_index,
                                                                      int64_t* __restrict__ out_ids, float* __restrict__ out_top,
                                                                      int64_t top_stride, float* __restrict__ out_logprob,
                                                                      float* __restrict__ out_lse, int32_t* __restrict__ out_rank) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ TopShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t r = blockIdx.x; r < N; r += gridDim.x) {
        const T* p = logits + r * row_stride;
        const int head = min(V, (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) / sizeof(T)));
        const int nvec = (V - head) / VEC;
        const int64_t t = targets ? targets[r * target_stride] : ignore_index;
        const bool ignored = t == ignore_index;
        const bool scored = !ignored && t >= 0 && t < V;
        const int ti = scored ? (int)t : 0;
        const float xt = (float)p[ti];

        if (tid == 0) sh.nsel = 0;
        clear_hist(sh, kTopBins);

        // sweep 1: max, rank, first digit
        float m = -__builtin_inff();
        int cnt = 0;
        sweep<1>(p, V, head, nvec, [&](int j, float x) {
            m = __builtin_fmaxf(m, x);
            cnt += (x > xt || (x == xt && j < ti)) ? 1 : 0;
            atomicAdd(&sh.hist[key_of(x + 0.0f) >> 21], 1u);
        });
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) {
            m = __builtin_fmaxf(m, __shfl_xor(m, d));
            cnt += __shfl_xor(cnt, d);
        }
        if (lane == 0) {
            sh.wmax[wave] = m;
            sh.wcnt[wave] = cnt;
        }
        uint32_t thr = 0, rem = (uint32_t)k;
        uint32_t cls = pick_bin(sh, 11, 21, thr, rem);            // (its first barrier publishes wmax / wcnt too)
        m = sh.wmax[0];
        cnt = sh.wcnt[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            m = __builtin_fmaxf(m, sh.wmax[w]);
            cnt += sh.wcnt[w];
        }

        // the k-th largest key
        clear_hist(sh, kTopBins);
        sweep<1>(p, V, head, nvec, [&](int, float x) {
            const uint32_t key = key_of(x + 0.0f);
            if ((key >> 21) == (thr >> 21)) atomicAdd(&sh.hist[(key >> 10) & 2047u], 1u);
        });
        cls = pick_bin(sh, 11, 10, thr, rem);
        if constexpr (sizeof(T) == 4) {
            clear_hist(sh, 1024);
            sweep<1>(p, V, head, nvec, [&](int, float x) {
                const uint32_t key = key_of(x + 0.0f);
                if ((key >> 10) == (thr >> 10)) atomicAdd(&sh.hist[key & 1023u], 1u);
            });
            cls = pick_bin(sh, 10, 0, thr, rem);
        } else {
            // a 2-byte element's fp32 image has zero bits at the bottom, 13 (fp16) or 16 (bf16) -- x + 0.0f keeps them: an exact sum,
            // and a NaN keeps its payload -- so the key's low 10 bits are all 0 (sign clear: key = u | 2^31) or all 1 (set: key = ~u)
            thr |= (thr & 0x80000000u) ? 0u : 1023u;
        }

        // the class at the threshold straddles the cut: take its `rem` lowest indices (the largest of ~j, as 20 bits)
        int last = 0x7FFFFFFF;
        if (cls > rem) {
            uint32_t ithr = 0;
            clear_hist(sh, 1024);
            sweep<1>(p, V, head, nvec, [&](int j, float x) {
                if (key_of(x + 0.0f) == thr) atomicAdd(&sh.hist[(~(uint32_t)j >> 10) & 1023u], 1u);
            });
            pick_bin(sh, 10, 10, ithr, rem);
            clear_hist(sh, 1024);
            sweep<1>(p, V, head, nvec, [&](int j, float x) {
                const uint32_t ik = ~(uint32_t)j & 0xFFFFFu;
                if (key_of(x + 0.0f) == thr && (ik >> 10) == (ithr >> 10)) atomicAdd(&sh.hist[ik & 1023u], 1u);
            });
            pick_bin(sh, 10, 0, ithr, rem);
            last = (int)(~ithr & 0xFFFFFu);
        }

        // last sweep: the integer sum of the weights; the selected pairs
        uint64_t S = 0;
        sweep<1>(p, V, head, nvec, [&](int j, float x) {
            S += weight_of(expf(x - m));
            const uint32_t key = key_of(x + 0.0f);
            if (key > thr || (key == thr && j <= last)) {
                const uint32_t slot = atomicAdd(&sh.nsel, 1u);
                if (slot < (uint32_t)KIVI_TOP_LOGPROBS_MAX) {
                    sh.pkey[slot] = key;
                    sh.pidx[slot] = j;
                }
            }
        });
#pragma unroll
        for (int d = 1; d < KIVI_WAVE; d <<= 1) S += shfl_xor64(S, d);
        if (lane == 0) sh.wsum[wave] = S;
        __syncthreads();
        if (tid < KIVI_WAVE) {
            S = 0;
            for (int w = 0; w < kWaves; ++w) S += sh.wsum[w];
            const float lse = m + logf((float)S * (1.0f / kWScale));
            const int n = min((int)sh.nsel, k);
            if (lane < n) {
                const uint32_t key = sh.pkey[lane];
                const int idx = sh.pidx[lane];
                int pos = 0;
                for (int i = 0; i < n; ++i) {
                    const uint32_t ki = sh.pkey[i];
                    pos += (ki > key || (ki == key && sh.pidx[i] < idx)) ? 1 : 0;
                }
                out_ids[r * top_stride + pos] = idx;
                out_top[r * top_stride + pos] = (float)p[idx] - lse;
            }
            if (lane == 0) {
                if (out_logprob) out_logprob[r] = ignored ? 0.0f : scored ? xt - lse : __builtin_nanf("");
                if (out_lse) out_lse[r] = lse;
                if (out_rank) out_rank[r] = scored ? cnt : -1;
            }
        }
        __syncthreads();                              // sh is reused by the block's next row
    }
}

}  // namespace

extern "C" int kivi_token_top_logprobs(const void* logits, int logits_bits, int64_t row_stride, int64_t N, int V, int k,
                                       const int64_t* targets, int64_t target_stride, int64_t ignore_index, int64_t* out_top_ids,
                                       float* out_top_logprobs, int64_t top_stride, float* out_logprob, float* out_lse,
                                       int32_t* out_rank, kivi_stream_t stream) {
    const int esz = kivi_logits_esz(logits_bits);
    KIVI_REQUIRE(esz, KIVI_EINVAL, "kivi_token_top_logprobs: logits_bits=%d (16: fp16, 32: fp32, KIVI_LOGITS_BF16: bf16)", logits_bits);
    KIVI_REQUIRE(N >= 1, KIVI_EINVAL, "kivi_token_top_logprobs: N=%lld (N >= 1)", (long long)N);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_token_top_logprobs: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(k >= 1 && k <= V && k <= KIVI_TOP_LOGPROBS_MAX, KIVI_EINVAL, "kivi_token_top_logprobs: k=%d (1 <= k <= min(V, %d))", k,
                 KIVI_TOP_LOGPROBS_MAX);
    KIVI_REQUIRE(row_stride >= V || N == 1, KIVI_EINVAL, "kivi_token_top_logprobs: row_stride=%lld below V=%d", (long long)row_stride,
                 V);
    KIVI_REQUIRE(top_stride >= k || N == 1, KIVI_EINVAL, "kivi_token_top_logprobs: top_stride=%lld below k=%d", (long long)top_stride,
                 k);
    KIVI_REQUIRE(logits && out_top_ids && out_top_logprobs, KIVI_EINVAL, "kivi_token_top_logprobs: null pointer");
    if (targets) {
        KIVI_REQUIRE(target_stride >= 1 || N == 1, KIVI_EINVAL, "kivi_token_top_logprobs: target_stride=%lld",
                     (long long)target_stride);
        KIVI_REQUIRE(out_logprob, KIVI_EINVAL, "kivi_token_top_logprobs: targets without out_logprob");
    } else {
        KIVI_REQUIRE(!out_logprob && !out_rank, KIVI_EINVAL, "kivi_token_top_logprobs: out_logprob or out_rank without targets");
    }
    KIVI_REQUIRE((uintptr_t)logits % esz == 0 && (uintptr_t)targets % 8 == 0 && (uintptr_t)out_top_ids % 8 == 0 &&
                     (uintptr_t)out_top_logprobs % 4 == 0 && (uintptr_t)out_logprob % 4 == 0 && (uintptr_t)out_lse % 4 == 0 &&
                     (uintptr_t)out_rank % 4 == 0,
                 KIVI_EALIGN, "kivi_token_top_logprobs: misaligned logits (%d-byte elements), targets or out_top_ids (8 bytes), "
                 "out_top_logprobs, out_logprob, out_lse or out_rank (4 bytes)", esz);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(N < KIVI_SAMPLE_MAX_B ? N : KIVI_SAMPLE_MAX_B));
    if (logits_bits == 16)
        KIVI_LAUNCH(token_top_logprobs_kernel<f16>, grid, dim3(kThreads), s, (const f16*)logits, row_stride, N, V, k, targets,
                    target_stride, ignore_index, out_top_ids, out_top_logprobs, top_stride, out_logprob, out_lse, out_rank);
    else if (logits_bits == KIVI_LOGITS_BF16)
        KIVI_LAUNCH(token_top_logprobs_kernel<bf16>, grid, dim3(kThreads), s, (const bf16*)logits, row_stride, N, V, k, targets,
                    target_stride, ignore_index, out_top_ids, out_top_logprobs, top_stride, out_logprob, out_lse, out_rank);
    else
        KIVI_LAUNCH(token_top_logprobs_kernel<float>, grid, dim3(kThreads), s, (const float*)logits, row_stride, N, V, k, targets,
                    target_stride, ignore_index, out_top_ids, out_top_logprobs, top_stride, out_logprob, out_lse, out_rank);
    return kivi_launch_status("kivi_token_top_logprobs");
}

extern "C" int kivi_token_logprob(const void* logits, int logits_bits, int64_t row_stride, int64_t N, int V, const int64_t* targets,
                                  int64_t target_stride, int64_t ignore_index, float* out_logprob, float* out_lse,
                                  int32_t* out_rank, kivi_stream_t stream) {
    const int esz = kivi_logits_esz(logits_bits);
    KIVI_REQUIRE(esz, KIVI_EINVAL, "kivi_token_logprob: logits_bits=%d (16: fp16, 32: fp32, KIVI_LOGITS_BF16: bf16)", logits_bits);
    KIVI_REQUIRE(N >= 1, KIVI_EINVAL, "kivi_token_logprob: N=%lld (N >= 1)", (long long)N);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_token_logprob: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(row_stride >= V || N == 1, KIVI_EINVAL, "kivi_token_logprob: row_stride=%lld below V=%d", (long long)row_stride, V);
    KIVI_REQUIRE(target_stride >= 1 || N == 1, KIVI_EINVAL, "kivi_token_logprob: target_stride=%lld", (long long)target_stride);
    KIVI_REQUIRE(logits && targets && out_logprob, KIVI_EINVAL, "kivi_token_logprob: null pointer");
    KIVI_REQUIRE((uintptr_t)logits % esz == 0 && (uintptr_t)targets % 8 == 0 && (uintptr_t)out_logprob % 4 == 0 &&
                     (uintptr_t)out_lse % 4 == 0 && (uintptr_t)out_rank % 4 == 0,
                 KIVI_EALIGN, "kivi_token_logprob: misaligned logits (%d-byte elements), targets (8 bytes), out_logprob, out_lse or "
                 "out_rank (4 bytes)", esz);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(N < KIVI_SAMPLE_MAX_B ? N : KIVI_SAMPLE_MAX_B));
    if (logits_bits == 16)
        KIVI_LAUNCH(token_logprob_kernel<f16>, grid, dim3(kThreads), s, (const f16*)logits, row_stride, N, V, targets, target_stride,
                    ignore_index, out_logprob, out_lse, out_rank);
    else if (logits_bits == KIVI_LOGITS_BF16)
        KIVI_LAUNCH(token_logprob_kernel<bf16>, grid, dim3(kThreads), s, (const bf16*)logits, row_stride, N, V, targets, target_stride,
                    ignore_index, out_logprob, out_lse, out_rank);
    else
        KIVI_LAUNCH(token_logprob_kernel<float>, grid, dim3(kThreads), s, (const float*)logits, row_stride, N, V, targets,
                    target_stride, ignore_index, out_logprob, out_lse, out_rank);
    return kivi_launch_status("kivi_token_logprob");
}
