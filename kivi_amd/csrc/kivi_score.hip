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

template <typename T>
using vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));

// f(j, x_j) for every j in [0, V) exactly once over the block: elements [0, head) and the tail one per thread, the rest as
// 16-byte vectors (p + head is 16-byte aligned; head and the tail are shorter than a vector, so shorter than the block).
template <typename T, typename F>
__device__ __forceinline__ void sweep(const T* __restrict__ p, int V, int head, int nvec, F&& f) {
    constexpr int VEC = 16 / sizeof(T);
    const int tid = threadIdx.x;
    if (tid < head) f(tid, (float)p[tid]);
    const vec16<T>* pv = reinterpret_cast<const vec16<T>*>(p + head);
#pragma unroll 2
    for (int i = tid; i < nvec; i += kThreads) {
        const vec16<T> v = pv[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) f(head + i * VEC + j, (float)v[j]);
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

}  // namespace

extern "C" int kivi_token_logprob(const void* logits, int logits_bits, int64_t row_stride, int64_t N, int V, const int64_t* targets,
                                  int64_t target_stride, int64_t ignore_index, float* out_logprob, float* out_lse,
                                  int32_t* out_rank, kivi_stream_t stream) {
    KIVI_REQUIRE(logits_bits == 16 || logits_bits == 32, KIVI_EINVAL, "kivi_token_logprob: logits_bits=%d (16: fp16, 32: fp32)",
                 logits_bits);
    KIVI_REQUIRE(N >= 1, KIVI_EINVAL, "kivi_token_logprob: N=%lld (N >= 1)", (long long)N);
    KIVI_REQUIRE(V >= 1 && V <= KIVI_SAMPLE_MAX_V, KIVI_EINVAL, "kivi_token_logprob: V=%d (1 <= V <= %d)", V, KIVI_SAMPLE_MAX_V);
    KIVI_REQUIRE(row_stride >= V || N == 1, KIVI_EINVAL, "kivi_token_logprob: row_stride=%lld below V=%d", (long long)row_stride, V);
    KIVI_REQUIRE(target_stride >= 1 || N == 1, KIVI_EINVAL, "kivi_token_logprob: target_stride=%lld", (long long)target_stride);
    KIVI_REQUIRE(logits && targets && out_logprob, KIVI_EINVAL, "kivi_token_logprob: null pointer");
    const int esz = logits_bits / 8;
    KIVI_REQUIRE((uintptr_t)logits % esz == 0 && (uintptr_t)targets % 8 == 0 && (uintptr_t)out_logprob % 4 == 0 &&
                     (uintptr_t)out_lse % 4 == 0 && (uintptr_t)out_rank % 4 == 0,
                 KIVI_EALIGN, "kivi_token_logprob: misaligned logits (%d-byte elements), targets (8 bytes), out_logprob, out_lse or "
                 "out_rank (4 bytes)", esz);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(N < KIVI_SAMPLE_MAX_B ? N : KIVI_SAMPLE_MAX_B));
    if (logits_bits == 16)
        KIVI_LAUNCH(token_logprob_kernel<f16>, grid, dim3(kThreads), s, (const f16*)logits, row_stride, N, V, targets, target_stride,
                    ignore_index, out_logprob, out_lse, out_rank);
    else
        KIVI_LAUNCH(token_logprob_kernel<float>, grid, dim3(kThreads), s, (const float*)logits, row_stride, N, V, targets,
                    target_stride, ignore_index, out_logprob, out_lse, out_rank);
    return kivi_launch_status("kivi_token_logprob");
}
