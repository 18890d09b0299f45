// kivi_stop_rows (include/kivi_hip.h): the finish tracker of a decode batch -- stop token ids, stop sequences
// and a length limit per row -- advanced by one token per row in ONE launch of ONE workgroup, which then counts the live rows of the
// whole table.  The work is integer compares: at most 16 ids and 8 x 16 sequence positions per row.
//
// Lanes: 16 per entry, 4 entries per wave, 16 per pass of the 256-thread workgroup.  Lane l of an entry's group holds ring slot l as
// it is AFTER the new token entered, compares ids[l] with the token, and position l of every sequence with the ring slot that
// position falls on (a 16-lane shuffle fetches it).  A wave ballot gathers the group's 16 verdicts; the group's lane 0 decides and
// writes the three state words, the lane of the new slot writes the ring word.  Every lane of a wave executes every ballot and
// shuffle: what depends on the entry (in range? live?) is a predicate on values, never a branch around them.
#include "kivi_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLanes = KIVI_STOP_MAX_LEN;            // lanes per entry
constexpr int kPerPass = kThreads / kLanes;          // entries per pass
static_assert(KIVI_STOP_MAX_IDS == kLanes && KIVI_STOP_MAX_LEN == 16 && KIVI_WAVE % kLanes == 0, "one lane per id and per position");
static_assert(sizeof(kivi_stop_params) == 624 && sizeof(kivi_stop_state) == 80, "record layouts of include/kivi_hip.h");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename R>
__global__ __launch_bounds__(kThreads) void stop_rows_kernel(int64_t* tokens, int64_t tok_stride, const kivi_stop_params* __restrict__ params,
                                                             kivi_stop_state* state, const R* __restrict__ rows, int n, int B,
                                                             int64_t pad, int32_t* n_live) {
    __shared__ int s_live[kThreads / KIVI_WAVE];
    const int l = threadIdx.x & (kLanes - 1), grp = threadIdx.x / kLanes;
    const int sh = (threadIdx.x & (KIVI_WAVE - 1)) & ~(kLanes - 1);         // where this group's verdicts sit in a wave ballot
    for (int base = 0; base < n; base += kPerPass) {                        // (block-uniform)
        const int i = base + grp;
        int64_t r = -1;
        if (i < n) r = rows ? (int64_t)rows[i] : (int64_t)i;
        const bool act = r >= 0 && r < B;                                   // group-uniform, as everything derived from r alone
        const kivi_stop_params* p = params + (act ? r : 0);
        kivi_stop_state* st = state + (act ? r : 0);
        int64_t t = -1;
        int produced = 0, reason = KIVI_STOP_TOKEN;
        if (act) {
            t = tokens[(int64_t)i * tok_stride];
            produced = st->produced;
            reason = st->reason;
        }
        const bool live = act && reason == KIVI_STOP_LIVE;
        const int32_t t32 = (t >= 0 && t <= 0x7FFFFFFFLL) ? (int32_t)t : -1;
        produced += live ? 1 : 0;
        const int slot = (produced - 1) & (kLanes - 1);
        int32_t ring = -1;                                                  // slot l of the ring with t in it
        int n_ids = 0, n_seqs = 0, limit = 0;
        if (live) {
            ring = l == slot ? t32 : st->ring[l];
            n_ids = clampi(p->n_ids, 0, KIVI_STOP_MAX_IDS);
            n_seqs = clampi(p->n_seqs, 0, KIVI_STOP_MAX_SEQS);
            limit = p->limit;
        }
        const bool id_hit = l < n_ids && t32 >= 0 && p->ids[l] == t32;      // (l < n_ids only in a live group: p is the row's)
        const unsigned id_bits = (unsigned)(__ballot(id_hit) >> sh) & 0xFFFFu;
        unsigned seq_bits = 0;
#pragma unroll
        for (int j = 0; j < KIVI_STOP_MAX_SEQS; j++) {
            const int m = j < n_seqs ? p->seq_len[j] : 0;
            const bool valid = m >= 1 && m <= KIVI_STOP_MAX_LEN && m <= produced;
            // position l of the sequence is produced token (produced - m + l), 0-based: ring slot (produced - m + l) % 16
            const int32_t have = __shfl(ring, (produced - (valid ? m : 0) + l) & (kLanes - 1), kLanes);
            const bool bad = valid && l < m && (have < 0 || p->seq[j][l] != have);
            const unsigned bad_bits = (unsigned)(__ballot(bad) >> sh) & 0xFFFFu;
            if (valid && bad_bits == 0) seq_bits |= 1u << j;
        }
        if (live) {
            if (l == slot) st->ring[slot] = t32;
            if (l == 0) {
                int why = KIVI_STOP_LIVE, index = -1;
                if (id_bits) {
                    why = KIVI_STOP_TOKEN;
                    index = __builtin_ctz(id_bits);
                } else if (seq_bits) {
                    why = KIVI_STOP_SEQUENCE;
                    index = __builtin_ctz(seq_bits);
                } else if (limit >= 1 && produced >= limit) {
                    why = KIVI_STOP_LENGTH;
                }
                st->produced = produced;
                st->reason = why;
                st->index = index;
            }
        } else if (act && l == 0) {
            tokens[(int64_t)i * tok_stride] = pad;                          // a finished row stays finished whatever it is fed
        }
    }
    __syncthreads();                                                        // the state words written above, now read by other lanes
    int c = 0;
    for (int r = threadIdx.x; r < B; r += kThreads) c += state[r].reason == KIVI_STOP_LIVE ? 1 : 0;
#pragma unroll
    for (int m = 1; m < KIVI_WAVE; m <<= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & (KIVI_WAVE - 1)) == 0) s_live[threadIdx.x / KIVI_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < kThreads / KIVI_WAVE; w++) total += s_live[w];
        *n_live = total;
    }
}

}  // namespace

extern "C" int kivi_stop_rows(int64_t* tokens, int64_t tok_stride, const kivi_stop_params* params, kivi_stop_state* state,
                              const void* rows, int rows_bytes, int n, int B, int64_t pad, int32_t* n_live, kivi_stream_t stream) {
    KIVI_REQUIRE(B >= 1 && B <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "kivi_stop_rows: B=%d (1 <= B <= %d)", B, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(n >= 0 && n <= KIVI_SAMPLE_MAX_B, KIVI_EINVAL, "kivi_stop_rows: n=%d (0 <= n <= %d)", n, KIVI_SAMPLE_MAX_B);
    KIVI_REQUIRE(rows || n <= B, KIVI_EINVAL, "kivi_stop_rows: n=%d entries for B=%d rows without a rows map", n, B);
    KIVI_REQUIRE(!rows || rows_bytes == 4 || rows_bytes == 8, KIVI_EINVAL, "kivi_stop_rows: rows_bytes=%d (4: int32, 8: int64)", rows_bytes);
    KIVI_REQUIRE(tok_stride >= 1 || n <= 1, KIVI_EINVAL, "kivi_stop_rows: tok_stride=%lld", (long long)tok_stride);
    KIVI_REQUIRE(params && state && n_live, KIVI_EINVAL, "kivi_stop_rows: null params, state or n_live");
    KIVI_REQUIRE(tokens || n == 0, KIVI_EINVAL, "kivi_stop_rows: null tokens with n=%d", n);
    KIVI_REQUIRE((uintptr_t)tokens % 8 == 0 && (uintptr_t)params % 8 == 0 && (uintptr_t)state % 8 == 0, KIVI_EALIGN,
                 "kivi_stop_rows: misaligned tokens, params or state (8 bytes)");
    KIVI_REQUIRE((!rows || (uintptr_t)rows % rows_bytes == 0) && (uintptr_t)n_live % 4 == 0, KIVI_EALIGN,
                 "kivi_stop_rows: misaligned rows (%d bytes) or n_live (4 bytes)", rows_bytes);
    const hipStream_t s = (hipStream_t)stream;
    if (rows && rows_bytes == 8)
        KIVI_LAUNCH(stop_rows_kernel<int64_t>, dim3(1), dim3(kThreads), s, tokens, tok_stride, params, state, (const int64_t*)rows, n, B,
                    pad, n_live);
    else
        KIVI_LAUNCH(stop_rows_kernel<int32_t>, dim3(1), dim3(kThreads), s, tokens, tok_stride, params, state, (const int32_t*)rows, n, B,
                    pad, n_live);
    return kivi_launch_status("kivi_stop_rows");
}
