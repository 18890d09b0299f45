// Snapshot of cache rows into a flat buffer and back (checkpoint / rollback): for every row b the byte
// ranges a list of slab descriptors names (include/kivi_hip.h, kivi_reorder_slab) are gathered into buf + b * buf_row_stride, slab
// after slab, each slab starting on a 16-byte boundary of the row (direction 0), or scattered back from there (direction 1).
//
// One launch.  A workgroup owns (row, chunk of one slab): kThreads * kInFlight units (16 bytes, or 4 for slabs that are only word
// aligned, such as the range words) of one row.  A thread takes units chunk + j * kThreads + tid, j < kInFlight: it works out the
// kInFlight source / destination pairs first, issues all of its loads, and only then stores -- kInFlight independent 16-byte loads
// per thread are in flight before the first store waits for one (the reorder kernel has one: DESIGN.md section 11).  Consecutive
// lanes touch consecutive units, in the cache (inside a run) and in the buffer.  No LDS, no scratch; every byte is read once and
// written once.
#include "kivi_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;
constexpr int kChunk = kThreads * kInFlight;   // units per workgroup

struct SSlab {
    char* base;
    int64_t rs, s0, s1, s2;
    int64_t boff;                        // byte offset of the slab inside a buffer row (a multiple of 16)
    uint32_t n1, n2, upr;                // level counts 1 and 2, units per run
    uint32_t units;                      // units per row (n0 * n1 * n2 * upr)
    uint32_t chunk0;                     // first chunk (blockIdx.x) of this slab
    uint32_t unit;                       // 16 or 4 bytes
};

struct SArgs {
    SSlab s[KIVI_REORDER_MAX_SLABS];
    char* buf;
    int64_t brs;
    int ns;
};

// FULL: every unit of the workgroup's chunk exists (all but the last chunk of a slab) -- no lane is masked, so the four loads and
// the four stores are straight-line code and no store waits for the one before it
template <typename T, bool SCATTER, bool FULL>
__device__ __forceinline__ void move_units(const SSlab& S, char* row, char* brow, uint32_t u0) {
    char* c[kInFlight];
    char* d[kInFlight];
    bool live[kInFlight];
    const bool flat = S.n1 == 1 && S.n2 == 1;          // one (count, stride) level: what the fp16 residual and window are
#pragma unroll
    for (int j = 0; j < kInFlight; ++j) {
        const uint32_t u = u0 + (uint32_t)j * kThreads;
        live[j] = FULL || u < S.units;
        uint32_t piece = live[j] ? u / S.upr : 0;
        const uint32_t w = live[j] ? u - piece * S.upr : 0;
        int64_t off = (int64_t)w * (int64_t)sizeof(T);
        if (flat) {
            off += (int64_t)piece * S.s0;
        } else {
            const uint32_t i2 = piece % S.n2;
            piece /= S.n2;
            off += (int64_t)(piece / S.n1) * S.s0 + (int64_t)(piece % S.n1) * S.s1 + (int64_t)i2 * S.s2;
        }
        c[j] = row + off;
        d[j] = brow + (int64_t)(live[j] ? u : 0) * (int64_t)sizeof(T);
    }
    T v[kInFlight];
#pragma unroll
    for (int j = 0; j < kInFlight; ++j)
        if (live[j]) v[j] = *reinterpret_cast<const T*>(SCATTER ? d[j] : c[j]);
#pragma unroll
    for (int j = 0; j < kInFlight; ++j)
        if (live[j]) *reinterpret_cast<T*>(SCATTER ? c[j] : d[j]) = v[j];
}

template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void snapshot_rows_kernel(const SArgs a) {
    // the slab of this chunk: the last one whose first chunk is <= blockIdx.x (constant indices: the descriptors stay in kernarg)
    SSlab S = a.s[0];
#pragma unroll
    for (int i = 1; i < KIVI_REORDER_MAX_SLABS; ++i)
        if (i < a.ns && blockIdx.x >= a.s[i].chunk0) S = a.s[i];
    const int64_t b = blockIdx.y;
    char* row = S.base + b * S.rs;
    char* brow = a.buf + b * a.brs + S.boff;
    const uint32_t u0 = (blockIdx.x - S.chunk0) * (uint32_t)kChunk + threadIdx.x;
    const bool full = (blockIdx.x - S.chunk0 + 1) * (uint32_t)kChunk <= S.units;      // (host: units < 2^31, no overflow)
    if (S.unit == 16) {
        if (full) move_units<u32x4, SCATTER, true>(S, row, brow, u0);
        else move_units<u32x4, SCATTER, false>(S, row, brow, u0);
    } else {
        move_units<uint32_t, SCATTER, false>(S, row, brow, u0);
    }
}

}  // namespace

extern "C" int kivi_cache_snapshot(const kivi_reorder_slab* slabs, int n_slabs, int B, void* buf, size_t buf_row_stride, int direction,
                                   kivi_stream_t stream) {
    KIVI_REQUIRE(n_slabs >= 1 && n_slabs <= KIVI_REORDER_MAX_SLABS, KIVI_EINVAL, "kivi_cache_snapshot: n_slabs=%d (1 .. %d)", n_slabs,
                 KIVI_REORDER_MAX_SLABS);
    KIVI_REQUIRE(B >= 1 && B < 65536, KIVI_EINVAL, "kivi_cache_snapshot: B=%d (1 .. 65535 rows)", B);
    KIVI_REQUIRE(slabs && buf, KIVI_EINVAL, "kivi_cache_snapshot: null slabs / buffer");
    KIVI_REQUIRE(direction == 0 || direction == 1, KIVI_EINVAL, "kivi_cache_snapshot: direction=%d (0 = gather into the buffer, 1 = scatter back)",
                 direction);
    KIVI_REQUIRE(buf_row_stride > 0 && buf_row_stride < ((size_t)1 << 62), KIVI_EINVAL, "kivi_cache_snapshot: buf_row_stride=%zu", buf_row_stride);
    KIVI_REQUIRE((uintptr_t)buf % 16 == 0 && buf_row_stride % 16 == 0, KIVI_EALIGN,
                 "kivi_cache_snapshot: the buffer and its row stride must be multiples of 16 bytes");
    SArgs a = {};
    a.buf = (char*)buf;
    a.brs = (int64_t)buf_row_stride;
    int64_t chunks = 0, row_bytes = 0;
    for (int i = 0; i < n_slabs; ++i) {
        const kivi_reorder_slab& s = slabs[i];
        KIVI_REQUIRE(s.n[0] >= 0 && s.n[1] >= 0 && s.n[2] >= 0 && s.run >= 0, KIVI_EINVAL, "kivi_cache_snapshot: slab %d: negative count", i);
        if (s.n[0] == 0 || s.n[1] == 0 || s.n[2] == 0 || s.run == 0) continue;       // nothing to move, no room in the buffer row
        KIVI_REQUIRE(s.base, KIVI_EINVAL, "kivi_cache_snapshot: slab %d: null base", i);
        const uint64_t bits = (uint64_t)(uintptr_t)s.base | (uint64_t)s.row_stride | (uint64_t)s.stride[0] | (uint64_t)s.stride[1] |
                              (uint64_t)s.stride[2] | (uint64_t)s.run;
        KIVI_REQUIRE(bits % 4 == 0, KIVI_EALIGN, "kivi_cache_snapshot: slab %d: base / strides / run not multiples of 4 bytes", i);
        const uint32_t unit = bits % 16 == 0 ? 16 : 4;
        const int64_t upr = s.run / unit;
        int64_t units = 1;
        bool fits = true;
        for (int64_t f : {s.n[0], s.n[1], s.n[2], upr}) {
            fits = fits && f < (1LL << 31) && units * f < (1LL << 31);
            units = fits ? units * f : 1;
        }
        KIVI_REQUIRE(fits, KIVI_EINVAL, "kivi_cache_snapshot: slab %d: 2^31 units per row or more", i);
        SSlab& d = a.s[a.ns++];
        d.base = (char*)s.base;
        d.rs = s.row_stride;
        d.s0 = s.stride[0];
        d.s1 = s.stride[1];
        d.s2 = s.stride[2];
        d.boff = row_bytes;
        d.n1 = (uint32_t)s.n[1];
        d.n2 = (uint32_t)s.n[2];
        d.upr = (uint32_t)upr;
        d.units = (uint32_t)units;
        d.chunk0 = (uint32_t)chunks;
        d.unit = unit;
        row_bytes += (units * unit + 15) / 16 * 16;
        chunks += (units + kChunk - 1) / kChunk;
        KIVI_REQUIRE(chunks < (1LL << 31), KIVI_EINVAL, "kivi_cache_snapshot: grid too large");
    }
    KIVI_REQUIRE((uint64_t)row_bytes <= (uint64_t)buf_row_stride, KIVI_EINVAL,
                 "kivi_cache_snapshot: buf_row_stride=%zu is below the %lld bytes the slabs of a row take", buf_row_stride, (long long)row_bytes);
    if (chunks == 0) return 0;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (direction == 0) KIVI_LAUNCH(snapshot_rows_kernel<false>, grid, dim3(kThreads), (hipStream_t)stream, a);
    else KIVI_LAUNCH(snapshot_rows_kernel<true>, grid, dim3(kThreads), (hipStream_t)stream, a);
    return kivi_launch_status("kivi_cache_snapshot");
}
