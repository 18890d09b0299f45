// Admission of new requests into rows of a living cache (continuous batching): for i < n_rows the byte ranges a
// list of admit slabs names (include/kivi_hip.h, kivi_admit_slab) are copied from row i of a SOURCE cache to row rows[i] of a
// DESTINATION cache.  The two caches are different allocations with their own strides (capacities differ) and their own offsets
// (the fp16 V window sits elsewhere in each), so every slab carries base, row stride and level strides per side; the level counts
// and the run length are shared.
//
// One launch.  A workgroup owns (source row, chunk of one slab): kThreads * kInFlight units (16 bytes, or 4 for slabs one of whose
// sides is only word aligned, such as the range words).  A thread takes units chunk + j * kThreads + tid, j < kInFlight: it works
// out its kInFlight source / destination pairs, issues all of its loads, and only then stores.  Consecutive lanes touch consecutive
// units inside a run on both sides.  No LDS, no scratch; the destination rows of a launch are distinct (the caller's contract), so
// every byte is written at most once.  A row index outside [0, B) is read as "leave this source row unused": nothing outside the
// destination's B rows is ever written.
#include "kivi_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;
constexpr int kChunk = kThreads * kInFlight;   // units per workgroup

struct ASlab {
    char* dbase;
    const char* sbase;
    int64_t drs, d0, d1, d2;             // destination: row stride, level strides (bytes)
    int64_t srs, s0, s1, s2;             // source
    uint32_t n1, n2, upr;                // level counts 1 and 2, units per run
    uint32_t units;                      // units per row (n0 * n1 * n2 * upr)
    uint32_t chunk0;                     // first chunk (blockIdx.x) of this slab
    uint32_t unit;                       // 16 or 4 bytes
};

struct AArgs {
    ASlab s[KIVI_REORDER_MAX_SLABS];
    const void* rows;
    int ns, rows64, B;
};

// FULL: every unit of the workgroup's chunk exists (all but the last chunk of a slab): no lane is masked, loads and stores are
// straight-line code
template <typename T, bool FULL>
__device__ __forceinline__ void admit_units(const ASlab& S, char* drow, const char* srow, uint32_t u0) {
    char* d[kInFlight];
    const char* c[kInFlight];
    bool live[kInFlight];
    const bool flat = S.n1 == 1 && S.n2 == 1;          // one (count, stride) level: the fp16 residual, the window segments
#pragma unroll
    for (int j = 0; j < kInFlight; ++j) {
        const uint32_t u = u0 + (uint32_t)j * kThreads;
        live[j] = FULL || u < S.units;
        uint32_t piece = live[j] ? u / S.upr : 0;
        const uint32_t w = live[j] ? u - piece * S.upr : 0;
        const int64_t in_run = (int64_t)w * (int64_t)sizeof(T);
        if (flat) {
            c[j] = srow + (int64_t)piece * S.s0 + in_run;
            d[j] = drow + (int64_t)piece * S.d0 + in_run;
        } else {
            const uint32_t i2 = piece % S.n2;
            piece /= S.n2;
            const int64_t i0 = piece / S.n1, i1 = piece % S.n1;
            c[j] = srow + i0 * S.s0 + i1 * S.s1 + (int64_t)i2 * S.s2 + in_run;
            d[j] = drow + i0 * S.d0 + i1 * S.d1 + (int64_t)i2 * S.d2 + in_run;
        }
    }
    T v[kInFlight];
#pragma unroll
    for (int j = 0; j < kInFlight; ++j)
        if (live[j]) v[j] = *reinterpret_cast<const T*>(c[j]);
#pragma unroll
    for (int j = 0; j < kInFlight; ++j)
        if (live[j]) *reinterpret_cast<T*>(d[j]) = v[j];
}

__global__ __launch_bounds__(kThreads) void admit_rows_kernel(const AArgs a) {
    const int64_t i = blockIdx.y;
    const int64_t r = a.rows64 ? reinterpret_cast<const int64_t*>(a.rows)[i] : (int64_t)reinterpret_cast<const int*>(a.rows)[i];
    if (r < 0 || r >= a.B) return;                     // (uniform over the workgroup) outside the destination: nothing is written
    // the slab of this chunk: the last one whose first chunk is <= blockIdx.x (constant indices: the descriptors stay in kernarg)
    ASlab S = a.s[0];
#pragma unroll
    for (int k = 1; k < KIVI_REORDER_MAX_SLABS; ++k)
        if (k < a.ns && blockIdx.x >= a.s[k].chunk0) S = a.s[k];
    char* drow = S.dbase + r * S.drs;
    const char* srow = S.sbase + i * S.srs;
    const uint32_t u0 = (blockIdx.x - S.chunk0) * (uint32_t)kChunk + threadIdx.x;
    const bool full = (blockIdx.x - S.chunk0 + 1) * (uint32_t)kChunk <= S.units;      // (host: units < 2^31, no overflow)
    if (S.unit == 16) {
        if (full) admit_units<u32x4, true>(S, drow, srow, u0);
        else admit_units<u32x4, false>(S, drow, srow, u0);
    } else {
        admit_units<uint32_t, false>(S, drow, srow, u0);
    }
}

}  // namespace

extern "C" int kivi_cache_admit(const kivi_admit_slab* slabs, int n_slabs, int n_rows, const void* rows, int rows_bytes, int B,
                                kivi_stream_t stream) {
    KIVI_REQUIRE(B >= 1 && B < 65536, KIVI_EINVAL, "kivi_cache_admit: B=%d (1 .. 65535 destination rows)", B);
    KIVI_REQUIRE(n_rows >= 1 && n_rows <= B, KIVI_EINVAL, "kivi_cache_admit: n_rows=%d (1 .. B = %d rows to admit)", n_rows, B);
    KIVI_REQUIRE(rows_bytes == 4 || rows_bytes == 8, KIVI_EINVAL, "kivi_cache_admit: rows_bytes=%d (int32 or int64 row indices)", rows_bytes);
    KIVI_REQUIRE(rows && (uintptr_t)rows % rows_bytes == 0, KIVI_EINVAL, "kivi_cache_admit: null / misaligned rows");
    KIVI_REQUIRE(n_slabs >= 0 && n_slabs <= KIVI_REORDER_MAX_SLABS && (n_slabs == 0 || slabs), KIVI_EINVAL,
                 "kivi_cache_admit: n_slabs=%d (at most %d)", n_slabs, KIVI_REORDER_MAX_SLABS);
    AArgs a = {};
    a.rows = rows;
    a.rows64 = rows_bytes == 8;
    a.B = B;
    int64_t chunks = 0;
    for (int i = 0; i < n_slabs; ++i) {
        const kivi_admit_slab& s = slabs[i];
        KIVI_REQUIRE(s.n[0] >= 0 && s.n[1] >= 0 && s.n[2] >= 0 && s.run >= 0, KIVI_EINVAL, "kivi_cache_admit: slab %d: negative count", i);
        if (s.n[0] == 0 || s.n[1] == 0 || s.n[2] == 0 || s.run == 0) continue;       // nothing to move
        const uint64_t bits = (uint64_t)(uintptr_t)s.dst_base | (uint64_t)s.dst_row_stride | (uint64_t)s.dst_stride[0] |
                              (uint64_t)s.dst_stride[1] | (uint64_t)s.dst_stride[2] | (uint64_t)(uintptr_t)s.src_base |
                              (uint64_t)s.src_row_stride | (uint64_t)s.src_stride[0] | (uint64_t)s.src_stride[1] |
                              (uint64_t)s.src_stride[2] | (uint64_t)s.run;
        KIVI_REQUIRE(s.dst_base && s.src_base && bits % 4 == 0, KIVI_EINVAL,
                     "kivi_cache_admit: slab %d: null base, or base / strides / run of a side not multiples of 4 bytes", i);
        const uint32_t unit = bits % 16 == 0 ? 16 : 4;
        const int64_t upr = s.run / unit;
        int64_t units = 1;
        bool fits = true;
        for (int64_t f : {s.n[0], s.n[1], s.n[2], upr}) {
            fits = fits && f < (1LL << 31) && units * f < (1LL << 31);
            units = fits ? units * f : 1;
        }
        KIVI_REQUIRE(fits, KIVI_EINVAL, "kivi_cache_admit: slab %d: 2^31 units per row or more", i);
        ASlab& d = a.s[a.ns++];
        d.dbase = (char*)s.dst_base;
        d.sbase = (const char*)s.src_base;
        d.drs = s.dst_row_stride;
        d.d0 = s.dst_stride[0];
        d.d1 = s.dst_stride[1];
        d.d2 = s.dst_stride[2];
        d.srs = s.src_row_stride;
        d.s0 = s.src_stride[0];
        d.s1 = s.src_stride[1];
        d.s2 = s.src_stride[2];
        d.n1 = (uint32_t)s.n[1];
        d.n2 = (uint32_t)s.n[2];
        d.upr = (uint32_t)upr;
        d.units = (uint32_t)units;
        d.chunk0 = (uint32_t)chunks;
        d.unit = unit;
        chunks += (units + kChunk - 1) / kChunk;
        KIVI_REQUIRE(chunks < (1LL << 31), KIVI_EINVAL, "kivi_cache_admit: grid too large");
    }
    if (chunks == 0) return 0;
    KIVI_LAUNCH(admit_rows_kernel, dim3((unsigned)chunks, (unsigned)n_rows), dim3(kThreads), (hipStream_t)stream, a);
    return kivi_launch_status("kivi_cache_admit");
}
