// The two-sided row copy over the slab walk of kivi_slab.h, and its two entry points (include/kivi_hip.h):
//   kivi_cache_admit     row i of a SOURCE cache -> row rows[i] of a DESTINATION cache (continuous batching).
//                        Its own is the row map: a row index outside [0, B) is read as "leave this source row unused", so nothing
//                        outside the destination's B rows is ever written; the destination rows of a launch are distinct (the
//                        caller's contract), so every byte is written at most once.
//   kivi_cache_snapshot  the slabs of every row gathered into buf + b * buf_row_stride (direction 0) or scattered back (1)
//                        (checkpoint / rollback).  Its own is the buffer-row format: slab after slab, each on
//                        a 16-byte boundary of the row, which is a slab side like any other (kivi_prepare_slabs, `dense`); the row
//                        map is the identity and the direction says which side is read.
//
// One launch.  A workgroup owns (row, chunk of one slab): kSlabChunk units (16 bytes, or 4 for slabs one of whose sides is only word
// aligned, such as the range words) of one row.  A thread takes units chunk + j * kSlabThreads + tid, j < kSlabInFlight: it works
// out its source / destination pairs, issues all of its loads, and only then stores -- kSlabInFlight independent 16-byte loads per
// thread are in flight before the first store waits for one (the reorder kernel has one).  Consecutive lanes touch consecutive
// units inside a run on both sides.  No LDS, no scratch; every byte is read once and written once.
#include <utility>

#include "kivi_common.h"
#include "kivi_slab.h"

namespace {

struct CArgs {
    KiviSlabs<2> slabs;                  // side 0 is read, side 1 is written
    const void* rows;                    // row i of side 0 -> row rows[i] of side 1; null: row i
    int rows64, B;
};

// FULL: every unit of the workgroup's chunk exists (all but the last chunk of a slab) -- no lane is masked, so the loads and the
// stores are straight-line code and no store waits for the one before it
template <typename T, bool FULL>
__device__ __forceinline__ void copy_units(const KiviSlab<2>& S, const char* srow, char* drow, uint32_t u0) {
    const char* c[kSlabInFlight];
    char* d[kSlabInFlight];
    bool live[kSlabInFlight];
#pragma unroll
    for (int j = 0; j < kSlabInFlight; ++j) {
        const uint32_t u = u0 + (uint32_t)j * kSlabThreads;
        live[j] = FULL || u < S.units;
        int64_t off[2];
        kivi_slab_offsets(S, live[j] ? u : 0, sizeof(T), off);
        c[j] = srow + off[0];
        d[j] = drow + off[1];
    }
    T v[kSlabInFlight];
#pragma unroll
    for (int j = 0; j < kSlabInFlight; ++j)
        if (live[j]) v[j] = *reinterpret_cast<const T*>(c[j]);
#pragma unroll
    for (int j = 0; j < kSlabInFlight; ++j)
        if (live[j]) *reinterpret_cast<T*>(d[j]) = v[j];
}

__global__ __launch_bounds__(kSlabThreads) void copy_rows_kernel(const CArgs a) {
    const int64_t i = blockIdx.y;
    int64_t r = i;
    if (a.rows) {
        r = a.rows64 ? reinterpret_cast<const int64_t*>(a.rows)[i] : (int64_t)reinterpret_cast<const int*>(a.rows)[i];
        if (r < 0 || r >= a.B) return;                 // (uniform over the workgroup) outside the destination: nothing is written
    }
    KiviSlab<2> S;
    KIVI_SLAB_OF_CHUNK(S, a.slabs, blockIdx.x);
    const char* srow = S.side[0].base + i * S.side[0].rs;
    char* drow = S.side[1].base + r * S.side[1].rs;
    const uint32_t u0 = (blockIdx.x - S.chunk0) * (uint32_t)kSlabChunk + threadIdx.x;
    const bool full = (blockIdx.x - S.chunk0 + 1) * (uint32_t)kSlabChunk <= S.units;  // (host: units < 2^31, no overflow)
    if (S.unit == 16) {
        if (full) copy_units<u32x4, true>(S, srow, drow, u0);
        else copy_units<u32x4, false>(S, srow, drow, u0);
    } else {
        copy_units<uint32_t, false>(S, srow, drow, u0);
    }
}

int launch(const char* name, const CArgs& a, int64_t chunks, int n_rows, kivi_stream_t stream) {
    if (chunks == 0) return 0;
    KIVI_LAUNCH(copy_rows_kernel, dim3((unsigned)chunks, (unsigned)n_rows), dim3(kSlabThreads), (hipStream_t)stream, a);
    return kivi_launch_status(name);
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
    CArgs a = {};
    a.rows = rows;
    a.rows64 = rows_bytes == 8;
    a.B = B;
    int64_t chunks = 0;
    if (const int rc = kivi_prepare_slabs("kivi_cache_admit", KIVI_EINVAL, slabs, n_slabs, kSlabChunk, &a.slabs, &chunks)) return rc;
    return launch("kivi_cache_admit", a, chunks, n_rows, stream);
}

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
    CArgs a = {};
    const KiviSlabSide dense = {(char*)buf, (int64_t)buf_row_stride, 0, 0, 0};
    int64_t chunks = 0, row_bytes = 0;
    if (const int rc = kivi_prepare_slabs("kivi_cache_snapshot", KIVI_EALIGN, slabs, n_slabs, kSlabChunk, &a.slabs, &chunks, &dense, &row_bytes))
        return rc;
    KIVI_REQUIRE((uint64_t)row_bytes <= (uint64_t)buf_row_stride, KIVI_EINVAL,
                 "kivi_cache_snapshot: buf_row_stride=%zu is below the %lld bytes the slabs of a row take", buf_row_stride, (long long)row_bytes);
    if (direction == 1)                                // the cache came out as side 0, the buffer as side 1: scatter reads the buffer
        for (int i = 0; i < a.slabs.ns; ++i) std::swap(a.slabs.s[i].side[0], a.slabs.s[i].side[1]);
    return launch("kivi_cache_snapshot", a, chunks, B, stream);
}
