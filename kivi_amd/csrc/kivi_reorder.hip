// In-place reorder of cache rows inside groups (beam search): row[b] <- row[idx[b]] for the byte ranges a list of slab descriptors
// names (include/kivi_hip.h, kivi_cache_reorder).  The caller describes WHAT moves -- for beam search only what was written after
// the fork point, so the traffic of a step scales with the generated tokens, not with the context.
//
// One launch over the slab walk of kivi_slab.h (units, chunks, the host preparation, the offsets of a unit).  This kernel's own is
// the exchange through LDS.  A workgroup owns (row group, chunk of one slab): the chunk is UC units at the same offsets in every
// row of the group.  It reads idx of its group (an index outside the group is read as the identity: such a row is left as it is,
// nothing outside the group is ever touched), marks the rows that some other row sources, loads those rows' chunk into LDS, waits
// at a barrier and writes the rows whose idx differs from their own index.  Every byte is read at most once and written at most
// once; identity rows that nobody sources are neither read nor written.  Chunks of different workgroups are disjoint, so the
// reorder is in place without scratch memory or a second pass.
#include "kivi_common.h"
#include "kivi_slab.h"

namespace {

constexpr int kThreads = 256;
constexpr int kLdsBytes = 65536;         // LDS per workgroup: group * UC 16-byte slots + 8 bytes of bookkeeping per row

struct RArgs {
    KiviSlabs<1> slabs;
    const void* idx;
    int idx64, group, uc;
};

__global__ __launch_bounds__(kThreads) void reorder_rows_kernel(const RArgs a) {
    extern __shared__ u32x4 lds[];
    const int G = a.group, uc = a.uc, tid = threadIdx.x;
    int* src = reinterpret_cast<int*>(lds + G * uc);
    int* need = src + G;
    const int64_t g0 = (int64_t)blockIdx.y * G;
    KiviSlab<1> S;
    KIVI_SLAB_OF_CHUNK(S, a.slabs, blockIdx.x);

    for (int b = tid; b < G; b += kThreads) {
        const int64_t v = a.idx64 ? reinterpret_cast<const int64_t*>(a.idx)[g0 + b] : (int64_t)reinterpret_cast<const int*>(a.idx)[g0 + b];
        src[b] = (v >= g0 && v < g0 + G) ? (int)(v - g0) : b;      // out of the group: leave the row alone
        need[b] = 0;
    }
    __syncthreads();
    for (int b = tid; b < G; b += kThreads)
        if (src[b] != b) need[src[b]] = 1;
    __syncthreads();

    // this thread's unit of the chunk (the same offset in every row) and its first row; rows step by kThreads / uc
    const int k = tid & (uc - 1), rstep = kThreads / uc;
    const uint32_t u = (blockIdx.x - S.chunk0) * (uint32_t)uc + (uint32_t)k;
    const bool live = u < S.units;
    const KiviSlabSide& e = S.side[0];
    int64_t off = 0;
    if (live) kivi_slab_offsets(S, u, S.unit, &off);
    char* base = e.base + g0 * e.rs + off;
    if (S.unit == 16) {
        for (int r = tid / uc; r < G; r += rstep)
            if (live && need[r]) lds[r * uc + k] = *reinterpret_cast<const u32x4*>(base + r * e.rs);
        __syncthreads();
        for (int b = tid / uc; b < G; b += rstep)
            if (live && src[b] != b) *reinterpret_cast<u32x4*>(base + b * e.rs) = lds[src[b] * uc + k];
    } else {
        uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
        for (int r = tid / uc; r < G; r += rstep)
            if (live && need[r]) l32[r * uc + k] = *reinterpret_cast<const uint32_t*>(base + r * e.rs);
        __syncthreads();
        for (int b = tid / uc; b < G; b += rstep)
            if (live && src[b] != b) *reinterpret_cast<uint32_t*>(base + b * e.rs) = l32[src[b] * uc + k];
    }
}

}  // namespace

extern "C" int kivi_cache_reorder(const kivi_reorder_slab* slabs, int n_slabs, int B, int group, const void* idx, int idx_bytes,
                                  kivi_stream_t stream) {
    KIVI_REQUIRE(B > 0 && group > 0 && group <= KIVI_REORDER_MAX_GROUP && B % group == 0 && B / group < 65536, KIVI_EINVAL,
                 "kivi_cache_reorder: bad group (B=%d group=%d; 1 <= group <= %d, B a multiple of group)", B, group,
                 KIVI_REORDER_MAX_GROUP);
    KIVI_REQUIRE(idx_bytes == 4 || idx_bytes == 8, KIVI_EINVAL, "kivi_cache_reorder: idx_bytes=%d (int32 or int64 indices)", idx_bytes);
    KIVI_REQUIRE(idx && (uintptr_t)idx % idx_bytes == 0, KIVI_EINVAL, "kivi_cache_reorder: null / misaligned idx");
    KIVI_REQUIRE(n_slabs >= 0 && n_slabs <= KIVI_REORDER_MAX_SLABS && (n_slabs == 0 || slabs), KIVI_EINVAL,
                 "kivi_cache_reorder: n_slabs=%d (at most %d)", n_slabs, KIVI_REORDER_MAX_SLABS);
    int uc = kThreads;                                    // units per chunk: a power of two, group * uc LDS slots
    while ((int64_t)group * (uc * 16 + 8) > kLdsBytes) uc >>= 1;
    RArgs a = {};
    a.idx = idx;
    a.idx64 = idx_bytes == 8;
    a.group = group;
    a.uc = uc;
    int64_t chunks = 0;
    if (const int rc = kivi_prepare_slabs("kivi_cache_reorder", KIVI_EINVAL, slabs, n_slabs, uc, &a.slabs, &chunks)) return rc;
    if (chunks == 0) return 0;
    const size_t lds = (size_t)group * uc * 16 + (size_t)group * 8;
    KIVI_LAUNCH_LDS(reorder_rows_kernel, dim3((unsigned)chunks, (unsigned)(B / group)), dim3(kThreads), lds, (hipStream_t)stream, a);
    return kivi_launch_status("kivi_cache_reorder");
}
