// The slab walk of the cache row movers ("The slab walk"): kivi_cache_reorder, kivi_cache_snapshot and
// kivi_cache_admit all move, for some rows, the byte ranges a list of slabs names (include/kivi_hip.h).  A slab is up to three
// (count, stride) levels of runs of `run` bytes; it is walked in UNITS of 16 bytes (4 where something of it is only word aligned),
// unit u = ((i0 * n1 + i1) * n2 + i2) * upr + w, and the grid's x dimension is cut into CHUNKS of units, slab after slab.
// Here, once: the device descriptor, the host preparation of a caller's list, the slab of a chunk and the byte offsets of a unit.
// Nothing in this file needs HIP: a plain C++ program can include it and run all of it (tests/test_slab_walk_cpu.py).
#pragma once
#include <stdint.h>

#include <initializer_list>

#include "../../include/kivi_hip.h"

#ifdef __HIPCC__
#define KIVI_SLAB_HD __host__ __device__ __forceinline__
#else
#define KIVI_SLAB_HD inline
#endif

void kivi_set_error(const char* fmt, ...);

// the two-sided copy kernel's geometry: a thread has kSlabInFlight units in flight, a workgroup takes kSlabChunk units of one row
constexpr int kSlabThreads = 256;
constexpr int kSlabInFlight = 4;
constexpr int kSlabChunk = kSlabThreads * kSlabInFlight;

struct KiviSlabSide {
    char* base;
    int64_t rs, s0, s1, s2;              // row stride, level strides (bytes)
};

template <int SIDES>
struct KiviSlab {
    KiviSlabSide side[SIDES];
    uint32_t n1, n2, upr;                // level counts 1 and 2, units per run
    uint32_t units;                      // units per row (n0 * n1 * n2 * upr)
    uint32_t chunk0;                     // first chunk (blockIdx.x) of this slab
    uint32_t unit;                       // 16 or 4 bytes
};

template <int SIDES>
struct KiviSlabs {
    KiviSlab<SIDES> s[KIVI_REORDER_MAX_SLABS];
    int ns;
};

inline void kivi_slab_sides(const kivi_reorder_slab& s, KiviSlabSide* side) {
    side[0] = {(char*)s.base, s.row_stride, s.stride[0], s.stride[1], s.stride[2]};
}
inline void kivi_slab_sides(const kivi_admit_slab& s, KiviSlabSide* side) {      // side 0 is read, side 1 is written
    side[0] = {(char*)s.src_base, s.src_row_stride, s.src_stride[0], s.src_stride[1], s.src_stride[2]};
    side[1] = {(char*)s.dst_base, s.dst_row_stride, s.dst_stride[0], s.dst_stride[1], s.dst_stride[2]};
}

// The caller's slabs -> device descriptors (empty slabs dropped) and the grid's chunk count, `uc` units per chunk.  `name`: the entry
// point, for the messages; `ealign`: what it returns for misalignment.  `dense` (snapshot): the LAST side is not the caller's but a
// flat buffer, rows at dense->base + b * dense->rs, in which the slabs of a row follow one another, each on a 16-byte boundary;
// *row_bytes is what they take.
template <int SIDES, typename In>
int kivi_prepare_slabs(const char* name, int ealign, const In* in, int n, int uc, KiviSlabs<SIDES>* out, int64_t* chunks,
                       const KiviSlabSide* dense = nullptr, int64_t* row_bytes = nullptr) {
    const int given = dense ? SIDES - 1 : SIDES;
    int64_t nchunks = 0, boff = 0;
    out->ns = 0;
    for (int i = 0; i < n; ++i) {
        const In& s = in[i];
        if (s.n[0] < 0 || s.n[1] < 0 || s.n[2] < 0 || s.run < 0) {
            kivi_set_error("%s: slab %d: negative count", name, i);
            return KIVI_EINVAL;
        }
        if (s.n[0] == 0 || s.n[1] == 0 || s.n[2] == 0 || s.run == 0) continue;       // nothing to move, no room in a buffer row
        KiviSlab<SIDES>& d = out->s[out->ns];
        kivi_slab_sides(s, d.side);
        uint64_t bits = (uint64_t)s.run | (dense ? (uint64_t)(uintptr_t)dense->base | (uint64_t)dense->rs : 0);
        bool null = false;
        for (int k = 0; k < given; ++k) {
            const KiviSlabSide& e = d.side[k];
            null = null || !e.base;
            bits |= (uint64_t)(uintptr_t)e.base | (uint64_t)e.rs | (uint64_t)e.s0 | (uint64_t)e.s1 | (uint64_t)e.s2;
        }
        if (null) {
            kivi_set_error("%s: slab %d: null base", name, i);
            return KIVI_EINVAL;
        }
        if (bits % 4) {
            kivi_set_error("%s: slab %d: base / strides / run of a side not multiples of 4 bytes", name, i);
            return ealign;
        }
        d.unit = bits % 16 == 0 ? 16 : 4;
        const int64_t upr = s.run / d.unit;
        int64_t units = 1;
        bool fits = true;
        for (int64_t f : {s.n[0], s.n[1], s.n[2], upr}) {
            fits = fits && f < (1LL << 31) && units * f < (1LL << 31);
            units = fits ? units * f : 1;
        }
        if (!fits) {
            kivi_set_error("%s: slab %d: 2^31 units per row or more", name, i);
            return KIVI_EINVAL;
        }
        if (dense) d.side[given] = {dense->base + boff, dense->rs, s.n[1] * s.n[2] * s.run, s.n[2] * s.run, s.run};
        d.n1 = (uint32_t)s.n[1];
        d.n2 = (uint32_t)s.n[2];
        d.upr = (uint32_t)upr;
        d.units = (uint32_t)units;
        d.chunk0 = (uint32_t)nchunks;
        ++out->ns;
        boff += (units * d.unit + 15) / 16 * 16;
        nchunks += (units + uc - 1) / uc;
        if (nchunks >= (1LL << 31)) {
            kivi_set_error("%s: grid too large", name);
            return KIVI_EINVAL;
        }
    }
    *chunks = nchunks;
    if (row_bytes) *row_bytes = boff;
    return 0;
}

// S = the slab of a chunk: the last one whose first chunk is <= chunk (constant indices: in a kernel the descriptors stay in
// kernarg).  A macro, not a function: written into the kernel's body the chain compiles to one scalar compare and branch per slab
// and loads only the descriptors it takes; through a function (by value or by reference) the compiler selects among speculated
// loads of all of them, which costs 30 SGPRs and about 2 us of a 15 us launch.
#define KIVI_SLAB_OF_CHUNK(S, a, chunk)                                          \
    do {                                                                         \
        S = (a).s[0];                                                            \
        _Pragma("unroll") for (int i_ = 1; i_ < KIVI_REORDER_MAX_SLABS; ++i_) {  \
            if (i_ < (a).ns && (chunk) >= (a).s[i_].chunk0) {                    \
                S = (a).s[i_];                                                   \
            }                                                                    \
        }                                                                        \
    } while (0)

// byte offsets of unit u (< S.units) of slab S inside a row, one per side (the index arithmetic is done once for all sides); `unit`
// is S.unit (a constant where the caller has one)
template <int SIDES>
KIVI_SLAB_HD void kivi_slab_offsets(const KiviSlab<SIDES>& S, uint32_t u, uint32_t unit, int64_t* off) {
    uint32_t piece = u / S.upr;
    const int64_t in_run = (int64_t)(u - piece * S.upr) * unit;
    if (S.n1 == 1 && S.n2 == 1) {                        // one (count, stride) level: the fp16 residual, the window
        for (int k = 0; k < SIDES; ++k) off[k] = (int64_t)piece * S.side[k].s0 + in_run;
        return;
    }
    const uint32_t i2 = piece % S.n2;
    piece /= S.n2;
    const int64_t i0 = piece / S.n1, i1 = piece % S.n1;
    for (int k = 0; k < SIDES; ++k) off[k] = i0 * S.side[k].s0 + i1 * S.side[k].s1 + (int64_t)i2 * S.side[k].s2 + in_run;
}
