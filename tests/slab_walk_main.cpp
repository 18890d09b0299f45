// Host play of the two-sided row copy (kivi_amd/csrc/kivi_rowcopy.hip) over kivi_amd/csrc/kivi_slab.h, built as plain C++ with
// -fsanitize=address,undefined by tests/test_slab_walk_cpu.py.  A list of slabs over host buffers is prepared by kivi_prepare_slabs
// and the kernel's grid is walked here: every chunk, row, thread and j < kSlabInFlight moves one unit with memcpy at the offsets of
// kivi_slab_offsets.  The result is compared with a nested-loop copy of the same slabs; a shadow array counts the writes of every
// destination byte (exactly one inside the slabs, none outside).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../kivi_amd/csrc/kivi_slab.h"

static char g_error[512];
void kivi_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static int g_failed = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
            ++g_failed;                       \
        }                                     \
    } while (0)

namespace {

constexpr int kRows = 3;
constexpr int64_t kRegion = 32768;                      // every slab lives in a region of its own of a row, on both sides
constexpr int64_t kSlabsMax = 14;
constexpr int64_t kDstRow = kSlabsMax * kRegion + 4096, kSrcRow = kSlabsMax * kRegion + 1024;   // row strides differ per side

struct Spec {                                            // one slab: offsets inside its region, level strides per side
    int64_t doff, d[3], soff, s[3], n[3], run;
    uint32_t unit, chunks;                               // what kivi_prepare_slabs has to make of it (0 chunks: dropped)
};

// 16-byte and 4-byte units of: a flat slab, a 3-level slab with other strides on each side, exactly one full chunk, a full chunk plus
// one unit (over five runs), a single unit; an empty slab between two live ones, twice
const Spec kSpecs[] = {
    {0, {64, 0, 0}, 16, {80, 0, 0}, {5, 1, 1}, 48, 16, 1},
    {32, {4096, 1024, 64}, 0, {2048, 512, 128}, {2, 3, 2}, 32, 16, 1},
    {0, {0, 0, 0}, 0, {0, 0, 0}, {1, 1, 1}, kSlabChunk * 16, 16, 1},
    {0, {64, 0, 0}, 0, {64, 0, 0}, {4, 0, 1}, 16, 16, 0},
    {16, {3296, 0, 0}, 48, {3312, 0, 0}, {5, 1, 1}, (kSlabChunk + 1) / 5 * 16, 16, 2},
    {4080, {0, 0, 0}, 8176, {0, 0, 0}, {1, 1, 1}, 16, 16, 1},
    {4, {16, 0, 0}, 8, {20, 0, 0}, {5, 1, 1}, 12, 4, 1},
    {8, {4096, 1024, 64}, 4, {2048, 512, 128}, {2, 3, 2}, 8, 4, 1},
    {4, {0, 0, 0}, 12, {0, 0, 0}, {1, 1, 1}, kSlabChunk * 4, 4, 1},
    {0, {0, 0, 0}, 0, {0, 0, 0}, {1, 1, 1}, 0, 4, 0},
    {8, {824, 0, 0}, 4, {828, 0, 0}, {5, 1, 1}, (kSlabChunk + 1) / 5 * 4, 4, 2},
    {4092, {0, 0, 0}, 8188, {0, 0, 0}, {1, 1, 1}, 4, 4, 1},
    {0, {1024, 0, 16}, 0, {512, 0, 16}, {3, 1, 4}, 16, 16, 1},          // n1 = 1 but n2 > 1: not the flat short cut
};
constexpr int kNSpecs = sizeof kSpecs / sizeof kSpecs[0];
static_assert(kNSpecs <= kSlabsMax && (kSlabChunk + 1) % 5 == 0, "the specs");

struct Arena {
    char* p;
    int64_t bytes;
    Arena(int64_t n, unsigned seed) : p((char*)aligned_alloc(64, (n + 63) / 64 * 64)), bytes(n) {
        for (int64_t i = 0; i < n; ++i) p[i] = (char)((seed = seed * 1664525u + 1013904223u) >> 24);
    }
    ~Arena() { free(p); }
};

// walk the grid of copy_rows_kernel on the host: side 0 is read, side 1 is written, row i -> row rows[i]
void play(const KiviSlabs<2>& a, int64_t chunks, const int* rows, const Arena& dst, std::vector<uint8_t>& shadow) {
    for (uint32_t chunk = 0; chunk < (uint32_t)chunks; ++chunk)
        for (int i = 0; i < kRows; ++i) {
            KiviSlab<2> S;
            KIVI_SLAB_OF_CHUNK(S, a, chunk);
            const char* srow = S.side[0].base + i * S.side[0].rs;
            char* drow = S.side[1].base + rows[i] * S.side[1].rs;
            for (uint32_t tid = 0; tid < (uint32_t)kSlabThreads; ++tid)
                for (int j = 0; j < kSlabInFlight; ++j) {
                    const uint32_t u = (chunk - S.chunk0) * (uint32_t)kSlabChunk + tid + (uint32_t)j * kSlabThreads;
                    if (u >= S.units) continue;
                    int64_t off[2];
                    kivi_slab_offsets(S, u, S.unit, off);
                    char* d = drow + off[1];
                    memcpy(d, srow + off[0], S.unit);
                    for (uint32_t b = 0; b < S.unit; ++b) ++shadow[d - dst.p + b];
                }
        }
}

void compare(const char* what, const Arena& got, const Arena& want, const std::vector<uint8_t>& shadow, const std::vector<uint8_t>& once) {
    int64_t bad = 0, counts = 0;
    for (int64_t i = 0; i < got.bytes; ++i) {
        bad += got.p[i] != want.p[i];
        counts += shadow[i] != once[i];
    }
    CHECK(bad == 0, "%s: %lld bytes differ from the nested-loop copy", what, (long long)bad);
    CHECK(counts == 0, "%s: %lld bytes not written exactly once inside the slabs / never outside", what, (long long)counts);
}

// kivi_cache_admit's walk: both sides from the caller, rows permuted
void admit_case() {
    Arena src(kRows * kSrcRow, 1), dst(kRows * kDstRow, 2), want(kRows * kDstRow, 2);
    std::vector<uint8_t> shadow(dst.bytes, 0), once(dst.bytes, 0);
    const int rows[kRows] = {2, 0, 1};
    kivi_admit_slab in[kNSpecs];
    for (int k = 0; k < kNSpecs; ++k) {
        const Spec& c = kSpecs[k];
        in[k] = {dst.p + k * kRegion + c.doff, kDstRow, {c.d[0], c.d[1], c.d[2]}, src.p + k * kRegion + c.soff, kSrcRow,
                 {c.s[0], c.s[1], c.s[2]}, {c.n[0], c.n[1], c.n[2]}, c.run};
        for (int i = 0; i < kRows; ++i)
            for (int64_t i0 = 0; i0 < c.n[0]; ++i0)
                for (int64_t i1 = 0; i1 < c.n[1]; ++i1)
                    for (int64_t i2 = 0; i2 < c.n[2]; ++i2) {
                        const int64_t d = rows[i] * kDstRow + k * kRegion + c.doff + i0 * c.d[0] + i1 * c.d[1] + i2 * c.d[2];
                        memcpy(want.p + d, src.p + i * kSrcRow + k * kRegion + c.soff + i0 * c.s[0] + i1 * c.s[1] + i2 * c.s[2], c.run);
                        for (int64_t b = 0; b < c.run; ++b) ++once[d + b];
                    }
    }
    KiviSlabs<2> a = {};
    int64_t chunks = -1;
    CHECK(kivi_prepare_slabs("admit", KIVI_EINVAL, in, kNSpecs, kSlabChunk, &a, &chunks) == 0, "prepare: %s", g_error);
    int live = 0;
    int64_t expect_chunks = 0;
    for (const Spec& c : kSpecs) {
        if (c.chunks) {
            CHECK(a.s[live].unit == c.unit && a.s[live].chunk0 == expect_chunks, "slab %d: unit %u chunk0 %u", live, a.s[live].unit, a.s[live].chunk0);
            ++live;
        }
        expect_chunks += c.chunks;
    }
    CHECK(a.ns == live && chunks == expect_chunks, "ns=%d chunks=%lld", a.ns, (long long)chunks);
    play(a, chunks, rows, dst, shadow);
    compare("admit", dst, want, shadow, once);
}

// kivi_cache_snapshot's walk: the cache side from the caller (the specs' source side), the other a dense buffer row
void snapshot_case(int direction) {
    const char* what = direction ? "scatter" : "gather";
    int64_t row_bytes = 0;
    for (const Spec& c : kSpecs) row_bytes += (c.n[0] * c.n[1] * c.n[2] * c.run + 15) / 16 * 16;
    const int64_t brs = row_bytes + 64;
    // gather: cache (read) -> buffer (written); scatter: buffer (read) -> cache (written)
    Arena cache(kRows * kSrcRow, 3), buf(kRows * brs, 4), want(direction ? kRows * kSrcRow : kRows * brs, direction ? 3 : 4);
    const Arena& dst = direction ? cache : buf;
    std::vector<uint8_t> shadow(dst.bytes, 0), once(dst.bytes, 0);
    const int rows[kRows] = {0, 1, 2};
    kivi_reorder_slab in[kNSpecs];
    int64_t boff = 0;
    for (int k = 0; k < kNSpecs; ++k) {
        const Spec& c = kSpecs[k];
        in[k] = {cache.p + k * kRegion + c.soff, kSrcRow, {c.n[0], c.n[1], c.n[2]}, {c.s[0], c.s[1], c.s[2]}, c.run};
        for (int i = 0; i < kRows; ++i)
            for (int64_t i0 = 0; i0 < c.n[0]; ++i0)
                for (int64_t i1 = 0; i1 < c.n[1]; ++i1)
                    for (int64_t i2 = 0; i2 < c.n[2]; ++i2) {
                        const int64_t in_cache = i * kSrcRow + k * kRegion + c.soff + i0 * c.s[0] + i1 * c.s[1] + i2 * c.s[2];
                        const int64_t in_buf = i * brs + boff + ((i0 * c.n[1] + i1) * c.n[2] + i2) * c.run;
                        const int64_t d = direction ? in_cache : in_buf;
                        memcpy(want.p + d, direction ? buf.p + in_buf : cache.p + in_cache, c.run);
                        for (int64_t b = 0; b < c.run; ++b) ++once[d + b];
                    }
        boff += (c.n[0] * c.n[1] * c.n[2] * c.run + 15) / 16 * 16;
    }
    KiviSlabs<2> a = {};
    const KiviSlabSide dense = {buf.p, brs, 0, 0, 0};
    int64_t chunks = -1, got_row_bytes = -1;
    CHECK(kivi_prepare_slabs("snapshot", KIVI_EALIGN, in, kNSpecs, kSlabChunk, &a, &chunks, &dense, &got_row_bytes) == 0, "prepare: %s", g_error);
    CHECK(got_row_bytes == row_bytes, "%s: row bytes %lld, expected %lld", what, (long long)got_row_bytes, (long long)row_bytes);
    int live = 0;
    for (const Spec& c : kSpecs)
        if (c.chunks) {
            CHECK(a.s[live].unit == c.unit, "%s: slab %d: unit %u", what, live, a.s[live].unit);
            ++live;
        }
    CHECK(a.ns == live, "%s: ns=%d", what, a.ns);
    if (direction)
        for (int i = 0; i < a.ns; ++i) std::swap(a.s[i].side[0], a.s[i].side[1]);
    play(a, chunks, rows, dst, shadow);
    compare(what, dst, want, shadow, once);
}

// what kivi_prepare_slabs refuses, and with which code
void refusals() {
    alignas(64) static char mem[4096];
    KiviSlabs<1> a = {};
    int64_t chunks = 0;
    const kivi_reorder_slab ok = {mem, 1024, {2, 1, 1}, {512, 0, 0}, 64};
    kivi_reorder_slab s = ok;
    s.n[1] = -1;
    CHECK(kivi_prepare_slabs("name", -77, &s, 1, 256, &a, &chunks) == KIVI_EINVAL && strstr(g_error, "name: slab 0: negative"), "%s", g_error);
    s = ok;
    s.base = nullptr;
    CHECK(kivi_prepare_slabs("name", -77, &s, 1, 256, &a, &chunks) == KIVI_EINVAL && strstr(g_error, "null base"), "%s", g_error);
    s = ok;
    s.stride[0] = 514;
    CHECK(kivi_prepare_slabs("name", -77, &s, 1, 256, &a, &chunks) == -77 && strstr(g_error, "multiples of 4"), "%s", g_error);
    s = ok;
    s.n[0] = 1LL << 31;
    CHECK(kivi_prepare_slabs("name", -77, &s, 1, 256, &a, &chunks) == KIVI_EINVAL && strstr(g_error, "2^31"), "%s", g_error);
    s = ok;
    s.n[0] = 1 << 16, s.n[1] = 1 << 15, s.run = 16;
    CHECK(kivi_prepare_slabs("name", -77, &s, 1, 256, &a, &chunks) == KIVI_EINVAL && strstr(g_error, "2^31"), "%s", g_error);
    CHECK(kivi_prepare_slabs("name", -77, &ok, 1, 256, &a, &chunks) == 0 && a.ns == 1 && chunks == 1 && a.s[0].units == 8 && a.s[0].upr == 4, "ok slab");
}

}  // namespace

int main() {
    admit_case();
    snapshot_case(0);
    snapshot_case(1);
    refusals();
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("slab walk ok\n");
    return g_failed != 0;
}
