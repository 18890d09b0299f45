// Host play of the offset admission of a packed store (kivi_amd/csrc/kivi_admit_shift.hip) over kivi_amd/csrc/kivi_admit_shift.h,
// built as plain C++ with -fsanitize=address,undefined by tests/test_admit_offset_cpu.py.  A randomly filled source store of 3 rows and a
// canary-filled destination of 3 rows, with different super-block counts and strides (the source keeps the head index outside the
// super-block index, the destination inside it, with spare words between heads), are run through every thread of the kernel's
// grid: the row lookup, one 16-byte load (or zeros under the shift), one 16-byte store, the range word.  Compared with a naive
// per-block copy written from the layout's description (not from the header's address function); a counter per destination byte
// shows that no byte is written twice and that nothing outside blocks [0, n + shift) of the admitted rows is written at all.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../kivi_amd/csrc/kivi_admit_shift.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            printf("FAILED %s:%d: ", __FILE__, __LINE__);     \
            printf(__VA_ARGS__);                              \
            printf("\n");                                     \
            ++g_failed;                                       \
        }                                                     \
    } while (0)

namespace {

constexpr int kHeads = 2, kSrcRows = 3, kDstRows = 3;

struct Store {
    int bits, rows, n_sb;
    int64_t W, ss, sh, sb, bytes;                          // words per super-block; strides and size in bytes
    std::vector<unsigned char> mem;
    std::vector<int32_t> range;
    Store(int bits_, int rows_, int n_sb_, bool head_outside, unsigned seed, bool canary) : bits(bits_), rows(rows_), n_sb(n_sb_) {
        W = bits == 2 ? 6144 : 10240;
        if (head_outside) sh = n_sb * W * 4 + 64, ss = W * 4, sb = kHeads * sh + 256;        // spare bytes between heads and rows
        else sh = W * 4, ss = kHeads * sh, sb = n_sb * ss;
        bytes = rows * sb;
        mem.resize(bytes);
        range.resize(rows * kHeads);
        for (auto& c : mem) c = canary ? 0xC5 : (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
        for (auto& w : range) w = canary ? 0x7EADBEEF : (int32_t)((seed = seed * 1664525u + 1013904223u) >> 8);
    }
};

// the pieces of block j of a (row, head), from the description in kivi_mfma_layout.h: (byte offset in the (row, head)'s store, bytes)
struct Piece {
    int64_t off, n;
};
std::vector<Piece> pieces(const Store& s, bool is_k, int64_t j) {
    const int64_t code_bytes = s.bits == 2 ? 1024 : 2048, region0 = 16 * code_bytes;
    const int64_t sb = j / 16 * s.ss, g = j % 16;
    std::vector<Piece> out = {{sb + g * code_bytes, code_bytes}};
    for (int region = 0; region < 2; ++region) {
        const int64_t r0 = sb + region0 + region * 4096;
        if (is_k)
            for (int q = 0; q < 16; ++q) out.push_back({r0 + ((g >> 3) * 1024 + q * 64 + (g & 7) * 8) * 2, 16});
        else
            out.push_back({r0 + g * 256, 256});
    }
    return out;
}

template <typename Row>
void one_case(int bits, bool is_k, int n_blocks, int shift, const std::vector<Row>& rows, bool descending) {
    const int n_rows = (int)rows.size(), total = n_blocks + shift;
    Store src(bits, kSrcRows, (n_blocks + 15) / 16 + 1, true, 11u * n_blocks + shift + bits, false);
    Store got(bits, kDstRows, (total + 15) / 16 + 2, false, 0, true), want = got;
    const Store orig = got;
    std::vector<unsigned char> inside(got.bytes, 0);       // the bytes an admission has to write
    for (int i = 0; i < n_rows; ++i) {
        const int64_t r = (int64_t)rows[i];
        if (r < 0 || r >= kDstRows) continue;
        for (int h = 0; h < kHeads; ++h) {
            const int64_t dbase = r * got.sb + h * got.sh, sbase = i * src.sb + h * src.sh;
            for (int j = 0; j < total; ++j) {
                const auto dst = pieces(got, is_k, j);
                for (size_t p = 0; p < dst.size(); ++p) {
                    memset(&inside[dbase + dst[p].off], 1, dst[p].n);
                    if (j < shift) memset(&want.mem[dbase + dst[p].off], 0, dst[p].n);
                    else memcpy(&want.mem[dbase + dst[p].off], &src.mem[sbase + pieces(src, is_k, j - shift)[p].off], dst[p].n);
                }
            }
            want.range[r * kHeads + h] = src.range[i * kHeads + h];
        }
    }
    const Store src_before = src;
    // the kernel's grid
    KiviAdmitGeom g = {};
    g.s_sb = src.sb, g.s_sh = src.sh, g.s_ss = src.ss, g.d_sb = got.sb, g.d_sh = got.sh, g.d_ss = got.ss;
    g.nh_kv = kHeads, g.n_blocks = (uint32_t)n_blocks, g.shift = (uint32_t)shift;
    const int64_t threads = kivi_admit_threads(bits, n_rows, kHeads, n_blocks, shift);
    CHECK(threads == (int64_t)n_rows * kHeads * total * (bits == 2 ? 96 : 160), "threads = %lld", (long long)threads);
    g.threads = (uint32_t)threads;
    std::vector<unsigned char> writes(got.bytes, 0), range_writes(kDstRows * kHeads, 0);
    const int64_t grid = (threads + kAdmitThreads - 1) / kAdmitThreads * kAdmitThreads;       // whole workgroups, as launched
    for (int64_t n = 0; n < grid; ++n) {
        const int64_t t = descending ? grid - 1 - n : n;
        if (t >= g.threads) continue;
        const KiviAdmitMove m = kivi_admit_move(bits, is_k, g, (uint32_t)t);
        CHECK((int)m.i < n_rows && m.h < (uint32_t)kHeads, "thread %lld -> row %u head %u", (long long)t, m.i, m.h);
        if ((int)m.i >= n_rows || m.h >= (uint32_t)kHeads) continue;
        const int64_t r = (int64_t)rows[m.i];
        if (r < 0 || r >= kDstRows) continue;
        unsigned char v[16] = {};
        if (m.copy) {
            CHECK(m.src >= 0 && m.src % 16 == 0 && m.src + 16 <= src.bytes, "thread %lld reads at %lld", (long long)t, (long long)m.src);
            memcpy(v, src.mem.data() + m.src, 16);        // (ASan sees a read outside the vector)
        }
        const int64_t at = r * g.d_sb + m.dst;
        CHECK(at >= 0 && at % 16 == 0 && at + 16 <= got.bytes, "thread %lld writes at %lld", (long long)t, (long long)at);
        memcpy(got.mem.data() + at, v, 16);
        for (int b = 0; b < 16; ++b) ++writes[at + b];
        if (m.range) {
            got.range[r * g.nh_kv + m.h] = src.range[(int64_t)m.i * g.nh_kv + m.h];
            ++range_writes[r * g.nh_kv + m.h];
        }
    }
    int64_t bad = 0, twice = 0, outside = 0, missed = 0, moved = 0;
    for (int64_t i = 0; i < got.bytes; ++i) {
        bad += got.mem[i] != want.mem[i];
        twice += writes[i] > 1;
        outside += !inside[i] && writes[i];
        missed += inside[i] && !writes[i];
        moved += !inside[i] && got.mem[i] != orig.mem[i];
    }
    const char* what = is_k ? "K" : "V";
    CHECK(bad == 0, "%s %d-bit n=%d shift=%d: %lld bytes differ from the per-block copy", what, bits, n_blocks, shift, (long long)bad);
    CHECK(twice == 0, "%s %d-bit n=%d shift=%d: %lld bytes written twice", what, bits, n_blocks, shift, (long long)twice);
    CHECK(outside == 0 && moved == 0, "%s %d-bit n=%d shift=%d: %lld bytes outside the admitted blocks written, %lld canaries changed", what, bits,
          n_blocks, shift, (long long)outside, (long long)moved);
    CHECK(missed == 0, "%s %d-bit n=%d shift=%d: %lld bytes of the admitted blocks never written", what, bits, n_blocks, shift, (long long)missed);
    CHECK(src.mem == src_before.mem && src.range == src_before.range, "%s %d-bit n=%d shift=%d: the source changed", what, bits, n_blocks, shift);
    for (int w = 0; w < kDstRows * kHeads; ++w) {
        CHECK(got.range[w] == want.range[w], "%s %d-bit n=%d shift=%d: range word %d is %#x, expected %#x", what, bits, n_blocks, shift, w,
              got.range[w], want.range[w]);
        CHECK(range_writes[w] == (want.range[w] != orig.range[w]), "%s %d-bit n=%d shift=%d: range word %d written %d times", what, bits, n_blocks,
              shift, w, range_writes[w]);
    }
}

}  // namespace

int main() {
    const std::vector<int32_t> rows32 = {2, 0};
    const std::vector<int64_t> rows64 = {2, 0}, with_strays = {2, 7, 0}, stray_low = {-1, 1};
    for (int bits : {2, 4})
        for (int is_k = 0; is_k < 2; ++is_k)
            for (int n_blocks : {3, 19})
                for (int shift : {0, 2, 14, 16, 37}) {
                    one_case(bits, is_k, n_blocks, shift, rows32, false);
                    one_case(bits, is_k, n_blocks, shift, rows64, shift == 14);
                    one_case(bits, is_k, n_blocks, shift, with_strays, shift == 2);
                    one_case(bits, is_k, n_blocks, shift, stray_low, false);
                }
    for (int is_k = 0; is_k < 2; ++is_k) one_case(2, is_k, 0, 5, rows32, false);          // no packed block yet: only the zeroed lead
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("admit walk ok\n");
    return g_failed != 0;
}
