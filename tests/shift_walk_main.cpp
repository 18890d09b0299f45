// Host play of the in-place block shift (kivi_amd/csrc/kivi_shift.hip) over kivi_amd/csrc/kivi_shift.h, built as plain C++ with
// -fsanitize=address,undefined by tests/test_rebase_cpu.py.  A randomly filled store of (B, n_sb, nh_kv, W) words is shifted the way
// the kernel's grid does it: every thread (one 16-byte unit position of one (row, head)), every batch of kShiftInFlight blocks -- the
// loads of the NEXT batch into a thread-private array, then the stores of the current one --, then the zeroing of the vacated blocks.
// Threads run one after the other in ascending AND in descending order: the result may not depend on it.  Compared with a naive out-of-place shift written
// from the layout's description (not from the header's address function); a shadow array records which thread touched every byte
// (read or written): one owner per byte, no owner outside the blocks in use.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../kivi_amd/csrc/kivi_shift.h"

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

constexpr int kB = 2, kHeads = 2;

struct Store {
    int bits, n_sb;
    int64_t W, ss, sh, sb, bytes;                          // words per super-block; strides and size in bytes
    std::vector<unsigned char> mem;
    Store(int bits_, int n_sb_, unsigned seed) : bits(bits_), n_sb(n_sb_) {
        W = bits == 2 ? 6144 : 10240;
        sh = W * 4, ss = kHeads * sh, sb = n_sb * ss, bytes = kB * sb;      // the super-block index outside the head index
        mem.resize(bytes);
        for (auto& c : mem) c = (unsigned char)((seed = seed * 1664525u + 1013904223u) >> 24);
    }
};

// the pieces of block j of a (row, head), from the description in kivi_mfma_layout.h: (byte offset in the store row, bytes, is scale)
struct Piece {
    int64_t off, n;
    bool scale;
};
std::vector<Piece> pieces(const Store& s, bool is_k, int64_t j) {
    const int64_t code_bytes = s.bits == 2 ? 1024 : 2048, region0 = 16 * code_bytes;
    const int64_t sb = j / 16 * s.ss, g = j % 16;
    std::vector<Piece> out = {{sb + g * code_bytes, code_bytes, false}};
    for (int region = 0; region < 2; ++region) {
        const int64_t r0 = sb + region0 + region * 4096;
        if (is_k)
            for (int q = 0; q < 16; ++q) out.push_back({r0 + ((g >> 3) * 1024 + q * 64 + (g & 7) * 8) * 2, 16, region == 0});
        else
            out.push_back({r0 + g * 256, 256, region == 0});
    }
    return out;
}

void one_case(int bits, bool is_k, int n_blocks, int shift, bool descending) {
    const int n_sb = (n_blocks + 15) / 16 + 1;             // one super-block more than in use: it has to stay as it is
    Store got(bits, n_sb, 7u * n_blocks + shift + bits), orig = got, want = got;
    const int n_keep = n_blocks - shift;
    std::vector<unsigned char> used(got.bytes, 0);
    uint32_t want_top[kB * kHeads] = {};
    for (int rh = 0; rh < kB * kHeads; ++rh) {
        const int64_t base = rh / kHeads * got.sb + rh % kHeads * got.sh;
        for (int j = 0; j < n_blocks; ++j) {
            const auto dst = pieces(got, is_k, j);
            const auto src = pieces(got, is_k, j + shift);
            for (size_t p = 0; p < dst.size(); ++p) {
                memset(&used[base + dst[p].off], 1, dst[p].n);
                if (j >= n_keep) {
                    memset(&want.mem[base + dst[p].off], 0, dst[p].n);
                    continue;
                }
                memcpy(&want.mem[base + dst[p].off], &orig.mem[base + src[p].off], dst[p].n);
                if (dst[p].scale)
                    for (int64_t i = 0; i < dst[p].n; i += 2) {
                        uint16_t h;
                        memcpy(&h, &orig.mem[base + src[p].off + i], 2);
                        if (h > want_top[rh]) want_top[rh] = h;
                    }
            }
        }
    }
    // the kernel's grid
    std::vector<int32_t> owner(got.bytes, -1);
    int64_t shared = 0;
    uint32_t got_top[kB * kHeads] = {};
    const int64_t threads = (int64_t)kB * kHeads * kivi_shift_block_units(bits);
    auto touch = [&](int64_t at, int32_t t) {
        for (int b = 0; b < 16; ++b) {
            shared += owner[at + b] != -1 && owner[at + b] != t;
            owner[at + b] = t;
        }
    };
    for (int64_t i = 0; i < threads; ++i) {
        const int64_t t = descending ? threads - 1 - i : i;
        int64_t rh;
        uint32_t u;
        kivi_shift_thread(bits, t, &rh, &u);
        CHECK(rh >= 0 && rh < kB * kHeads && u < kivi_shift_block_units(bits), "thread %lld -> (%lld, %u)", (long long)t, (long long)rh, u);
        const int64_t base = rh / kHeads * got.sb + rh % kHeads * got.sh;
        unsigned char* p = got.mem.data() + base;
        uint32_t top = 0;
        unsigned char cur[kShiftInFlight][16], nxt[kShiftInFlight][16];
        auto load = [&](int64_t j, unsigned char* v) {             // unit u of block j + shift, if block j is a destination
            if (j >= n_keep) return;
            const int64_t off = kivi_shift_offset(bits, is_k, got.ss, j + shift, u);
            memcpy(v, p + off, 16);
            touch(base + off, (int32_t)t);
        };
        for (int k = 0; k < kShiftInFlight; ++k) load(k, cur[k]);
        for (int64_t j0 = 0; j0 < n_keep; j0 += kShiftInFlight) {
            for (int k = 0; k < kShiftInFlight; ++k) load(j0 + kShiftInFlight + k, nxt[k]);      // the next batch first
            for (int k = 0; k < kShiftInFlight; ++k)
                if (j0 + k < n_keep) {
                    const int64_t off = kivi_shift_offset(bits, is_k, got.ss, j0 + k, u);
                    memcpy(p + off, cur[k], 16);
                    touch(base + off, (int32_t)t);
                    if (kivi_shift_is_scale(bits, u))
                        for (int i = 0; i < 16; i += 2) {
                            uint16_t h;
                            memcpy(&h, cur[k] + i, 2);
                            if (h > top) top = h;
                        }
                }
            memcpy(cur, nxt, sizeof cur);
        }
        for (int64_t j = n_keep; j < n_blocks; ++j) {
            const int64_t off = kivi_shift_offset(bits, is_k, got.ss, j, u);
            memset(p + off, 0, 16);
            touch(base + off, (int32_t)t);
        }
        if (kivi_shift_is_scale(bits, u) && n_keep > 0 && top > got_top[rh]) got_top[rh] = top;
    }
    int64_t bad = 0, outside = 0, untouched = 0, moved = 0, dirty = 0;
    for (int64_t i = 0; i < got.bytes; ++i) {
        bad += got.mem[i] != want.mem[i];
        outside += !used[i] && owner[i] != -1;
        untouched += used[i] && owner[i] == -1;
        moved += !used[i] && got.mem[i] != orig.mem[i];
    }
    for (int rh = 0; rh < kB * kHeads; ++rh)
        for (int j = n_keep; j < n_blocks; ++j)
            for (const Piece& pc : pieces(got, is_k, j))
                for (int64_t i = 0; i < pc.n; ++i) dirty += got.mem[rh / kHeads * got.sb + rh % kHeads * got.sh + pc.off + i] != 0;
    const char* what = is_k ? "K" : "V";
    CHECK(bad == 0, "%s %d-bit n_blocks=%d shift=%d: %lld bytes differ from the out-of-place shift", what, bits, n_blocks, shift, (long long)bad);
    CHECK(shared == 0, "%s %d-bit n_blocks=%d shift=%d: %lld byte touches by a second thread", what, bits, n_blocks, shift, (long long)shared);
    CHECK(outside == 0 && moved == 0, "%s %d-bit n_blocks=%d shift=%d: %lld bytes outside the blocks in use touched, %lld changed", what, bits,
          n_blocks, shift, (long long)outside, (long long)moved);
    CHECK(untouched == 0, "%s %d-bit n_blocks=%d shift=%d: %lld bytes of the blocks in use never touched", what, bits, n_blocks, shift,
          (long long)untouched);
    CHECK(dirty == 0, "%s %d-bit n_blocks=%d shift=%d: %lld bytes of the vacated blocks are not zero", what, bits, n_blocks, shift, (long long)dirty);
    for (int rh = 0; rh < kB * kHeads; ++rh)
        CHECK(got_top[rh] == want_top[rh], "%s %d-bit n_blocks=%d shift=%d: largest kept scale of unit %d: %#x, expected %#x", what, bits, n_blocks,
              shift, rh, got_top[rh], want_top[rh]);
}

// the units of a block tile its pieces exactly: every byte of every piece belongs to one unit, at both widths
void units_tile_a_block() {
    for (int bits : {2, 4})
        for (int is_k = 0; is_k < 2; ++is_k) {
            Store s(bits, 3, 1);
            for (int64_t j : {0, 7, 8, 15, 16, 40}) {
                std::vector<int> hits(s.sb, 0);
                for (uint32_t u = 0; u < kivi_shift_block_units(bits); ++u) {
                    const int64_t off = kivi_shift_offset(bits, is_k, s.ss, j, u);
                    CHECK(off % 16 == 0 && off >= 0 && off + 16 <= (int64_t)hits.size(), "unit %u of block %lld at %lld", u, (long long)j, (long long)off);
                    for (int b = 0; b < 16; ++b) ++hits[off + b];
                }
                int64_t wrong = 0, total = 0;
                for (const Piece& pc : pieces(s, is_k, j))
                    for (int64_t i = 0; i < pc.n; ++i) wrong += hits[pc.off + i] != 1, ++total;
                CHECK(wrong == 0 && total == 16 * (int64_t)kivi_shift_block_units(bits), "%d-bit is_k=%d block %lld: %lld bytes of its pieces not in one unit",
                      bits, is_k, (long long)j, (long long)wrong);
            }
        }
}

}  // namespace

int main() {
    static_assert(kShiftInFlight > 3 && kShiftInFlight < 15, "shifts below and above the batch are among the cases");
    units_tile_a_block();
    for (int bits : {2, 4})
        for (int is_k = 0; is_k < 2; ++is_k)
            for (int n_blocks : {13, 16, 17, 40, 48, 49})         // ends inside, at and just past a super-block
                for (int shift : {1, 3, 8, 15, 16, 17, 33, n_blocks})
                    if (shift <= n_blocks)
                        for (int descending = 0; descending < 1 + (shift == 1 || shift == 8 || shift == 17); ++descending)
                            one_case(bits, is_k, n_blocks, shift, descending);
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("shift walk ok\n");
    return g_failed != 0;
}
