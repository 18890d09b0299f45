// Host walk of the tile plan of kivi_prefill_attention (kivi_amd/csrc/kivi_prefill.hip) over kivi_amd/csrc/kivi_prefill_plan.h,
// built as plain C++ with -fsanitize=address,undefined by tests/test_prefill_attn_cpu.py.  For every T and lead of the issue's
// list, the whole grid of a (B = 2, nh = 3) call is walked the way the kernel walks it -- every block its rows and the key tiles it
// stages, every wave of the block its 32 rows and the tiles it multiplies -- and compared with the definition of a live pair
// (lead <= j <= i), written here without the header's functions:
//   * the union of the visited tiles covers exactly the live pairs: every live pair lies in a visited tile of its row's wave, once;
//   * no tile without a live pair is visited (neither by a block nor by a wave);
//   * "partial" is flagged exactly where a visited tile mixes live and dead pairs of the rows that visit it;
//   * every query row of every (batch row, head) belongs to exactly one block and one wave;
//   * the block order starts with the last query tile, and a wave's tiles are a prefix of its block's.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../kivi_amd/csrc/kivi_prefill_plan.h"

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

constexpr int kB = 2, kNh = 3;

bool live_pair(int i, int j, int lead) { return lead <= j && j <= i; }

// live and dead pairs of the rectangle rows [q0, q1) x the 32 keys of tile kt
void count(int q0, int q1, int kt, int lead, int64_t& live, int64_t& dead) {
    live = dead = 0;
    for (int i = q0; i < q1; ++i)
        for (int j = kt * kPrefillKTile; j < (kt + 1) * kPrefillKTile; ++j) (live_pair(i, j, lead) ? live : dead) += 1;
}

void one_case(int T, int raw_lead) {
    const int lead = kivi_prefill_clamp_lead(raw_lead, T);
    CHECK(lead >= 0 && lead <= T && (raw_lead < 0 || raw_lead > T || lead == raw_lead), "T=%d lead=%d clamps to %d", T, raw_lead, lead);
    const int64_t blocks = kivi_prefill_blocks(kB, kNh, T);
    const int nqt = (T + kPrefillQTile - 1) / kPrefillQTile, nkt = (T + kPrefillKTile - 1) / kPrefillKTile;
    CHECK(blocks == (int64_t)kB * kNh * nqt && kivi_prefill_qtiles(T) == nqt, "T=%d: %lld blocks", T, (long long)blocks);
    std::vector<int> row_owner((size_t)kB * kNh * T, 0);                 // blocks (waves) that own the row
    std::vector<int> covered((size_t)T * T, 0);                          // per (i, j) of unit (0, 0): visited how often
    int last_q0 = T;
    for (int64_t x = 0; x < blocks; ++x) {
        const KiviPrefillBlock blk = kivi_prefill_block(kB, kNh, T, (uint32_t)x);
        CHECK(blk.b >= 0 && blk.b < kB && blk.h >= 0 && blk.h < kNh, "T=%d block %lld -> row %d head %d", T, (long long)x, blk.b, blk.h);
        CHECK(blk.q0 >= 0 && blk.q0 < blk.q1 && blk.q1 <= T && blk.q0 % kPrefillQTile == 0 && blk.q1 - blk.q0 <= kPrefillQTile,
              "T=%d block %lld -> rows [%d, %d)", T, (long long)x, blk.q0, blk.q1);
        if (blk.b < 0 || blk.b >= kB || blk.h < 0 || blk.h >= kNh || blk.q0 < 0 || blk.q1 > T) continue;
        CHECK(blk.q0 <= last_q0, "T=%d block %lld: rows from %d after rows from %d (the longest tiles come first)", T, (long long)x,
              blk.q0, last_q0);
        last_q0 = blk.q0;
        const KiviPrefillTiles bt = kivi_prefill_tiles(blk.q0, blk.q1, lead);
        CHECK(bt.kt0 >= 0 && bt.kt0 <= bt.kt1 && bt.kt1 <= nkt, "T=%d lead=%d rows [%d, %d): tiles [%d, %d)", T, lead, blk.q0, blk.q1, bt.kt0,
              bt.kt1);
        for (int kt = 0; kt < nkt; ++kt) {
            int64_t live, dead;
            count(blk.q0, blk.q1, kt, lead, live, dead);
            const bool visited = kt >= bt.kt0 && kt < bt.kt1;
            CHECK(visited == (live > 0), "T=%d lead=%d block rows [%d, %d) tile %d: visited %d, %lld live pairs", T, lead, blk.q0, blk.q1, kt,
                  (int)visited, (long long)live);
            if (visited)
                CHECK(kivi_prefill_partial(blk.q0, blk.q1, lead, kt) == (dead > 0), "T=%d lead=%d block rows [%d, %d) tile %d: partial %d, %lld dead",
                      T, lead, blk.q0, blk.q1, kt, (int)kivi_prefill_partial(blk.q0, blk.q1, lead, kt), (long long)dead);
        }
        // the four waves of the block, as the kernel cuts them
        for (int wave = 0; wave < kPrefillThreads / 64; ++wave) {
            const int wq0 = blk.q0 + wave * kPrefillWaveRows, wq1 = wq0 + kPrefillWaveRows < blk.q1 ? wq0 + kPrefillWaveRows : blk.q1;
            if (wq0 >= wq1) continue;
            for (int i = wq0; i < wq1; ++i) ++row_owner[((size_t)blk.b * kNh + blk.h) * T + i];
            const KiviPrefillTiles wt = kivi_prefill_tiles(wq0, wq1, lead);
            CHECK(wt.kt0 == wt.kt1 || (wt.kt0 == bt.kt0 && wt.kt1 <= bt.kt1), "T=%d lead=%d wave rows [%d, %d): tiles [%d, %d) of [%d, %d)", T,
                  lead, wq0, wq1, wt.kt0, wt.kt1, bt.kt0, bt.kt1);
            for (int kt = 0; kt < nkt; ++kt) {
                int64_t live, dead;
                count(wq0, wq1, kt, lead, live, dead);
                const bool visited = kt >= wt.kt0 && kt < wt.kt1;
                CHECK(visited == (live > 0), "T=%d lead=%d wave rows [%d, %d) tile %d: visited %d, %lld live pairs", T, lead, wq0, wq1, kt,
                      (int)visited, (long long)live);
                if (!visited) continue;
                const bool partial = kivi_prefill_partial(wq0, wq1, lead, kt);
                CHECK(partial == (dead > 0), "T=%d lead=%d wave rows [%d, %d) tile %d: partial %d, %lld dead pairs", T, lead, wq0, wq1, kt,
                      (int)partial, (long long)dead);
                if (blk.b == 0 && blk.h == 0)
                    for (int i = wq0; i < wq1; ++i)
                        for (int j = kt * kPrefillKTile; j < (kt + 1) * kPrefillKTile && j < T; ++j)
                            if (!partial || live_pair(i, j, lead)) ++covered[(size_t)i * T + j];      // what the kernel's mask lets through
            }
        }
    }
    int64_t bad_rows = 0, bad_pairs = 0;
    for (int c : row_owner) bad_rows += c != 1;
    for (int i = 0; i < T; ++i)
        for (int j = 0; j < T; ++j) bad_pairs += covered[(size_t)i * T + j] != (live_pair(i, j, lead) ? 1 : 0);
    CHECK(bad_rows == 0, "T=%d lead=%d: %lld query rows do not belong to exactly one block and wave", T, lead, (long long)bad_rows);
    CHECK(bad_pairs == 0, "T=%d lead=%d: %lld pairs are not covered exactly when they are live", T, lead, (long long)bad_pairs);
}

}  // namespace

int main() {
    for (int T : {1, 15, 16, 17, 33, 64, 130, 1000})
        for (int lead : {0, 1, 5, 31, 32, 33, 64, T - 1, T}) one_case(T, lead);
    one_case(130, -3);                                     // clamped to 0
    one_case(130, 1 << 30);                                // clamped to T
    CHECK(kivi_prefill_blocks(1 << 15, 1 << 10, 1 << 20) == (int64_t)1 << 38, "the block count is taken in 64 bits");
    if (g_failed) printf("%d checks failed\n", g_failed);
    else printf("prefill plan ok\n");
    return g_failed != 0;
}
