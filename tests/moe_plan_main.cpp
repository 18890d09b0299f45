// Stand-alone program over kivi_amd/csrc/kivi_moe_plan.h, the host-side arithmetic of kivi_moe_route / kivi_moe_experts (DESIGN.md
// section 29), built with -fsanitize=address,undefined by tests/test_moe_cpu.py and run as a child process.
//   1. the tile bound min(E, N K) + N K / TILE is at least the true tile count of adversarial count vectors -- everything on one
//      expert; one pair on as many experts as possible and the rest on one; every expert one pair short of / exactly at / one pair
//      past a full tile; random splits -- and is reached exactly by a vector of its own;
//   2. a tile list built the way the plan kernel builds it (experts ascending, tiles of at most TILE rows) written into an array of
//      exactly the bound's length stays inside it and covers every row of `pairs` once;
//   3. grid sizes and workspace bytes: the regions of the workspace do not overlap and end at the size, the grids cover the work;
//   4. the refusals: shapes outside the supported range give -1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kivi_amd/csrc/kivi_moe_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s: ", #cond);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            failures++;                                   \
        }                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// counts must sum to N * K with no expert above N (a token names an expert once)
static void hold(const std::vector<int64_t>& counts, int64_t N, int E, int K, const char* what) {
    const int64_t nk = N * K, bound = kivi_moe_plan_max_tiles(N, E, K);
    int64_t sum = 0;
    for (int e = 0; e < E; e++) {
        sum += counts[e];
        CHECK(counts[e] >= 0 && counts[e] <= N, "%s: N=%lld E=%d K=%d counts[%d]=%lld", what, (long long)N, E, K, e, (long long)counts[e]);
    }
    CHECK(sum == nk, "%s: N=%lld E=%d K=%d sum %lld", what, (long long)N, E, K, (long long)sum);
    const int64_t tiles = kivi_moe_plan_tiles_of(counts.data(), E);
    CHECK(tiles <= bound, "%s: N=%lld E=%d K=%d tiles %lld > bound %lld", what, (long long)N, E, K, (long long)tiles, (long long)bound);
    // the plan kernel's walk into an array of exactly the bound's length (the sanitizer watches the writes)
    std::vector<int> list((size_t)bound * KIVI_MOE_TILE_WORDS, -1);
    std::vector<int> covered((size_t)nk, 0);
    int64_t t = 0, off = 0;
    for (int e = 0; e < E; e++) {
        for (int64_t j = 0; j * KIVI_MOE_TOKEN_TILE < counts[e]; j++, t++) {
            int* tl = &list[(size_t)t * KIVI_MOE_TILE_WORDS];
            const int64_t left = counts[e] - j * KIVI_MOE_TOKEN_TILE;
            tl[0] = e;
            tl[1] = (int)(off + j * KIVI_MOE_TOKEN_TILE);
            tl[2] = (int)(left < KIVI_MOE_TOKEN_TILE ? left : KIVI_MOE_TOKEN_TILE);
            for (int r = 0; r < tl[2]; r++) covered[(size_t)tl[1] + r]++;
        }
        off += counts[e];
    }
    CHECK(t == tiles, "%s: walked %lld tiles, counted %lld", what, (long long)t, (long long)tiles);
    for (int64_t p = 0; p < nk; p++) CHECK(covered[(size_t)p] == 1, "%s: row %lld covered %d times", what, (long long)p, covered[(size_t)p]);
}

static void spread(std::vector<int64_t>& counts, int64_t rest, int64_t N, int E, int from) {
    for (int e = from; rest > 0; e = (e + 1) % E) {             // the rest wherever there is room
        const int64_t room = N - counts[e], take = room < rest ? room : rest;
        counts[e] += take;
        rest -= take;
    }
}

static void bounds() {
    const int T = KIVI_MOE_TOKEN_TILE;
    const int shapes[][2] = {{1, 1}, {2, 1}, {2, 2}, {8, 2}, {12, 4}, {60, 4}, {128, 8}, {256, 16}, {256, 1}, {17, 16}};
    const int64_t tokens[] = {1, 2, 5, 15, 16, 17, 31, 32, 33, 64, 255, 256, 257, 1000, 4099};
    for (auto& s : shapes) {
        const int E = s[0], K = s[1];
        for (int64_t N : tokens) {
            const int64_t nk = N * K;
            std::vector<int64_t> c(E, 0);
            spread(c, nk, N, E, 0);                             // as few experts as possible, each full
            hold(c, N, E, K, "packed");
            c.assign(E, 0);                                     // one pair on as many experts as possible, the rest packed
            int64_t rest = nk;
            for (int e = 0; e < E && rest > 0; e++, rest--) c[e] = 1;
            spread(c, rest, N, E, E - 1);
            hold(c, N, E, K, "one pair each");
            for (int d = -1; d <= 1; d++) {                     // experts at a tile boundary - 1, + 0, + 1
                c.assign(E, 0);
                rest = nk;
                for (int e = 0; e < E && rest > 0; e++) {
                    int64_t want = T * (1 + e % 3) + d;
                    want = want > N ? N : want;
                    want = want > rest ? rest : want;
                    c[e] = want;
                    rest -= want;
                }
                spread(c, rest, N, E, 0);
                hold(c, N, E, K, "tile boundaries");
            }
            for (int rep = 0; rep < 8; rep++) {                 // random splits
                c.assign(E, 0);
                rest = nk;
                while (rest > 0) {
                    const int e = (int)(rng() % (uint64_t)E);
                    const int64_t room = N - c[e];
                    if (room == 0) continue;
                    int64_t take = 1 + (int64_t)(rng() % (uint64_t)(2 * T + 2));
                    take = take > room ? room : take;
                    take = take > rest ? rest : take;
                    c[e] += take;
                    rest -= take;
                }
                hold(c, N, E, K, "random");
            }
        }
    }
    // the bound is reached: E < T experts with one pair past a full tile each, N = T + 1 tokens, K = E
    {
        const int E = 8, K = 8;
        const int64_t N = T + 1;
        std::vector<int64_t> c(E, T + 1);
        hold(c, N, E, K, "tight");
        CHECK(kivi_moe_plan_tiles_of(c.data(), E) == kivi_moe_plan_max_tiles(N, E, K), "the bound is not tight where it should be");
    }
}

static void sizes() {
    const int64_t geoms[][5] = {{1, 4096, 14336, 8, 2}, {64, 2048, 768, 128, 8}, {5, 256, 96, 60, 4}, {1000, 256, 128, 8, 2}, {1, 32, 32, 1, 1}};
    for (auto& g : geoms) {
        const int64_t N = g[0], H = g[1], I = g[2];
        const int E = (int)g[3], K = (int)g[4];
        const int64_t nk = kivi_moe_plan_pairs(N, E, K), ws = kivi_moe_plan_workspace_bytes(N, H, I, E, K);
        CHECK(nk == N * K, "pairs");
        const int64_t act = kivi_moe_plan_act_bytes(nk, I);
        CHECK(act % 16 == 0 && act >= nk * I * 2 && act < nk * I * 2 + 16, "act region %lld", (long long)act);
        CHECK(ws == act + nk * H * 4, "workspace %lld", (long long)ws);
        CHECK(kivi_moe_plan_grids_ok(N, H, I), "grids refused");
        CHECK(kivi_moe_plan_route_blocks(N) * 4 >= N && (kivi_moe_plan_route_blocks(N) - 1) * 4 < N, "route blocks");
        CHECK(kivi_moe_plan_row_blocks(I) * KIVI_MOE_ROW_TILE == I && kivi_moe_plan_row_blocks(H) * KIVI_MOE_ROW_TILE == H, "row blocks");
        const int64_t cb = kivi_moe_plan_combine_blocks(N, H);
        CHECK(cb * 256 >= N * (H / 4) && (cb - 1) * 256 < N * (H / 4), "combine blocks");
    }
}

static void refusals() {
    CHECK(kivi_moe_plan_pairs(0, 8, 2) == -1 && kivi_moe_plan_pairs(-3, 8, 2) == -1, "N < 1");
    CHECK(kivi_moe_plan_pairs(4, 0, 1) == -1 && kivi_moe_plan_pairs(4, 257, 2) == -1, "E outside [1, 256]");
    CHECK(kivi_moe_plan_pairs(4, 8, 0) == -1 && kivi_moe_plan_pairs(4, 8, 9) == -1 && kivi_moe_plan_pairs(4, 64, 17) == -1, "K");
    CHECK(kivi_moe_plan_pairs(4, 256, 16) == 64 && kivi_moe_plan_pairs(4, 1, 1) == 4, "the corners of the range");
    const int64_t top = ((int64_t)1 << 31) - 1;
    CHECK(kivi_moe_plan_pairs(top, 8, 1) == top && kivi_moe_plan_pairs(top, 8, 2) == -1, "N * K < 2^31");
    CHECK(kivi_moe_plan_pairs(top / 16, 16, 16) == top / 16 * 16 && kivi_moe_plan_pairs(top / 16 + 1, 16, 16) == -1, "N * K < 2^31");
    CHECK(kivi_moe_plan_max_tiles(top, 8, 1) < ((int64_t)1 << 31), "the bound fits an int");
    CHECK(kivi_moe_plan_max_tiles(0, 8, 2) == -1 && kivi_moe_plan_max_tiles(4, 300, 2) == -1, "max_tiles of a refused shape");
    CHECK(kivi_moe_plan_dtype_ok(16) && kivi_moe_plan_dtype_ok(0x110) && !kivi_moe_plan_dtype_ok(32) && !kivi_moe_plan_dtype_ok(0), "dtypes");
    CHECK(!kivi_moe_plan_dims_ok(0, 32) && !kivi_moe_plan_dims_ok(48, 32) && !kivi_moe_plan_dims_ok(32, 80) && kivi_moe_plan_dims_ok(96, 32), "H, I");
    CHECK(kivi_moe_plan_workspace_bytes(4, 48, 32, 8, 2) == -1 && kivi_moe_plan_workspace_bytes(4, 64, 32, 8, 9) == -1, "workspace of a refused shape");
    CHECK(!kivi_moe_plan_grids_ok(1, 16 * 65536, 32) && !kivi_moe_plan_grids_ok(1, 32, 16 * 65536) && kivi_moe_plan_grids_ok(1, 16 * 65535, 32),
          "row blocks beyond a grid's second dimension");
}

int main() {
    bounds();
    sizes();
    refusals();
    if (failures) return 1;
    std::printf("moe plan ok\n");
    return 0;
}
