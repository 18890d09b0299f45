// Stand-alone program over kivi_amd/csrc/kivi_w4_plan.h, the host-side arithmetic of the 4-bit weight entries,
// built with -fsanitize=address,undefined by tests/test_w4_cpu.py and run as a child process.
//   1. the layout: every element (o, k) of a weight lands on its own 4-bit field inside the code buffer, and every field is used
//      (written into an array of exactly kivi_w4_plan_code_words words: the sanitizer watches the writes); likewise the halves of
//      the scale / mn buffers;
//   2. the runs of tiles of the 8 waves partition the stripe's tiles in order, also where K / 128 is no multiple of 8 or below it,
//      and every run holds whole groups;
//   3. grids, buffer sizes, the token tiles and passes for N in {1, 16, 17, 32, 33, 64, 65, 4096};
//   4. the refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kivi_amd/csrc/kivi_w4_plan.h"

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

static void layout() {
    const int64_t shapes[][3] = {{16, 128, 64}, {16, 128, 128}, {48, 384, 64}, {32, 896, 128}, {64, 1152, 64}};
    for (auto& s : shapes) {
        const int64_t O = s[0], K = s[1];
        const int G = (int)s[2];
        const int64_t words = kivi_w4_plan_code_words(O, K, G), halves = kivi_w4_plan_sm_halves(O, K, G);
        CHECK(words == O * K / 8 && halves == O * K / G, "sizes O=%lld K=%lld", (long long)O, (long long)K);
        CHECK(kivi_w4_plan_bytes(O, K, G) == words * 4 + 2 * halves * 2, "bytes O=%lld K=%lld", (long long)O, (long long)K);
        std::vector<uint32_t> code((size_t)words, 0u);
        for (int64_t o = 0; o < O; o++)
            for (int64_t k = 0; k < K; k++) {
                const int64_t w = kivi_w4_plan_word(o, k, K);
                const int b = kivi_w4_plan_bit(k);
                CHECK(w >= 0 && w < words && b >= 0 && b <= 28 && b % 4 == 0, "word %lld bit %d", (long long)w, b);
                if (w < 0 || w >= words) continue;
                CHECK(((code[(size_t)w] >> b) & 15u) == 0u, "field (%lld, %lld) taken twice", (long long)o, (long long)k);
                code[(size_t)w] |= 15u << b;
                // the 8 elements of a chunk share a word; a lane's word j of tile t holds elements 32 j + 8 kb + e of row r
                const int64_t tile = w / KIVI_W4_TILE_WORDS, in = w % KIVI_W4_TILE_WORDS, lane = in / 4, j = in % 4;
                CHECK(tile == (o / 16) * (K / 128) + k / 128 && lane % 16 == o % 16 && 32 * j + 8 * (lane / 16) + (k & 7) == k % 128,
                      "lane / word of (%lld, %lld)", (long long)o, (long long)k);
            }
        for (int64_t w = 0; w < words; w++) CHECK(code[(size_t)w] == 0xFFFFFFFFu, "word %lld not filled", (long long)w);
        std::vector<int> sm((size_t)halves, 0);
        for (int64_t o = 0; o < O; o++)
            for (int64_t g = 0; g < K / G; g++) {
                const int64_t h = kivi_w4_plan_sm_half(o, g, K, G);
                CHECK(h >= 0 && h < halves, "half %lld", (long long)h);
                if (h >= 0 && h < halves) sm[(size_t)h]++;
            }
        for (int64_t h = 0; h < halves; h++) CHECK(sm[(size_t)h] == 1, "half %lld used %d times", (long long)h, sm[(size_t)h]);
    }
}

static void stretches() {
    for (int64_t K = 128; K <= 128 * 90; K += 128) {
        const int64_t T = kivi_w4_plan_tiles(K);
        CHECK(kivi_w4_plan_wave_tile0(K, 0) == 0 && kivi_w4_plan_wave_tile0(K, KIVI_W4_WAVES) == T, "ends K=%lld", (long long)K);
        int64_t longest = 0, shortest = T;
        for (int w = 0; w < KIVI_W4_WAVES; w++) {
            const int64_t a = kivi_w4_plan_wave_tile0(K, w), b = kivi_w4_plan_wave_tile0(K, w + 1);
            CHECK(a <= b, "order K=%lld w=%d", (long long)K, w);
            longest = b - a > longest ? b - a : longest;
            shortest = b - a < shortest ? b - a : shortest;
            // a run starts and ends on a tile, a tile holds whole groups of 64 and of 128
            CHECK((a * KIVI_W4_K_TILE) % 128 == 0 && (a * KIVI_W4_K_TILE) % 64 == 0, "group alignment");
        }
        CHECK(longest - shortest <= 1, "K=%lld dealt unevenly: %lld vs %lld", (long long)K, (long long)longest, (long long)shortest);
    }
    // K / 128 = 1, 3, 7, 9: fewer tiles than waves, and 7 and 9 dealt over 8
    CHECK(kivi_w4_plan_wave_tile0(128, 7) == 0 && kivi_w4_plan_wave_tile0(128, 8) == 1, "one tile goes to the last wave");
    CHECK(kivi_w4_plan_wave_tile0(384, 3) == 1 && kivi_w4_plan_wave_tile0(384, 6) == 2, "three tiles");
    CHECK(kivi_w4_plan_wave_tile0(896, 1) == 0 && kivi_w4_plan_wave_tile0(896, 2) == 1, "seven tiles");
    CHECK(kivi_w4_plan_wave_tile0(1152, 7) == 7 && kivi_w4_plan_wave_tile0(1152, 8) == 9, "nine tiles: the last wave takes two");
}

static void sizes() {
    const int64_t tokens[] = {1, 16, 17, 32, 33, 64, 65, 4096};
    const int tiles[] = {1, 1, 2, 2, 4, 4, 4, 4}, tiles_gu[] = {1, 1, 2, 2, 2, 2, 2, 2};
    const int64_t chunks[] = {1, 1, 1, 1, 1, 1, 2, 64}, chunks_gu[] = {1, 1, 1, 1, 2, 2, 3, 128};
    for (int i = 0; i < 8; i++) {
        CHECK(kivi_w4_plan_token_tiles(tokens[i], false) == tiles[i] && kivi_w4_plan_token_tiles(tokens[i], true) == tiles_gu[i],
              "token tiles of N=%lld", (long long)tokens[i]);
        CHECK(kivi_w4_plan_chunks(tokens[i], false) == chunks[i] && kivi_w4_plan_chunks(tokens[i], true) == chunks_gu[i],
              "passes of N=%lld", (long long)tokens[i]);
        CHECK(16 * kivi_w4_plan_token_tiles(tokens[i], false) <= KIVI_W4_TOKEN_CHUNK, "a pass beyond the chunk");
    }
    CHECK(kivi_w4_plan_stripes(4096) == 256 && kivi_w4_plan_tiles(11008) == 86 && kivi_w4_plan_stripes(22016) == 1376, "llama-2-7b grids");
    CHECK(kivi_w4_plan_elem_blocks(16, 128) == 1 && kivi_w4_plan_elem_blocks(48, 384) == 9 && kivi_w4_plan_elem_blocks(4096, 11008) == 22016,
          "element grids");
    CHECK(kivi_w4_plan_bytes(4096, 4096, 128) == 4096 * 4096 / 2 + 4 * 4096 * 32, "bytes of a 4096 x 4096 weight");
    CHECK(kivi_w4_plan_bytes(4096, 11008, 64) == (int64_t)4096 * 11008 / 2 + (int64_t)4 * 4096 * 172, "bytes at group 64");
}

static void refusals() {
    CHECK(kivi_w4_plan_dtype_ok(16) && kivi_w4_plan_dtype_ok(0x110) && !kivi_w4_plan_dtype_ok(32) && !kivi_w4_plan_dtype_ok(0), "dtypes");
    CHECK(kivi_w4_plan_group_ok(64) && kivi_w4_plan_group_ok(128) && !kivi_w4_plan_group_ok(32) && !kivi_w4_plan_group_ok(256) &&
          !kivi_w4_plan_group_ok(0) && !kivi_w4_plan_group_ok(96), "groups");
    CHECK(kivi_w4_plan_shape_ok(16, 128, 64) && kivi_w4_plan_shape_ok(4096, 11008, 128), "the range");
    CHECK(!kivi_w4_plan_shape_ok(0, 128, 64) && !kivi_w4_plan_shape_ok(24, 128, 64) && !kivi_w4_plan_shape_ok(-16, 128, 64), "O");
    CHECK(!kivi_w4_plan_shape_ok(16, 0, 64) && !kivi_w4_plan_shape_ok(16, 64, 64) && !kivi_w4_plan_shape_ok(16, 192, 64) &&
          !kivi_w4_plan_shape_ok(16, -128, 128), "K");
    CHECK(!kivi_w4_plan_shape_ok(16, 128, 32), "G");
    CHECK(!kivi_w4_plan_shape_ok((int64_t)1 << 30, (int64_t)1 << 20, 128) && kivi_w4_plan_shape_ok((int64_t)1 << 20, (int64_t)1 << 19, 128),
          "O * K < 2^40");
    CHECK(kivi_w4_plan_code_words(24, 128, 64) == -1 && kivi_w4_plan_sm_halves(16, 192, 64) == -1 && kivi_w4_plan_bytes(16, 128, 32) == -1,
          "sizes of a refused shape");
    const int64_t top = ((int64_t)1 << 31) - 1;
    CHECK(kivi_w4_plan_tokens_ok(1, 16) && !kivi_w4_plan_tokens_ok(0, 16) && !kivi_w4_plan_tokens_ok(-1, 16), "N >= 1");
    CHECK(kivi_w4_plan_tokens_ok(top / 16, 16) && !kivi_w4_plan_tokens_ok(top / 16 + 1, 16), "N * O < 2^31");
    CHECK(kivi_w4_plan_tokens_ok(524287, 4096) && !kivi_w4_plan_tokens_ok(524288, 4096), "N * O < 2^31 at O = 4096");
}

int main() {
    layout();
    stretches();
    sizes();
    refusals();
    if (failures) return 1;
    std::printf("w4 plan ok\n");
    return 0;
}
