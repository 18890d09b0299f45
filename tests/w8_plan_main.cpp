// Stand-alone program over kivi_amd/csrc/kivi_w8_plan.h, the host-side arithmetic of the FP8 weight entries,
// built with -fsanitize=address,undefined by tests/test_w8_cpu.py and run as a child process.
//   1. operand forming: over the stripes, tiles, steps and lanes of a weight every byte (o, k) is read exactly once, inside the
//      buffer (counted in an array of exactly O * K entries: the sanitizer watches the writes), the 8 elements a lane feeds one
//      MFMA step are consecutive, and all bytes of a tile of a stripe share the scale the kernel reads for it, which lies inside
//      the scale buffer -- also where the last block-row of scales is partial (O = 144);
//   2. the runs of tiles of the 8 waves partition the stripe's tiles in order, also where K / 128 is no multiple of 8 or below it;
//   3. grids, buffer sizes, the token tiles and passes for N in {1, 16, 17, 32, 33, 64, 65, 4096};
//   4. the refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kivi_amd/csrc/kivi_w8_plan.h"

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

static void operands() {
    const int64_t shapes[][2] = {{16, 128}, {48, 384}, {144, 896}, {272, 1152}};
    for (auto& s : shapes) {
        const int64_t O = s[0], K = s[1];
        const int64_t scales = kivi_w8_plan_scales(O, K);
        CHECK(scales == ((O + 127) / 128) * (K / 128), "scales O=%lld K=%lld", (long long)O, (long long)K);
        CHECK(kivi_w8_plan_bytes(O, K) == O * K + 4 * scales, "bytes O=%lld K=%lld", (long long)O, (long long)K);
        std::vector<int> read((size_t)(O * K), 0), scale_used((size_t)scales, 0);
        for (int64_t stripe = 0; stripe < kivi_w8_plan_stripes(O); stripe++)
            for (int64_t tile = 0; tile < kivi_w8_plan_tiles(K); tile++) {
                const int64_t si = kivi_w8_plan_stripe_scale_row(stripe) * kivi_w8_plan_scale_cols(K) + tile;   // what the kernel reads
                CHECK(si >= 0 && si < scales, "scale %lld of stripe %lld tile %lld", (long long)si, (long long)stripe, (long long)tile);
                if (si >= 0 && si < scales) scale_used[(size_t)si]++;
                for (int step = 0; step < 4; step++)
                    for (int lane = 0; lane < 64; lane++) {
                        const int64_t o = stripe * KIVI_W8_ROW_TILE + (lane & 15), k0 = kivi_w8_plan_step_k(tile, step, lane >> 4);
                        CHECK(k0 % 8 == 0 && k0 / 128 == tile, "step k %lld", (long long)k0);
                        // the lane's 16-byte load of half step >> 1 covers it: bytes 128 tile + 64 h + 16 kb .. + 16
                        const int64_t load = tile * 128 + 64 * (step >> 1) + 16 * (lane >> 4);
                        CHECK(k0 >= load && k0 + 8 <= load + 16 && load % 16 == 0, "load %lld", (long long)load);
                        for (int e = 0; e < 8; e++) {
                            const int64_t k = k0 + e;
                            CHECK(o < O && k < K, "(%lld, %lld) outside", (long long)o, (long long)k);
                            if (o >= O || k >= K) continue;
                            read[(size_t)(o * K + k)]++;
                            CHECK(kivi_w8_plan_scale_index(o, k, K) == si, "scale of (%lld, %lld)", (long long)o, (long long)k);
                        }
                    }
            }
        for (int64_t i = 0; i < O * K; i++) CHECK(read[(size_t)i] == 1, "byte %lld read %d times", (long long)i, read[(size_t)i]);
        for (int64_t i = 0; i < scales; i++) CHECK(scale_used[(size_t)i] >= 1, "scale %lld unused", (long long)i);
    }
    CHECK(kivi_w8_plan_scale_index(127, 127, 384) == 0 && kivi_w8_plan_scale_index(128, 0, 384) == 3 &&
          kivi_w8_plan_scale_index(143, 383, 384) == 5, "the block-row changes at row 128");
    CHECK(kivi_w8_plan_stripe_scale_row(7) == 0 && kivi_w8_plan_stripe_scale_row(8) == 1, "8 stripes per block-row");
}

static void stretches() {
    for (int64_t K = 128; K <= 128 * 90; K += 128) {
        const int64_t T = kivi_w8_plan_tiles(K);
        CHECK(kivi_w8_plan_wave_tile0(K, 0) == 0 && kivi_w8_plan_wave_tile0(K, KIVI_W8_WAVES) == T, "ends K=%lld", (long long)K);
        int64_t longest = 0, shortest = T;
        for (int w = 0; w < KIVI_W8_WAVES; w++) {
            const int64_t a = kivi_w8_plan_wave_tile0(K, w), b = kivi_w8_plan_wave_tile0(K, w + 1);
            CHECK(a <= b, "order K=%lld w=%d", (long long)K, w);
            longest = b - a > longest ? b - a : longest;
            shortest = b - a < shortest ? b - a : shortest;
        }
        CHECK(longest - shortest <= 1, "K=%lld dealt unevenly: %lld vs %lld", (long long)K, (long long)longest, (long long)shortest);
    }
    // K / 128 = 1, 3, 7, 9: fewer tiles than waves, and 7 and 9 dealt over 8
    CHECK(kivi_w8_plan_wave_tile0(128, 7) == 0 && kivi_w8_plan_wave_tile0(128, 8) == 1, "one tile goes to the last wave");
    CHECK(kivi_w8_plan_wave_tile0(384, 3) == 1 && kivi_w8_plan_wave_tile0(384, 6) == 2, "three tiles");
    CHECK(kivi_w8_plan_wave_tile0(896, 1) == 0 && kivi_w8_plan_wave_tile0(896, 2) == 1, "seven tiles");
    CHECK(kivi_w8_plan_wave_tile0(1152, 7) == 7 && kivi_w8_plan_wave_tile0(1152, 8) == 9, "nine tiles: the last wave takes two");
}

static void sizes() {
    const int64_t tokens[] = {1, 16, 17, 32, 33, 64, 65, 4096};
    const int tiles[] = {1, 1, 2, 2, 4, 4, 4, 4}, tiles_gu[] = {1, 1, 2, 2, 2, 2, 2, 2};
    const int64_t chunks[] = {1, 1, 1, 1, 1, 1, 2, 64}, chunks_gu[] = {1, 1, 1, 1, 2, 2, 3, 128};
    for (int i = 0; i < 8; i++) {
        CHECK(kivi_w8_plan_token_tiles(tokens[i], false) == tiles[i] && kivi_w8_plan_token_tiles(tokens[i], true) == tiles_gu[i],
              "token tiles of N=%lld", (long long)tokens[i]);
        CHECK(kivi_w8_plan_chunks(tokens[i], false) == chunks[i] && kivi_w8_plan_chunks(tokens[i], true) == chunks_gu[i],
              "passes of N=%lld", (long long)tokens[i]);
        CHECK(16 * kivi_w8_plan_token_tiles(tokens[i], false) <= KIVI_W8_TOKEN_CHUNK, "a pass beyond the chunk");
    }
    CHECK(kivi_w8_plan_stripes(4096) == 256 && kivi_w8_plan_tiles(11008) == 86 && kivi_w8_plan_stripes(22016) == 1376, "llama-2-7b grids");
    CHECK(kivi_w8_plan_elem_blocks(16, 128) == 1 && kivi_w8_plan_elem_blocks(48, 384) == 9 && kivi_w8_plan_elem_blocks(4096, 11008) == 22016,
          "element grids");
    CHECK(kivi_w8_plan_bytes(4096, 4096) == 4096 * 4096 + 4 * 32 * 32, "bytes of a 4096 x 4096 weight");
    CHECK(kivi_w8_plan_bytes(144, 384) == 144 * 384 + 4 * 2 * 3, "bytes with a partial block-row");
}

static void refusals() {
    CHECK(kivi_w8_plan_dtype_ok(16) && kivi_w8_plan_dtype_ok(0x110) && !kivi_w8_plan_dtype_ok(32) && !kivi_w8_plan_dtype_ok(0), "dtypes");
    CHECK(kivi_w8_plan_shape_ok(16, 128) && kivi_w8_plan_shape_ok(4096, 11008) && kivi_w8_plan_shape_ok(144, 384), "the range");
    CHECK(!kivi_w8_plan_shape_ok(0, 128) && !kivi_w8_plan_shape_ok(24, 128) && !kivi_w8_plan_shape_ok(-16, 128), "O");
    CHECK(!kivi_w8_plan_shape_ok(16, 0) && !kivi_w8_plan_shape_ok(16, 64) && !kivi_w8_plan_shape_ok(16, 192) &&
          !kivi_w8_plan_shape_ok(16, -128), "K");
    CHECK(!kivi_w8_plan_shape_ok((int64_t)1 << 30, (int64_t)1 << 20) && kivi_w8_plan_shape_ok((int64_t)1 << 20, (int64_t)1 << 19),
          "O * K < 2^40");
    CHECK(kivi_w8_plan_scales(24, 128) == -1 && kivi_w8_plan_bytes(16, 192) == -1, "sizes of a refused shape");
    const int64_t top = ((int64_t)1 << 31) - 1;
    CHECK(kivi_w8_plan_tokens_ok(1, 16) && !kivi_w8_plan_tokens_ok(0, 16) && !kivi_w8_plan_tokens_ok(-1, 16), "N >= 1");
    CHECK(kivi_w8_plan_tokens_ok(top / 16, 16) && !kivi_w8_plan_tokens_ok(top / 16 + 1, 16), "N * O < 2^31");
    CHECK(kivi_w8_plan_tokens_ok(524287, 4096) && !kivi_w8_plan_tokens_ok(524288, 4096), "N * O < 2^31 at O = 4096");
}

int main() {
    operands();
    stretches();
    sizes();
    refusals();
    if (failures) return 1;
    std::printf("w8 plan ok\n");
    return 0;
}
