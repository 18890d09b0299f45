// Stand-alone program over kivi_amd/csrc/kivi_moe_w8_plan.h, the host-side arithmetic of the FP8 expert entry (DESIGN.md section
// 36), built with -fsanitize=address,undefined by tests/test_moe_w8_cpu.py and run as a child process.  It walks the two expert
// launches as moe_gemm_w8_kernel walks them -- every (tile, stripe, wave, stretch, lane), the tile list cut from a count vector
// as moe_plan_kernel cuts it -- forming every address with the header's functions, the ones the kernel calls:
//   1. weight bytes: inside the slab of the tile's expert; over a launch every byte of an expert is read exactly once per tile of
//      that expert, no byte of an expert without pairs is read (counted in arrays of exactly the buffers' sizes: the sanitizer
//      watches the writes);
//   2. scale words: inside the grid, and the scale of every byte the lane multiplies by it (kivi_w8_plan_scale_index on the expert's
//      stacked matrix); gate stripes take block-row r0 / 128, up stripes (I + r0) / 128, down stripes r0 / 128;
//   3. token rows and activation rows: inside x / the activations, the four steps of the four waves cover a row once; the operand
//      rule equals kivi_w8_plan_step_k;
//   4. the rows written: every activation and every fp32 pair output once, inside the workspace of kivi_moe_plan_workspace_bytes;
//   5. the published geometries (Mixtral-8x7B, Qwen3-30B-A3B), bounds only; the refusals.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../kivi_amd/csrc/kivi_moe_w8_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) {                          \
                std::printf("FAILED %s: ", #cond);        \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
            failures++;                                   \
        }                                                 \
    } while (0)

struct Tile {
    int e, first, rows;
};

// moe_plan_kernel's cut of the experts' segments
static std::vector<Tile> cut(const std::vector<int64_t>& counts) {
    std::vector<Tile> tiles;
    int64_t off = 0;
    for (size_t e = 0; e < counts.size(); e++) {
        for (int64_t j = 0; j * KIVI_MOE_TOKEN_TILE < counts[e]; j++) {
            const int64_t left = counts[e] - j * KIVI_MOE_TOKEN_TILE;
            tiles.push_back({(int)e, (int)(off + j * KIVI_MOE_TOKEN_TILE), (int)(left < KIVI_MOE_TOKEN_TILE ? left : KIVI_MOE_TOKEN_TILE)});
        }
        off += counts[e];
    }
    return tiles;
}

// One launch: GATEUP walks R = I rows over C = H, else R = H rows over C = I.  `exact`: count every read and write in arrays of the
// buffers' sizes; otherwise bounds only, over the first and the last tile.
static void launch(bool gateup, int64_t N, int64_t H, int64_t I, int E, int K, int64_t x_stride, const std::vector<int64_t>& counts,
                   bool exact) {
    const int64_t nk = N * K, R = gateup ? I : H, C = gateup ? H : I, NM = gateup ? 2 : 1, slab = NM * R;
    const int64_t wbytes = gateup ? kivi_moe_w8_plan_gate_up_bytes(E, H, I) : kivi_moe_w8_plan_down_bytes(E, H, I);
    const int64_t swords = gateup ? kivi_moe_w8_plan_gate_up_scales(E, H, I) : kivi_moe_w8_plan_down_scales(E, H, I);
    const int64_t src_elems = gateup ? (N - 1) * x_stride + H : nk * I, src_stride = gateup ? x_stride : I;
    const int64_t ws = kivi_moe_plan_workspace_bytes(N, H, I, E, K);
    CHECK(ws == kivi_moe_plan_act_bytes(nk, I) + nk * H * 4 && kivi_moe_w8_plan_y_offset(nk, I) % 16 == 0, "workspace");
    CHECK(wbytes == (int64_t)E * slab * C && swords == (int64_t)E * (slab / 128) * (C / 128), "sizes");
    const std::vector<Tile> tiles = cut(counts);
    CHECK((int64_t)tiles.size() == kivi_moe_plan_tiles_of(counts.data(), E) && (int64_t)tiles.size() <= kivi_moe_plan_max_tiles(N, E, K),
          "tiles %zu", tiles.size());
    std::vector<int> tiles_of((size_t)E, 0);
    for (const Tile& t : tiles) tiles_of[(size_t)t.e]++;
    std::vector<uint8_t> read(exact ? (size_t)wbytes : 0, 0), wrote(exact ? (size_t)(nk * R) : 0, 0), row_cover((size_t)C, 0);
    const int64_t stretches = kivi_moe_w8_plan_stretches(C);
    CHECK(stretches * 128 == C, "C=%lld blocks unevenly", (long long)C);
    for (size_t ti = 0; ti < tiles.size(); ti++) {
        if (!exact && ti != 0 && ti + 1 != tiles.size()) continue;
        const Tile& t = tiles[ti];
        CHECK(t.e >= 0 && t.e < E && t.rows >= 1 && t.rows <= KIVI_MOE_TOKEN_TILE && t.first >= 0 && t.first <= nk - t.rows, "tile");
        for (int64_t stripe = 0; stripe < kivi_moe_plan_row_blocks(R); stripe++) {
            const int64_t r0 = stripe * KIVI_MOE_ROW_TILE;
            const bool cover = ti == 0 && stripe == 0;
            if (cover) row_cover.assign((size_t)C, 0);
            for (int wave = 0; wave < KIVI_MOE_W8_WAVES; wave++)
                for (int64_t st = wave; st < stretches; st += KIVI_MOE_W8_WAVES)
                    for (int lane = 0; lane < 64; lane++) {
                        const int r = lane & 15, kb = lane >> 4;
                        for (int m = 0; m < NM; m++) {
                            const int64_t row = m * R + r0 + r;           // row of the expert's stacked matrix
                            const int64_t sw = kivi_moe_w8_plan_scale_word(t.e, slab, m * R + r0, C, st);
                            CHECK(sw >= 0 && sw < swords, "scale word %lld of %lld", (long long)sw, (long long)swords);
                            CHECK(sw == (int64_t)t.e * (slab / 128) * (C / 128) + (m * R + r0) / 128 * (C / 128) + st, "block-row of m=%d", m);
                            for (int h = 0; h < 2; h++) {
                                const int64_t b = kivi_moe_w8_plan_weight_byte(t.e, slab, row, C, st, h, kb);
                                CHECK(b % 16 == 0 && b >= (int64_t)t.e * slab * C && b + 16 <= (int64_t)(t.e + 1) * slab * C,
                                      "byte %lld outside the slab of expert %d", (long long)b, t.e);
                                if (b < 0 || b + 16 > wbytes) continue;
                                const int64_t k = b - ((int64_t)t.e * slab + row) * C;
                                CHECK(k >= 0 && k + 16 <= C && k / 128 == st, "k=%lld", (long long)k);
                                CHECK(sw == (int64_t)t.e * (slab / 128) * (C / 128) + kivi_w8_plan_scale_index(row, k, C), "scale of a byte");
                                // the low 8 bytes are step 2 h, the high 8 step 2 h + 1: against these elements of the source row
                                CHECK(kivi_moe_w8_plan_step_k(st, 2 * h, kb) == k && kivi_moe_w8_plan_step_k(st, 2 * h + 1, kb) == k + 8, "steps");
                                if (exact)
                                    for (int i = 0; i < 16; i++) read[(size_t)(b + i)]++;
                            }
                        }
                        if (r >= t.rows) continue;                        // columns past the tile's rows load nothing
                        const int64_t srow = gateup ? (t.first + r) % N : t.first + r;    // (a stand-in for pairs[first + r] / K: any token)
                        for (int step = 0; step < 4; step++) {
                            CHECK(kivi_moe_w8_plan_step_k(st, step, kb) == kivi_w8_plan_step_k(st, step, kb), "the operand rule");
                            const int64_t s = kivi_moe_w8_plan_src_elem(srow, src_stride, st, step, kb);
                            CHECK(s % 8 == 0 && s >= srow * src_stride && s + 8 <= srow * src_stride + C && s + 8 <= src_elems, "source %lld",
                                  (long long)s);
                            if (cover && r == 0)
                                for (int i = 0; i < 8; i++) row_cover[(size_t)(s - srow * src_stride + i)]++;
                        }
                    }
            if (cover)
                for (int64_t k = 0; k < C; k++) CHECK(row_cover[(size_t)k] == 1, "source element %lld fed %d times", (long long)k, row_cover[(size_t)k]);
            for (int lane = 0; lane < 64; lane++) {                       // the epilogue of wave 0
                const int r = lane & 15, kb = lane >> 4;
                if (r >= t.rows) continue;
                const int64_t at = kivi_moe_w8_plan_dst_elem(t.first + r, R, r0, kb);
                CHECK(at % 4 == 0 && at >= 0 && at + 4 <= nk * R, "row written at %lld", (long long)at);
                const int64_t end = gateup ? (at + 4) * 2 : kivi_moe_w8_plan_y_offset(nk, I) + (at + 4) * 4;
                CHECK(end <= ws && (!gateup || end <= kivi_moe_w8_plan_y_offset(nk, I)), "past the workspace: %lld of %lld", (long long)end,
                      (long long)ws);
                if (exact && at >= 0 && at + 4 <= nk * R)
                    for (int i = 0; i < 4; i++) wrote[(size_t)(at + i)]++;
            }
        }
    }
    if (!exact) return;
    for (int e = 0; e < E; e++)
        for (int64_t i = 0; i < slab * C; i++)
            if (read[(size_t)(e * slab * C + i)] != tiles_of[(size_t)e]) {
                CHECK(false, "byte %lld of expert %d read %d times for %d tiles", (long long)i, e, read[(size_t)(e * slab * C + i)], tiles_of[(size_t)e]);
                break;
            }
    for (int64_t i = 0; i < nk * R; i++)
        if (wrote[(size_t)i] != 1) {
            CHECK(false, "output element %lld written %d times", (long long)i, wrote[(size_t)i]);
            break;
        }
}

// count vectors of N * K pairs over E experts: everything on one expert, spread as evenly as it goes from the LAST expert down,
// and the crafted 0 / 1 / 16 / 17 / 33 / rest
static std::vector<std::vector<int64_t>> vectors(int64_t N, int E, int K) {
    const int64_t nk = N * K;
    std::vector<std::vector<int64_t>> out;
    std::vector<int64_t> one((size_t)E, 0), even((size_t)E, 0), crafted((size_t)E, 0);
    one[(size_t)(E - 1)] = N < nk ? N : nk;                                // an expert holds a token at most once
    int64_t left = nk - one[(size_t)(E - 1)];
    for (int e = 0; left > 0; e++) {
        one[(size_t)e] = left < N ? left : N;
        left -= one[(size_t)e];
    }
    out.push_back(one);
    for (int64_t p = 0; p < nk; p++) even[(size_t)(E - 1 - p % E)]++;
    out.push_back(even);
    const int64_t want[] = {0, 1, 16, 17, 33};
    if (nk >= 67 + 5 && E >= 7) {
        left = nk;
        for (int e = 0; e < 5; e++) crafted[(size_t)e] = want[e], left -= want[e];
        for (int e = 5; left > 0; e = e + 1 < E ? e + 1 : 5) crafted[(size_t)e]++, left--;
        out.push_back(crafted);
    }
    return out;
}

static void shapes() {
    const int64_t Hs[] = {256, 640}, Is[] = {128, 384}, Ns[] = {1, 5, 64};
    const int EK[][2] = {{8, 2}, {128, 8}};
    for (int64_t H : Hs)
        for (int64_t I : Is)
            for (auto& ek : EK)
                for (int64_t N : Ns) {
                    if (ek[0] == 128 && N == 64 && H == 640) continue;      // (the arrays of the largest case: bounds below)
                    for (const auto& counts : vectors(N, ek[0], ek[1])) {
                        launch(true, N, H, I, ek[0], ek[1], H + 8 * (N % 2), counts, true);
                        launch(false, N, H, I, ek[0], ek[1], H, counts, true);
                    }
                }
    // bounds only: the largest test shape and the two published geometries, first and last tile of every count vector
    const int64_t geo[][5] = {{640, 384, 128, 8, 64}, {4096, 14336, 8, 2, 64}, {4096, 14336, 8, 2, 1}, {2048, 768, 128, 8, 256},
                              {2048, 768, 128, 8, 1}};
    for (auto& g : geo)
        for (const auto& counts : vectors(g[4], (int)g[2], (int)g[3])) {
            launch(true, g[4], g[0], g[1], (int)g[2], (int)g[3], g[0], counts, false);
            launch(false, g[4], g[0], g[1], (int)g[2], (int)g[3], g[0], counts, false);
        }
    // the last byte of the last expert, the last scale, at Mixtral-8x7B: 64-bit arithmetic
    CHECK(kivi_moe_w8_plan_weight_byte(7, 2 * 14336, 2 * 14336 - 1, 4096, 31, 1, 3) + 16 == (int64_t)8 * 2 * 14336 * 4096, "last byte");
    CHECK(kivi_moe_w8_plan_gate_up_bytes(256, 16 * 65535 / 128 * 128, 16 * 65535 / 128 * 128) > ((int64_t)1 << 40), "beyond 2^40 in 64 bits");
    CHECK(kivi_moe_w8_plan_scale_word(127, 2 * 768, 768 + 752, 2048, 15) + 1 == kivi_moe_w8_plan_gate_up_scales(128, 2048, 768), "last scale");
    CHECK(kivi_moe_w8_plan_scale_word(0, 2 * 384, 384, 640, 0) == 3 * 5 && kivi_moe_w8_plan_scale_word(0, 2 * 384, 383 / 16 * 16, 640, 0) == 2 * 5,
          "the up rows start on a block-row of their own");
}

static void refusals() {
    CHECK(kivi_moe_w8_plan_dims_ok(128, 128) && kivi_moe_w8_plan_dims_ok(4096, 14336) && kivi_moe_w8_plan_dims_ok(2048, 768) &&
          kivi_moe_w8_plan_dims_ok(640, 384), "the range");
    CHECK(!kivi_moe_w8_plan_dims_ok(256, 96) && !kivi_moe_w8_plan_dims_ok(96, 256) && !kivi_moe_w8_plan_dims_ok(0, 128) &&
          !kivi_moe_w8_plan_dims_ok(128, 0) && !kivi_moe_w8_plan_dims_ok(192, 128) && !kivi_moe_w8_plan_dims_ok(-128, 128) &&
          !kivi_moe_w8_plan_dims_ok(128, 64), "multiples of 128");
    for (int64_t H = 128; H <= 1024; H += 128) CHECK(kivi_moe_plan_dims_ok(H, H) && kivi_moe_w8_plan_dims_ok(H, H), "inside the fp16 range");
}

int main() {
    shapes();
    refusals();
    if (failures) return 1;
    std::printf("moe w8 plan ok\n");
    return 0;
}
