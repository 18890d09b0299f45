// Stand-alone program over kivi_amd/csrc/kivi_lora_plan.h, the host-side arithmetic of kivi_lora_shrink / kivi_lora_expand (DESIGN.md
// section 34), built with -fsanitize=address,undefined by tests/test_lora_cpu.py and run as a child process.  It walks every block,
// wave and lane of both launches exactly as kivi_lora.hip does -- the same guards, the same offset functions -- over heap buffers of
// exactly the stated sizes, touching every address a lane forms (the sanitizer watches the reads and writes):
//   1. every address of shrink (A, x, t, slots, ranks) and of expand (B, t, y, scale) lies inside its buffer, x and y as strided views;
//   2. every (j, k) of an active token's A row and every (o, j) of its B rows is visited exactly once, every t[n, j] below the walked
//      ranks and every y[n, o] written exactly once; tokens of a slot outside [0, S) are neither read nor written;
//   3. the grids cover the work, t holds N * R floats;
//   4. the refusals: shapes outside the supported range are not accepted.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../kivi_amd/csrc/kivi_lora_plan.h"

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

template <typename T>
struct Exact {                      // a heap block of exactly n elements: one element past it is the sanitizer's
    T* p;
    explicit Exact(int64_t n) : p(new T[(size_t)n]()) {}
    ~Exact() { delete[] p; }
    Exact(const Exact&) = delete;
};

static void walk(int64_t Bt, int64_t Q, int64_t K, int64_t O, int R, int S, const std::vector<int>& slot_of_row, const std::vector<int>& rank_of) {
    const int64_t N = Bt * Q, x_stride = K + 8, y_stride = O + 2;
    CHECK(kivi_lora_plan_tokens_ok(N, Q) && kivi_lora_plan_dim_ok(K) && kivi_lora_plan_dim_ok(O) && kivi_lora_plan_rank_ok(R) &&
              kivi_lora_plan_slots_ok(S) && kivi_lora_plan_expand_grid_ok(O), "a supported shape is refused: N=%lld K=%lld O=%lld R=%d",
          (long long)N, (long long)K, (long long)O, R);
    CHECK(kivi_lora_plan_t_bytes(N, R) == N * R * 4, "t bytes");
    Exact<uint16_t> A((int64_t)S * R * K), Bm((int64_t)S * O * R), x((N - 1) * x_stride + K), y((N - 1) * y_stride + O);
    Exact<float> t(kivi_lora_plan_t_bytes(N, R) / 4), scale(S);
    Exact<int> slots(Bt), ranks(S);
    for (int64_t b = 0; b < Bt; b++) slots.p[b] = slot_of_row[(size_t)b];
    for (int s = 0; s < S; s++) ranks.p[s] = rank_of[(size_t)s];
    std::vector<int> t_writes((size_t)(N * R), 0), y_writes((size_t)(N * O), 0);
    uint64_t sink = 0;

    // ---- shrink: grid (N, R / 4), 4 waves of 64 lanes
    const int64_t gy = kivi_lora_plan_shrink_grid_y(R);
    CHECK(gy * KIVI_LORA_SHRINK_WAVES == R, "shrink grid does not cover R=%d", R);
    for (int64_t n = 0; n < N; n++) {
        std::vector<int> seen((size_t)(R * K), 0);
        int active = 0;
        for (int64_t by = 0; by < gy; by++) {
            const int s = slots.p[n / Q];
            if (!kivi_lora_plan_slot_ok(s, S)) continue;
            active = kivi_lora_plan_active_ranks(ranks.p[s], R);
            if (kivi_lora_plan_shrink_rank((int)by, 0) >= active) continue;
            for (int w = 0; w < KIVI_LORA_SHRINK_WAVES; w++) {
                const int j = kivi_lora_plan_shrink_rank((int)by, w);
                CHECK(j < active, "a wave past the walked ranks: j=%d active=%d", j, active);
                for (int lane = 0; lane < KIVI_LORA_WAVE; lane++)
                    for (int64_t i = 0; kivi_lora_plan_lane_unit(lane, i) < kivi_lora_plan_units(K); i++) {
                        const int64_t u = kivi_lora_plan_lane_unit(lane, i);
                        const int64_t a = kivi_lora_plan_a_unit(s, R, K, j, u), xo = kivi_lora_plan_x_unit(n, x_stride, u);
                        for (int e = 0; e < KIVI_LORA_UNIT; e++) {
                            sink += A.p[a + e] + x.p[xo + e];
                            CHECK(a + e == ((int64_t)s * R + j) * K + u * 8 + e, "A offset");
                            seen[(size_t)(j * K + u * 8 + e)]++;
                        }
                    }
                t.p[kivi_lora_plan_t_at(n, R, j)] = 1.0f;
                t_writes[(size_t)(n * R + j)]++;
            }
        }
        for (int64_t j = 0; j < R; j++)
            for (int64_t k = 0; k < K; k++)
                CHECK(seen[(size_t)(j * K + k)] == (j < active ? 1 : 0), "shrink n=%lld (j=%lld, k=%lld) visited %d times, active=%d",
                      (long long)n, (long long)j, (long long)k, seen[(size_t)(j * K + k)], active);
    }

    // ---- expand: grid (N, ceil(O / 512)), 256 threads of two outputs
    const int64_t ey = kivi_lora_plan_expand_grid_y(O);
    CHECK(ey * KIVI_LORA_EXPAND_THREADS * KIVI_LORA_EXPAND_OUTS >= O && (ey - 1) * KIVI_LORA_EXPAND_THREADS * KIVI_LORA_EXPAND_OUTS < O, "expand grid");
    for (int64_t n = 0; n < N; n++) {
        std::vector<int> seen((size_t)(O * R), 0);
        int rr = 0;
        for (int64_t by = 0; by < ey; by++) {
            const int s = slots.p[n / Q];
            if (!kivi_lora_plan_slot_ok(s, S)) continue;
            rr = kivi_lora_plan_active_ranks(ranks.p[s], R);
            for (int tid = 0; tid < KIVI_LORA_EXPAND_THREADS; tid++) {
                const int64_t o = kivi_lora_plan_expand_out(by, tid);
                if (rr == 0 || o >= O) continue;
                sink += (uint64_t)scale.p[s];
                for (int j8 = 0; j8 * KIVI_LORA_UNIT < rr; j8++)
                    for (int r = 0; r < KIVI_LORA_EXPAND_OUTS; r++) {
                        const int64_t b = kivi_lora_plan_b_unit(s, O, R, o + r, j8);
                        for (int e = 0; e < KIVI_LORA_UNIT; e++) {
                            sink += Bm.p[b + e] + (uint64_t)t.p[kivi_lora_plan_t_at(n, R, 0) + j8 * KIVI_LORA_UNIT + e];
                            CHECK(t_writes[(size_t)(n * R + j8 * KIVI_LORA_UNIT + e)] == 1, "expand reads a t that shrink did not write");
                            seen[(size_t)((o + r) * R + j8 * KIVI_LORA_UNIT + e)]++;
                        }
                    }
                const int64_t yo = kivi_lora_plan_y_at(n, y_stride, o);
                CHECK(yo % 2 == 0, "the word of y is not on 4 bytes");
                for (int r = 0; r < KIVI_LORA_EXPAND_OUTS; r++) {
                    y.p[yo + r] = (uint16_t)(y.p[yo + r] + 1);
                    y_writes[(size_t)(n * O + o + r)]++;
                }
            }
        }
        for (int64_t o = 0; o < O; o++) {
            for (int64_t j = 0; j < R; j++)
                CHECK(seen[(size_t)(o * R + j)] == (j < rr ? 1 : 0), "expand n=%lld (o=%lld, j=%lld) visited %d times", (long long)n,
                      (long long)o, (long long)j, seen[(size_t)(o * R + j)]);
            CHECK(y_writes[(size_t)(n * O + o)] == (rr > 0 ? 1 : 0), "y[%lld, %lld] written %d times", (long long)n, (long long)o,
                  y_writes[(size_t)(n * O + o)]);
        }
    }
    for (int64_t n = 0; n < N; n++) {
        const int s = slots.p[n / Q];
        const int want = kivi_lora_plan_slot_ok(s, S) ? kivi_lora_plan_active_ranks(ranks.p[s], R) : 0;
        for (int j = 0; j < R; j++) CHECK(t_writes[(size_t)(n * R + j)] == (j < want ? 1 : 0), "t[%lld, %d] written %d times", (long long)n, j, t_writes[(size_t)(n * R + j)]);
    }
    if (sink == 0x5EED) std::printf(" ");
}

static void walks() {
    const int64_t Ks[] = {8, 24, 256, 1032, 4096, 11008}, Os[] = {8, 264, 4096}, rows[][2] = {{1, 1}, {3, 5}, {17, 5}};
    const int Rs[] = {8, 64};
    const int S = 3;
    // shrink never sees O and expand never sees K: every K with the smallest O, every O with the smallest K
    std::vector<std::pair<int64_t, int64_t>> shapes;
    for (int64_t K : Ks) shapes.push_back({K, Os[0]});
    for (int64_t O : Os) shapes.push_back({Ks[0], O});
    for (auto& ko : shapes) {
        const int64_t K = ko.first, O = ko.second;
        for (int R : Rs)
            for (auto& bq : rows) {
                const int64_t Bt = bq[0], Q = bq[1];
                // slots: repeats, the base model (-1), values outside [-1, S) that must leave their rows alone; ranks: 1, 5 and R
                const int pattern[] = {2, -1, 0, 1, 0, S, -7, 2};
                std::vector<int> slots((size_t)Bt), ranks = {1, 5 < R ? 5 : R, R};
                for (int64_t b = 0; b < Bt; b++) slots[(size_t)b] = pattern[(b + (K / 8) % 3) % 8];
                if (Bt == 1) slots[0] = (K == 24 ? -1 : (int)((K / 8 + O / 8 + R) % 3));
                walk(Bt, Q, K, O, R, S, slots, ranks);
            }
    }
    // ranks of 0 and beyond R: nothing walked, R walked
    walk(3, 1, 24, 8, 8, 2, {0, 1, 0}, {0, 99});
}

static void refusals() {
    CHECK(!kivi_lora_plan_dtype_ok(32) && !kivi_lora_plan_dtype_ok(0) && kivi_lora_plan_dtype_ok(16) && kivi_lora_plan_dtype_ok(0x110), "dtypes");
    for (int R : {0, 4, 12, 24, 48, 128, -8}) CHECK(!kivi_lora_plan_rank_ok(R), "R=%d accepted", R);
    for (int R : {8, 16, 32, 64}) CHECK(kivi_lora_plan_rank_ok(R), "R=%d refused", R);
    for (int64_t d : {(int64_t)0, (int64_t)-8, (int64_t)4, (int64_t)12, (int64_t)4100, (int64_t)1 << 31}) CHECK(!kivi_lora_plan_dim_ok(d), "dim %lld accepted", (long long)d);
    CHECK(kivi_lora_plan_dim_ok(8) && kivi_lora_plan_dim_ok(11008), "dims refused");
    CHECK(!kivi_lora_plan_tokens_ok(0, 1) && !kivi_lora_plan_tokens_ok(4, 0) && !kivi_lora_plan_tokens_ok(7, 2) &&
              !kivi_lora_plan_tokens_ok((int64_t)1 << 31, 1) && kivi_lora_plan_tokens_ok(15, 5) && kivi_lora_plan_tokens_ok(1, 1), "tokens");
    CHECK(!kivi_lora_plan_slots_ok(0) && !kivi_lora_plan_slots_ok(-1) && kivi_lora_plan_slots_ok(1), "S");
    CHECK(kivi_lora_plan_t_bytes(0, 8) == -1 && kivi_lora_plan_t_bytes(4, 12) == -1 && kivi_lora_plan_t_bytes(85, 64) == 85 * 64 * 4, "t bytes");
    CHECK(!kivi_lora_plan_slot_ok(-1, 3) && !kivi_lora_plan_slot_ok(3, 3) && kivi_lora_plan_slot_ok(0, 3) && kivi_lora_plan_slot_ok(2, 3), "slot guard");
    CHECK(kivi_lora_plan_active_ranks(0, 64) == 0 && kivi_lora_plan_active_ranks(-3, 64) == 0 && kivi_lora_plan_active_ranks(1, 64) == 8 &&
              kivi_lora_plan_active_ranks(8, 64) == 8 && kivi_lora_plan_active_ranks(9, 64) == 16 && kivi_lora_plan_active_ranks(64, 64) == 64 &&
              kivi_lora_plan_active_ranks(5, 8) == 8 && kivi_lora_plan_active_ranks(2147483647, 16) == 16, "walked ranks");
    CHECK(kivi_lora_plan_expand_grid_ok(512 * 65535) && !kivi_lora_plan_expand_grid_ok(512 * 65535 + 8), "expand grid limit");
}

int main() {
    walks();
    refusals();
    if (failures) return 1;
    std::printf("lora plan ok\n");
    return 0;
}
