// Host-side arithmetic of the sparse expert block (kivi_moe_route / kivi_moe_experts, include/kivi_hip.h): the
// bound on the tile list, grid sizes, workspace bytes and the refusals.  Plain C++: included by kivi_moe.hip and by the stand-alone
// program tests/moe_plan_main.cpp, which holds the bound to the true tile count of adversarial count vectors.
//
// The host never learns how many pairs an expert received.  A tile holds at most KIVI_MOE_TOKEN_TILE pairs of ONE expert, so the
// tile count of a step is sum_e ceil(c_e / TILE) with sum_e c_e = N * K.  Every expert with c_e > 0 owns at most one partly filled
// tile, and there are at most min(E, N * K) such experts; full tiles number at most floor(N * K / TILE):
//     tiles <= min(E, N * K) + N * K / TILE
// The expert launches are sized by this bound; blocks past the device-side tile count return.
#pragma once
#include <stdint.h>

#define KIVI_MOE_TOKEN_TILE 16    // pairs per tile: the column count of v_mfma_f32_16x16x32
#define KIVI_MOE_ROW_TILE 16      // weight rows per block: the row count of the same instruction
#define KIVI_MOE_MAX_E 256
#define KIVI_MOE_MAX_K 16
#define KIVI_MOE_TILE_WORDS 3     // int32 per entry of the tile list: expert, first row of `pairs`, rows
#define KIVI_MOE_NORM_TOPK 1      // flags of kivi_moe_route
#define KIVI_MOE_ROUND_WEIGHTS 2
#define KIVI_MOE_F16 16           // dtype codes: the `logits_bits` values of the fused logits entries
#define KIVI_MOE_BF16 0x110

// N * K, or -1 where the shape is outside the supported range (E in [1, 256], K in [1, min(E, 16)], N >= 1, N * K < 2^31)
static inline int64_t kivi_moe_plan_pairs(int64_t N, int E, int K) {
    if (N < 1 || E < 1 || E > KIVI_MOE_MAX_E || K < 1 || K > KIVI_MOE_MAX_K || K > E) return -1;
    if (N > (((int64_t)1 << 31) - 1) / K) return -1;
    return N * K;
}

// the bound above (-1: unsupported shape); always < 2^31
static inline int64_t kivi_moe_plan_max_tiles(int64_t N, int E, int K) {
    const int64_t nk = kivi_moe_plan_pairs(N, E, K);
    if (nk < 0) return -1;
    return (nk < E ? nk : E) + nk / KIVI_MOE_TOKEN_TILE;
}

// the true tile count of a count vector (the test program's side of the bound)
static inline int64_t kivi_moe_plan_tiles_of(const int64_t* counts, int E) {
    int64_t t = 0;
    for (int e = 0; e < E; e++) t += (counts[e] + KIVI_MOE_TOKEN_TILE - 1) / KIVI_MOE_TOKEN_TILE;
    return t;
}

static inline bool kivi_moe_plan_dtype_ok(int dtype) { return dtype == KIVI_MOE_F16 || dtype == KIVI_MOE_BF16; }
static inline bool kivi_moe_plan_dims_ok(int64_t H, int64_t I) { return H >= 32 && I >= 32 && H % 32 == 0 && I % 32 == 0; }

// Workspace of kivi_moe_experts: the activations a (N * K, I) in the dtype, then the expert outputs y (N * K, H) in fp32, each
// region starting on 16 bytes.  -1: unsupported shape.
static inline int64_t kivi_moe_plan_act_bytes(int64_t nk, int64_t I) { return (nk * I * 2 + 15) / 16 * 16; }
static inline int64_t kivi_moe_plan_workspace_bytes(int64_t N, int64_t H, int64_t I, int E, int K) {
    const int64_t nk = kivi_moe_plan_pairs(N, E, K);
    if (nk < 0 || !kivi_moe_plan_dims_ok(H, I)) return -1;
    if (I > (((int64_t)1 << 62) / nk) / 2 || H > (((int64_t)1 << 62) / nk) / 4) return -1;
    return kivi_moe_plan_act_bytes(nk, I) + nk * H * 4;
}

// Grids.  Route: one wave per token, four waves per block.  Experts: grid.x walks the tile bound, grid.y the blocks of ROW_TILE
// weight rows (I / 16 for gate / up, H / 16 for down; at most 65535).  Combine: one thread per four output channels.
static inline int64_t kivi_moe_plan_route_blocks(int64_t N) { return (N + 3) / 4; }
static inline int64_t kivi_moe_plan_row_blocks(int64_t rows) { return rows / KIVI_MOE_ROW_TILE; }
static inline int64_t kivi_moe_plan_combine_blocks(int64_t N, int64_t H) { return (N * (H / 4) + 255) / 256; }
static inline bool kivi_moe_plan_grids_ok(int64_t N, int64_t H, int64_t I) {
    return kivi_moe_plan_row_blocks(I) <= 65535 && kivi_moe_plan_row_blocks(H) <= 65535 && kivi_moe_plan_combine_blocks(N, H) < ((int64_t)1 << 31);
}
