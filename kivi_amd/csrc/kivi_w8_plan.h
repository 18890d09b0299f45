// Host-side arithmetic of the FP8 weight entries (kivi_w8_dequant / kivi_w8_linear / kivi_w8_gate_up, include/kivi_hip.h;
// DESIGN.md section 35): the supported range, buffer sizes, grids, token chunks, the stretch of the reduction axis each wave of a
// block walks and the scale of an element.  Plain C++: included by kivi_w8.hip and by the stand-alone program tests/w8_plan_main.cpp.
//
// A weight (O, K) stays ROW-MAJOR, one e4m3fn byte per element -- the checkpoint's own bytes -- with one fp32 scale per block of
// 128 x 128 elements, (ceil(O / 128), K / 128) row-major.  A block of the linear owns a stripe of 16 rows and walks it in tiles of
// 128 reduction elements; 16 divides 128, so a tile lies inside ONE scale block: scale (stripe >> 3, tile).  Its 8 waves take
// CONTIGUOUS runs of tiles: wave w walks [T w / 8, T (w + 1) / 8) with T = K / 128 (integer division), so which elements a wave
// adds is a function of K alone.  Tokens go through in chunks of up to 64 (four 16-column accumulator tiles).
#pragma once
#include <stdint.h>

#define KIVI_W8_ROW_TILE 16       // output rows per stripe: the row count of v_mfma_f32_16x16x32
#define KIVI_W8_K_TILE 128        // reduction elements per tile
#define KIVI_W8_BLOCK 128         // the scale block is KIVI_W8_BLOCK x KIVI_W8_BLOCK
#define KIVI_W8_WAVES 8           // waves per block
#define KIVI_W8_TOKEN_CHUNK 64    // most tokens per pass over the stripe (gate_up: 32)
#define KIVI_W8_F16 16            // dtype codes: the `logits_bits` values of the fused logits entries
#define KIVI_W8_BF16 0x110

static inline bool kivi_w8_plan_dtype_ok(int dtype) { return dtype == KIVI_W8_F16 || dtype == KIVI_W8_BF16; }
// O a positive multiple of 16, K a positive multiple of 128, O * K < 2^40 (every index below fits 63 bits)
static inline bool kivi_w8_plan_shape_ok(int64_t O, int64_t K) {
    return O >= KIVI_W8_ROW_TILE && O % KIVI_W8_ROW_TILE == 0 && K >= KIVI_W8_K_TILE && K % KIVI_W8_K_TILE == 0 &&
           O < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && O <= (((int64_t)1 << 40) - 1) / K;
}
// N >= 1 with N * O < 2^31
static inline bool kivi_w8_plan_tokens_ok(int64_t N, int64_t O) { return N >= 1 && O >= 1 && N <= (((int64_t)1 << 31) - 1) / O; }

// the scale grid: ceil(O / 128) block-rows (the last may be partial) of K / 128 blocks
static inline int64_t kivi_w8_plan_scale_rows(int64_t O) { return (O + KIVI_W8_BLOCK - 1) / KIVI_W8_BLOCK; }
static inline int64_t kivi_w8_plan_scale_cols(int64_t K) { return K / KIVI_W8_BLOCK; }
static inline int64_t kivi_w8_plan_scales(int64_t O, int64_t K) {
    return kivi_w8_plan_shape_ok(O, K) ? kivi_w8_plan_scale_rows(O) * kivi_w8_plan_scale_cols(K) : -1;
}
// the fp32 scale of element (o, k)
static inline int64_t kivi_w8_plan_scale_index(int64_t o, int64_t k, int64_t K) {
    return (o / KIVI_W8_BLOCK) * kivi_w8_plan_scale_cols(K) + k / KIVI_W8_BLOCK;
}
// bytes of the two buffers together (-1: unsupported shape): O * K codes and 4 per scale
static inline int64_t kivi_w8_plan_bytes(int64_t O, int64_t K) {
    return kivi_w8_plan_shape_ok(O, K) ? O * K + 4 * kivi_w8_plan_scales(O, K) : -1;
}

// grids: linear / gate_up one block per stripe; dequant one thread per 8 consecutive elements of a row
static inline int64_t kivi_w8_plan_stripes(int64_t O) { return O / KIVI_W8_ROW_TILE; }
static inline int64_t kivi_w8_plan_tiles(int64_t K) { return K / KIVI_W8_K_TILE; }
static inline int64_t kivi_w8_plan_elem_blocks(int64_t O, int64_t K) { return (O * (K / 8) + 255) / 256; }
// the scale block-row of a stripe: every tile of the stripe reads scale (this, tile)
static inline int64_t kivi_w8_plan_stripe_scale_row(int64_t stripe) { return stripe / (KIVI_W8_BLOCK / KIVI_W8_ROW_TILE); }

// the accumulator tiles (16 token columns each) a block carries per pass over its stripe -- 1, 2 or 4; gate_up, which carries them
// for two matrices, at most 2 -- and the passes of a call
static inline int kivi_w8_plan_token_tiles(int64_t N, bool gate_up) { return N <= 16 ? 1 : (N <= 32 || gate_up) ? 2 : 4; }
static inline int64_t kivi_w8_plan_chunks(int64_t N, bool gate_up) {
    const int64_t per = 16 * kivi_w8_plan_token_tiles(N, gate_up);
    return (N + per - 1) / per;
}

// first tile of wave w (w = KIVI_W8_WAVES: one past the last tile): waves whose run is empty add nothing
static inline int64_t kivi_w8_plan_wave_tile0(int64_t K, int w) { return kivi_w8_plan_tiles(K) * w / KIVI_W8_WAVES; }

// Operand forming on the row-major weight.  Lane (r = lane & 15, kb = lane >> 4) loads, for half h in {0, 1} of a tile, the 16
// bytes of row r at k = 128 tile + 64 h + 16 kb; their low 8 feed MFMA step 2 h against x[k .. k + 8), their high 8 step 2 h + 1
// against x[k + 8 .. k + 16).  -> the first reduction element of (tile, step, kb): the sum over a step's 32 elements is in no
// particular order of k, and both operands are read by this one rule.
static inline int64_t kivi_w8_plan_step_k(int64_t tile, int step, int kb) {
    return tile * KIVI_W8_K_TILE + 64 * (step >> 1) + 16 * kb + 8 * (step & 1);
}
