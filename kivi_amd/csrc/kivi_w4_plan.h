// Host-side arithmetic of the 4-bit weight entries (kivi_w4_pack / kivi_w4_dequant / kivi_w4_linear / kivi_w4_gate_up,
// include/kivi_hip.h): the supported range, buffer sizes, grids, token chunks and the stretch of the reduction
// axis each wave of a block walks.  Plain C++: included by kivi_w4.hip and by the stand-alone program tests/w4_plan_main.cpp.
//
// A weight (O, K) is cut into tiles of 16 rows x 128 reduction elements (1 KiB of codes = one 16-byte load per lane of a wave); the
// K / 128 tiles of a 16-row stripe are contiguous.  A block owns one stripe; its 8 waves take CONTIGUOUS runs of tiles: wave w walks
// tiles [T w / 8, T (w + 1) / 8) with T = K / 128 (integer division), so which elements a wave adds is a function of K alone.  A
// tile holds whole quantisation groups (G divides 128).  Tokens go through in chunks of up to 64 (four 16-column accumulator tiles).
#pragma once
#include <stdint.h>

#define KIVI_W4_ROW_TILE 16       // output rows per stripe: the row count of v_mfma_f32_16x16x32
#define KIVI_W4_K_TILE 128        // reduction elements per tile
#define KIVI_W4_TILE_WORDS 256    // int32 code words per tile
#define KIVI_W4_WAVES 8           // waves per block
#define KIVI_W4_TOKEN_CHUNK 64    // most tokens per pass over the stripe (gate_up: 32)
#define KIVI_W4_F16 16            // dtype codes: the `logits_bits` values of the fused logits entries
#define KIVI_W4_BF16 0x110

static inline bool kivi_w4_plan_dtype_ok(int dtype) { return dtype == KIVI_W4_F16 || dtype == KIVI_W4_BF16; }
static inline bool kivi_w4_plan_group_ok(int G) { return G == 64 || G == 128; }
// O a positive multiple of 16, K a positive multiple of 128, G in {64, 128}, O * K < 2^40 (every index below fits 63 bits)
static inline bool kivi_w4_plan_shape_ok(int64_t O, int64_t K, int G) {
    return kivi_w4_plan_group_ok(G) && O >= KIVI_W4_ROW_TILE && O % KIVI_W4_ROW_TILE == 0 && K >= KIVI_W4_K_TILE &&
           K % KIVI_W4_K_TILE == 0 && O < ((int64_t)1 << 31) && K < ((int64_t)1 << 31) && O <= (((int64_t)1 << 40) - 1) / K;
}
// N >= 1 with N * O < 2^31
static inline bool kivi_w4_plan_tokens_ok(int64_t N, int64_t O) { return N >= 1 && O >= 1 && N <= (((int64_t)1 << 31) - 1) / O; }

// sizes of the three buffers (-1: unsupported shape): O * K / 8 code words; O * K / G halves of scale and as many of mn
static inline int64_t kivi_w4_plan_code_words(int64_t O, int64_t K, int G) { return kivi_w4_plan_shape_ok(O, K, G) ? O * K / 8 : -1; }
static inline int64_t kivi_w4_plan_sm_halves(int64_t O, int64_t K, int G) { return kivi_w4_plan_shape_ok(O, K, G) ? O * (K / G) : -1; }
static inline int64_t kivi_w4_plan_bytes(int64_t O, int64_t K, int G) {
    return kivi_w4_plan_shape_ok(O, K, G) ? O * K / 2 + 4 * O * (K / G) : -1;
}

// grids: linear / gate_up one block per stripe; pack / dequant one thread per 8 consecutive elements of a row
static inline int64_t kivi_w4_plan_stripes(int64_t O) { return O / KIVI_W4_ROW_TILE; }
static inline int64_t kivi_w4_plan_tiles(int64_t K) { return K / KIVI_W4_K_TILE; }
static inline int64_t kivi_w4_plan_elem_blocks(int64_t O, int64_t K) { return (O * (K / 8) + 255) / 256; }

// the accumulator tiles (16 token columns each) a block carries per pass over its stripe -- 1, 2 or 4; gate_up, which carries them
// for two matrices, at most 2 (four would not fit the register file) -- and the passes of a call
static inline int kivi_w4_plan_token_tiles(int64_t N, bool gate_up) { return N <= 16 ? 1 : (N <= 32 || gate_up) ? 2 : 4; }
static inline int64_t kivi_w4_plan_chunks(int64_t N, bool gate_up) {
    const int64_t per = 16 * kivi_w4_plan_token_tiles(N, gate_up);
    return (N + per - 1) / per;
}

// first tile of wave w (w = KIVI_W4_WAVES: one past the last tile): waves whose run is empty add nothing
static inline int64_t kivi_w4_plan_wave_tile0(int64_t K, int w) { return kivi_w4_plan_tiles(K) * w / KIVI_W4_WAVES; }

// word of (row o, reduction element k) in the code buffer and the bit of its 4-bit field ("WT4", kivi_mfma_layout.h)
static inline int64_t kivi_w4_plan_word(int64_t o, int64_t k, int64_t K) {
    const int64_t tile = (o / 16) * kivi_w4_plan_tiles(K) + k / 128;
    const int kk = (int)(k % 128);
    return tile * KIVI_W4_TILE_WORDS + ((o % 16) + 16 * ((kk >> 3) & 3)) * 4 + (kk >> 5);
}
static inline int kivi_w4_plan_bit(int64_t k) { return 4 * (int)((k & 7) >> 1) + 16 * (int)(k & 1); }
// half of (row o, group g) in the scale / mn buffers
static inline int64_t kivi_w4_plan_sm_half(int64_t o, int64_t g, int64_t K, int G) { return ((o / 16) * (K / G) + g) * 16 + o % 16; }
