// Host-side arithmetic of the per-request LoRA side path (kivi_lora_shrink / kivi_lora_expand, include/kivi_hip.h; DESIGN.md
// section 34): the shape checks, the grids, the bytes of t, the unit-to-lane walk of a shrink wave and every element offset the two
// kernels form.  Plain C++: included by kivi_lora.hip, which indexes with these functions and nothing else, and by the stand-alone
// program tests/lora_plan_main.cpp, which walks every block, wave and lane over buffers of exactly the stated sizes.
//
// Tables: A (S, R, K), B (S, O, R) contiguous in the dtype; x (N, K) by x_stride, y (N, O) by y_stride; t (N, R) fp32.  Token n
// belongs to row n / Q.  A unit is 8 consecutive elements (16 bytes).  All offsets are int64 element counts.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KIVI_LORA_HD __host__ __device__ __forceinline__
#else
#define KIVI_LORA_HD static inline
#endif

#define KIVI_LORA_F16 16          // dtype codes: the `logits_bits` values of the fused logits entries
#define KIVI_LORA_BF16 0x110
#define KIVI_LORA_UNIT 8          // elements per 16-byte unit
#define KIVI_LORA_WAVE 64
#define KIVI_LORA_SHRINK_WAVES 4  // ranks per shrink block, one wave each
#define KIVI_LORA_EXPAND_THREADS 256
#define KIVI_LORA_EXPAND_OUTS 2   // adjacent outputs per expand thread: one 32-bit word of y
#define KIVI_LORA_MAX_GRID_Y 65535

KIVI_LORA_HD bool kivi_lora_plan_dtype_ok(int dtype) { return dtype == KIVI_LORA_F16 || dtype == KIVI_LORA_BF16; }
KIVI_LORA_HD bool kivi_lora_plan_rank_ok(int R) { return R == 8 || R == 16 || R == 32 || R == 64; }
// K and O: positive multiples of 8
KIVI_LORA_HD bool kivi_lora_plan_dim_ok(int64_t d) { return d >= KIVI_LORA_UNIT && d % KIVI_LORA_UNIT == 0 && d < ((int64_t)1 << 31); }
// N = B * Q tokens: N >= 1, Q >= 1, whole rows, N a grid's first dimension
KIVI_LORA_HD bool kivi_lora_plan_tokens_ok(int64_t N, int64_t Q) { return N >= 1 && Q >= 1 && N % Q == 0 && N < ((int64_t)1 << 31); }
KIVI_LORA_HD bool kivi_lora_plan_slots_ok(int64_t S) { return S >= 1 && S < ((int64_t)1 << 31); }

KIVI_LORA_HD int64_t kivi_lora_plan_t_bytes(int64_t N, int R) {
    return kivi_lora_plan_rank_ok(R) && N >= 1 && N < ((int64_t)1 << 31) ? N * R * 4 : -1;
}

// the ranks a slot's launches walk: ranks[s] rounded up to 8, at most R; nothing for a rank below 1
KIVI_LORA_HD int kivi_lora_plan_active_ranks(int rank, int R) {
    if (rank < 1) return 0;
    const int64_t up = ((int64_t)rank + 7) / 8 * 8;
    return up < R ? (int)up : R;
}
KIVI_LORA_HD bool kivi_lora_plan_slot_ok(int slot, int S) { return slot >= 0 && slot < S; }

// grids: shrink (N, R / 4), four waves per block; expand (N, ceil(O / 2 / 256)), one thread per two outputs
KIVI_LORA_HD int64_t kivi_lora_plan_shrink_grid_y(int R) { return R / KIVI_LORA_SHRINK_WAVES; }
KIVI_LORA_HD int64_t kivi_lora_plan_expand_grid_y(int64_t O) {
    const int64_t per = (int64_t)KIVI_LORA_EXPAND_THREADS * KIVI_LORA_EXPAND_OUTS;
    return (O + per - 1) / per;
}
KIVI_LORA_HD bool kivi_lora_plan_expand_grid_ok(int64_t O) { return kivi_lora_plan_expand_grid_y(O) <= KIVI_LORA_MAX_GRID_Y; }

// shrink: the rank of wave w of block y; the units of a row; lane l takes units l, l + 64, l + 128, ... below K / 8
KIVI_LORA_HD int kivi_lora_plan_shrink_rank(int block_y, int wave) { return block_y * KIVI_LORA_SHRINK_WAVES + wave; }
KIVI_LORA_HD int64_t kivi_lora_plan_units(int64_t K) { return K / KIVI_LORA_UNIT; }
KIVI_LORA_HD int64_t kivi_lora_plan_lane_unit(int lane, int64_t i) { return lane + i * KIVI_LORA_WAVE; }
KIVI_LORA_HD int64_t kivi_lora_plan_a_unit(int64_t s, int R, int64_t K, int64_t j, int64_t u) { return (s * R + j) * K + u * KIVI_LORA_UNIT; }
KIVI_LORA_HD int64_t kivi_lora_plan_x_unit(int64_t n, int64_t x_stride, int64_t u) { return n * x_stride + u * KIVI_LORA_UNIT; }
KIVI_LORA_HD int64_t kivi_lora_plan_t_at(int64_t n, int R, int64_t j) { return n * R + j; }

// expand: the first output of thread `tid` of block y (the thread returns when it is >= O); 8 ranks of a B row; the word of y
KIVI_LORA_HD int64_t kivi_lora_plan_expand_out(int64_t block_y, int tid) {
    return (block_y * KIVI_LORA_EXPAND_THREADS + tid) * KIVI_LORA_EXPAND_OUTS;
}
KIVI_LORA_HD int64_t kivi_lora_plan_b_unit(int64_t s, int64_t O, int R, int64_t o, int64_t j8) { return (s * O + o) * R + j8 * KIVI_LORA_UNIT; }
KIVI_LORA_HD int64_t kivi_lora_plan_y_at(int64_t n, int64_t y_stride, int64_t o) { return n * y_stride + o; }
