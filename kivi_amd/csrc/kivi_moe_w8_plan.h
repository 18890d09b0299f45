// Host-side arithmetic of the FP8 expert entry (kivi_moe_experts_w8, include/kivi_hip.h): the served shapes and
// EVERY address the kernel forms -- weight bytes, scale words, token rows, activation rows, fp32 pair rows -- in 64 bits.  Plain
// C++: included by kivi_moe.hip and by the stand-alone program tests/moe_w8_plan_main.cpp, which walks every (tile, stripe, wave,
// stretch, lane) and holds each address inside its buffer.
//
// The buffers are the checkpoint's own, stacked over the experts: gate_up (E, 2 I, H) and down (E, H, I), one e4m3fn byte per element,
// row-major, and their fp32 block scales (E, 2 I / 128, H / 128) and (E, H / 128, I / 128).  H and I are multiples of 128, so a slab
// holds a whole number of block-rows, a 16-row stripe lies inside one block-row, the up rows begin on a block-row of their own,
// and the 128-element stretch of the reduction axis a wave owns is exactly one scale block: one fp32 per (stripe, stretch).
// The plan (tile list, pairs, bound, workspace) is kivi_moe_plan.h's, the operand rule kivi_w8_plan_step_k.
#pragma once
#include <stdint.h>

#include "kivi_moe_plan.h"
#include "kivi_w8_plan.h"

#if defined(__HIPCC__)
#define KIVI_MOE_W8_HD __host__ __device__ __forceinline__
#else
#define KIVI_MOE_W8_HD static inline
#endif

#define KIVI_MOE_W8_WAVES 4       // waves of a block: wave w walks the stretches w, w + 4, w + 8, ... of the reduction axis

// H and I positive multiples of 128 (which is also what kivi_moe_plan_dims_ok asks)
KIVI_MOE_W8_HD bool kivi_moe_w8_plan_dims_ok(int64_t H, int64_t I) {
    return H >= KIVI_W8_BLOCK && I >= KIVI_W8_BLOCK && H % KIVI_W8_BLOCK == 0 && I % KIVI_W8_BLOCK == 0;
}

// sizes of the four buffers: bytes of the codes, fp32 words of the scales
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_gate_up_bytes(int64_t E, int64_t H, int64_t I) { return E * 2 * I * H; }
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_down_bytes(int64_t E, int64_t H, int64_t I) { return E * H * I; }
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_gate_up_scales(int64_t E, int64_t H, int64_t I) {
    return E * (2 * I / KIVI_W8_BLOCK) * (H / KIVI_W8_BLOCK);
}
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_down_scales(int64_t E, int64_t H, int64_t I) {
    return E * (H / KIVI_W8_BLOCK) * (I / KIVI_W8_BLOCK);
}

// stretches of 128 reduction elements of a row of C columns; wave w walks w, w + WAVES, ...
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_stretches(int64_t C) { return C / KIVI_W8_K_TILE; }

// A matrix stack (E, rows, C): `rows` = 2 I for gate_up (gate rows [0, I), up rows [I, 2 I)), H for down.
// -> the byte at which lane (r, kb) starts its 16-byte load of half h in {0, 1} of stretch `st` of row `row` of expert e
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_weight_byte(int64_t e, int64_t rows, int64_t row, int64_t C, int64_t st, int h, int kb) {
    return (e * rows + row) * C + st * KIVI_W8_K_TILE + 64 * h + 16 * kb;
}
// -> the fp32 word of the scale of stretch `st` of the 16-row stripe that begins at row `row0` of expert e
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_scale_word(int64_t e, int64_t rows, int64_t row0, int64_t C, int64_t st) {
    return (e * (rows / KIVI_W8_BLOCK) + row0 / KIVI_W8_BLOCK) * (C / KIVI_W8_BLOCK) + st;
}
// the operand rule of kivi_w8_plan_step_k, restated for the device (the test program holds the two equal): the first reduction
// element lane kb feeds MFMA step `step` of stretch `st`
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_step_k(int64_t st, int step, int kb) {
    return st * KIVI_W8_K_TILE + 64 * (step >> 1) + 16 * kb + 8 * (step & 1);
}
// -> the first of the 8 elements lane kb feeds MFMA step `step` of stretch `st`, in the row of a token (x, `stride` = x_stride,
// `row` = pair / K) or of a pair's activations (`stride` = I, `row` = the pair's position in `pairs`)
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_src_elem(int64_t row, int64_t stride, int64_t st, int step, int kb) {
    return row * stride + kivi_moe_w8_plan_step_k(st, step, kb);
}
// -> the first of the 4 elements lane (token column, kb) writes: row `pos` (position in `pairs`) of the activations (R = I, the
// dtype) or of the pair outputs (R = H, fp32), weight rows r0 + 4 kb .. + 3
KIVI_MOE_W8_HD int64_t kivi_moe_w8_plan_dst_elem(int64_t pos, int64_t R, int64_t r0, int kb) { return pos * R + r0 + 4 * kb; }
// the fp32 pair outputs begin this many bytes into the workspace (kivi_moe_plan_workspace_bytes: activations, then outputs)
static inline int64_t kivi_moe_w8_plan_y_offset(int64_t nk, int64_t I) { return kivi_moe_plan_act_bytes(nk, I); }
