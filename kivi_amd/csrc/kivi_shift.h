// Where the 16-byte units of a 32-token block live inside a (batch row, kv head)'s packed store (kivi_mfma_layout.h), for the
// in-place block shift of kivi_shift.hip.  A block is its code words plus its scale and zero-point pieces;
// every piece is a 16-byte-aligned run, so a block is a fixed number of 16-byte UNITS:
//   unit u < C                   codes: byte u * 16 of the block's C * 16 code bytes (C = 64 at 2 bits, 128 at 4 bits)
//   unit C + p,      p < 16      scale region (region 0), piece p
//   unit C + 16 + p, p < 16      zero-point region (region 1), piece p
//     K: piece p = (c, kb) holds the 8 channels 32 c + 8 kb .. + 7 of the block's group: halves
//        (g >> 3) * 1024 + p * 64 + (g & 7) * 8 of the region (kt_sm_half), g = the block's index inside its super-block
//     V: piece p holds tokens 2 p, 2 p + 1 (4 channel groups each): bytes g * 256 + p * 16 of the region (vt_half)
// Block j of the store lies in super-block j / 16, `ss` bytes apart.  Nothing in this file needs HIP: a plain C++ program can
// include it and walk all of it (tests/test_rebase_cpu.py).
#pragma once
#include <stdint.h>

#include "kivi_mfma_layout.h"

#ifdef __HIPCC__
#define KIVI_SHIFT_HD __host__ __device__ __forceinline__
#else
#define KIVI_SHIFT_HD inline
#endif

// the shift kernel's geometry: a thread owns one unit column of one (row, head) and moves it in batches of kShiftInFlight blocks
constexpr int kShiftThreads = 256;
constexpr int kShiftInFlight = 8;
constexpr int kShiftRegionUnits = 16;                   // scale (or zero-point) units of a block
constexpr int kShiftRegionBytes = 4096;                 // 16 blocks x 128 halves

KIVI_SHIFT_HD uint32_t kivi_shift_code_units(int bits) { return (bits == 2 ? KIVI_MF_BLOCK_WORDS : KIVI_MF4_BLOCK_WORDS) / 4; }
KIVI_SHIFT_HD uint32_t kivi_shift_block_units(int bits) { return kivi_shift_code_units(bits) + 2 * kShiftRegionUnits; }
KIVI_SHIFT_HD int64_t kivi_shift_sb_bytes(int bits) { return (bits == 2 ? KIVI_MF_SB_WORDS : KIVI_MF4_SB_WORDS) * 4; }
// true for the units that hold scales (region 0): what the range words are recomputed from
KIVI_SHIFT_HD bool kivi_shift_is_scale(int bits, uint32_t u) {
    const uint32_t c = kivi_shift_code_units(bits);
    return u >= c && u < c + kShiftRegionUnits;
}

// byte offset of unit u (< kivi_shift_block_units(bits)) of block j inside the (row, head)'s store; ss: super-block stride in bytes
KIVI_SHIFT_HD int64_t kivi_shift_offset(int bits, bool is_k, int64_t ss, int64_t j, uint32_t u) {
    const uint32_t c = kivi_shift_code_units(bits);
    const int64_t sb = (j >> 4) * ss;
    const uint32_t g = (uint32_t)(j & 15);
    if (u < c) return sb + (int64_t)g * (c * 16) + (int64_t)u * 16;
    const uint32_t r = (u - c) / kShiftRegionUnits, p = (u - c) % kShiftRegionUnits;
    const int64_t region = (int64_t)(bits == 2 ? KIVI_MF_SB_SCALE_WORD0 : KIVI_MF4_SB_SCALE_WORD0) * 4 + (int64_t)r * kShiftRegionBytes;
    const uint32_t in_region = is_k ? ((g >> 3) * 1024 + p * 64 + (g & 7) * 8) * 2 : g * 256 + p * 16;
    return sb + region + in_region;
}

// thread t of the grid -> (row * nh_kv + head, unit): the unit index runs fastest, so that consecutive lanes take consecutive units
KIVI_SHIFT_HD void kivi_shift_thread(int bits, int64_t t, int64_t* row_head, uint32_t* u) {
    const uint32_t n = kivi_shift_block_units(bits);
    *row_head = t / n;
    *u = (uint32_t)(t - *row_head * n);
}
