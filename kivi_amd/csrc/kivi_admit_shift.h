// The thread map of kivi_mf_store_admit (kivi_admit_shift.hip): rows of a SOURCE packed store of the
// matrix-pipe layout into chosen rows of a DESTINATION store, `shift` 32-token blocks further from token 0, the blocks under the
// shift zeroed.  A block is the 16-byte UNITS of kivi_shift.h (codes, scale pieces, zero-point pieces); each side has its own row /
// head / super-block strides.  The two stores are different allocations and the destination rows are distinct, so -- unlike the
// in-place shift -- nothing needs ordering: a THREAD owns ONE unit of ONE destination block of one (source row, head),
//   t = ((i * nh_kv + h) * (n_blocks + shift) + jd) * units + u          (the unit runs fastest: consecutive lanes, consecutive units)
// and the grid grows with the length, so one admitted row of a long cache still fills the machine.  Thread t
//   jd >= shift   loads unit u of source block jd - shift and stores it as unit u of destination block jd,
//   jd <  shift   stores zeros (no load),
//   jd == 0, u == 0   also replaces the destination's range word of (row, head) by the source's.
// Every destination byte of blocks [0, n_blocks + shift) of an admitted (row, head) is written by exactly one thread, nothing else
// is written.  Nothing in this file needs HIP: a plain C++ program can include it and walk the grid (tests/admit_walk_main.cpp).
#pragma once
#include "kivi_shift.h"

constexpr int kAdmitThreads = 256;

struct KiviAdmitGeom {
    int64_t s_sb, s_sh, s_ss;            // source: row, head, super-block strides (bytes)
    int64_t d_sb, d_sh, d_ss;            // destination
    uint32_t nh_kv, n_blocks, shift;     // n_blocks: blocks of the source; n_blocks + shift < 2^31
    uint32_t threads;                    // n_rows * nh_kv * (n_blocks + shift) * units of a block, < 2^31
};

struct KiviAdmitMove {
    uint32_t i, h;                       // source row, kv head
    int64_t src;                         // byte offset of the unit from the source store's base (copy only)
    int64_t dst;                         // byte offset of the unit inside the DESTINATION ROW (the caller adds rows[i] * d_sb)
    bool copy;                           // false: the unit lies under the shift and is zeroed
    bool range;                          // this thread also moves the range word of (i, h)
};

// threads of the grid, as int64 (the entry point refuses 2^31 and above)
KIVI_SHIFT_HD int64_t kivi_admit_threads(int bits, int64_t n_rows, int64_t nh_kv, int64_t n_blocks, int64_t shift) {
    return n_rows * nh_kv * (n_blocks + shift) * (int64_t)kivi_shift_block_units(bits);
}

// thread t < g.threads -> what it moves (32-bit arithmetic: the grid is below 2^31 threads)
KIVI_SHIFT_HD KiviAdmitMove kivi_admit_move(int bits, bool is_k, const KiviAdmitGeom& g, uint32_t t) {
    const uint32_t n = kivi_shift_block_units(bits), total = g.n_blocks + g.shift;
    const uint32_t q = t / n, u = t - q * n;                 // q = (i * nh_kv + h) * total + jd
    const uint32_t rh = q / total, jd = q - rh * total;
    KiviAdmitMove m;
    m.i = rh / g.nh_kv;
    m.h = rh - m.i * g.nh_kv;
    m.copy = jd >= g.shift;
    m.range = jd == 0 && u == 0;
    m.src = m.copy ? (int64_t)m.i * g.s_sb + (int64_t)m.h * g.s_sh + kivi_shift_offset(bits, is_k, g.s_ss, (int64_t)jd - g.shift, u) : 0;
    m.dst = (int64_t)m.h * g.d_sh + kivi_shift_offset(bits, is_k, g.d_ss, jd, u);
    return m;
}
