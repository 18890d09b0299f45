// The walk of a decode row under a LEAD: `lead` keys at the front of a batch row are masked (left padding, the
// front of a rebased or admitted row), so their packed K need not be read or multiplied -- their scores are the clamped fp16 minimum,
// their probabilities exact zeros -- and their packed V is multiplied by exact zeros.  The one-launch row kernels (mf_row_kernel,
// unsliced mf_row4_kernel) skip them in whole units:
//   K   512-token super-blocks; a wave takes super-blocks first + wave, first + wave + nw, ... where first = clamp(lead, 0, Tq) / 512
//       is the first super-block that holds a key at or past the lead (the one straddling the lead is walked whole);
//   V   32-token blocks; the live blocks [clamp(lead, 0, Tv) / 32, ceil(Tv / 32)) are dealt to the waves in contiguous runs whose
//       lengths differ by at most one, so no wave idles over a skipped range.
// Nothing in this file needs HIP: a plain C++ program can include it and walk the plan (tests/lead_plan_main.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KIVI_LEAD_HD __host__ __device__ __forceinline__
#else
#define KIVI_LEAD_HD inline
#endif

constexpr int kLeadSbTokens = 512;                        // a super-block of packed K (and of packed V)
constexpr int kLeadBlockTokens = 32;                      // a block of the packed V stream

struct KiviLeadKWalk {
    int sb_first, sb_stride, n_sb;       // this wave's super-blocks: sb_first + i * sb_stride, i < n_sb
    int ng_total;                        // 32-token groups of the sequence, counted from group 0 of sb_first (MfKSeq)
};

struct KiviLeadVRange {
    int b_lo, b_hi;                      // this wave's V blocks [b_lo, b_hi); b_lo == b_hi: none
};

// the device clamps what the caller promises: a negative lead promises nothing, one past the store covers the whole store
KIVI_LEAD_HD int kivi_lead_clamp(int lead, int T) { return lead < 0 ? 0 : (lead > T ? T : lead); }

// first super-block of packed K that holds a key at or past the lead; ceil(Tq / 512), i.e. none, when the lead covers all of them
KIVI_LEAD_HD int kivi_lead_k_first(int lead, int Tq) {
    const int p = kivi_lead_clamp(lead, Tq);
    return p >= Tq ? (Tq + kLeadSbTokens - 1) / kLeadSbTokens : p / kLeadSbTokens;
}

// first block of packed V that holds a key at or past the lead; ceil(Tv / 32), i.e. none, when the lead covers all of them
KIVI_LEAD_HD int kivi_lead_v_first(int lead, int Tv) {
    const int p = kivi_lead_clamp(lead, Tv);
    return p >= Tv ? (Tv + kLeadBlockTokens - 1) / kLeadBlockTokens : p / kLeadBlockTokens;
}

// score slots [0, this) of a row belong to skipped super-blocks: the kernels fill them with -65504 (never past the packed keys)
KIVI_LEAD_HD int kivi_lead_k_fill(int sb_first, int Tq) { return sb_first * kLeadSbTokens < Tq ? sb_first * kLeadSbTokens : Tq; }

// super-blocks [sb_lo, nsb) of a row of Tq packed keys (Tq a multiple of 32, nsb = ceil(Tq / 512)) dealt round-robin to `nw` waves
KIVI_LEAD_HD KiviLeadKWalk kivi_lead_k_wave(int sb_lo, int nsb, int Tq, int wave, int nw) {
    KiviLeadKWalk w;
    w.sb_first = sb_lo + wave;
    w.sb_stride = nw;
    w.n_sb = nsb > sb_lo + wave ? (nsb - sb_lo - wave + nw - 1) / nw : 0;
    const int last = w.sb_first + (w.n_sb - 1) * nw;      // this wave's last super-block: the only one that may be partial
    const int left = (Tq >> 5) - 16 * last;
    w.ng_total = w.n_sb > 0 ? 16 * (w.n_sb - 1) + (left < 16 ? left : 16) : 0;
    return w;
}

// blocks [vb_lo, vb_hi) dealt to `nw` waves in contiguous runs of floor or ceil((vb_hi - vb_lo) / nw) blocks, the longer runs first
KIVI_LEAD_HD KiviLeadVRange kivi_lead_v_wave(int vb_lo, int vb_hi, int wave, int nw) {
    KiviLeadVRange r;
    const int nb = vb_hi > vb_lo ? vb_hi - vb_lo : 0;
    const int base = nb / nw, rem = nb - base * nw;
    r.b_lo = vb_lo + wave * base + (wave < rem ? wave : rem);
    r.b_hi = r.b_lo + base + (wave < rem ? 1 : 0);
    return r;
}
