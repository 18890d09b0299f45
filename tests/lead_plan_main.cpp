// Host walk of the decode row kernels' plan under a lead (kivi_amd/csrc/kivi_lead_plan.h), built with
// -fsanitize=address,undefined by tests/test_decode_lead_cpu.py.  For every store length, lead and wave count it checks that
//   * the super-blocks of packed K / blocks of packed V the waves visit are exactly those that hold a key at or past the clamped
//     lead (the unit straddling the lead is walked whole; nothing wholly under the lead is visited);
//   * every visited unit is visited by exactly one wave, and every 32-token group of a visited super-block exactly once, none past Tq;
//   * the V ranges of the waves are contiguous, in order, and differ by at most one block;
//   * the score slots filled for skipped super-blocks end where the first visited one starts and never reach past the packed keys.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../kivi_amd/csrc/kivi_lead_plan.h"

#define CHECK(c)                                                                                                        \
    do {                                                                                                                \
        if (!(c)) {                                                                                                     \
            fprintf(stderr, "%s:%d: %s  (T=%d lead=%d waves=%d)\n", __FILE__, __LINE__, #c, g_T, g_lead, g_nw);         \
            exit(1);                                                                                                    \
        }                                                                                                               \
    } while (0)

static int g_T, g_lead, g_nw;

static void walk_k(int Tq, int lead, int nw) {
    g_T = Tq; g_lead = lead; g_nw = nw;
    const int nsb = (Tq + kLeadSbTokens - 1) / kLeadSbTokens, ngroups = Tq / 32;
    const int p = kivi_lead_clamp(lead, Tq);
    CHECK(p >= 0 && p <= Tq && (lead < 0 || lead > Tq || p == lead));
    const int first = kivi_lead_k_first(lead, Tq);
    CHECK(first >= 0 && first <= nsb);
    std::vector<int> sb_seen(nsb, 0), g_seen(ngroups, 0);
    for (int w = 0; w < nw; w++) {
        const KiviLeadKWalk k = kivi_lead_k_wave(first, nsb, Tq, w, nw);
        CHECK(k.n_sb >= 0 && k.sb_stride == nw && k.ng_total >= 0 && k.ng_total <= 16 * k.n_sb);
        CHECK((k.n_sb == 0) == (k.ng_total == 0));
        for (int i = 0; i < k.n_sb; i++) {
            const int sb = k.sb_first + i * k.sb_stride;
            CHECK(sb >= first && sb < nsb);
            sb_seen[sb]++;
            const int ng = k.ng_total - 16 * i < 16 ? k.ng_total - 16 * i : 16;      // as MfKSeq is walked: only the last may be partial
            CHECK(ng >= 1);
            for (int g = 0; g < ng; g++) {
                CHECK(sb * 16 + g < ngroups);
                g_seen[sb * 16 + g]++;
            }
        }
    }
    for (int sb = 0; sb < nsb; sb++) {
        const int end = (sb + 1) * kLeadSbTokens < Tq ? (sb + 1) * kLeadSbTokens : Tq;   // keys [sb * 512, end)
        const bool holds_live = end > p;                                                // a key at or past the clamped lead
        CHECK(sb_seen[sb] == (holds_live ? 1 : 0));
        if ((sb + 1) * kLeadSbTokens <= p) CHECK(sb_seen[sb] == 0);                      // a whole super-block under the lead
    }
    for (int g = 0; g < ngroups; g++) CHECK(g_seen[g] == sb_seen[g / 16]);
    const int fill = kivi_lead_k_fill(first, Tq);
    CHECK(fill >= 0 && fill <= Tq && fill % 32 == 0 && fill <= p);
    for (int sb = 0; sb < nsb; sb++) CHECK((sb * kLeadSbTokens < fill) == (sb_seen[sb] == 0));
}

static void walk_v(int Tv, int lead, int nw) {
    g_T = Tv; g_lead = lead; g_nw = nw;
    const int nb = (Tv + kLeadBlockTokens - 1) / kLeadBlockTokens;
    const int p = kivi_lead_clamp(lead, Tv);
    const int first = kivi_lead_v_first(lead, Tv);
    CHECK(first >= 0 && first <= nb);
    std::vector<int> seen(nb, 0);
    int prev_hi = first, lo_len = INT_MAX, hi_len = 0;
    for (int w = 0; w < nw; w++) {
        const KiviLeadVRange r = kivi_lead_v_wave(first, nb, w, nw);
        CHECK(r.b_lo == prev_hi && r.b_hi >= r.b_lo && r.b_hi <= nb);                   // contiguous, in wave order
        prev_hi = r.b_hi;
        const int len = r.b_hi - r.b_lo;
        lo_len = len < lo_len ? len : lo_len;
        hi_len = len > hi_len ? len : hi_len;
        for (int b = r.b_lo; b < r.b_hi; b++) seen[b]++;
    }
    CHECK(prev_hi == nb);
    CHECK(hi_len - lo_len <= 1);                                                        // no wave idles over the skipped range
    for (int b = 0; b < nb; b++) {
        const int end = (b + 1) * kLeadBlockTokens < Tv ? (b + 1) * kLeadBlockTokens : Tv;
        CHECK(seen[b] == (end > p ? 1 : 0));
        if ((b + 1) * kLeadBlockTokens <= p) CHECK(seen[b] == 0);
        // whole super-blocks under the lead: none of their blocks is streamed
        if ((b / 16 + 1) * kLeadSbTokens <= p) CHECK(seen[b] == 0);
    }
}

int main() {
    // K stores hold whole 32-token groups; V stores end anywhere.  4352 / 4480 / 5184 and 4350 / 4478 / 5182: the long rows of
    // tests/test_decode_lead_long_gpu.py (9 and 11 super-blocks, the last one partial)
    const int k_lengths[] = {0, 32, 480, 512, 544, 1088, 4096, 8192 + 128, 4352, 4480, 5184};
    const int v_lengths[] = {0, 32, 480, 512, 544, 1088, 4096, 8192 + 128, 4350, 4478, 5182};
    long cases = 0;
    for (int Tq : k_lengths)
        for (int Tv : v_lengths) {
            const int n = (Tq > Tv ? Tq : Tv) + 33;                                     // a row: the packed keys, a residual, the new token
            const int nsb = (Tq + kLeadSbTokens - 1) / kLeadSbTokens;
            const int leads[] = {-7, INT_MIN, 0, 1, 511, 512, 513, 1023, 1024, Tq - 1, Tq, Tq + 1, Tv - 1, Tv, Tv + 1, n - 1, INT_MAX,
                                 // the pads of longpad_masks.leadwalk_mask for 4 and 8 waves
                                 33, 2047, 2048, 2049, 4095, 4096, 4097, 512 * (nsb - 4) - 96, 512 * (nsb - 4), 512 * (nsb - 8) - 96,
                                 512 * (nsb - 8), 512 * (nsb - 1)};
            for (int lead : leads)
                for (int nw : {4, 8}) {
                    walk_k(Tq, lead, nw);
                    walk_v(Tv, lead, nw);
                    // packed values end inside a block (Tv = kv length - window length is any number)
                    for (int d : {1, 13, 31})
                        if (Tv - d >= 0) walk_v(Tv - d, lead, nw);
                    cases++;
                }
        }
    if (cases != 11 * 11 * 29 * 2) return 1;
    printf("lead plan ok\n");
    return 0;
}
