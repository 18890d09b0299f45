// The tile plan of kivi_prefill_attention (kivi_prefill.hip): causal attention of a prompt over itself with
// `lead` leading pads per batch row.  A pair (query i, key j) of a row is LIVE when lead <= j <= i (which implies i >= lead); every
// other pair is dead.  Queries are cut into tiles of kPrefillQTile rows, keys into tiles of kPrefillKTile keys; a key tile is the
// full rectangle rows x 32 keys, also where it reaches past the diagonal or past T (those pairs have j > i: dead).
//   block order   block x of the grid -> (query tile, head, batch row), the LAST query tile first: its blocks walk the most key
//                 tiles, so they start first and the short ones fill the machine's tail;
//   visited       the key tiles that hold a live pair of the rows [q0, q1): [lead / 32, (q1 - 1) / 32], none when lead >= q1
//                 (every row of the tile is a pad).  A tile wholly under the lead or wholly above the diagonal is never loaded;
//   partial       a visited tile that also holds a dead pair: only there is a score compared against (lead, i).
// The same two functions serve a block (its 128 rows: what is staged) and a wave (its 32 rows: what is computed and masked).
// Nothing in this file needs HIP: a plain C++ program can include it and walk the plan (tests/prefill_plan_main.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KIVI_PREFILL_HD __host__ __device__ __forceinline__
#else
#define KIVI_PREFILL_HD inline
#endif

constexpr int kPrefillThreads = 256;                      // four waves
constexpr int kPrefillWaveRows = 32;                      // query rows of a wave: two 16-column matrix tiles
constexpr int kPrefillQTile = 4 * kPrefillWaveRows;       // query rows of a block
constexpr int kPrefillKTile = 32;                         // keys of a staged tile: one k step of v_mfma_f32_16x16x32_f16

struct KiviPrefillBlock {
    int b, h;                            // batch row, query head
    int q0, q1;                          // query rows [q0, q1), q1 <= T
};

struct KiviPrefillTiles {
    int kt0, kt1;                        // key tiles [kt0, kt1); kt0 == kt1: nothing is visited
};

KIVI_PREFILL_HD int kivi_prefill_qtiles(int T) { return (T + kPrefillQTile - 1) / kPrefillQTile; }

// blocks of the grid, as int64 (the entry point refuses 2^31 and above)
KIVI_PREFILL_HD int64_t kivi_prefill_blocks(int64_t B, int64_t nh, int64_t T) {
    return B * nh * ((T + kPrefillQTile - 1) / kPrefillQTile);
}

KIVI_PREFILL_HD int kivi_prefill_clamp_lead(int lead, int T) { return lead < 0 ? 0 : (lead > T ? T : lead); }

// block x < kivi_prefill_blocks -> its rows: x = (nqt - 1 - query tile) * (B * nh) + b * nh + h
KIVI_PREFILL_HD KiviPrefillBlock kivi_prefill_block(int B, int nh, int T, uint32_t x) {
    const uint32_t units = (uint32_t)B * (uint32_t)nh, rev = x / units, u = x - rev * units;
    const int qt = kivi_prefill_qtiles(T) - 1 - (int)rev;
    KiviPrefillBlock blk;
    blk.b = (int)(u / (uint32_t)nh);
    blk.h = (int)(u - (uint32_t)blk.b * (uint32_t)nh);
    blk.q0 = qt * kPrefillQTile;
    blk.q1 = blk.q0 + kPrefillQTile < T ? blk.q0 + kPrefillQTile : T;
    return blk;
}

// the key tiles the rows [q0, q1) visit under `lead` (already clamped to [0, T]); q0 < q1
KIVI_PREFILL_HD KiviPrefillTiles kivi_prefill_tiles(int q0, int q1, int lead) {
    KiviPrefillTiles t;
    if (lead >= q1) {
        t.kt0 = t.kt1 = 0;
        return t;
    }
    t.kt0 = lead / kPrefillKTile;
    t.kt1 = (q1 - 1) / kPrefillKTile + 1;
    return t;
}

// does the VISITED tile kt of the rows [q0, q1) hold a dead pair?  All pairs are live exactly when every row is live (lead <= q0),
// every key is at or past the lead, and the tile's last key is at or under the first row's diagonal.
KIVI_PREFILL_HD bool kivi_prefill_partial(int q0, int q1, int lead, int kt) {
    (void)q1;
    const int k0 = kt * kPrefillKTile, klast = k0 + kPrefillKTile - 1;
    return !(lead <= q0 && lead <= k0 && klast <= q0);
}
