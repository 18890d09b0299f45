// kivi_mf_store_shift (include/kivi_hip.h): the 32-token blocks of one packed store (KT or VT, 2- or 4-bit super-blocks) moved
// `shift_blocks` blocks towards token 0, IN PLACE, for every (batch row, kv head): block j <- block j + shift for
// j < n_blocks - shift, then blocks [n_blocks - shift, n_blocks) zeroed (the store's "never written slots are zero" invariant:
// kivi_vt_pack_at reads, modifies and writes partly filled blocks).  What a living cache needs to drop its leading tokens (rebase,
// DESIGN.md section 17).  A shift by whole blocks keeps every code, scale and zero point bit for bit: K groups and V tokens only
// change the block they sit in (kivi_shift.h has the addresses).
//
// In place without races.  The super-blocks in use hold many blocks per (row, head) and nearly every source range is some other
// block's destination, so the two-sided walk of kivi_rowcopy.hip (disjoint sides) cannot do this.  Here a THREAD owns one 16-byte
// unit position u of a block (kivi_shift.h: 96 units at 2 bits, 160 at 4) for one (row, head), over the WHOLE block range:
//   * it walks j upward in batches of kShiftInFlight blocks.  The loads of batch n + 1 (unit u of blocks j + shift) are issued,
//     then the stores of batch n (unit u of blocks j), whose data was requested one iteration earlier: up to two batches of loads
//     are in flight and reads overlap writes;
//   * unit u of block j and unit u' of block j' share a byte only for u == u' and j == j' (the units of a block are disjoint, and
//     a unit position maps to disjoint addresses in different blocks), so every byte of the unit column u is read and written by
//     this one thread only -- there is no other thread to race with, in this workgroup or another;
//   * within the thread the order is program order on the same addresses, which the hardware keeps (a wave's accesses to one
//     address complete in issue order) and the compiler must keep: the store pointer is not __restrict__, the accesses are plain
//     loads and stores through it, nothing is marked non-temporal;
//   * block x is READ (as the source of block x - shift) in the load phase of batch (x - shift) / F, which is issued one iteration
//     before that batch is stored, and WRITTEN in the store phase of batch x / F >= (x - shift) / F: the read is issued in an
//     earlier iteration than the write, for every shift >= 1, also when the shift is smaller than the batch (F = kShiftInFlight).
//     The destination lies below the source throughout, so no block is read after it was overwritten;
//   * the vacated blocks are zeroed last, by the same thread that read them.
// So no barrier, atomic or scratch buffer is needed, and the block range of a (row, head) is NOT split across threads or
// workgroups: two segments of one unit column would race at their seam.  The price: the grid is B * nh_kv * 96 (160) threads
// whatever the length, each with up to 2 x kShiftInFlight 16-byte loads in flight -- a small B * nh_kv cannot fill the machine (DESIGN.md
// section 17 has the numbers).
//
// Range words.  A rebased row must equal a cache built from the kept tokens alone, and the sticky marks of dropped tokens would
// break that: the caller zeroes the store's B * nh_kv words on the same stream before this launch, and every thread that owns a
// SCALE unit (region 0) keeps the largest fp16 bit pattern among the scales it moves and marks once, at the end of its walk
// (mf_range_mark: thresholds on that maximum give the marks the writers would have left scale by scale; a mark per unit moved
// would serialise on the word's one address).  With nothing kept the words stay zero, as in a store nothing was written to.
#include "kivi_common.h"
#include "kivi_shift.h"

namespace {

struct SArgs {
    char* store;                         // NOT __restrict__: sources and destinations alias by design
    int* range;
    int64_t sb, sh, ss;                  // row, head, super-block strides (bytes)
    int64_t threads;                     // B * nh_kv * units of a block
    int nh_kv, n_blocks, shift;
};

__device__ __forceinline__ uint32_t max_half(uint32_t top, u32x4 v) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = v[i] & 0xFFFFu, hi = v[i] >> 16;
        top = top > lo ? top : lo;
        top = top > hi ? top : hi;
    }
    return top;
}

template <int BITS, bool IS_K>
__global__ __launch_bounds__(kShiftThreads) void store_shift_kernel(const SArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kShiftThreads + threadIdx.x;
    if (t >= a.threads) return;
    int64_t rh;
    uint32_t u;
    kivi_shift_thread(BITS, t, &rh, &u);
    const int64_t b = rh / a.nh_kv, h = rh - b * a.nh_kv;
    char* base = a.store + b * a.sb + h * a.sh;
    const bool scales = kivi_shift_is_scale(BITS, u);
    const int64_t n_keep = a.n_blocks - a.shift;
    uint32_t top = 0;
    // cur: the batch about to be stored; nxt: the batch after it, requested BEFORE cur is stored (reads and writes overlap)
    u32x4 cur[kShiftInFlight], nxt[kShiftInFlight];
#pragma unroll
    for (int k = 0; k < kShiftInFlight; ++k) {
        cur[k] = u32x4{0u, 0u, 0u, 0u};
        if (k < n_keep) cur[k] = *reinterpret_cast<const u32x4*>(base + kivi_shift_offset(BITS, IS_K, a.ss, k + a.shift, u));
    }
    for (int64_t j0 = 0; j0 < n_keep; j0 += kShiftInFlight) {
#pragma unroll
        for (int k = 0; k < kShiftInFlight; ++k) {
            const int64_t j = j0 + kShiftInFlight + k;
            nxt[k] = u32x4{0u, 0u, 0u, 0u};
            if (j < n_keep) nxt[k] = *reinterpret_cast<const u32x4*>(base + kivi_shift_offset(BITS, IS_K, a.ss, j + a.shift, u));
        }
#pragma unroll
        for (int k = 0; k < kShiftInFlight; ++k)
            if (j0 + k < n_keep) *reinterpret_cast<u32x4*>(base + kivi_shift_offset(BITS, IS_K, a.ss, j0 + k, u)) = cur[k];
        if (scales) {
#pragma unroll
            for (int k = 0; k < kShiftInFlight; ++k) top = max_half(top, cur[k]);
        }
#pragma unroll
        for (int k = 0; k < kShiftInFlight; ++k) cur[k] = nxt[k];
    }
    for (int64_t j = n_keep; j < a.n_blocks; ++j)
        *reinterpret_cast<u32x4*>(base + kivi_shift_offset(BITS, IS_K, a.ss, j, u)) = u32x4{0u, 0u, 0u, 0u};
    if (scales && n_keep > 0) mf_range_mark(a.range + rh, top);
}

}  // namespace

extern "C" int kivi_mf_store_shift(void* store, int64_t st_sb, int64_t st_sh, int64_t st_ss, void* range, int bits, int is_k, int B,
                                   int nh_kv, int64_t n_blocks, int64_t shift_blocks, kivi_stream_t stream) {
    KIVI_REQUIRE(bits == 2 || bits == 4, KIVI_EINVAL, "kivi_mf_store_shift: bits=%d (2 or 4)", bits);
    KIVI_REQUIRE(B >= 1 && B < 65536, KIVI_EINVAL, "kivi_mf_store_shift: B=%d (1 .. 65535 rows)", B);
    KIVI_REQUIRE(nh_kv >= 1 && nh_kv < 65536, KIVI_EINVAL, "kivi_mf_store_shift: nh_kv=%d (1 .. 65535 heads)", nh_kv);
    KIVI_REQUIRE(n_blocks >= 0 && n_blocks < (1LL << 31), KIVI_EINVAL, "kivi_mf_store_shift: n_blocks=%lld (0 .. 2^31 - 1 blocks in use)",
                 (long long)n_blocks);
    KIVI_REQUIRE(shift_blocks >= 0 && shift_blocks <= n_blocks, KIVI_EINVAL, "kivi_mf_store_shift: shift_blocks=%lld (0 .. n_blocks = %lld)",
                 (long long)shift_blocks, (long long)n_blocks);
    KIVI_REQUIRE(store && range, KIVI_EINVAL, "kivi_mf_store_shift: null store / range words");
    // the strides (in words, as the packers take them) have to hold the super-blocks in use without two units sharing a byte
    const int64_t W = kivi_shift_sb_bytes(bits) / 4, n_sb = (n_blocks + KIVI_MF_SB_BLOCKS - 1) / KIVI_MF_SB_BLOCKS;
    const int64_t lim = 1LL << 40;
    KIVI_REQUIRE(st_sb >= 0 && st_sh >= 0 && st_ss >= 0 && st_sb < lim && st_sh < lim && st_ss < lim, KIVI_EINVAL,
                 "kivi_mf_store_shift: strides %lld / %lld / %lld words", (long long)st_sb, (long long)st_sh, (long long)st_ss);
    const int64_t head_ext = (n_sb - 1) * st_ss + W, sb_ext = (nh_kv - 1) * st_sh + W;     // one head's / one super-block index's extent
    const bool fits = n_sb == 0 ||
                      ((n_sb == 1 || st_ss >= W) && (nh_kv == 1 || st_sh >= W) &&
                       (nh_kv == 1 || n_sb == 1 || st_sh >= head_ext || st_ss >= sb_ext) &&
                       (B == 1 || st_sb >= (n_sb - 1) * st_ss + (nh_kv - 1) * st_sh + W));
    KIVI_REQUIRE(fits, KIVI_EINVAL, "kivi_mf_store_shift: strides %lld / %lld / %lld words are too small for %lld blocks of %d heads "
                 "(%lld super-blocks of %lld words)", (long long)st_sb, (long long)st_sh, (long long)st_ss, (long long)n_blocks, nh_kv,
                 (long long)n_sb, (long long)W);
    KIVI_REQUIRE((uintptr_t)store % 16 == 0 && st_sb % 4 == 0 && st_sh % 4 == 0 && st_ss % 4 == 0 && (uintptr_t)range % 4 == 0, KIVI_EALIGN,
                 "kivi_mf_store_shift: the store and its strides must be multiples of 16 bytes (the range words: of 4)");
    if (shift_blocks == 0 || n_blocks == 0) return 0;
    SArgs a = {};
    a.store = (char*)store;
    a.range = (int*)range;
    a.sb = st_sb * 4, a.sh = st_sh * 4, a.ss = st_ss * 4;
    a.nh_kv = nh_kv, a.n_blocks = (int)n_blocks, a.shift = (int)shift_blocks;
    a.threads = (int64_t)B * nh_kv * kivi_shift_block_units(bits);
    KIVI_REQUIRE(a.threads < (1LL << 31), KIVI_EINVAL, "kivi_mf_store_shift: B * nh_kv = %lld: grid too large", (long long)B * nh_kv);
    const dim3 grid((unsigned)((a.threads + kShiftThreads - 1) / kShiftThreads)), block(kShiftThreads);
    const hipStream_t s = (hipStream_t)stream;
    if (bits == 2 && is_k) KIVI_LAUNCH((store_shift_kernel<2, true>), grid, block, s, a);
    else if (bits == 2) KIVI_LAUNCH((store_shift_kernel<2, false>), grid, block, s, a);
    else if (is_k) KIVI_LAUNCH((store_shift_kernel<4, true>), grid, block, s, a);
    else KIVI_LAUNCH((store_shift_kernel<4, false>), grid, block, s, a);
    return kivi_launch_status("kivi_mf_store_shift");
}
