// kivi_mf_store_admit (include/kivi_hip.h): rows of ONE packed store of the matrix-pipe layout (KT or VT, 2- or 4-bit super-blocks)
// of a SOURCE cache into chosen rows of a DESTINATION cache, `shift_blocks` 32-token blocks further from token 0 -- the admission
// of a short prompt at an offset: destination row rows[i], block j + shift <- source row i, block j; the
// destination's blocks [0, shift) zeroed; the destination's range word of (row, head) replaced by the source's.  A shift by whole
// blocks keeps every code, scale and zero point bit for bit, and a multiple of lcm(residual_length, 32) tokens keeps every K group
// whole (kivi_shift.h has the addresses, the in-place direction is kivi_shift.hip).
//
// Why the lead is zeroed and not left: the row held another request.  A zero block holds no scale and adds no mark, so the range
// word of the source IS the word of the row afterwards; under the 2D mask a zero block dequantises to 0 (scale 0, zero point 0), its
// scores are 0 + the mask's fp16 minimum and its values enter as 0 * p: nothing non-finite can come out of the bytes of a finished
// request.  It is also what "never written slots are zero" means for kivi_vt_pack_at.
//
// The walk (kivi_admit_shift.h): one thread per 16-byte unit of a destination block, the unit index fastest.  Source and
// destination are different allocations and the destination rows are distinct, so every byte is written by one thread and no read
// can see a write: no ordering, no barrier, and the block range of a (row, head) is split over as many threads and workgroups as it
// has units -- the grid is n_rows * nh_kv * (n_blocks + shift) * units threads, so ONE admitted row of a long cache fills the
// machine (the in-place shift's B * nh_kv * units threads would leave it idle).  One 16-byte load and one 16-byte store per thread,
// nothing under the shift is loaded; memory-level parallelism comes from occupancy (no LDS, no scratch, a handful of registers).
// The range word is one 4-byte load and store of the thread that owns unit 0 of block 0.  A row index outside [0, B) leaves that
// source row unused (the rule of kivi_cache_admit): nothing outside the destination's B rows is ever written.
#include "kivi_common.h"
#include "kivi_admit_shift.h"

namespace {

struct AArgs {
    KiviAdmitGeom g;
    const char* __restrict__ src;
    char* __restrict__ dst;
    const int* __restrict__ src_range;
    int* __restrict__ dst_range;
    const void* rows;
    int rows64, B;
};

template <int BITS, bool IS_K>
__global__ __launch_bounds__(kAdmitThreads) void store_admit_kernel(const AArgs a) {
    const uint32_t t = blockIdx.x * (uint32_t)kAdmitThreads + threadIdx.x;
    if (t >= a.g.threads) return;
    const KiviAdmitMove m = kivi_admit_move(BITS, IS_K, a.g, t);
    const int64_t r = a.rows64 ? reinterpret_cast<const int64_t*>(a.rows)[m.i] : (int64_t)reinterpret_cast<const int*>(a.rows)[m.i];
    if (r < 0 || r >= a.B) return;                     // outside the destination: nothing is written
    u32x4 v = u32x4{0u, 0u, 0u, 0u};
    if (m.copy) v = *reinterpret_cast<const u32x4*>(a.src + m.src);
    *reinterpret_cast<u32x4*>(a.dst + r * a.g.d_sb + m.dst) = v;
    if (m.range) a.dst_range[r * a.g.nh_kv + m.h] = a.src_range[(int64_t)m.i * a.g.nh_kv + m.h];
}

// the `fits` test of kivi_mf_store_shift for one side: strides (words) that hold n_blocks blocks of nh_kv heads of `rows` rows
bool side_fits(int bits, int64_t rows, int64_t nh_kv, int64_t n_blocks, int64_t sb, int64_t sh, int64_t ss) {
    const int64_t W = kivi_shift_sb_bytes(bits) / 4, n_sb = (n_blocks + KIVI_MF_SB_BLOCKS - 1) / KIVI_MF_SB_BLOCKS;
    if (n_sb == 0) return true;
    const int64_t head_ext = (n_sb - 1) * ss + W, sb_ext = (nh_kv - 1) * sh + W;
    return (n_sb == 1 || ss >= W) && (nh_kv == 1 || sh >= W) && (nh_kv == 1 || n_sb == 1 || sh >= head_ext || ss >= sb_ext) &&
           (rows == 1 || sb >= (n_sb - 1) * ss + (nh_kv - 1) * sh + W);
}

}  // namespace

extern "C" int kivi_mf_store_admit(void* dst, int64_t dst_sb, int64_t dst_sh, int64_t dst_ss, void* dst_range, const void* src,
                                   int64_t src_sb, int64_t src_sh, int64_t src_ss, const void* src_range, int bits, int is_k,
                                   int n_rows, const void* rows, int rows_bytes, int B, int nh_kv, int64_t n_blocks,
                                   int64_t shift_blocks, kivi_stream_t stream) {
    KIVI_REQUIRE(bits == 2 || bits == 4, KIVI_EINVAL, "kivi_mf_store_admit: bits=%d (2 or 4)", bits);
    KIVI_REQUIRE(B >= 1 && B < 65536, KIVI_EINVAL, "kivi_mf_store_admit: B=%d (1 .. 65535 destination rows)", B);
    KIVI_REQUIRE(n_rows >= 1 && n_rows <= B, KIVI_EINVAL, "kivi_mf_store_admit: n_rows=%d (1 .. B = %d rows to admit)", n_rows, B);
    KIVI_REQUIRE(rows_bytes == 4 || rows_bytes == 8, KIVI_EINVAL, "kivi_mf_store_admit: rows_bytes=%d (int32 or int64 row indices)", rows_bytes);
    KIVI_REQUIRE(rows && (uintptr_t)rows % rows_bytes == 0, KIVI_EINVAL, "kivi_mf_store_admit: null / misaligned rows");
    KIVI_REQUIRE(nh_kv >= 1 && nh_kv < 65536, KIVI_EINVAL, "kivi_mf_store_admit: nh_kv=%d (1 .. 65535 heads)", nh_kv);
    KIVI_REQUIRE(n_blocks >= 0 && shift_blocks >= 0 && n_blocks < (1LL << 31) && shift_blocks < (1LL << 31) &&
                 n_blocks + shift_blocks < (1LL << 31), KIVI_EINVAL,
                 "kivi_mf_store_admit: n_blocks=%lld, shift_blocks=%lld (both >= 0, their sum below 2^31)", (long long)n_blocks, (long long)shift_blocks);
    KIVI_REQUIRE(dst && dst_range && src && src_range, KIVI_EINVAL, "kivi_mf_store_admit: null store / range words");
    const int64_t lim = 1LL << 40;
    KIVI_REQUIRE(dst_sb >= 0 && dst_sh >= 0 && dst_ss >= 0 && dst_sb < lim && dst_sh < lim && dst_ss < lim && src_sb >= 0 && src_sh >= 0 &&
                 src_ss >= 0 && src_sb < lim && src_sh < lim && src_ss < lim, KIVI_EINVAL,
                 "kivi_mf_store_admit: strides %lld / %lld / %lld <- %lld / %lld / %lld words", (long long)dst_sb, (long long)dst_sh,
                 (long long)dst_ss, (long long)src_sb, (long long)src_sh, (long long)src_ss);
    KIVI_REQUIRE(side_fits(bits, B, nh_kv, n_blocks + shift_blocks, dst_sb, dst_sh, dst_ss), KIVI_EINVAL,
                 "kivi_mf_store_admit: destination strides %lld / %lld / %lld words are too small for %lld blocks of %d heads",
                 (long long)dst_sb, (long long)dst_sh, (long long)dst_ss, (long long)(n_blocks + shift_blocks), nh_kv);
    KIVI_REQUIRE(side_fits(bits, n_rows, nh_kv, n_blocks, src_sb, src_sh, src_ss), KIVI_EINVAL,
                 "kivi_mf_store_admit: source strides %lld / %lld / %lld words are too small for %lld blocks of %d heads",
                 (long long)src_sb, (long long)src_sh, (long long)src_ss, (long long)n_blocks, nh_kv);
    KIVI_REQUIRE((uintptr_t)dst % 16 == 0 && dst_sb % 4 == 0 && dst_sh % 4 == 0 && dst_ss % 4 == 0 && (uintptr_t)dst_range % 4 == 0 &&
                 (uintptr_t)src % 16 == 0 && src_sb % 4 == 0 && src_sh % 4 == 0 && src_ss % 4 == 0 && (uintptr_t)src_range % 4 == 0, KIVI_EALIGN,
                 "kivi_mf_store_admit: the stores and their strides must be multiples of 16 bytes (the range words: of 4)");
    if (n_blocks == 0 && shift_blocks == 0) return 0;
    const int64_t threads = kivi_admit_threads(bits, n_rows, nh_kv, n_blocks, shift_blocks);
    KIVI_REQUIRE(threads < (1LL << 31), KIVI_EINVAL, "kivi_mf_store_admit: %lld units to move: grid too large (2^31 threads or more)",
                 (long long)threads);
    AArgs a = {};
    a.g.s_sb = src_sb * 4, a.g.s_sh = src_sh * 4, a.g.s_ss = src_ss * 4;
    a.g.d_sb = dst_sb * 4, a.g.d_sh = dst_sh * 4, a.g.d_ss = dst_ss * 4;
    a.g.nh_kv = (uint32_t)nh_kv, a.g.n_blocks = (uint32_t)n_blocks, a.g.shift = (uint32_t)shift_blocks;
    a.g.threads = (uint32_t)threads;
    a.src = (const char*)src, a.dst = (char*)dst;
    a.src_range = (const int*)src_range, a.dst_range = (int*)dst_range;
    a.rows = rows, a.rows64 = rows_bytes == 8, a.B = B;
    const dim3 grid((unsigned)((threads + kAdmitThreads - 1) / kAdmitThreads)), block(kAdmitThreads);
    const hipStream_t s = (hipStream_t)stream;
    if (bits == 2 && is_k) KIVI_LAUNCH((store_admit_kernel<2, true>), grid, block, s, a);
    else if (bits == 2) KIVI_LAUNCH((store_admit_kernel<2, false>), grid, block, s, a);
    else if (is_k) KIVI_LAUNCH((store_admit_kernel<4, true>), grid, block, s, a);
    else KIVI_LAUNCH((store_admit_kernel<4, false>), grid, block, s, a);
    return kivi_launch_status("kivi_mf_store_admit");
}
