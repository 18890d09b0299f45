/*
 * kivi_hip.h -- C ABI of libkivi_hip.so: the MI355X (gfx950) implementation of
 * KIVI's quant/ hot path.  Plain pointers and sizes only: every pointer is a
 * DEVICE pointer owned by the caller, every kernel is enqueued on the
 * hipStream_t passed as `stream` (NULL = the default stream) and nothing here
 * synchronises or allocates.  Return value: 0 on success, a positive hipError_t
 * if a launch failed, a negative KIVI_E* code if the arguments are rejected
 * (kivi_last_error() then holds a message; thread-local).
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the jy-yuan/KIVI tree).  INTEGRATION.md shows the binding a maintainer of
 * the reference would add.
 *
 * Layout vocabulary (reference: models/llama_kivi.py:454-455, "hook state"):
 *   fpi = 32 / bits codes per int32 word, element i of a word at bit bits*i
 *   K_code_T (B, nh_kv, D, Tq/fpi) int32   K_scale_T, K_mn_T (B, nh_kv, D, Tq/g) fp16
 *   V_code   (B, nh_kv, Tv, D/fpi) int32   V_scale,  V_mn    (B, nh_kv, Tv, D/g) fp16
 * Strides are in ELEMENTS of the tensor they describe (int32 words / halves).
 *
 * SURFACE.  The reference's boundary for this path is two functions (pybind.cpp:5-8) + the Python pack module; what a
 * caller is meant to bind here is correspondingly small:
 *   SUPPORTED   pack / unpack:  kivi_quant_pack_lastdim, kivi_quant_pack_k_tmajor, kivi_unpack_dequant_lastdim,
 *                               kivi_pack_codes_lastdim, kivi_unpack_codes_lastdim
 *               fused GEMVs:    kivi_gemv_k, kivi_gemv_v (hook-state tensors), kivi_gemv_outer_dim, kivi_gemv_awq (the
 *                               reference extension's own argument layouts)
 *               a layer step:   kivi_decode_layer (hook-state cache: any 2- / 4-bit shape), kivi_mf_decode_layer and its
 *                               hipGraph form kivi_mf_decode_layer_dyn + kivi_mf_step_* (matrix-pipe cache: g = 32, D = 128,
 *                               2-bit with nh / nh_kv in {1, 4, 8} or 4-bit with nh / nh_kv in {1, 4}), with the packers of that
 *                               cache: kivi_kt_pack, kivi_vt_pack, kivi_vt_pack_at, kivi_kt_relayout, kivi_vt_relayout
 *               beam search:    kivi_cache_reorder (in-place row reorder of either cache layout, from a fork point on)
 *               admission:      kivi_cache_admit (rows of one cache into chosen rows of another, living one: continuous batching),
 *                               kivi_mf_store_admit (a packed store into chosen rows of another at a block offset, the lead zeroed:
 *                               a short prompt admitted without the pads)
 *               rebase:         kivi_mf_store_shift (the blocks of a packed store moved towards token 0 in place: a living cache
 *                               drops its leading tokens)
 *               rollback:       kivi_cache_snapshot (the fp16 residual / window and range words of a cache into a flat buffer and
 *                               back: checkpoint and restore of either cache layout)
 *               sampling:       kivi_sample (temperature / top-k / top-p / min-p draw of one token per row, Philox RNG state on
 *                               the device), kivi_sample_rows (the same draw with per-row parameters, seeds, streams and
 *                               greedy rows read from device memory), kivi_sample_rows_pen (the same with repetition /
 *                               presence / frequency penalties per row over a history table in device memory), kivi_seen_mark
 *                               (clears and marks rows of that table), kivi_sample_rows_con (the same with a constraint per
 *                               row: an allow mask, a list of biased or suppressed tokens, a minimum of new tokens),
 *                               kivi_allow_mark (writes rows of the allow masks from id lists)
 *               finishing:      kivi_stop_rows (stop token ids, stop sequences and a length limit per row, tracked in device
 *                               memory: one launch per decode step, the live rows counted on the device)
 *               scoring:       kivi_token_logprob (log-probability and rank of one given token per row of logits),
 *                              kivi_token_top_logprobs (the same plus the k most likely tokens with theirs)
 *               prompt pass:    kivi_prefill_attention (causal grouped-query attention over fp16 q / k / v with leading pads)
 *   BUILDING BLOCKS (what the layer steps are composed of; exported for tests, tools and callers that keep their own cache
 *               bookkeeping -- same contracts, but no stability promise beyond the ABI version):  kivi_gemv_k_paged,
 *               kivi_decode_scores, kivi_softmax_scaled, kivi_decode_output, kivi_decode_softmax_output, kivi_decode_attend,
 *               kivi_gqa_scores, kivi_gqa_output, kivi_gqa_decode, kivi_mf_launch_plan
 *   INSTRUMENTATION (bench.py, tools/, the parity sweeps; not part of the drop-in):  kivi_gemv_{k,v}_variant*, kivi_event_*,
 *               kivi_set_launch_events, kivi_last_timed_kernel, kivi_debug_set_stamps
 * Environment: the product library reads no environment variable; tuning knobs, losing / result-changing kernel variants and the
 * stamping instantiations exist only in -DKIVI_TUNING builds (tools/build_variant.sh).
 */
#ifndef KIVI_HIP_H
#define KIVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KIVI_ABI_VERSION 3   /* 3: range words carry an explicit byte 2 (a zero word = default placement); sliced launches always take
                                  ticket ids, the workspace's counter area holds a device error word; KIVI_ETIMEOUT, kivi_device_error */

#define KIVI_EINVAL (-1)       /* unsupported bits / group size / shape */
#define KIVI_EALIGN (-2)       /* pointer or stride alignment the kernels rely on is violated */
#define KIVI_EUNSUPPORTED (-3) /* valid in the reference, not implemented here */
#define KIVI_ETIMEOUT (-4)     /* a block of an EARLIER sliced launch gave up waiting for a partner block (see kivi_device_error) */

typedef void* kivi_stream_t; /* hipStream_t */

int kivi_abi_version(void);
const char* kivi_last_error(void);
/* Sticky, asynchronous device-side error of this process (like a stream error of the runtime): 0, or KIVI_ETIMEOUT when a block of
 * a sliced one-launch decode step (kivi_gqa_decode / kivi_mf_decode_layer*, rows cut into S > 1 slices) gave up after ~1 s of
 * waiting for a partner block of its unit -- that unit's output of that step is NaN.  The blocks report through one word of
 * host-visible memory the library owns (the only allocation it ever makes: 64 bytes of pinned host memory, on first use), so the
 * host can look without synchronising: the NEXT kivi_gqa_decode / kivi_mf_decode_layer* call returns KIVI_ETIMEOUT once (with a
 * message naming the unit) and clears the error -- the arrival counters of the timed-out launch have been put back to zero by its
 * last block, the call after that runs normally.  kivi_device_error() returns and clears the same state explicitly (after a
 * stream synchronisation it is exact).  The same code is also left in the device error word of the launch's workspace (word
 * 16375 of the counter area) for callers that keep everything on the device. */
int kivi_device_error(void);

/* ---------------------------------------------------------------- pack --- */

/*
 * Fused group-wise asymmetric quantise + pack along the LAST dim.
 * Replaces triton_quantize_and_pack_along_last_dim (quant/new_pack.py:217-252:
 * two Triton kernels + five elementwise torch kernels + an int32 temporary) and
 * its pure-torch twin quant_and_pack_vcache (quant/new_pack.py:30-48).
 *   x      (rows, T) fp16, contiguous          T % group_size == 0, T % fpi == 0
 *   code   (rows, T/fpi) int32                 scale, mn (rows, T/group_size) fp16
 * bits in {2,4,8}.  Results are bit-identical to the reference op sequence
 * (per-op fp16 rounding, round-half-even); a constant group (scale 0 -> 0/0)
 * yields code 0 as the reference's CUDA float->int conversion does.
 */
int kivi_quant_pack_lastdim(const void* x, void* code, void* scale, void* mn, int64_t rows, int64_t T,
                            int group_size, int bits, kivi_stream_t stream);

/*
 * Per-channel K quantise + pack straight from the un-transposed K tensor:
 * reads k[b, h, t, :] = k + b*k_sb + h*k_sh + t*k_st (D contiguous halves) and
 * writes the hook-state layout (groups of `group_size` TOKENS per channel d):
 *   code [b, h, d, code_off + t/fpi],  scale/mn [b, h, d, sm_off + t/group_size]
 * Replaces `key_states.transpose(2, 3).contiguous()` + the pack call at
 * models/llama_kivi.py:345 and :436 (and quant_and_pack_kcache,
 * quant/new_pack.py:8-27, whose codes are the transpose of these).
 * The *_off arguments let a pre-allocated cache be appended in place.
 */
int kivi_quant_pack_k_tmajor(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_st, void* code, int64_t code_sb,
                             int64_t code_sh, int64_t code_sr, int64_t code_off, void* scale, void* mn,
                             int64_t sm_sb, int64_t sm_sh, int64_t sm_sr, int64_t sm_off, int B, int nh, int64_t T,
                             int D, int group_size, int bits, kivi_stream_t stream);

/*
 * Unpack + dequantise along the last dim: out = fp16(fp16(fp16(q) * scale) + mn).
 * Replaces unpack_and_dequant_vcache (quant/new_pack.py:69-83); with the K^T
 * layout it also serves unpack_and_dequant_kcache (:51-66).
 */
int kivi_unpack_dequant_lastdim(const void* code, const void* scale, const void* mn, void* out, int64_t rows,
                                int64_t T, int group_size, int bits, kivi_stream_t stream);

/* Raw code pack along the last dim: pack_tensor (quant/new_pack.py:86-107) / _pack_along_last_dim (:132-154).
 * data (rows, T) int32 -> code (rows, T/fpi) int32, OR of data << bits*i (no masking, like the reference). */
int kivi_pack_codes_lastdim(const void* data_i32, void* code, int64_t rows, int64_t T, int bits,
                            kivi_stream_t stream);

/* Raw code unpack (quant/new_pack.py:110-129, unpack_tensor with pack_dim = last): int16 out. */
int kivi_unpack_codes_lastdim(const void* code, void* out_i16, int64_t rows, int64_t T, int bits,
                              kivi_stream_t stream);

/* ---------------------------------------------------------- fused GEMV --- */

/*
 * qK^T over the packed per-channel K cache, hook-state layout, no transposes:
 *   out[b, h, t] = fp16( sum_d q[b,h,d] * (scale[b,hk,d,t/g] * code[b,hk,d,t] + mn[b,hk,d,t/g]) )
 * with hk = h / (nh / nh_kv), fp32 arithmetic, one final rounding.
 * Replaces cuda_bmm_fA_qB_outer (quant/matmul.py:178-219, including its three
 * `.transpose(1,2).contiguous()` copies) -> kivi_gemv.gemv_forward_cuda_outer_dim
 * (quant/csrc/gemv_cuda.cu:511-557) -> bgemv2/4_kernel_outer_dim (:265-427) at the
 * call site models/llama_kivi.py:324.  bits in {2,4}; q_len must be 1.
 *   q    (B, nh, D)  at q + b*q_sb + h*q_sh          out (B, nh, T) at out + b*out_sb + h*out_sh
 *   code (B, nh_kv, D, >=T/fpi) strides code_sb/sh/sr  scale, mn (B, nh_kv, D, >=T/g) strides sm_sb/sh/sr
 */
int kivi_gemv_k(const void* q, int64_t q_sb, int64_t q_sh, const void* code, int64_t code_sb, int64_t code_sh,
                int64_t code_sr, const void* scale, const void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr,
                void* out, int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int D, int64_t T,
                int group_size, int bits, kivi_stream_t stream);

/*
 * Same product over PAGED per-channel K storage (what an in-place, appendable cache needs: with the plain
 * (B, nh_kv, D, capacity) layout every channel row is strided by the capacity and HBM efficiency collapses,
 * see DESIGN.md).  A page holds `page_tokens` tokens of all D channels as its own contiguous block:
 *   code  (B, nh_kv, P, D, page_tokens/fpi)   strides code_sb, code_sh, code_sp (page), code_sr (channel row)
 *   scale (B, nh_kv, P, D, page_tokens/g)     strides sm_sb,   sm_sh,   sm_sp,          sm_sr
 * Token t lives in page t / page_tokens.  `variant` = -1 picks the default kernel.  No reference twin: the
 * reference re-allocates the whole packed K with torch.cat instead (models/llama_kivi.py:350-352).
 */
int kivi_gemv_k_paged(int variant, int64_t page_tokens, int64_t code_sp, int64_t sm_sp, const void* q, int64_t q_sb,
                      int64_t q_sh, const void* code, int64_t code_sb, int64_t code_sh, int64_t code_sr,
                      const void* scale, const void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr, void* out,
                      int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int D, int64_t T, int group_size,
                      int bits, kivi_stream_t stream);

/*
 * sV over the packed per-token V cache:
 *   out[b, h, d] = fp16( sum_t a[b,h,t] * (scale[b,hk,t,d/g] * code[b,hk,t,d] + mn[b,hk,t,d/g]) )
 * Replaces the same reference chain at the call site models/llama_kivi.py:382
 * (fA there is the non-contiguous slice attn_weights[..., :-value_full_length];
 * a_sb/a_sh carry its strides so no copy is needed).
 *   a    (B, nh, Tv) at a + b*a_sb + h*a_sh          out (B, nh, D)
 *   code (B, nh_kv, Tv, D/fpi) strides code_sb/sh/sr  scale, mn (B, nh_kv, Tv, D/g) strides sm_sb/sh/sr
 */
int kivi_gemv_v(const void* a, int64_t a_sb, int64_t a_sh, const void* code, int64_t code_sb, int64_t code_sh,
                int64_t code_sr, const void* scale, const void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr,
                void* out, int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int64_t Tv, int D,
                int group_size, int bits, kivi_stream_t stream);

/*
 * ABI twin of the reference's native entry point on ITS kernel-input layout
 * (torch::Tensor gemv_forward_cuda_outer_dim, quant/csrc/gemv_cuda.h:13-21,
 * gemv_cuda.cu:511-557): in (BS, 1, IC) fp16, kernel (BS_kv, OC/fpi, IC) int32,
 * scale/zeros (BS_kv, OC/g, IC) fp16, out (BS, 1, OC) fp16, BS_kv = BS*nh_kv/nh.
 * Kept for callers that already hold transposed tensors (quant/gemv.py:117,154).
 */
int kivi_gemv_outer_dim(const void* in, const void* kernel, const void* scale, const void* zeros, void* out,
                        int64_t BS, int64_t IC, int64_t OC, int bit, int group_size, int nh, int nh_kv,
                        kivi_stream_t stream);

/*
 * ABI twin of the reference's second native entry point, the legacy AWQ-style inner-dim 4-bit GEMV
 * (torch::Tensor gemv_forward_cuda, quant/csrc/gemv_cuda.h:4-10, gemv_cuda.cu:60-246): in (B, IC) fp16,
 * kernel (OC, IC/8) int32 packed along IC, scale / zeros (OC, sz_pitch >= IC/g) fp16, out (B, OC) fp16;
 * bit must be 4 and group_size 64 or 128 like the reference.  Off the KV-cache path (surface parity only).
 */
int kivi_gemv_awq(const void* in, const void* kernel, const void* scale, const void* zeros, void* out, int64_t B,
                  int64_t IC, int64_t OC, int bit, int group_size, int64_t sz_pitch, kivi_stream_t stream);

/* --------------------------------------------------- fused decode step --- */

/*
 * The three launches of one decode step of the attention hook (models/llama_kivi.py:314-399) for one layer.
 * Together they replace ~20 kernels of the reference sequence with identical roundings:
 *
 * kivi_decode_scores: out[b,h,:T] = fused qK^T over the packed K pages (as kivi_gemv_k_paged) and
 *   out[b,h,T:T+res_len+1] = q . k for the fp16 residual keys plus the new one (:333-337); also appends `knew`
 *   to the residual buffer at index res_len (the torch.cat of :334).  `out` is the pre-scale score row (:339 cat).
 * kivi_softmax_scaled: probs = softmax_fp32(fp16(scores * inv_scale) [+ mask, clamped at fp16 min]) -> fp16
 *   (:339 division, :364-372 mask, :375 softmax).  rows = B*nh, row pitches in halves, mask (B,1,1,n) or NULL.
 * kivi_decode_output: out[b,h,:] = fp16( fp16(fused sV over the packed V) + fp16(probs[..., Tv:] @ V_window) )
 *   (:382-384; window = rows [win_start, win_start+res_len) of `vres` plus `vnew`), appends `vnew` to the window
 *   (:377) and, if `flush`, quantises the oldest window row into cache row Tv (:386-399), bit-identical to
 *   kivi_quant_pack_lastdim.  The caller advances its lengths afterwards.
 * Return KIVI_EUNSUPPORTED when no tuned kernel covers the shape (callers then compose the unfused entry points).
 */
int kivi_decode_scores(int64_t page_tokens, int64_t code_sp, int64_t sm_sp, const void* q, int64_t q_sb, int64_t q_sh,
                       const void* code, int64_t code_sb, int64_t code_sh, int64_t code_sr, const void* scale,
                       const void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr, void* kres, int64_t kres_sb,
                       int64_t kres_sh, int64_t kres_st, const void* knew, int64_t knew_sb, int64_t knew_sh, int res_len,
                       void* out, int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int D, int64_t T,
                       int group_size, int bits, kivi_stream_t stream);
int kivi_softmax_scaled(const void* scores, void* probs, int64_t rows, int64_t n, int64_t s_pitch, int64_t p_pitch,
                        float inv_scale, const void* mask, int64_t mask_sb, int nh, kivi_stream_t stream);
int kivi_decode_output(const void* probs, int64_t a_sb, int64_t a_sh, void* code, int64_t code_sb, int64_t code_sh,
                       int64_t code_sr, void* scale, void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr, void* vres,
                       int64_t vres_sb, int64_t vres_sh, int64_t vres_st, int win_start, int res_len, const void* vnew,
                       int64_t vnew_sb, int64_t vnew_sh, int flush, void* out, int64_t out_sb, int64_t out_sh, int B,
                       int nh, int nh_kv, int64_t Tv, int D, int group_size, int bits, kivi_stream_t stream);

/* kivi_softmax_scaled + kivi_decode_output in ONE call: `scores` are the pre-softmax rows written by
 * kivi_decode_scores (row length Tv + res_len + 1).  MHA rows of <= 8192 keys: one launch, every block turns its
 * row into fp16 probabilities in LDS (bit-identical to kivi_softmax_scaled) and goes on with the sV product.
 * Grouped queries (nh > nh_kv) or longer rows: a row-softmax launch first OVERWRITES `scores` with the probabilities
 * (same arithmetic), then the sV launch reads them; `scores` is scratch in that case despite the const. */
int kivi_decode_softmax_output(const void* scores, int64_t a_sb, int64_t a_sh, float inv_scale, const void* mask,
                               int64_t mask_sb, void* code, int64_t code_sb, int64_t code_sh, int64_t code_sr,
                               void* scale, void* mn, int64_t sm_sb, int64_t sm_sh, int64_t sm_sr, void* vres,
                               int64_t vres_sb, int64_t vres_sh, int64_t vres_st, int win_start, int res_len,
                               const void* vnew, int64_t vnew_sb, int64_t vnew_sh, int flush, void* out, int64_t out_sb,
                               int64_t out_sh, int B, int nh, int nh_kv, int64_t Tv, int D, int group_size, int bits,
                               kivi_stream_t stream);

/* Everything of the decode step that follows the packed qK^T GEMV, in ONE launch: residual scores
 * q . [fp16 K residual | new key] (+ append of the new key), scale + mask + softmax, packed sV + fp16 V window
 * (+ append of the new value, + quantisation of the oldest window token).  A layer's decode step is then
 * kivi_gemv_k_paged (scores[..., :Tq]) followed by this call.  `scores` rows have length Tq + k_res_len + 1 ==
 * Tv + v_res_len + 1.  KIVI_EUNSUPPORTED when a shape / alignment requirement is not met (use the finer entry points). */
typedef struct kivi_decode_attend_args {
    const void* q; int64_t q_sb, q_sh;                           /* (B, nh, D) queries */
    void* kres; int64_t kres_sb, kres_sh, kres_st;               /* (B, nh_kv, R, D) fp16 K residual buffer */
    const void* knew; int64_t knew_sb, knew_sh; int k_res_len;   /* (B, nh_kv, D) new key; keys already in kres */
    void* scores; int64_t s_sb, s_sh;                            /* (B, nh, >= n) pre-softmax score rows; scratch:
        on return the rows may hold the probabilities instead */
    float inv_scale; const void* mask; int64_t mask_sb;          /* 1/sqrt(D); additive (B,1,1,n) fp16 mask or NULL */
    void* v_code; int64_t vc_sb, vc_sh, vc_sr;                   /* packed V (B, nh_kv, >=Tv+1, D/fpi) */
    void* v_scale; void* v_mn; int64_t vs_sb, vs_sh, vs_sr;
    void* vres; int64_t vres_sb, vres_sh, vres_st; int v_win_start, v_res_len;   /* fp16 V window buffer */
    const void* vnew; int64_t vnew_sb, vnew_sh; int v_flush;     /* new value; quantise the oldest window token */
    void* out; int64_t out_sb, out_sh;                           /* (B, nh, D) attention output */
    int B, nh, nh_kv, D, group_size, v_bits; int64_t Tq, Tv;
    void* workspace; int64_t workspace_bytes;                    /* optional (may be NULL): zero-initialised device
        scratch, >= 65536 + 4096 + B*nh*512 + 4 * B*nh*D*65 bytes.  With it, rows are split over several blocks when
        B*nh_kv is too small to fill the GPU (long context, small batch) or the probabilities of a block's rows would
        not fit a small LDS budget (grouped queries, long rows); counters in it are left at zero after every call. */
    /* optional (k_code may be NULL): the packed-K side of the same step, as kivi_gemv_k_paged takes it.  With it the
       call covers the WHOLE step -- the library runs the packed qK^T itself (do not call kivi_gemv_k_paged first) and,
       for the MHA decode shape (rows <= 8192 keys, nothing split), fuses it into the same launch: the block that
       owns a (b, head) row computes the row's packed scores into LDS and goes straight on (no score round trip
       through HBM, one launch per layer). */
    const void* k_code; int64_t kc_sb, kc_sh, kc_sp, kc_sr;
    const void* k_scale; const void* k_mn; int64_t ks_sb, ks_sh, ks_sp, ks_sr;
    int64_t k_page_tokens; int k_bits;
} kivi_decode_attend_args;
int kivi_decode_attend(const kivi_decode_attend_args* args, kivi_stream_t stream);

/* ------------------------------------ grouped queries on the matrix pipe --- */

/*
 * MFMA-friendly cache layout (group_size 32, head_dim 128; bits = 2: nh / nh_kv in {1, 4, 8}; bits = 4: nh / nh_kv = 4 (round 4) or 1 (round 6: multi-head KIVI-4, e.g. LongChat-7B-32K),
 * the reference's published Mistral-7B + KIVI-4 shape): round 2 introduced it for grouped-query models, round 3 uses it for
 * multi-head models too (the matrix pipe takes the per-code multiply-adds off the vector ALU, which is what bounds the
 * hook-layout kernels).  Every entry point below takes `bits` and refuses (KIVI_EUNSUPPORTED) what is outside these sets.
 * Same codes, scales and zero points as the hook-state tensors above -- kivi_kt_relayout / kivi_vt_relayout convert
 * both ways bit for bit -- stored so that one masked code word IS a B-operand register of v_mfma_f32_16x16x32_f16
 * (kivi_amd/csrc/kivi_mfma_layout.h): per (batch row, kv head) a sequence of super-blocks of 512 tokens,
 *   [ codes 16 x 256 words | scale 16 x 128 halves | mn 16 x 128 halves ] = 6144 int32 words each (bits = 2), or
 *   [ codes 16 x 512 words | scale 16 x 128 halves | mn 16 x 128 halves ] = 10240 words (bits = 4: sb_s >= 10240),
 * addressed as base + b*sb_b + hk*sb_h + (t / 512)*sb_s (strides in words).  Never-written slots must be ZERO.
 * RANGE WORDS ("range flags"): every store comes with `range`, B * nh_kv int32 (index b * nh_kv + hk), zeroed by the caller
 *   together with the store.  The matrix pipe takes q * scale (qK^T) and p * scale (sV) as fp16 hi / lo pairs; with the default
 *   placement of q and p a group scale >= 512 would overflow them where the reference's fp32 `scale * code + zero`
 *   (quant/csrc/gemv_cuda.cu:407-413) stays finite, and group scales in the fp16 subnormals would leave the hi part without its
 *   low bits.  So every entry point that WRITES scales (kivi_kt_pack, kivi_vt_pack, the relayouts towards the layout, the V flush
 *   inside kivi_gqa_decode) marks BYTE 0 of the unit's word when it writes a scale >= 256 (inf / NaN included), BYTE 1 when it
 *   writes a scale >= 2^-8 and BYTE 2 with every scale it writes ("the writers of this unit keep byte 1"; byte stores of the value
 *   1: concurrent writers never lose a mark), and the consumers take the operand lower for a unit with byte 0 set (finite for
 *   every finite fp16 scale: qK^T places q 2^10 lower; sV needs 2^7 and splits it -- the part that rounds no probability goes
 *   into their placement, at most 3 bits into the unit's scales, exact for scales >= 2^-11), q / p 2^8 higher for a unit with byte 2 set
 *   and bytes 0, 1 clear (all its scales are KNOWN to be < 2^-8),
 *   unchanged otherwise -- in particular for a ZERO word: a store filled by a caller's own packer, or copied without its words, gets
 *   the default placement (ABI version 2 placed it higher and overflowed on ordinary data).  Sticky (never cleared by the
 *   library); a caller that copies a store copies its words; a caller that writes scales itself marks the bytes the same way.
 * The reference has no counterpart: it expands codes / scale / mn nh / nh_kv times (models/mistral_kivi.py:58-67,
 * :381-385, :441-445) or lets the CUDA kernel map heads (quant/csrc/gemv_cuda.cu:361-365).
 *
 * kivi_kt_pack: per-channel K quantise + pack of whole 32-token blocks (T % 32 == 0) from un-transposed keys
 *   k[b, h, t, :] = k + b*k_sb + h*k_sh + t*k_st (16-byte aligned rows) straight into the layout at token_offset (prompt pass
 *   models/llama_kivi.py:436, residual flush :343-356); bit-identical to kivi_quant_pack_k_tmajor + relayout.
 * kivi_vt_pack: per-token V quantise + pack of tokens [0, T) of a prompt (any T; 16-byte aligned rows) into the VT
 *   layout at token 0 -- triton_quantize_and_pack_along_last_dim (new_pack.py:217-252) as llama_kivi.py:441-448 applies
 *   it to value_states[:, :, :-R], without the intermediate hook-state tensors.
 * kivi_kt_relayout / kivi_vt_relayout: to_ref != 0 writes tokens [0, T) of the hook-state tensors
 *   (K_code_T (B,nh_kv,D,T/fpi) / V_code (B,nh_kv,T,D/fpi), fpi = 32 / bits, + scale, mn) from the layout, to_ref == 0 the reverse.
 * kivi_gqa_scores: out[b, h, :T] = packed qK^T (the arithmetic of kivi_gemv_k: fp32 accumulate, one fp16 rounding; the
 *   q * scale products enter the matrix pipe as exact hi + lo fp16 pairs).  = cuda_bmm_fA_qB_outer at llama_kivi.py:324.
 * kivi_gqa_output (nh / nh_kv in {1, 4}): out[b, h, :128] = packed sV for given fp16 attention weights
 *   probs[b, h, :T] = probs + b*p_sb + h*p_sh (rows 16-byte aligned, pitch >= T rounded up to 8) -- cuda_bmm_fA_qB_outer
 *   at llama_kivi.py:382 on the VT layout: fp32 accumulate of exact products, one fp16 rounding.  `workspace`: 64 KiB of
 *   arrival counters (zeroed once by the caller) + 4 * B * nh bytes (rounded up to 256) + B * nh_kv * slices * 2 *
 *   (nh / nh_kv) * 128 floats, slices <= max(1, ceil(T / 512)).
 */
int kivi_kt_pack(const void* k, int64_t k_sb, int64_t k_sh, int64_t k_st, void* kt, int64_t kt_sb, int64_t kt_sh,
                 int64_t kt_ss, void* kt_range, int64_t token_offset, int B, int nh_kv, int64_t T, int D, int group_size,
                 int bits, kivi_stream_t stream);
int kivi_vt_pack(const void* v, int64_t v_sb, int64_t v_sh, int64_t v_st, void* vt, int64_t vt_sb, int64_t vt_sh,
                 int64_t vt_ss, void* vt_range, int B, int nh_kv, int64_t T, int D, int group_size, int bits,
                 kivi_stream_t stream);
/* kivi_vt_pack_at: tokens [0, T) of v quantised per token into the VT layout at ANY token_offset (partly filled 32-token blocks are
 * read, modified and written; other tokens' codes are kept): bit-identical to the V flush of the decode step, range marks included */
int kivi_vt_pack_at(const void* v, int64_t v_sb, int64_t v_sh, int64_t v_st, void* vt, int64_t vt_sb, int64_t vt_sh,
                    int64_t vt_ss, void* vt_range, int64_t token_offset, int B, int nh_kv, int64_t T, int D, int group_size,
                    int bits, kivi_stream_t stream);
/* (kt_range / vt_range may be null when to_ref != 0: reading a store does not touch its flags) */
int kivi_kt_relayout(int to_ref, void* kt, int64_t kt_sb, int64_t kt_sh, int64_t kt_ss, void* kt_range, void* code,
                     int64_t code_sb, int64_t code_sh, int64_t code_sr, void* scale, void* mn, int64_t sm_sb, int64_t sm_sh,
                     int64_t sm_sr, int B, int nh_kv, int64_t T, int D, int group_size, int bits, kivi_stream_t stream);
int kivi_vt_relayout(int to_ref, void* vt, int64_t vt_sb, int64_t vt_sh, int64_t vt_ss, void* vt_range, void* code,
                     int64_t code_sb, int64_t code_sh, int64_t code_sr, void* scale, void* mn, int64_t sm_sb, int64_t sm_sh,
                     int64_t sm_sr, int B, int nh_kv, int64_t T, int D, int group_size, int bits, kivi_stream_t stream);
int kivi_gqa_scores(const void* q, int64_t q_sb, int64_t q_sh, const void* kt, int64_t kt_sb, int64_t kt_sh, int64_t kt_ss,
                    const void* kt_range, void* out, int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int D, int64_t T,
                    int group_size, int bits, kivi_stream_t stream);
int kivi_gqa_output(const void* probs, int64_t p_sb, int64_t p_sh, const void* vt, int64_t vt_sb, int64_t vt_sh, int64_t vt_ss,
                    const void* vt_range, void* out, int64_t out_sb, int64_t out_sh, int B, int nh, int nh_kv, int D, int64_t T,
                    int group_size, int bits, void* workspace, int64_t workspace_bytes, kivi_stream_t stream);

/*
 * kivi_gqa_decode: the whole decode step of one layer over the KT / VT layouts.  ONE launch (packed qK^T -> LDS scores [softmax
 * statistics per 512-token segment inside the K walk] -> residual scores -> window -> packed sV with the probabilities made on the
 * fly) when the score rows of a (batch row, kv head) unit fit the LDS and the units fill the chip:
 *   nh == nh_kv      rows of <= 16 super-blocks + a full residual (8320 keys) and (>= 192 units, or <= 4096 packed keys at any batch)
 *                                                                                                      -> mf_row_kernel (2- and 4-bit codes)
 *   nh / nh_kv == 4  rows of <= 18 super-blocks + a full residual (9344 keys) and >= 128 units (4-bit codes: >= 192) -> mf_row4_kernel
 *                    (2-bit rows of <= ~6.3k keys with >= 3 blocks per CU: the instantiation that fits three blocks per CU)
 *   nh / nh_kv == 8  rows of <= 4608 keys and >= 192 units                                            -> mf_row4_kernel<R = 8>
 * The plan is made for the LONGEST row of the step's geometry class (ceil(Tq / 512) * 512 + residual_length keys: kivi_mf_step_key),
 * whether the lengths are passed by value or device-resident, so an eager step and a replayed one of the same position take the same form.
 * For nh / nh_kv in {4, 8} LONGER rows (and rows of few units, to fill the chip) are cut into S slices of whole super-blocks, one
 * block per slice, still in ONE launch: the slices of a unit exchange their (max, sum exp) through `stats` (arrival counters in the
 * second half of the workspace's counter area), form the same probabilities a single block would, and their partial outputs meet
 * in `workspace` (S slots per unit).  Blocks of such a launch wait for each other, so their ids are ALWAYS handed out in start
 * order by ticket counters (the last eight words of the counter area, one per blockIdx % 8: a single counter serialises a launch's
 * atomics on one address; ABI version 2 skipped the ticket when the grid fitted the chip, which an ordinary launch cannot
 * guarantee: other streams, a CU mask): a waiting block's partners have started, or belong to the units at the dispatch front
 * and start as soon as any older block finishes.  The wait is bounded (~1 s); a block that gives up poisons its
 * unit's output with NaN, records KIVI_ETIMEOUT (kivi_device_error; word 16375 of the counter area) and the launch's last blocks
 * still put every counter back to zero.  At most 8183 units take a sliced form.
 * Otherwise two launches (incl. multi-head rows beyond 16 super-blocks: the sliced one-launch form of such rows is reachable through
 * KIVI_GQA_SLICES(n) only -- measured slower than the two launches):
 *   1. packed qK^T on the matrix pipe + fp16 residual scores + K append (llama_kivi.py:323-337); the epilogue applies
 *      1/sqrt(D) and the mask (:339, :364-372), writes the scaled scores to `scores` and (max, sum exp) of every
 *      512-token segment to `stats`;
 *   2. packed sV on the matrix pipe with the softmax applied on the fly (p = fp16(exp(x - max) / sum), :375) + fp16
 *      window (:377-384) + V append + quantisation of the token leaving the window into the VT layout (:386-399);
 *      rows are cut into slices, partial sums meet in `workspace`.
 * Lengths: Tq packed keys (multiple of 32) + k_res_len residual keys == Tv packed values + v_res_len window values.
 * `stats`: >= B * nh * (ceil(Tq / 512) + 4) * 2 floats.  `workspace`: 64 KiB of arrival counters (zeroed once by the
 * caller) followed by B * nh_kv * 2 * (slices + 1) * (nh / nh_kv) * 128 floats (1 <= slices <= max(1, ceil(Tv / 512));
 * + 1: the slot of the unit's window block).
 * Bounds the step writes against: residual_length (k_res_len < residual_length: the K append goes to row k_res_len of
 * kres), v_window_rows (v_win_start + v_res_len + 1 <= v_window_rows: the V append), vt_superblocks (Tv + 1 <= 512 *
 * vt_superblocks when v_flush), kt_superblocks (Tq <= 512 * kt_superblocks).
 * flags: KIVI_GQA_FORCE_SPLIT = the two-launch form even where the one-launch form applies, KIVI_GQA_FORCE_ROW = the
 * one-launch form for any number of units (rows that fit the LDS as above), KIVI_GQA_SLICES(n) = n slices per row (nh / nh_kv in
 * {4, 8}) -- tests and tuning.  KIVI_GQA_DUMP_SCORES (tests): the one-launch form also writes the fp16 rows its softmax statistics
 * are taken from (scaled, mask added: what the two-launch form leaves in `scores`) to `scores` -- nh / nh_kv in {4, 8}: the product
 * kernel, through a run-time pointer; nh == nh_kv: separate instantiations.
 * kt_range / vt_range: the range flags of the two stores (see above); the V flush may set vt_range.
 */
#define KIVI_GQA_FORCE_SPLIT 1
#define KIVI_GQA_FORCE_ROW 2
#define KIVI_GQA_DUMP_SCORES 8
#define KIVI_GQA_SLICES(n) (((n) & 0xFF) << 8)
/* the fp16 value window is a RING of v_window_rows rows (row of window token t = (v_win_start + t) mod v_window_rows):
 * residual_length + 1 rows suffice and nothing is ever compacted; nh / nh_kv in {1, 4} */
#define KIVI_GQA_WINDOW_RING 4
/*
 * Device-resident step lengths (hipGraph capture).  A decode step's launches depend on six lengths that change every step;
 * with `dyn_step` = a DEVICE pointer to a kivi_mf_step the kernels read them from there, and the launch geometry (grids, LDS,
 * slices) is sized for the step's whole geometry class: every step with the same kivi_mf_step_key -- the same number of
 * 512-token super-blocks of packed keys and values and the same one- / two-launch decision -- can REPLAY the captured
 * launches after the caller has updated the six numbers in device memory.  The host-side lengths passed with the call are the
 * ones of the step being captured (validated as usual); keeping later steps inside the caller's buffers is the caller's job
 * (kivi_mf_step_advance is the same bookkeeping kivi_mf_decode_layer does).  Buffers named by the arguments (q, new key /
 * value, mask with a fixed row pitch, out, scratch) must stay where they are across replays.
 */
typedef struct {
    int64_t Tq, Tv;                                    /* packed keys (multiple of 32), packed values */
    int32_t k_res_len, v_res_len, v_win_start, v_flush;
} kivi_mf_step;
typedef struct {
    int B, nh, nh_kv, D, group_size, bits;
    float inv_scale;
    const void* q; int64_t q_sb, q_sh;
    const void* mask; int64_t mask_sb;
    void* kt; int64_t kt_sb, kt_sh, kt_ss; int64_t Tq;
    void* kres; int64_t kres_sb, kres_sh, kres_st; const void* knew; int64_t knew_sb, knew_sh; int k_res_len;
    void* vt; int64_t vt_sb, vt_sh, vt_ss; int64_t Tv;
    void* vres; int64_t vres_sb, vres_sh, vres_st; int v_win_start, v_res_len;
    const void* vnew; int64_t vnew_sb, vnew_sh; int v_flush;
    void* scores; int64_t s_sb, s_sh;
    void* stats; int64_t stats_bytes;
    void* workspace; int64_t workspace_bytes;
    void* out; int64_t out_sb, out_sh;
    int residual_length; int64_t v_window_rows, kt_superblocks, vt_superblocks;
    int flags;
    void* kt_range; void* vt_range;                    /* B * nh_kv int32 each */
    const void* dyn_step;                              /* device kivi_mf_step or null (lengths from the fields above) */
} kivi_gqa_decode_args;
int kivi_gqa_decode(const kivi_gqa_decode_args* args, kivi_stream_t stream);
/*
 * The same step with a per-row LEAD (additive; kivi_gqa_decode is this call with lead = NULL).  `lead`: DEVICE memory, B int32, 4-byte
 * aligned (KIVI_EALIGN otherwise, before anything is enqueued).  The host never reads it, so the call can be captured and the values
 * rewritten between replays, like *dyn_step.  lead[b] = p is a promise of the caller about batch row b:
 *   - its additive mask holds the fp16 minimum (-65504) at keys [0, p) -- leading pads, the front of a rebased or admitted row;
 *   - key n - 1, the new token, is unmasked (so no row is fully masked).
 * The mask is still passed and still applied to every key the kernels read: the lead is a licence to SKIP, it never replaces the
 * mask.  The device clamps p to [0, Tq] for the packed keys and to [0, Tv] for the packed values; NULL promises nothing and the
 * launches are exactly those of kivi_gqa_decode.  A lead that promises more than the mask masks is the caller's error: the results
 * are as if those keys were masked.
 * Honoured by the one-launch forms with a block per row (nh == nh_kv, 2 and 4 bits; nh / nh_kv = 4 at 2 and 4 bits and 8 at 2 bits,
 * unsliced: kivi_mf_launch_plan == 1): no whole 512-token super-block of packed K or V under the lead is loaded or multiplied (the V
 * stream skips at its 32-token blocks and its live blocks are dealt to the waves again), the score slots of skipped keys hold exactly
 * -65504 (what KIVI_GQA_DUMP_SCORES shows there); the fp16 residual, the window, the appends and the flushes are never skipped.  A
 * masked key's probability is an exact zero, so the skip changes no term of the step: only the grouping of the fp32 partial sums of
 * the sV product moves with the waves' ranges.
 * Accepted and IGNORED -- bit for bit the call without it, the mask alone keeps them correct -- by the sliced one-launch forms, the
 * two-launch form, kivi_decode_layer (hook-state layout: it has no such argument) and kivi_mf_extend_layer.  The lead never enters
 * kivi_mf_launch_plan: an eager step and a replayed one still take the same form.
 */
int kivi_gqa_decode_lead(const kivi_gqa_decode_args* args, const int32_t* lead, kivi_stream_t stream);
/* the launch plan kivi_gqa_decode follows for a step of this geometry: 0 = two launches, S >= 1 = one launch with every row cut
 * into S slices (1: a block per row); -1: bad arguments.  dyn != 0: the plan of the step's whole geometry class (dyn_step). */
int kivi_mf_launch_plan(int B, int nh, int nh_kv, int64_t Tq, int k_res_len, int residual_length, int flags, int bits, int dyn);

/* ------------------------------------------------------ layer step --- */

/*
 * One decode step of one layer in ONE host call: kivi_gemv_k_paged + kivi_decode_attend + the cache bookkeeping of
 * the hook (models/llama_kivi.py:314-399): lengths, the K flush when the residual reaches R tokens (:343-356, packed
 * in place at the end of the prefix), the V flush of the token leaving the window (:386-399), window compaction.
 * Stateless: the descriptor names the caller's buffers (all device memory, layouts as in kivi_gemv_k_paged /
 * kivi_decode_attend; `scores` = (B, nh, s_pitch) fp16 scratch rows), `state` = {k_quant_len, k_res_len, v_quant_len,
 * v_win_start, v_res_len, kv_seq_len} is read and advanced.  KIVI_EUNSUPPORTED = no tuned kernel for the shape, state
 * untouched (except a completed window compaction): compose the step from the entry points above.
 * Failure atomicity: every argument the K flush could reject is validated before the first launch, so an argument
 * error never leaves a half-done step; `state` is written after each phase that has been enqueued (window compaction,
 * attend launch, K flush).  If the K flush LAUNCH itself fails after the attend launch was enqueued, the state reads
 * k_res_len == residual_length ("flush pending") and the next call performs that flush first.
 */
typedef struct {
    int B, nh_kv, D, k_bits, v_bits, group_size, residual_length;
    float inv_scale;                                   /* 1 / sqrt(D) */
    int64_t cap, page_tokens, v_window_rows, s_pitch;
    void* k_code; int64_t kc_sb, kc_sh, kc_sp, kc_sr;  /* (B, nh_kv, P, D, page_tokens/fpi) int32 */
    void* k_scale; void* k_mn; int64_t ks_sb, ks_sh, ks_sp, ks_sr;
    void* k_res; int64_t kr_sb, kr_sh, kr_st;          /* (B, nh_kv, R, D) fp16 */
    void* v_code; int64_t vc_sb, vc_sh, vc_sr;         /* (B, nh_kv, cap, D/fpi) int32 */
    void* v_scale; void* v_mn; int64_t vs_sb, vs_sh, vs_sr;
    void* v_res; int64_t vr_sb, vr_sh, vr_st;          /* (B, nh_kv, v_window_rows, D) fp16, contiguous */
    void* scores; int64_t s_sb, s_sh;
    void* workspace; int64_t workspace_bytes;          /* as in kivi_decode_attend_args */
} kivi_layer_desc;
int kivi_decode_layer(const kivi_layer_desc* layer, int64_t* state, const void* q, int64_t q_sb, int64_t q_sh, int nh,
                      const void* knew, int64_t kn_sb, int64_t kn_sh, const void* vnew, int64_t vn_sb, int64_t vn_sh,
                      const void* mask, int64_t mask_sb, void* out, int64_t out_sb, int64_t out_sh, kivi_stream_t stream);

/*
 * The same for a cache in the KT / VT layouts (kivi_gqa_decode + bookkeeping + the K flush through kivi_kt_pack every
 * residual_length steps + window compaction), same state array and the same atomicity contract.
 */
typedef struct {
    int B, nh_kv, D, bits, group_size, residual_length;
    float inv_scale;
    int64_t cap, v_window_rows, s_pitch;               /* cap: tokens the stores can hold (512 * super-blocks) */
    void* kt; int64_t kt_sb, kt_sh, kt_ss;
    void* vt; int64_t vt_sb, vt_sh, vt_ss;
    void* k_res; int64_t kr_sb, kr_sh, kr_st;          /* (B, nh_kv, R, D) fp16 */
    void* v_res; int64_t vr_sb, vr_sh, vr_st;          /* (B, nh_kv, v_window_rows, D) fp16, contiguous */
    void* scores; int64_t s_sb, s_sh;                  /* (B, nh, s_pitch) fp16 scratch rows */
    void* stats; int64_t stats_bytes;
    void* workspace; int64_t workspace_bytes;
    int flags;                                         /* KIVI_GQA_* */
    void* kt_range; void* vt_range;                    /* range flags of the two stores: B * nh_kv int32 each */
} kivi_mf_layer_desc;
int kivi_mf_decode_layer(const kivi_mf_layer_desc* layer, int64_t* state, const void* q, int64_t q_sb, int64_t q_sh, int nh,
                         const void* knew, int64_t kn_sb, int64_t kn_sh, const void* vnew, int64_t vn_sb, int64_t vn_sh,
                         const void* mask, int64_t mask_sb, void* out, int64_t out_sb, int64_t out_sh, kivi_stream_t stream);
/* with a per-row lead (kivi_gqa_decode_lead: B int32 of device memory or NULL; NULL = kivi_mf_decode_layer) */
int kivi_mf_decode_layer_lead(const kivi_mf_layer_desc* layer, int64_t* state, const void* q, int64_t q_sb, int64_t q_sh, int nh,
                              const void* knew, int64_t kn_sb, int64_t kn_sh, const void* vnew, int64_t vn_sb, int64_t vn_sh,
                              const void* mask, int64_t mask_sb, void* out, int64_t out_sb, int64_t out_sh, const int32_t* lead,
                              kivi_stream_t stream);

/*
 * The attend phase of the same step with device-resident lengths, for hipGraph capture (see kivi_mf_step above): launches
 * kivi_gqa_decode with dyn_step = `dev_step` and NOTHING else -- no bookkeeping, no K flush.  `host_step` = the lengths of the
 * step being enqueued (what *dev_step will hold when the launches run).  The caller, per step: writes the lengths to
 * *dev_step, replays (or calls this), kivi_mf_step_advance(host_step, ...), and when that returns 1 packs the full K residual
 * with kivi_kt_pack at token offset Tq and sets Tq += residual_length, k_res_len = 0.  A captured step may be replayed while
 * kivi_mf_step_key of the current lengths equals the key at capture time (and the cache buffers have not been reallocated).
 */
int kivi_mf_decode_layer_dyn(const kivi_mf_layer_desc* layer, const kivi_mf_step* host_step, const void* dev_step, const void* q,
                             int64_t q_sb, int64_t q_sh, int nh, const void* knew, int64_t kn_sb, int64_t kn_sh, const void* vnew,
                             int64_t vn_sb, int64_t vn_sh, const void* mask, int64_t mask_sb, void* out, int64_t out_sb,
                             int64_t out_sh, kivi_stream_t stream);
/* with a per-row lead (kivi_gqa_decode_lead): the buffer must stay where it is across replays, its values may change between them */
int kivi_mf_decode_layer_dyn_lead(const kivi_mf_layer_desc* layer, const kivi_mf_step* host_step, const void* dev_step, const void* q,
                                  int64_t q_sb, int64_t q_sh, int nh, const void* knew, int64_t kn_sb, int64_t kn_sh, const void* vnew,
                                  int64_t vn_sb, int64_t vn_sh, const void* mask, int64_t mask_sb, void* out, int64_t out_sb,
                                  int64_t out_sh, const int32_t* lead, kivi_stream_t stream);
/*
 * kivi_mf_extend_layer: Q >= 1 new tokens of one layer at once over a cache in the KT / VT layouts (same descriptor, same state
 * array as kivi_mf_decode_layer; the ring window flag is required).  q (B, nh, Q, D), knew / vnew (B, nh_kv, Q, D) fp16 (RoPE
 * applied; rows addressed as base + b*sb + h*sh + i*st, 16-byte aligned), out (B, nh, Q, D).  Chunk row i sits at position
 * P0 + i (P0 = state[5]) and attends to the whole cache as it stood before the call (packed K / V, the K residual, the V window) and
 * to chunk tokens 0..i (causal, always); `mask` (optional) is an additive fp16 mask, row i of batch b at mask + b*mask_sb +
 * i*mask_sq, P0 + Q keys (mask_sq >= P0 + Q); mask_sq == 0 broadcasts one key row per batch row to all Q chunk rows (a padding
 * mask: mask_sb >= P0 + Q, bit-identical to the same row written out Q times; the kernel reads it per row as it reads a full mask).  Per row the arithmetic of one decode step (llama_kivi.py:314-399): fp32 sums of
 * q * (scale * code + zero), fp16 scores / sqrt(D) in fp16, + mask, fp32 softmax, fp16 probabilities, fp16(fp16(packed sV) +
 * fp16(fp16 sV)) (the kernel reads the keys twice: the row's softmax statistics, then the probabilities).  In stream order: the attention launch, the K flushes (the residual filled to R and
 * packed with kivi_kt_pack, whole R-runs packed straight from knew, the rest copied into the residual), kivi_vt_pack_at of the
 * values that leave the window, the new window rows.  The resulting cache (9-tuple and range words) is bit-identical to Q
 * kivi_mf_decode_layer steps fed the same keys and values.  Everything is validated before the first launch; `state` is written
 * once, at the end.  KIVI_EINVAL for Q < 1, a mask pitch below P0 + Q (mask_sb when mask_sq == 0), a capacity below P0 + Q,
 * inconsistent lengths, a score dump (below) whose buffer cannot hold the rows.
 * layer->flags & KIVI_GQA_DUMP_SCORES (tests): the attention launch also writes the fp16 row each chunk row's softmax consumes,
 * fp16(fp16(q.k) / sqrt(D)) with the mask added and clamped at the fp16 minimum, before the causal mask: key t of chunk row i of
 * query head h, batch row b at layer->scores + b*s_sb + h*s_sh + i*s_pitch + t (halves), for the keys the row sees, t < P0 + i + 1;
 * the other halves are not written.  Requires scores != null, s_pitch >= P0 + Q, s_sh >= Q * s_pitch, s_sb >= nh * s_sh.  Without
 * the flag `scores` is not touched (extend needs no scratch).
 */
int kivi_mf_extend_layer(const kivi_mf_layer_desc* layer, int64_t* state, int Q, const void* q, int64_t q_sb, int64_t q_sh,
                         int64_t q_st, int nh, const void* knew, int64_t kn_sb, int64_t kn_sh, int64_t kn_st, const void* vnew,
                         int64_t vn_sb, int64_t vn_sh, int64_t vn_st, const void* mask, int64_t mask_sb, int64_t mask_sq, void* out,
                         int64_t out_sb, int64_t out_sh, int64_t out_st, kivi_stream_t stream);
/*
 * kivi_cache_reorder: row[b] <- row[idx[b]] IN PLACE, for every byte range the slabs name (beam search: HF's
 * _reorder_cache, models/llama_kivi.py:951-957, without the copy of the whole cache).  Rows come in groups of `group`
 * consecutive rows and idx[b] must lie in b's group (beam search: group = num_beams; an arbitrary reorder: group = B).  `idx`: B
 * int32 (idx_bytes 4) or int64 (8) indices in DEVICE memory, read on the device (never copied to the host); an index outside its
 * group leaves the row as it is.  A slab is one store of one layer, restricted to what has to move: byte (i0, i1, i2, j) of row b is
 * base + b*row_stride + i0*stride[0] + i1*stride[1] + i2*stride[2] + j, j < run, i_k < n[k].  Slabs and their pieces must not
 * overlap.  Base, strides and run are multiples of 16 bytes (16-byte moves) or of 4 (word moves).  One launch: a workgroup loads a
 * chunk of every row its group sources into LDS, then writes the rows whose index differs from their own; identity rows nobody
 * sources are not touched.  KIVI_EINVAL (before anything is enqueued) for group < 1 or > KIVI_REORDER_MAX_GROUP, B not a multiple of
 * group, a null or misaligned idx, more than KIVI_REORDER_MAX_SLABS slabs, negative counts, a null base or 4-byte misalignment.
 */
#define KIVI_REORDER_MAX_SLABS 32
#define KIVI_REORDER_MAX_GROUP 1024
typedef struct kivi_reorder_slab {
    void* base;
    int64_t row_stride;
    int64_t n[3];
    int64_t stride[3];
    int64_t run;
} kivi_reorder_slab;
int kivi_cache_reorder(const kivi_reorder_slab* slabs, int n_slabs, int B, int group, const void* idx, int idx_bytes,
                       kivi_stream_t stream);
/*
 * kivi_cache_snapshot: the byte ranges the slabs name, of every row, gathered into a flat buffer (direction 0) or scattered back
 * from it (direction 1): checkpoint and rollback of a cache.  The slabs are those of kivi_cache_reorder
 * (one store each, up to three (count, stride) levels, `run` bytes; base, strides and run multiples of 16 bytes, or of 4 for word
 * moves).  Row b of the buffer starts at buf + b*buf_row_stride; inside it the slabs follow each other in the order given, byte
 * (i0, i1, i2, j) of a slab at ((i0*n[1] + i1)*n[2] + i2)*run + j from the slab's start, and every slab starts on a 16-byte boundary
 * (a slab with a zero count or run takes no room).  One launch, no LDS, no scratch memory; a thread issues four independent loads
 * before its first store.  The cache side of direction 1 may be another allocation than the one direction 0 read (the cache grew).
 * Before anything is enqueued: KIVI_EINVAL for n_slabs outside [1, KIVI_REORDER_MAX_SLABS], B outside [1, 65535], a null slabs /
 * buf / slab base, a negative count, buf_row_stride zero or below what the slabs of a row take, direction not 0 or 1; KIVI_EALIGN for
 * a slab base / stride / run that is not a multiple of 4 bytes, buf or buf_row_stride not a multiple of 16.
 */
int kivi_cache_snapshot(const kivi_reorder_slab* slabs, int n_slabs, int B, void* buf, size_t buf_row_stride, int direction,
                        kivi_stream_t stream);
/*
 * kivi_cache_admit: row rows[i] of a DESTINATION cache <- row i of a SOURCE cache, i < n_rows, for every byte range the slabs name
 * (continuous batching, DESIGN.md section 16: a new request's prompt, run as a prompt pass of its own at the living caches' length,
 * takes over the row of a finished request; no other row, no buffer address and no length changes).  The two caches are different
 * allocations and may differ in capacity (other strides) and in where their fp16 V window sits, so an admit slab names both sides:
 * byte (i0, i1, i2, j), j < run, i_k < n[k], of the slab is
 *   source       src_base + i       * src_row_stride + i0*src_stride[0] + i1*src_stride[1] + i2*src_stride[2] + j
 *   destination  dst_base + rows[i] * dst_row_stride + i0*dst_stride[0] + i1*dst_stride[1] + i2*dst_stride[2] + j
 * The level counts and the run are shared.  Slabs and their pieces must not overlap on the destination side, and the source must
 * not overlap the destination.  Moves are 16 bytes wide when base, row stride, level strides and run of BOTH sides are multiples
 * of 16, 4 bytes wide otherwise.  `rows`: n_rows int32 (rows_bytes 4) or int64 (8) indices in DEVICE memory, read on the device;
 * they must be distinct (every destination byte is then written at most once); a value outside [0, B) leaves that source row
 * unused -- nothing outside the destination's B rows is ever written (the rule of kivi_cache_reorder).  The source holds at least
 * n_rows rows.  One launch: grid (chunks of a slab, n_rows), no LDS, no scratch, four independent loads per thread before its first
 * store.  Slabs with a zero count or run move nothing; when nothing is left, nothing is enqueued and the call returns 0.
 * KIVI_EINVAL (before anything is enqueued) for B outside [1, 65535], n_rows outside [1, B], rows_bytes not 4 or 8, a null or
 * misaligned rows, n_slabs outside [0, KIVI_REORDER_MAX_SLABS] or null slabs with n_slabs > 0, a negative count, a null base on
 * either side, a base / stride / run of either side that is not a multiple of 4 bytes, 2^31 units per row or more, a grid of 2^31
 * chunks or more.
 */
typedef struct kivi_admit_slab {
    void* dst_base;
    int64_t dst_row_stride;
    int64_t dst_stride[3];
    const void* src_base;
    int64_t src_row_stride;
    int64_t src_stride[3];
    int64_t n[3];
    int64_t run;
} kivi_admit_slab;
int kivi_cache_admit(const kivi_admit_slab* slabs, int n_slabs, int n_rows, const void* rows, int rows_bytes, int B,
                     kivi_stream_t stream);
/*
 * kivi_mf_store_shift: the 32-token blocks of ONE packed store of the matrix-pipe layout (KT: is_k != 0, or VT; 2- or 4-bit
 * super-blocks) moved shift_blocks blocks towards token 0, in place, for all B rows and nh_kv heads (rebase of a living cache,
 * DESIGN.md section 17): block j <- block j + shift_blocks for j in [0, n_blocks - shift_blocks), then blocks
 * [n_blocks - shift_blocks, n_blocks) zeroed ("never written slots are zero" holds afterwards).  n_blocks: the blocks in use before
 * the call.  A block is its code words plus its scale and zero-point pieces, wherever its super-block keeps them; a partly filled
 * last V block moves whole.  Every code, scale and zero point keeps its bits.  store / st_sb / st_sh / st_ss (words) / range: as
 * for kivi_kt_pack.  The RANGE WORDS are recomputed, not kept: the caller zeroes the store's B * nh_kv words on the same stream
 * before the call, and the launch marks them from the scales it moves -- the words of a store written from the kept tokens alone
 * (nothing kept: zero).  One launch, no LDS, no scratch, no second copy of the store: a thread owns one 16-byte unit position of a
 * block for one (row, head) over the whole block range, so every byte is touched by one thread only, in program order, destination
 * below source (kivi_amd/csrc/kivi_shift.hip).
 * Before anything is enqueued: KIVI_EINVAL for bits not 2 or 4, B outside [1, 65535], nh_kv < 1, n_blocks < 0, shift_blocks outside
 * [0, n_blocks], a null store or range, strides too small for n_blocks; KIVI_EALIGN for a base or stride that is not a multiple of
 * 16 bytes.  shift_blocks == 0 or n_blocks == 0: nothing is enqueued, returns 0.
 */
int kivi_mf_store_shift(void* store, int64_t st_sb, int64_t st_sh, int64_t st_ss, void* range, int bits, int is_k, int B, int nh_kv,
                        int64_t n_blocks, int64_t shift_blocks, kivi_stream_t stream);
/*
 * kivi_mf_store_admit: ONE packed store of the matrix-pipe layout (KT: is_k != 0, or VT; 2- or 4-bit super-blocks) of a SOURCE cache
 * into chosen rows of a DESTINATION cache, shift_blocks 32-token blocks further from token 0 (the admission of a short prompt at an
 * offset).  For i < n_rows, every kv head and every block j < n_blocks (the blocks in use of the source):
 *   destination row rows[i], block j + shift_blocks <- source row i, block j   (its code words, scale and zero-point pieces, wherever
 *                                                      each side's super-block keeps them; a partly filled last V block moves whole)
 *   destination row rows[i], blocks [0, shift_blocks) <- 0
 *   destination range word of (rows[i], head)         <- the source's word of (i, head): replaced, not OR-ed -- zero blocks hold no
 *                                                      scale and add no mark, so the source's word is the row's
 * Every code, scale and zero point keeps its bits.  dst / dst_sb / dst_sh / dst_ss (words) / dst_range and the src_ five: as for
 * kivi_kt_pack, each side with its own strides; the range words of a side are rows x nh_kv contiguous int32.  The two stores are
 * different allocations.  `rows`: n_rows int32 (rows_bytes 4) or int64 (8) indices in DEVICE memory, read on the device; they must be
 * distinct; a value outside [0, B) leaves that source row unused -- nothing outside the destination's B rows is ever written (the
 * rule of kivi_cache_admit).  The source holds at least n_rows rows.  One launch of n_rows * nh_kv * (n_blocks + shift_blocks) *
 * (units of a block) threads, one 16-byte unit each (kivi_amd/csrc/kivi_admit_shift.h has the map): no LDS, no scratch, no atomics.
 * shift_blocks == 0 is legal: the plain move of the blocks and the range words.
 * Before anything is enqueued: KIVI_EINVAL for bits not 2 or 4, B outside [1, 65535], n_rows outside [1, B], rows_bytes not 4 or 8, a
 * null or misaligned rows, nh_kv < 1, a negative block count, n_blocks + shift_blocks >= 2^31, a null store or range pointer on
 * either side, strides of the destination too small for n_blocks + shift_blocks blocks or of the source for n_blocks, a grid of
 * 2^31 threads or more; KIVI_EALIGN for a base or stride that is not a multiple of 16 bytes (range words: of 4).
 * n_blocks == 0 and shift_blocks == 0: nothing is enqueued, returns 0.
 */
int kivi_mf_store_admit(void* dst, int64_t dst_sb, int64_t dst_sh, int64_t dst_ss, void* dst_range, const void* src, int64_t src_sb,
                        int64_t src_sh, int64_t src_ss, const void* src_range, int bits, int is_k, int n_rows, const void* rows,
                        int rows_bytes, int B, int nh_kv, int64_t n_blocks, int64_t shift_blocks, kivi_stream_t stream);
/*
 * kivi_sample: one token per row drawn from (B, V) logits the way transformers' do_sample path does:
 * s = float(logit) / temperature; keep s >= the top_k-th largest s (ties kept; top_k = 0 or >= V: off); renormalise over those and
 * keep a token when the probability mass strictly above it is < top_p (whole tie classes; 1: off); keep p >= min_p * p_max (0: off);
 * then the first token in vocabulary order whose inclusive running sum of kept probabilities exceeds u * (kept mass).
 * Probabilities are integer weights floor(exp(s - max) * 2^40), so every sum is exact and the token is reproducible bit for bit.
 *   logits      row b at logits + b * row_stride (elements); fp16 (logits_bits 16), fp32 (32) or bf16 (KIVI_LOGITS_BF16, below); any
 *               V-long row, e.g. the
 *               (B, 1, V) output of lm_head read in place
 *   rng_state   two int64 in device memory, {seed, n}.  u = (x0 >> 8) * 2^-24 with x0 the first word of Philox4x32-10 at
 *               key (seed low 32 bits, seed high 32 bits), counter (b, 0, n low 32 bits, n high 32 bits).  A second one-thread
 *               launch of the same call adds 1 to n after the draw: a captured graph replays without host writes.
 *   out_tokens  int64, token of row b at out_tokens[b * out_stride]
 * -inf logits are legal and never drawn; a row that is all -inf or holds NaN / +inf gets some token in [0, V).
 * KIVI_EINVAL (nothing enqueued) for a logits_bits that is none of the three, B outside [1, KIVI_SAMPLE_MAX_B], V outside [1, KIVI_SAMPLE_MAX_V],
 * row_stride < V or out_stride < 1 (B > 1), temperature not finite and > 0, top_k < 0, top_p outside (0, 1], min_p outside [0, 1),
 * a null pointer; KIVI_EALIGN for logits not aligned to its element, rng_state or out_tokens not 8-byte aligned.
 *
 * KIVI_LOGITS_BF16: a third value of `logits_bits`, here and in every entry below that takes one
 * (kivi_sample_rows / _pen / _con, kivi_token_logprob, kivi_token_top_logprobs): the rows are bf16, 2-byte elements.  float(logit) of
 * a bf16 element is its exact fp32 image (its 16 bits over 16 zero bits), so every result -- tokens, history-table updates,
 * log-probabilities, lse, ranks, top-k ids -- holds the bits the same entry gives with logits_bits 32 on the row converted to fp32.
 * 16 and 32 keep their meaning; any other value is KIVI_EINVAL.
 */
#define KIVI_LOGITS_BF16 0x110 /* 16-bit elements, bit 8: the brain-float layout */
#define KIVI_SAMPLE_MAX_B 65535
#define KIVI_SAMPLE_MAX_V (1 << 20)
int kivi_sample(const void* logits, int logits_bits, int64_t row_stride, int B, int V, float temperature, int top_k, float top_p,
                float min_p, int64_t* rng_state, int64_t* out_tokens, int64_t out_stride, kivi_stream_t stream);
/*
 * kivi_sample_rows: kivi_sample with the parameters and the RNG stream of every row read from device memory:
 * requests with different parameters -- greedy ones among them -- share one launch, and a row's token is a function of its logits,
 * its record and its draw index alone, not of the row it sits in.  Row b is processed exactly as kivi_sample processes a row, with
 * temperature / top_k / top_p / min_p of rows[b] (the same fp32 arithmetic, tie classes and 2^40 integer weights), and
 *   u = (x0 >> 8) * 2^-24, x0 the first word of Philox4x32-10 at key (seed low 32 bits, seed high 32 bits) and counter
 *   (rows[b].stream, 0, n low 32 bits, n high 32 bits), n = draw_index[b].
 * THE IDENTITY: kivi_sample on B rows at {seed, n} gives, token for token, what kivi_sample_rows gives with rows[b].seed = seed,
 * rows[b].stream = b, draw_index[b] = n and the same four parameters in every record.
 *   rows        B records in device memory, read only
 *   draw_index  int64[B] in device memory; after its draw the workgroup of row b stores n + 1 itself (one launch in all: a captured
 *               graph replays without host writes, and a host write to one row's record or index touches no other row)
 *   flags       KIVI_SAMPLE_ROW_GREEDY: the token is the lowest index j that maximises float(logit[j]) (the tie rule of
 *               kivi_token_logprob's rank; a -inf logit is chosen only when the whole row is -inf).  No random number is consumed,
 *               temperature and the filters are ignored; draw_index[b] still advances, so it counts calls.
 * logits, out_tokens and the unusual rows (all -inf, NaN, +inf: some token in [0, V)) as in kivi_sample.
 * The values INSIDE the records cannot be checked by the host entry (the caller validates them; kivi_amd/sampling.py does).  A record
 * outside the contract degrades, it never loops and never indexes outside its row:  top_k < 0 is read as 0 (off);  top_p is clamped
 * into (0, 1] (NaN or > 1: 1, off; <= 0: the smallest positive float, the top tie class alone);  min_p is clamped into [0, 1) (NaN
 * or < 0: 0, off; >= 1: the largest float below 1);  a temperature that is not finite or is <= 0 makes the row greedy.
 * KIVI_EINVAL (nothing enqueued) for a logits_bits that is none of the three, B outside [1, KIVI_SAMPLE_MAX_B], V outside [1, KIVI_SAMPLE_MAX_V],
 * row_stride < V or out_stride < 1 (B > 1), a null logits / rows / draw_index / out_tokens; KIVI_EALIGN for logits not aligned to
 * its element, rows, draw_index or out_tokens not 8-byte aligned.
 */
#define KIVI_SAMPLE_ROW_GREEDY 1u
typedef struct {         /* 32 bytes, 8-byte aligned */
    float temperature;   /* finite, > 0 (ignored for a greedy row) */
    int32_t top_k;       /* >= 0, 0 = off */
    float top_p;         /* (0, 1], 1 = off */
    float min_p;         /* [0, 1), 0 = off */
    int64_t seed;        /* Philox key (low 32 bits, high 32 bits) */
    uint32_t stream;     /* Philox counter word 0 */
    uint32_t flags;      /* KIVI_SAMPLE_ROW_* */
} kivi_sample_row;
int kivi_sample_rows(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                     int64_t* draw_index, int64_t* out_tokens, int64_t out_stride, kivi_stream_t stream);
/*
 * kivi_sample_rows_pen: kivi_sample_rows with a repetition, a presence and a frequency penalty per row (HF's
 * and vLLM's repetition_penalty over prompt and output tokens, OpenAI's and vLLM's presence_penalty / frequency_penalty over output
 * tokens), applied where the logit is read, in the same single launch.
 *   seen   the history table: one uint16 per (row, token), row b at seen + b * seen_stride (elements), seen_stride >= V, rows
 *          16-byte aligned.  Bit 15: the token occurred in the row's prompt.  Bits 0-14: c, the number of times the row has emitted
 *          the token, saturating at 32767.  any = (word != 0).
 *   pen    one kivi_sample_penalty per row in device memory, read only: theta = repetition, presence, frequency
 * THE PENALISED LOGIT, before the temperature (the order of HF's _get_logits_processor), for greedy rows too.  Every operation is
 * one correctly rounded IEEE fp32 operation and none is contracted into an fma, so an fp32 restatement on the CPU gives the same bits:
 *   x = float(logit)
 *   if any:    x = (x > 0) ? x / theta : x * theta
 *   t = frequency * float(c);  x = x - t            (always; c = 0 leaves x unchanged)
 *   if c > 0:  x = x - presence
 *   s = (temperature != 1 ? x / temperature : x) + 0.0f, and from there kivi_sample_rows unchanged: thresholds, tie classes, the
 *   2^40 integer weights, Philox, the greedy tie rule.
 * After writing its token j, the workgroup of row b adds 1 to the count of seen[b][j] unless it is 32767 (one lane, a plain 16-bit
 * vector store; the prompt bit stays), and stores draw_index[b] + 1: one launch, which a captured graph replays without host writes.
 * IDENTITY A: with every record neutral (1, 0, 0) the tokens are bit for bit those of kivi_sample_rows, whatever the table holds (a
 * workgroup whose record is neutral takes the unpenalised path and reads no table word but the one it counts).
 * IDENTITY B: with any records and table the tokens are bit for bit those of kivi_sample_rows on the fp32 logits the rule gives.
 * A record outside the contract degrades as kivi_sample_rows' do: theta not finite or <= 0 is read as 1, a presence or frequency
 * that is not finite as 0; the kernel never loops and never indexes outside its row of logits or of the table.
 * Refusals (nothing enqueued) as kivi_sample_rows, and KIVI_EINVAL for a null pen / seen or seen_stride < V; KIVI_EALIGN for pen
 * not 4-byte aligned, seen not 16-byte aligned, seen_stride not a multiple of 8.
 */
typedef struct {         /* 16 bytes, 4-byte aligned */
    float repetition;    /* theta: finite, > 0; 1 = off */
    float presence;      /* finite; 0 = off */
    float frequency;     /* finite; 0 = off */
    uint32_t reserved;   /* 0 */
} kivi_sample_penalty;
int kivi_sample_rows_pen(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                         int64_t* draw_index, const kivi_sample_penalty* pen, uint16_t* seen, int64_t seen_stride,
                         int64_t* out_tokens, int64_t out_stride, kivi_stream_t stream);
/*
 * kivi_seen_mark: writes rows of the history table of kivi_sample_rows_pen.  Entry i of the call (i < n) serves table row rows[i]
 * (rows: int32[n] in device memory, distinct, each a row of the table -- the entry cannot check them, the caller does; a negative
 * one is skipped; null: row i) with the tokens tokens[i * tok_row_stride + t], t in [lead[i], T).
 *   KIVI_SEEN_CLEAR   the row's seen_stride words are zeroed first (16-byte stores)
 *   KIVI_SEEN_PROMPT  bit 15 of every token's word is set
 *   KIVI_SEEN_OUTPUT  1 is added to every token's count instead: exact, duplicates count, saturating at 32767
 * At most one of PROMPT / OUTPUT.  Token ids outside [0, V) are skipped.  lead (int32[n] in device memory or null = 0) is clamped
 * to [0, T] on the device and never read on the host, as in kivi_prefill_attention.  Two tokens share a 32-bit word of the table:
 * the marks are atomics on that word.  T == 0 with CLEAR is legal and resets the rows (tokens may then be null); T == 0 without it
 * enqueues nothing.  One launch, n workgroups.
 * KIVI_EINVAL (nothing enqueued) for flags 0, unknown or PROMPT | OUTPUT, V outside [1, KIVI_SAMPLE_MAX_V], n outside
 * [1, KIVI_SAMPLE_MAX_B], T < 0, a null seen, seen_stride < V, null tokens with marks and T > 0, tok_row_stride < T (n > 1);
 * KIVI_EALIGN for seen not 16-byte aligned, seen_stride not a multiple of 8, rows or lead not 4-byte, tokens not 8-byte aligned.
 */
#define KIVI_SEEN_CLEAR 1
#define KIVI_SEEN_PROMPT 2
#define KIVI_SEEN_OUTPUT 4
int kivi_seen_mark(uint16_t* seen, int64_t seen_stride, int V, const int32_t* rows, int n, const int64_t* tokens,
                   int64_t tok_row_stride, int T, const int32_t* lead, int flags, kivi_stream_t stream);
/*
 * kivi_sample_rows_con: kivi_sample_rows_pen with a constraint per row: an allow mask (what a grammar engine
 * hands a sampler at every step), a short list of tokens with an additive bias (logit_bias; -inf: a banned token), and list entries
 * that are suppressed until the row has made a number of draws (min_new_tokens over the eos / stop ids) -- applied where the logit
 * is read, in the same single launch, for greedy rows too.
 *   con    one kivi_sample_constraint per row in device memory, read only
 *   allow  the allow masks: uint32 words, row b at allow + b * allow_stride (words); bit (e & 31) of word (e >> 5) is 1 when token e
 *          is allowed; allow_stride >= ceil(V / 32) and a multiple of 4, the base 16-byte aligned; bits at or beyond V are ignored.
 *          Read only for rows whose record sets KIVI_CONSTRAINT_MASK; may be null when none does (a null allow reads as "no mask").
 *   list   the lists: kivi_sample_list_entry, row b at list + b * list_stride (entries), list_stride in [0, KIVI_SAMPLE_MAX_LIST], the
 *          base 8-byte aligned; a row's first n_list entries count, in ascending token order, one per token (sorting and merging
 *          is the host's duty).  May be null when every n_list is 0 (a null list reads as empty lists).
 *   pen / seen / seen_stride as in kivi_sample_rows_pen, or BOTH null: no penalties, and the drawn token is not counted.
 * THE RULE, before the temperature; every operation one correctly rounded IEEE fp32 operation, none contracted into an fma:
 *   x = float(logit)
 *   if token e has a list entry:
 *       if (entry.word & KIVI_LIST_SUPPRESS) and draw_index[b] < suppress_until:  masked = true
 *       else:                                                                     x = x + entry.value
 *   x = the penalised logit of kivi_sample_rows_pen on x   (only with pen / seen and a record that is not neutral; unchanged)
 *   if masked or (KIVI_CONSTRAINT_MASK and bit e of the row's allow mask is 0):   x = -inf
 *   s = (temperature != 1 ? x / temperature : x) + 0.0f, and from there kivi_sample_rows unchanged.
 * suppress_until is a draw index: the host stores (the row's draw index when the request is bound) + min_new_tokens, and the store
 * of draw_index[b] + 1 that every launch makes advances the row towards it -- inside a captured graph too.
 * A row whose every token is masked is an all -inf row: some token in [0, V), as in kivi_sample.
 * IDENTITY A: with every constraint record neutral (no MASK, n_list 0), whatever allow and list hold, tokens, draw_index and the
 * history table are bit for bit those of kivi_sample_rows_pen (with null pen / seen: the tokens those of kivi_sample_rows): a
 * workgroup whose record is neutral takes that kernel's path and reads neither allow nor list.
 * IDENTITY B: with any records the tokens are bit for bit those of kivi_sample_rows on the fp32 logits the rule gives.
 * A record outside the contract degrades and never faults: n_list is clamped to [0, min(KIVI_SAMPLE_MAX_LIST, list_stride)]; a
 * NaN value reads as 0; only bits 0-19 of an entry's word are read as its token, and an id >= V matches nothing; for an unsorted or
 * duplicated list which entry applies to a token is unspecified; nothing is read outside the row's list, mask, logits or table.
 * Refusals (nothing enqueued): everything kivi_sample_rows refuses; KIVI_EINVAL for a null con, exactly one of pen / seen null,
 * seen_stride < V (with a table), allow_stride < ceil(V / 32) (with allow), list_stride outside [0, KIVI_SAMPLE_MAX_LIST];
 * KIVI_EALIGN for pen not 4-byte, seen not 16-byte aligned, seen_stride not a multiple of 8, con not 8-byte, allow not 16-byte
 * aligned, allow_stride not a multiple of 4 (with allow), list not 8-byte aligned.
 */
#define KIVI_SAMPLE_MAX_LIST 1024
#define KIVI_CONSTRAINT_MASK 1u          /* kivi_sample_constraint.flags: the row's allow mask is in force */
#define KIVI_LIST_TOKEN 0x000FFFFFu      /* kivi_sample_list_entry.word: bits 0-19, the token id */
#define KIVI_LIST_SUPPRESS 0x80000000u   /* kivi_sample_list_entry.word: bit 31, masked while draw_index < suppress_until */
typedef struct {             /* 32 bytes, 8-byte aligned */
    uint32_t flags;          /* KIVI_CONSTRAINT_* */
    int32_t n_list;          /* live entries of the row's list */
    int64_t suppress_until;  /* SUPPRESS entries mask their token while draw_index < this */
    uint32_t reserved[4];    /* 0 */
} kivi_sample_constraint;
typedef struct {             /* 8 bytes */
    uint32_t word;           /* KIVI_LIST_TOKEN | KIVI_LIST_SUPPRESS; the other bits 0 */
    float value;             /* any fp32 but NaN, +-inf included */
} kivi_sample_list_entry;
int kivi_sample_rows_con(const void* logits, int logits_bits, int64_t row_stride, int B, int V, const kivi_sample_row* rows,
                         int64_t* draw_index, const kivi_sample_penalty* pen, uint16_t* seen, int64_t seen_stride,
                         const kivi_sample_constraint* con, const uint32_t* allow, int64_t allow_stride,
                         const kivi_sample_list_entry* list, int64_t list_stride, int64_t* out_tokens, int64_t out_stride,
                         kivi_stream_t stream);
/*
 * kivi_allow_mark: writes rows of the allow masks of kivi_sample_rows_con from lists of token ids; kivi_seen_mark's sibling.  Entry i
 * of the call (i < n) serves mask row rows[i] (int32[n] in device memory, distinct, each a row of the masks -- the caller's duty; a
 * negative one is skipped; null: row i) with the ids tokens[i * tok_row_stride + t], t in [0, len[i]) (len: int32[n] in device
 * memory, clamped to [0, T] on the device and never read on the host; null: T).
 *   KIVI_ALLOW_NONE   the row's ceil(V / 32) words are zeroed first     KIVI_ALLOW_ALL    ... set to all ones first
 *   KIVI_ALLOW_SET    the bit of every id is set (an atomic OR)         KIVI_ALLOW_UNSET  ... cleared (an atomic AND)
 * At most one of NONE / ALL and one of SET / UNSET; a fence and a barrier put the marks after the fill.  Ids outside [0, V) are
 * skipped.  The words of a row beyond ceil(V / 32) and the rows not named are never written.  T == 0 (or no SET / UNSET) with a fill
 * only fills (tokens may then be null); without one it enqueues nothing.  One launch, n workgroups.
 * KIVI_EINVAL (nothing enqueued) for flags 0, unknown, NONE | ALL or SET | UNSET, V outside [1, KIVI_SAMPLE_MAX_V], n outside
 * [1, KIVI_SAMPLE_MAX_B], T < 0, a null allow, allow_stride < ceil(V / 32), null tokens with marks and T > 0, tok_row_stride < T
 * (n > 1); KIVI_EALIGN for allow not 16-byte aligned, allow_stride not a multiple of 4, rows or len not 4-byte, tokens not 8-byte
 * aligned.
 */
#define KIVI_ALLOW_NONE 1
#define KIVI_ALLOW_ALL 2
#define KIVI_ALLOW_SET 4
#define KIVI_ALLOW_UNSET 8
int kivi_allow_mark(uint32_t* allow, int64_t allow_stride, int V, const int32_t* rows, int n, const int64_t* tokens,
                    int64_t tok_row_stride, int T, const int32_t* len, int flags, kivi_stream_t stream);
/*
 * kivi_stop_rows: the finish tracker of a decode batch, advanced by one token per row: stop token ids, stop
 * sequences and a length limit per row, state in device memory, so that a captured step knows which rows are live without asking the
 * host.  Entry i of the call (i < n) serves table row r = rows[i] (rows: n int32 (rows_bytes 4) or int64 (8) indices in DEVICE
 * memory, distinct -- the caller's duty, as for kivi_seen_mark; a value outside [0, B) leaves the entry unused: its token is neither
 * read nor written; null: r = i, and n <= B) with the token t = tokens[i * tok_stride]:
 *   state[r].reason != 0 (the row has finished):  tokens[i * tok_stride] = pad, nothing else changes.
 *   state[r].reason == 0 (live):  produced += 1, and t enters the ring at slot (produced - 1) % KIVI_STOP_MAX_LEN (a t outside
 *     [0, 2^31) enters as -1 and matches nothing).  The row finishes when
 *       (a) t == ids[j] for some j < n_ids                                            reason 1, index = the lowest such j
 *       (b) for some j < n_seqs, m = seq_len[j] <= produced and seq[j][0..m) equals the last m produced tokens
 *                                                                                     reason 2, index = the lowest such j
 *       (c) produced == limit                                                         reason 3, index = -1
 *     with the priority (a), (b), (c) when several hold.  t itself stays in the token buffer: the stop is part of the output.
 * Only tokens produced since the row's state was last reset count (the host rebinds a row by rewriting its two records: produced 0,
 * reason 0, index -1): a sequence never matches across two requests nor into a prompt.
 * After the n entries *n_live = the number of rows of the WHOLE table (B rows) with reason == 0.  n == 0 is legal and only counts
 * (tokens and rows may then be null).
 * The values INSIDE the records cannot be checked by the host entry (kivi_amd/stopping.py validates them).  A record outside the
 * contract degrades, it never indexes outside itself: n_ids is clamped into [0, KIVI_STOP_MAX_IDS], n_seqs into
 * [0, KIVI_STOP_MAX_SEQS], a seq_len outside [1, KIVI_STOP_MAX_LEN] never matches, a limit < 1 never ends the row.
 * One launch of ONE 256-thread workgroup (n_live counts the whole table): 16 lanes per entry -- lane l compares ids[l] and position
 * l of every sequence, a wave ballot gathers the matches --, 16 entries per pass; a barrier, then the count.  No LDS atomics, no
 * scratch, every global write an ordinary vector store, no host read, no allocation: capturable.
 * KIVI_EINVAL (nothing enqueued) for B outside [1, KIVI_SAMPLE_MAX_B], n outside [0, KIVI_SAMPLE_MAX_B], n > B without rows,
 * rows_bytes not 4 or 8 (with rows), tok_stride < 1 (n > 1), a null params / state / n_live, null tokens with n > 0; KIVI_EALIGN for
 * tokens, params or state not 8-byte aligned, rows not aligned to rows_bytes, n_live not 4-byte aligned.
 */
#define KIVI_STOP_MAX_IDS 16
#define KIVI_STOP_MAX_SEQS 8
#define KIVI_STOP_MAX_LEN 16
#define KIVI_STOP_LIVE 0
#define KIVI_STOP_TOKEN 1
#define KIVI_STOP_SEQUENCE 2
#define KIVI_STOP_LENGTH 3
typedef struct {                                         /* 624 bytes, 8-byte aligned; host-written, read only by the kernel */
    int32_t n_ids;                                       /* [0, KIVI_STOP_MAX_IDS] */
    int32_t n_seqs;                                      /* [0, KIVI_STOP_MAX_SEQS] */
    int32_t limit;                                       /* >= 1: the tokens the row may produce (INT32_MAX: none in practice) */
    int32_t reserved;                                    /* 0 */
    int32_t ids[KIVI_STOP_MAX_IDS];                      /* stop token ids, >= 0 */
    int32_t seq_len[KIVI_STOP_MAX_SEQS];                 /* [1, KIVI_STOP_MAX_LEN] */
    int32_t seq[KIVI_STOP_MAX_SEQS][KIVI_STOP_MAX_LEN];  /* seq[j][0..seq_len[j]), oldest token first */
} kivi_stop_params;
typedef struct {                                         /* 80 bytes, 8-byte aligned */
    int32_t produced;                                    /* tokens since the row was bound (at the finish: the output's length) */
    int32_t reason;                                      /* KIVI_STOP_* */
    int32_t index;                                       /* which id / sequence matched; -1: live or length */
    int32_t reserved;                                    /* 0 */
    int32_t ring[KIVI_STOP_MAX_LEN];                     /* produced token p (0-based) at slot p % KIVI_STOP_MAX_LEN */
} kivi_stop_state;
int kivi_stop_rows(int64_t* tokens, int64_t tok_stride, const kivi_stop_params* params, kivi_stop_state* state, const void* rows,
                   int rows_bytes, int n, int B, int64_t pad, int32_t* n_live, kivi_stream_t stream);
/*
 * kivi_token_logprob: the log-probability of one given token per row of (N, V) logits, log-softmax + gather in one launch without
 * an fp32 (N, V) intermediate (teacher-forced scoring, perplexity, the log-probabilities of generated tokens).
 * Per row r, with t = targets[r * target_stride] and x_j = float(logit[r, j]):
 *   m = max_j x_j;  S = sum_j floor(exp(x_j - m) * 2^40), a 64-bit integer sum of the weights kivi_sample draws from, so the result
 *   does not depend on the order of the additions (the same row gives the same bits strided or contiguous, eager or replayed);
 *   lse = m + log(S * 2^-40);  out_logprob[r] = x_t - lse;  out_lse[r] = lse (when given);
 *   out_rank[r] (when given) = #{j : x_j > x_t, or x_j == x_t and j < t}: 0 exactly when argmax of the row is t.
 *   t == ignore_index: logprob 0, rank -1, lse written.  Any other t outside [0, V): logprob NaN, rank -1, lse written.
 *   logits      fp16 (logits_bits 16), fp32 (32) or bf16 (KIVI_LOGITS_BF16); row r starts at logits + r * row_stride elements and is
 *               contiguous
 *   targets     int64;  out_logprob / out_lse fp32 and out_rank int32, N contiguous entries each; out_lse and out_rank may be null
 * -inf logits are legal and weigh 0; a target on one gives -inf.  A row that is all -inf or holds NaN / +inf gets some value.
 * One 1024-thread workgroup per row, rows taken grid-stride: N is not bounded by the grid.
 * KIVI_EINVAL (nothing enqueued) for a logits_bits that is none of the three, N < 1, V outside [1, KIVI_SAMPLE_MAX_V], row_stride < V or
 * target_stride < 1 (N > 1), a null logits / targets / out_logprob; KIVI_EALIGN for logits not aligned to its element, targets not
 * 8-byte aligned, an output not 4-byte aligned.
 */
int kivi_token_logprob(const void* logits, int logits_bits, int64_t row_stride, int64_t N, int V, const int64_t* targets,
                       int64_t target_stride, int64_t ignore_index, float* out_logprob, float* out_lse, int32_t* out_rank,
                       kivi_stream_t stream);
/*
 * kivi_token_top_logprobs: the k most likely tokens of every row of (N, V) logits with their log-probabilities, and -- with
 * targets -- everything kivi_token_logprob gives, in one launch (the `logprobs` / `top_logprobs=k` pair of a serving interface;
 * DESIGN.md section 23).  Per row r, with x_j = float(logit[r, j]):
 *   m, S and lse are those of kivi_token_logprob; with targets, out_logprob / out_lse / out_rank follow its rules (ignore_index,
 *   targets out of range, -inf) and hold the same bits as it writes for the same row.
 *   Order: token j comes before j' iff x_j > x_j', or x_j == x_j' and j < j' (the order out_rank counts in; -0 and +0 tie).
 *   out_top_ids[r * top_stride + i] = the token of rank i, out_top_logprobs[r * top_stride + i] = x_id - lse, for i in [0, k);
 *   an entry on a -inf logit is exactly -inf.  So out_top_ids[r, 0] is the row's argmax, and a scored target of rank < k has
 *   out_top_ids[r, rank] == t and out_top_logprobs[r, rank] bit-identical to out_logprob[r].
 *   targets     int64 or null; null: out_logprob and out_rank must be null (out_lse may be given).  A row whose target is ignored
 *               or out of range still gets its list.
 *   out_top_ids int64, out_top_logprobs fp32: k entries per row, rows top_stride elements apart; nothing else is written
 * A row that is all -inf or holds NaN / +inf gets some value.  The same row gives the same bits strided or contiguous, at any
 * element alignment, eager or replayed: integer LDS atomics only, every output element written by one lane.
 * One 1024-thread workgroup per row, rows taken grid-stride; the row is read 3 (fp16, bf16) or 4 (fp32) times, 2 more when the tie class
 * at the k-th place straddles the cut.
 * KIVI_EINVAL (nothing enqueued) for every case of kivi_token_logprob (targets only when given), k outside
 * [1, min(V, KIVI_TOP_LOGPROBS_MAX)], top_stride < k (N > 1), a null out_top_ids / out_top_logprobs, out_logprob or out_rank
 * without targets, targets without out_logprob; KIVI_EALIGN as there, and for out_top_ids off 8 bytes or out_top_logprobs off 4.
 */
#define KIVI_TOP_LOGPROBS_MAX 32
int kivi_token_top_logprobs(const void* logits, int logits_bits, int64_t row_stride, int64_t N, int V, int k,
                            const int64_t* targets, int64_t target_stride, int64_t ignore_index, int64_t* out_top_ids,
                            float* out_top_logprobs, int64_t top_stride, float* out_logprob, float* out_lse, int32_t* out_rank,
                            kivi_stream_t stream);
/*
 * kivi_prefill_attention: the attention of a prompt pass over fp16 q / k / v -- causal, grouped-query, with leading pads per batch
 * row (the reference's prompt pass, models/llama_kivi.py:401-452, without the repeat_kv copies and without a
 * (B, 1, T, T) mask).  q and out are (B, nh, T, D), k and v (B, nh_kv, T, D) fp16, each by its strides (batch, head, token) in
 * elements, channel stride 1: the transposed views of (B, T, heads, D) projections go in as they are, and out may be laid out
 * (B, T, nh * D).  Query head h reads kv head h / (nh / nh_kv) (quant/csrc/gemv_cuda.cu:361-365).
 *   lead   device memory, one int32 per batch row: the number of leading masked tokens, clamped to [0, T] on the device and never
 *          read on the host; null: no pads
 *   for a query i >= lead[b]:  out[b, h, i, :] = softmax_j(scale * q_i . k_j) v_j over the keys j in [lead[b], i]
 *   for a query i <  lead[b] (a pad): exact zeros
 * Arithmetic: q k^T on v_mfma_f32_16x16x32_f16 with fp32 accumulation; scale and an online softmax in fp32 (exp2); the
 * probabilities rounded to fp16 for the product with v (fp32 accumulation); one division by the fp32 sum and one rounding to fp16 at
 * the end.  Inputs are finite by contract.  One launch, no workspace, every output element written once.
 * KIVI_EINVAL (nothing enqueued) for D != 128; B, nh, nh_kv or T < 1; nh not a multiple of nh_kv; nh / nh_kv outside {1, 2, 4, 8};
 * a null q / k / v / out; a scale that is not finite and positive; a grid of 2^31 blocks or more (B * nh * ceil(T / 128)).
 * KIVI_EALIGN for a base pointer or a stride that is not a multiple of 16 bytes, or lead off 4 bytes.
 */
int kivi_prefill_attention(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_st, const void* k, int64_t k_sb, int64_t k_sh,
                           int64_t k_st, const void* v, int64_t v_sb, int64_t v_sh, int64_t v_st, void* out, int64_t o_sb,
                           int64_t o_sh, int64_t o_st, const int32_t* lead, int B, int nh, int nh_kv, int T, int D, float scale,
                           kivi_stream_t stream);
/*
 * kivi_qk_rope: a layer's q and k projections made ready for the attention in one launch -- the optional
 * per-head RMSNorm (HF's Qwen3RMSNorm), the rotary embedding, and the placement into the head-major layout, the nh / nh_kv = R query
 * heads of every kv head padded to Rp >= R by zero heads (a group of R heads then runs as the matrix-pipe layout's ratio Rp).
 *   q_in   (B, Q, nh, D), k_in (B, Q, nh_kv, D) fp16 by their strides (batch, token, head) in elements, channel stride 1: the views of
 *          the projections' outputs go in as they are
 *   cos, sin   (Bc, Q, D) fp16 tables, batch stride cs_sb (0: one table for every row) and token stride cs_st in elements
 *   q_weight, k_weight   D fp16 each, or null: no head norm;  eps: its epsilon
 *   q_out  (B, nh_kv * Rp, Q, D), k_out (B, nh_kv, Q, D) fp16, contiguous.  Query head kv * R + r lands at kv * Rp + r; the heads
 *          kv * Rp + [R, Rp) are written as zeros on every call.  Every element of both outputs is written once, nothing else is.
 * Arithmetic, per head x (D channels): with a weight, y = fp16(w * fp16(x * rsqrt(mean(x^2) + eps))), the inner value evaluated in
 * fp64 and rounded once (HF evaluates it in fp32: about one element in a thousand then sits an fp16 ulp off this, the formula's
 * own value), else y = x; then out = fp16(fp16(y * cos) + fp16(rot(y) * sin)), rot(y)[i] = -y[i + 64], rot(y)[i + 64] = y[i] -- each
 * product and the sum rounded to fp16 on its own, which is what torch computes for `y * cos + rotate_half(y) * sin` on fp16 tensors,
 * bit for bit.  One wave per (row, token, head).
 * KIVI_EINVAL (nothing enqueued) for D != 128; B, Q, nh or nh_kv < 1; nh not a multiple of nh_kv; Rp outside [R, 64]; a null q_in /
 * k_in / cos / sin / q_out / k_out; a negative stride; eps negative or not finite; 2^31 blocks or more.  KIVI_EALIGN for a pointer
 * off 2 bytes.
 */
int kivi_qk_rope(const void* q_in, int64_t q_sb, int64_t q_st, int64_t q_sh, const void* k_in, int64_t k_sb, int64_t k_st,
                 int64_t k_sh, const void* cos, const void* sin, int64_t cs_sb, int64_t cs_st, const void* q_weight,
                 const void* k_weight, float eps, void* q_out, void* k_out, int B, int Q, int nh, int nh_kv, int Rp, int D,
                 kivi_stream_t stream);
/*
 * kivi_qkv_rope_bf16: the way into the fp16 attention for a model whose dense layers run in bf16 -- what
 * kivi_qk_rope does to q and k, and the placement of v, from bf16 projections to fp16 tensors in one launch.
 *   q_in   (B, Q, nh, D), k_in, v_in (B, Q, nh_kv, D) bf16 by their strides (batch, token, head) in elements, channel stride 1
 *   cos, sin   (Bc, Q, D) FP32 tables, batch stride cs_sb (0: one table for every row) and token stride cs_st in elements
 *   q_weight, k_weight   D bf16 each, or null: no head norm;  eps: its epsilon
 *   q_out  (B, nh_kv * Rp, Q, D), k_out, v_out (B, nh_kv, Q, D) fp16, contiguous.  Query head kv * R + r lands at kv * Rp + r; the
 *          heads kv * Rp + [R, Rp) are written as zeros on every call.  Every element of the three outputs is written once, nothing
 *          else is.
 * Arithmetic, with every input taken as the exact number it holds: with a weight, y = w * x * rsqrt(mean(x^2) + eps), else y = x;
 * out = y * cos + rot(y) * sin, rot(y)[i] = -y[i + 64], rot(y)[i + 64] = y[i]; the whole expression is evaluated in fp64 and rounded
 * ONCE, to fp16 (round to nearest even): each element is the fp16 neighbour of the formula's value, whatever the order of the
 * reduction.  v_out = fp16(v_in), round to nearest even.  A finite result beyond +-65504 is stored as +-65504; NaN stays NaN.
 * (Not the operation sequence of a bf16 torch model, which rounds to bf16 after every step: nothing downstream is bf16.)
 * One wave per (row, token, head slot); no LDS, no scratch.
 * KIVI_EINVAL (nothing enqueued) for D != 128; B, Q, nh or nh_kv < 1; nh not a multiple of nh_kv; Rp outside [R, 64]; a null q_in /
 * k_in / v_in / cos / sin / q_out / k_out / v_out; a negative stride; eps negative or not finite; 2^31 blocks or more.  KIVI_EALIGN
 * for a 2-byte pointer off 2 bytes, cos or sin off 4.
 */
int kivi_qkv_rope_bf16(const void* q_in, int64_t q_sb, int64_t q_st, int64_t q_sh, const void* k_in, int64_t k_sb, int64_t k_st,
                       int64_t k_sh, const void* v_in, int64_t v_sb, int64_t v_st, int64_t v_sh, const void* cos, const void* sin,
                       int64_t cs_sb, int64_t cs_st, const void* q_weight, const void* k_weight, float eps, void* q_out, void* k_out,
                       void* v_out, int B, int Q, int nh, int nh_kv, int Rp, int D, kivi_stream_t stream);
/*
 * The sparse mixture-of-experts feed-forward block (Mixtral, Qwen3-MoE).  Two entries, both launches only --
 * no host read, no copy to the host -- so a stream capture may hold them.  N tokens, E experts, K = top_k experts per token; pair
 * n * K + k is slot k of token n.  `dtype`: 16 (fp16) or KIVI_LOGITS_BF16 (bf16).
 *
 * kivi_moe_route
 *   logits   (N, E) in the dtype, row n at logits + n * row_stride elements
 *   flags    KIVI_MOE_NORM_TOPK: the K weights of a token are divided by their sum; KIVI_MOE_ROUND_WEIGHTS: see w
 *   idx      (N, K) int32: the K largest LOGITS of the row, descending, equal logits (-0 equals +0) to the lower expert
 *   w        (N, K) fp32: softmax over all E logits in fp32 (max subtracted, expf, one division by the sum) taken at idx; with
 *            NORM_TOPK divided by the sum of the K, added in slot order; with ROUND_WEIGHTS rounded once to the dtype and stored as
 *            that value's fp32 image (HF's Qwen3-MoE router casts the weights to the model dtype, Mixtral's does not)
 *   counts   (E) int32 pairs per expert;  offsets (E + 1) their exclusive prefix sum
 *   pairs    (N * K) int32 pair ids grouped by expert: expert e owns pairs[offsets[e] .. offsets[e + 1]), in no specified order
 *   pos      (N, K) int32: pairs[pos[n, k]] == n * K + k
 *   tiles    (kivi_moe_max_tiles(N, E, K), 3) int32 (expert, first row of `pairs`, rows <= KIVI_MOE_TOKEN_TILE): every expert's
 *            segment cut into tiles, experts ascending; n_tiles: one int32, the number of entries written
 * The host never learns the counts: kivi_moe_max_tiles = min(E, N * K) + N * K / KIVI_MOE_TOKEN_TILE bounds the tile count.
 *
 * kivi_moe_experts
 *   x        (N, H) in the dtype, row stride x_stride elements (a multiple of 8), 16-byte aligned
 *   w, pairs, pos, tiles, n_tiles   as kivi_moe_route left them for the same N, E, K
 *   gate_up  (E, 2 I, H) contiguous, rows [0, I) of an expert its gate matrix, [I, 2 I) its up matrix;  down (E, H, I) contiguous
 *   out      (N, H) in the dtype, row stride out_stride elements (a multiple of 4), 8-byte aligned; every element written once
 *   workspace   kivi_moe_workspace_bytes(N, H, I, E, K) bytes, 16-byte aligned
 * a = silu(x Wg^T) * (x Wu^T) per pair on the matrix pipe (fp32 accumulation), rounded once to the dtype; y = a Wd^T in fp32;
 * out[n] = sum_k w[n, k] * y[pair n * K + k], fused multiply-adds in slot order k = 0 .. K - 1, rounded once.  No atomics on
 * floating-point values.  The order in which a pair's sums are taken depends on H and I only: a token's output bits do not depend
 * on N, on the other tokens or on where the plan put the pair.
 *
 * KIVI_EINVAL (nothing enqueued) for a dtype that is neither; N < 1; E outside [1, 256]; top_k outside [1, min(E, 16)];
 * N * top_k >= 2^31; H or I not a positive multiple of 32 (or beyond 16 * 65535); unknown flags; a row stride smaller than the row;
 * a null pointer; a workspace smaller than kivi_moe_workspace_bytes.  KIVI_EALIGN for a misaligned pointer or stride.
 * kivi_moe_max_tiles / kivi_moe_workspace_bytes return KIVI_EINVAL (-1) for the same shapes.
 */
#define KIVI_MOE_TOKEN_TILE 16
#define KIVI_MOE_NORM_TOPK 1
#define KIVI_MOE_ROUND_WEIGHTS 2
int kivi_moe_max_tiles(int N, int E, int top_k);
int64_t kivi_moe_workspace_bytes(int N, int H, int I, int E, int top_k);
int kivi_moe_route(const void* logits, int64_t row_stride, int dtype, int N, int E, int top_k, int flags, void* idx, void* w,
                   void* counts, void* offsets, void* pairs, void* pos, void* tiles, void* n_tiles, kivi_stream_t stream);
int kivi_moe_experts(const void* x, int64_t x_stride, int dtype, int N, int H, int I, int E, int top_k, const void* w,
                     const void* pairs, const void* pos, const void* tiles, const void* n_tiles, const void* gate_up,
                     const void* down, void* out, int64_t out_stride, void* workspace, int64_t workspace_bytes,
                     kivi_stream_t stream);
/*
 * kivi_moe_experts_w8: kivi_moe_experts over experts held in the fine-grained FP8 format of section 35, as a
 * checkpoint stacks them.  Three launches (gate/up, down, combine), nothing read back.
 *   gate_up        (E, 2 I, H) row-major, one OCP e4m3fn byte per element, no NaN byte; gate rows [0, I), up rows [I, 2 I)
 *   gate_up_scale  (E, 2 I / 128, H / 128) fp32, the factor one MULTIPLIES by (`gate_up_proj_scale_inv`)
 *   down           (E, H, I) bytes;   down_scale  (E, H / 128, I / 128) fp32
 *   every other argument as kivi_moe_experts; the plan is kivi_moe_route's, the workspace kivi_moe_workspace_bytes's.
 * The represented weight is the real number e4m3(byte) * scale[row / 128, col / 128]; the result is kivi_moe_experts' contract over
 * those weights: x stays 16-bit, fp32 accumulation (per 128-element stretch on the matrix pipe, then one fused multiply-add by the
 * block's scale), silu(g) * u rounded once to the dtype, the pair outputs combined in slot order and rounded once.  A token's bits
 * depend on H and I only.  No atomics.
 * KIVI_EINVAL / KIVI_EALIGN as kivi_moe_experts, and KIVI_EINVAL for H or I not a positive multiple of 128 or a null scale pointer,
 * KIVI_EALIGN for a scale pointer off 4 bytes.
 */
int kivi_moe_experts_w8(const void* x, int64_t x_stride, int dtype, int N, int H, int I, int E, int top_k, const void* w,
                        const void* pairs, const void* pos, const void* tiles, const void* n_tiles, const void* gate_up,
                        const void* gate_up_scale, const void* down, const void* down_scale, void* out, int64_t out_stride,
                        void* workspace, int64_t workspace_bytes, kivi_stream_t stream);
/*
 * Weight-only 4-bit dense layers.  A weight W (O, K) is quantised in groups of G in {64, 128} along K:
 * codes, scale and mn are exactly what the reference's last-dim quantiser (quant/new_pack.py:217-252 at 4 bits; kivi_quant.h) gives
 * for the FP16 IMAGE of W viewed as (1, 1, O, K) -- a bf16 weight is rounded once to fp16 first --, degenerate groups (constant,
 * inf, NaN) resolving as kivi_quant.h documents; scale and mn are fp16 for fp16 and bf16 models alike.  The represented weight is the
 * real number W~[o, k] = code * scale + mn.  `dtype`: 16 (fp16) or KIVI_LOGITS_BF16 (bf16).
 *
 * Layout "WT4" (kivi_amd/csrc/kivi_mfma_layout.h): tiles of 16 rows x 128 reduction elements, 256 int32 words each, the K / 128
 * tiles of a 16-row stripe contiguous.  Element (o, k): tile (o / 16) * (K / 128) + k / 128, and with kk = k % 128 word
 * ((o % 16) + 16 * ((kk >> 3) & 3)) * 4 + (kk >> 5) of the tile, bits 4 * ((k & 7) >> 1) + 16 * (k & 1).
 *   qweight  O * K / 8 int32;   scales, mins  O * K / G halves each: (row o, group g) at ((o / 16) * (K / G) + g) * 16 + o % 16
 *
 * kivi_w4_pack      w (O, K) in the dtype, row stride w_stride elements -> qweight, scales, mins.  W is read once.
 * kivi_w4_dequant   out[o, k] = round_to_dtype(fmaf(code, scale, mn)), the fused multiply-add in fp32; row stride out_stride
 * kivi_w4_linear    y[n, o] = sum_k x[n, k] * W~[o, k] (+ bias[o]): accumulated in fp32, rounded once to the dtype.  x (N, K) by
 *                   x_stride, y (N, O) by y_stride, bias (O) in the dtype or null.  Any N >= 1: tokens go through in chunks of 64
 *                   (kivi_w4_gate_up: of 32), one pass over the stripe's codes per chunk.
 * kivi_w4_gate_up   y[n, i] = silu(g) * u with g, u the two linears of the gate and the up matrix (I, K) in fp32, rounded once
 * Launches only: a stream capture may hold them.  The order in which a token's sums are taken depends on K and G only, not on N, on
 * the token's position or on the other tokens; no atomics.
 *
 * KIVI_EINVAL (nothing enqueued) for a dtype that is neither; O not a positive multiple of 16; K not a positive multiple of 128;
 * group not 64 or 128; N < 1 or N * O >= 2^31; a row stride smaller than the row; a null pointer (bias may be null).  KIVI_EALIGN
 * for x, w, out or qweight off 16 bytes, scales, mins or y off 8, a stride of x, w or out that is not a multiple of 8 elements,
 * of y not of 4.  kivi_w4_bytes: the bytes of the three buffers together, O * K / 2 + 4 * O * K / G (KIVI_EINVAL for such a shape).
 */
int64_t kivi_w4_bytes(int O, int K, int group);
int kivi_w4_pack(const void* w, int64_t w_stride, int dtype, int O, int K, int group, void* qweight, void* scales, void* mins,
                 kivi_stream_t stream);
int kivi_w4_dequant(const void* qweight, const void* scales, const void* mins, int O, int K, int group, int dtype, void* out,
                    int64_t out_stride, kivi_stream_t stream);
int kivi_w4_linear(const void* x, int64_t x_stride, int dtype, int N, int O, int K, int group, const void* qweight,
                   const void* scales, const void* mins, const void* bias, void* y, int64_t y_stride, kivi_stream_t stream);
int kivi_w4_gate_up(const void* x, int64_t x_stride, int dtype, int N, int I, int K, int group, const void* gate_qweight,
                    const void* gate_scales, const void* gate_mins, const void* up_qweight, const void* up_scales,
                    const void* up_mins, void* y, int64_t y_stride, kivi_stream_t stream);
/*
 * FP8 weights under 16-bit activations, W8A16.  The two buffers of a weight (O, K) are those of a fine-grained
 * FP8 checkpoint, as they are on disk: `weight` (O, K) row-major, one OCP e4m3fn byte per element, no NaN byte (0x7F, 0xFF);
 * `scale_inv` (ceil(O / 128), K / 128) fp32 row-major, the factor one MULTIPLIES by.  The represented weight is the real number
 * W~[o, k] = e4m3(weight[o, k]) * scale_inv[o / 128, k / 128].  `dtype`: 16 (fp16) or KIVI_LOGITS_BF16 (bf16).
 *
 * kivi_w8_dequant   out[o, k] = round_to_dtype(fp32(e4m3) * scale), the product rounded to fp32 first; row stride out_stride
 * kivi_w8_linear    y[n, o] = sum_k x[n, k] * W~[o, k] (+ bias[o]): x is not quantised; accumulated in fp32, rounded once to the
 *                   dtype.  x (N, K) by x_stride, y (N, O) by y_stride, bias (O) in the dtype or null.  Any N >= 1: tokens go
 *                   through in chunks of 64 (kivi_w8_gate_up: of 32), one pass over the stripe's bytes per chunk.
 * kivi_w8_gate_up   y[n, i] = silu(g) * u with g, u the two linears of the gate and the up matrix (I, K) in fp32, rounded once
 * Launches only: a stream capture may hold them.  The order in which a token's sums are taken depends on K only, not on N, on the
 * token's position or on the other tokens; no atomics.
 *
 * KIVI_EINVAL (nothing enqueued) for a dtype that is neither; O not a positive multiple of 16; K not a positive multiple of 128;
 * N < 1 or N * O >= 2^31; a row stride smaller than the row; a null pointer (bias may be null).  KIVI_EALIGN for x, out or weight
 * off 16 bytes, scale_inv off 4, y off 8, a stride of x or out that is not a multiple of 8 elements, of y not of 4.
 * kivi_w8_bytes: the bytes of the two buffers together, O * K + 4 * ceil(O / 128) * (K / 128) (KIVI_EINVAL for such a shape).
 */
int64_t kivi_w8_bytes(int O, int K);
int kivi_w8_dequant(const void* weight, const void* scale_inv, int O, int K, int dtype, void* out, int64_t out_stride,
                    kivi_stream_t stream);
int kivi_w8_linear(const void* x, int64_t x_stride, int dtype, int N, int O, int K, const void* weight, const void* scale_inv,
                   const void* bias, void* y, int64_t y_stride, kivi_stream_t stream);
int kivi_w8_gate_up(const void* x, int64_t x_stride, int dtype, int N, int I, int K, const void* gate_weight,
                    const void* gate_scale_inv, const void* up_weight, const void* up_scale_inv, void* y, int64_t y_stride,
                    kivi_stream_t stream);
/*
 * Per-request LoRA adapters: the batched low-rank side path of a linear layer, two launches, nothing read
 * back, so a stream capture may hold them.  S slots of table rank R in {8, 16, 32, 64}; A (S, R, K) and B (S, O, R) contiguous in
 * the dtype -- 16 (fp16) or KIVI_LOGITS_BF16 (bf16) --, an adapter of rank r < R in rows / columns [0, r) of its slot and zeros
 * behind them; scale (S) fp32; ranks (S) int32; slots (N / Q) int32, one per row of the pass: token n belongs to row n / Q.
 *
 * kivi_lora_shrink   t[n, j] = sum_k A[s, j, k] * x[n, k] for s = slots[n / Q] in [0, S): fp32, the order of the sum a function of
 *                    K alone.  x (N, K) by x_stride elements (a multiple of 8), 16-byte aligned; t (N, R) fp32, contiguous.
 * kivi_lora_expand   y[n, o] <- round_dtype(fmaf(scale[s], sum_j B[s, o, j] * t[n, j], y[n, o])), the sum in fp32 with j ascending,
 *                    in place.  y (N, O) by y_stride elements (even), 4-byte aligned.
 * Both walk ranks [0, ranks[s] rounded up to 8) only, and a row whose slot lies outside [0, S) -- -1 names the base model -- is
 * neither read nor written: its bytes stay.  A token's bits depend on its x, its slot and that slot's tables alone.  No atomics.
 *
 * KIVI_EINVAL (nothing enqueued) for a dtype that is neither; N < 1, Q < 1 or N not a multiple of Q; K or O not a positive multiple of
 * 8; R not one of the four; S < 1; a row stride smaller than the row; a null pointer.  KIVI_EALIGN for x, A or B off 16 bytes, an
 * x_stride that is not a multiple of 8, y off 4 bytes or an odd y_stride, slots, ranks, scale or t off 4 bytes.
 */
int kivi_lora_shrink(const void* x, int64_t x_stride, int dtype, int64_t N, int64_t Q, int K, const void* slots, int S, int R,
                     const void* ranks, const void* A, void* t, kivi_stream_t stream);
int kivi_lora_expand(const void* t, const void* slots, int S, int R, const void* ranks, const void* scale, const void* B, void* y,
                     int64_t y_stride, int dtype, int64_t N, int64_t Q, int O, kivi_stream_t stream);
/* geometry class of a step (-1: bad arguments): the super-block counts of both stores and whether the step flushes a value; the
 * launch plan (one launch / S slices / two launches) is a function of the class and of constants of the call (shape, bits, flags) */
int64_t kivi_mf_step_key(const kivi_mf_step* step, int B, int nh, int nh_kv, int residual_length, int flags);
/* lengths after the attend phase of one step (llama_kivi.py:333-336, :377, :386-399); returns 1 when the K residual is full
 * (the K flush of :343-356 is due), 0 otherwise, < 0 on inconsistent lengths.  window_rows: rows of the ring window buffer. */
int kivi_mf_step_advance(kivi_mf_step* step, int residual_length, int64_t window_rows);
/* *dev_step <- *host_step by a one-thread kernel on `stream` (the values travel as kernel arguments: the host struct may be
 * reused as soon as the call returns, nothing synchronises) */
int kivi_mf_step_upload(const kivi_mf_step* host_step, void* dev_step, kivi_stream_t stream);

/* ------------------------------------------------- tuning / bench hooks --- */

/* Kernel variants of kivi_gemv_k (same arguments + variant id; -1 = the default heuristic).
 * Used by bench.py and the parity tests to check every variant; not part of the drop-in surface. */
int kivi_gemv_k_num_variants(void);
const char* kivi_gemv_k_variant_name(int variant);
int kivi_gemv_k_variant(int variant, const void* q, int64_t q_sb, int64_t q_sh, const void* code, int64_t code_sb,
                        int64_t code_sh, int64_t code_sr, const void* scale, const void* mn, int64_t sm_sb,
                        int64_t sm_sh, int64_t sm_sr, void* out, int64_t out_sb, int64_t out_sh, int B, int nh,
                        int nh_kv, int D, int64_t T, int group_size, int bits, kivi_stream_t stream);

int kivi_gemv_v_num_variants(void);
const char* kivi_gemv_v_variant_name(int variant);
int kivi_gemv_v_variant(int variant, const void* a, int64_t a_sb, int64_t a_sh, const void* code, int64_t code_sb,
                        int64_t code_sh, int64_t code_sr, const void* scale, const void* mn, int64_t sm_sb,
                        int64_t sm_sh, int64_t sm_sr, void* out, int64_t out_sb, int64_t out_sh, int B, int nh,
                        int nh_kv, int64_t Tv, int D, int group_size, int bits, kivi_stream_t stream);

/* Per-dispatch timing: the NEXT fused-GEMV launch issued by this thread stamps `start` / `stop` (hipEvent_t
 * from kivi_event_create) with the dispatch's own begin / end (hipExtLaunchKernelGGL), i.e. what a profiler
 * reports as the kernel duration.  kivi_event_elapsed_us synchronises on `stop`. */
void* kivi_event_create(void);
void kivi_event_destroy(void* event);
void kivi_set_launch_events(void* start, void* stop);
float kivi_event_elapsed_us(void* start, void* stop);
/* source text of the kernel instantiation the last consumed event pair bracketed ("" if none yet) */
const char* kivi_last_timed_kernel(void);
/* Diagnostic, -DKIVI_TUNING builds only (the product library accepts the call and ignores it): device buffer of (blocks x 4 waves
 * x 16) uint64 that the stamping instantiations of the row kernels fill with per-wave phase time stamps (shader clock; slot 1 =
 * 100 MHz realtime at entry); null switches it off (default). */
void kivi_debug_set_stamps(void* device_buffer);

#ifdef __cplusplus
}
#endif
#endif /* KIVI_HIP_H */
