"""GPU: decode steps under LONG left pads against the fp64 reference.

A short prompt admitted into a living cache of length L (continuous batching) decodes with its first L - len(prompt) keys masked at
the fp16 minimum.  With L in the thousands the mask covers whole 512-token super-blocks, whole slices of the sliced one-launch form,
often the whole packed K and V stores -- mask code that the 7-to-9-key pads of the other stage tests never reach (the statistics of a
segment whose every score sits at the clamp, the (M, L) exchange of a slice with only masked keys, pass A of the three-pass softmax,
p'' placed by a maximum that comes from the fp16 residual alone, partial outputs of exactly zero meeting in the workspace).  The twelve
patterns of tests/longpad_masks.py, one per batch row, at every step across one K flush:

Matrix-pipe layout (`_longpad_stages`; forms "row", "split" and the sliced one-launch form), against tests/torch_ref64.py on the GPU:
  A. the rows the softmax consumed (KIVI_GQA_DUMP_SCORES) at the GEMV bar 1e-3 + 1 ulp on live keys.  Dead positions are filled ON BOTH
     SIDES with the reference's row of the same step WITHOUT the mask -- not with zeros: the bar is rtol * max(|ref|, rms(row)), the
     GEMV's rounding error scales with the row's data and not with its mask, and a row with one or two live keys among zeros would lose
     the rms term.  Dead keys themselves: at most -60000 and within 32 (the spacing of that binade) of the reference's.
  B. the output at 2e-3 + 1 ulp of the reference's attend half run on the GPU's own rows.
  The product instantiation (a clone without the dump flag) gives the same bits at every step and the same state at the end; the
  9-tuple is bit-identical to the reference's at step 0, at the K flush, after it and at the end; the patterns keep their meaning
  (longpad_masks.assert_patterns on the reference's rows).

Hook-state layout (no score dump): end to end per row at the allowance of test_extend_stages_gpu._e2e_rows, against the composed
path at 2e-3 + 1 ulp, 9-tuples bit-identical."""
import pytest
import torch

import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from longpad_masks import ROWS, assert_patterns, longpad_mask
from test_extend_gpu import _assert_same_state
from test_extend_stages_gpu import _e2e_rows

pytestmark = pytest.mark.gpu
D, G32 = 128, 32


def _same_tuple(layer, past, what):
    t = layer.as_tuple()
    for i, (a, b) in enumerate(zip(t[:8], past[:8])):
        if b is None:
            assert a is None or a.numel() == 0, (what, "9-tuple member", i)
        else:
            assert a is not None and same_bits(a, b), (what, "9-tuple member", i)
    assert t[8] == past[8], what


def _lengths(past, bits):
    """Packed K / V lengths of a reference 9-tuple."""
    return (0 if past[0] is None else past[0].shape[-1] * (32 // bits)), (0 if past[4] is None else past[4].shape[2])


def _longpad_stages(nh, nh_kv, T0, R, kind, bits, form):
    from kivi_amd import _lib
    from kivi_amd.attention import KiviConfig, KiviLayerCacheMF, kivi_attention_decode, make_layer_cache
    B = ROWS
    steps = (R - T0 % R) + 3                    # exactly one K flush (at step index steps - 4) and three steps after it
    flush = steps - 4
    cfg = KiviConfig(bits, bits, G32, R)
    k0, v0 = make_kv(1, B, nh_kv, T0, D, kind).cuda(), make_kv(2, B, nh_kv, T0, D).cuda()
    layer = make_layer_cache(cfg, B, nh_kv, D, T0 + 8, "cuda", num_heads=nh)     # small capacity: the cache must grow
    assert isinstance(layer, KiviLayerCacheMF)
    if form.startswith("slices"):
        forced = _lib.gqa_slices(int(form[6:]))
    else:
        forced = _lib.GQA_FORCE_SPLIT if form == "split" else _lib.GQA_FORCE_ROW
    # (the two-launch form keeps its score rows in memory: nothing to dump)
    layer.flags = forced if form == "split" else forced | _lib.GQA_DUMP_SCORES
    layer.prefill(k0, v0)
    product = layer.clone()
    product.flags = forced
    if form.startswith("slices"):
        plan = _lib.load().kivi_mf_launch_plan(B, nh, nh_kv, layer.k_quant_len, layer.k_res_len, R, layer.flags, bits, 0)
        assert plan == int(form[6:]), ("the shape must take the sliced form from the first step on", plan)
    past = T64.prefill_cache(k0, v0, bits, bits, G32, R)
    _same_tuple(layer, past, "after the prompt pass")
    worst_a = worst_b = 0.0
    for s in range(steps):
        q = make_kv(100 + s, B, nh, 1, D).cuda()
        kn, vn = make_kv(200 + s, B, nh_kv, 1, D, kind).cuda(), make_kv(300 + s, B, nh_kv, 1, D).cuda()
        n = T0 + s + 1
        Tq, Tv = _lengths(past, bits)
        mask = longpad_mask(n, Tq, Tv, "cuda")
        layer.ensure_room(1)
        layer._desc(nh, q.device)[4][0].fill_(float("nan"))          # the scratch rows of this step (a stale row must not pass)
        out = kivi_attention_decode(q, kn, vn, layer, attention_mask=mask)
        x_gpu = layer._native[4][0][:B, :nh, :, :n].clone()           # the rows the softmax / the sV launch consumed
        out_p = kivi_attention_decode(q, kn, vn, product, attention_mask=mask)
        assert torch.isfinite(out).all(), s
        assert same_bits(out, out_p), ("the product instantiation differs from the dumped one", s)
        ref, new_past, pre = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, attention_mask=mask)
        _, _, pre0 = T64.decode_step(q, kn, vn, past, bits, bits, G32, R)
        count = assert_patterns(pre, ref, Tq, what=(form, s))
        assert bool((count[5] == n - Tq).all()), (s, "row 5: the fp16 residual and the new token")
        # A: the rows the softmax consumed
        assert not torch.isnan(x_gpu).any(), ("a key of the row was not written", s)
        live = pre.float() > -60000
        ok, ra = gemv_close(torch.where(live, x_gpu, pre0), torch.where(live, pre, pre0), rtol=1e-3, ulps=1)
        assert ok, ("stage A", s, ra)
        xd, pd = x_gpu.float()[~live], pre.float()[~live]
        assert bool((xd <= -60000).all()) and bool(((xd - pd).abs() <= 32).all()), ("masked keys", s)
        # B: the attend half on the kernel's own rows
        ref_b, _, _ = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, attention_mask=mask, scores_override=x_gpu)
        ok, rb = gemv_close(out, ref_b, rtol=2e-3, ulps=1)
        assert ok, ("stage B", s, rb)
        worst_a, worst_b = max(worst_a, ra), max(worst_b, rb)
        past = new_past
        if s == flush:
            assert _lengths(past, bits)[0] == Tq + R, "the K flush"
        if s in (0, flush, flush + 1, steps - 1):
            _same_tuple(layer, past, ("step", s))
    assert layer.k_res_len == 3
    _assert_same_state(layer, product)
    print(f"long pads {form} {nh}/{nh_kv} T0={T0} R={R} {kind} {bits}-bit: worst ratio: scores {worst_a:.3f} of 1e-3+1ulp, "
          f"attend {worst_b:.3f} of 2e-3+1ulp over {steps} steps")


@pytest.mark.parametrize("form", ["row", "split"])
@pytest.mark.parametrize("nh,nh_kv,T0,R,kind,bits", [(4, 4, 1100, 32, "randn", 2), (4, 4, 1100, 64, "outlier", 2),
                                                      (8, 2, 1100, 128, "outlier", 2), (16, 2, 1100, 32, "randn", 2),
                                                      (8, 2, 1100, 32, "outlier", 4), (4, 4, 1100, 32, "randn", 4)])
def test_mf_long_pads_match_reference(nh, nh_kv, T0, R, kind, bits, form):
    """Two whole super-blocks and a partial one under the twelve patterns: the one-launch row kernels (mf_row_kernel: pass A of the
    three-pass softmax rewrites the row with the mask; mf_row4_kernel for nh / nh_kv = 4 and 8) and the two-launch form (mf_k_kernel's
    per-segment statistics, mf_v_kernel's partial sums in the workspace)."""
    _longpad_stages(nh, nh_kv, T0, R, kind, bits, form)


@pytest.mark.parametrize("nh,nh_kv,T0,R,kind,bits,S", [(8, 2, 1100, 128, "outlier", 2, 2), (8, 2, 1100, 96, "randn", 2, 3),
                                                        (16, 2, 2100, 32, "outlier", 2, 4), (4, 4, 1100, 32, "outlier", 2, 2),
                                                        (8, 2, 1100, 128, "outlier", 4, 2)])
def test_mf_sliced_long_pads_match_reference(nh, nh_kv, T0, R, kind, bits, S):
    """The shapes of test_mf_sliced_rows_match_reference_logic (the launch plan returns S for them): slices whose every key is masked,
    empty slices, the (max, sum exp) exchange with a partner at the clamp."""
    _longpad_stages(nh, nh_kv, T0, R, kind, bits, f"slices{S}")


@pytest.mark.parametrize("nh,nh_kv,T0,rows", [(4, 4, 1100, None), (8, 2, 1100, None), (8, 2, 2100, [0, 4, 8])],
                         ids=["decode_row", "row_softmax_shared_unpack", "few_units_split_rows"])
def test_hook_state_long_pads_match_reference(nh, nh_kv, T0, rows):
    """The hook-state layout end to end (it has no score dump): (4, 4) the one-launch decode_row_kernel, (8, 2) the row-softmax launch
    plus the shared-unpack sV, and at T0 = 2100 with three batch rows (patterns 0, 4, 8) the form with the fewest units, rows split
    over blocks that meet in the workspace as in test_long_context_small_batch_split_rows."""
    from kivi_amd.attention import KiviConfig, KiviLayerCache, kivi_attention_decode
    bits, R, steps = 2, 32, 8
    B = ROWS if rows is None else len(rows)
    cfg = KiviConfig(bits, bits, G32, R)
    k0, v0 = make_kv(1, B, nh_kv, T0, D).cuda(), make_kv(2, B, nh_kv, T0, D).cuda()
    layer = KiviLayerCache(cfg, B, nh_kv, D, T0 + 16, "cuda")
    layer.prefill(k0, v0)
    composed = layer.clone()
    past = T64.prefill_cache(k0, v0, bits, bits, G32, R)
    worst_e = worst_a = worst_c = 0.0
    for s in range(steps):
        q, kn, vn = make_kv(100 + s, B, nh, 1, D).cuda(), make_kv(200 + s, B, nh_kv, 1, D).cuda(), make_kv(300 + s, B, nh_kv, 1, D).cuda()
        n = T0 + s + 1
        Tq, Tv = _lengths(past, bits)
        mask = longpad_mask(n, Tq, Tv, "cuda", rows)
        out = kivi_attention_decode(q, kn, vn, layer, attention_mask=mask)
        assert not getattr(layer, "_attend_unfusable", False) and not getattr(layer, "_fused_unsupported", False)
        assert torch.isfinite(out).all(), s
        ref, past, pre = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, attention_mask=mask)
        assert_patterns(pre, ref, Tq, rows, what=("hook-state", s))
        _, re_ = gemv_close(out, ref, rtol=3e-3, ulps=1)              # reported (and logged) against the plain bar, asserted per row below
        ratio, allow = _e2e_rows(out, ref, pre, torch.ones((1, n), dtype=torch.bool))
        worst_e, worst_a = max(worst_e, re_), max(worst_a, (ratio / allow).max().item())
        assert bool((ratio <= allow).all()), ("end to end", s, re_, (ratio / allow).max().item())
        out_c = kivi_attention_decode(q, kn, vn, composed, attention_mask=mask, fused_kernels=False)
        ok, rc = gemv_close(out, out_c, rtol=2e-3, ulps=1)
        assert ok, ("fused against composed", s, rc)
        worst_c = max(worst_c, rc)
    _same_tuple(layer, past, "fused, last step")
    _same_tuple(composed, past, "composed, last step")
    print(f"long pads hook-state {nh}/{nh_kv} T0={T0}: worst end to end {worst_e:.3f} of 3e-3+1ulp ({worst_a:.3f} of the allowance), "
          f"fused against composed {worst_c:.3f} of 2e-3+1ulp")
