"""GPU: decode steps that skip every row's leading pads.

1. Stages under a lead: the procedure of test_longpad_gpu._longpad_stages (the twelve patterns of longpad_masks.longpad_mask, every
   step across one K flush, the fp64 reference of tests/torch_ref64.py) with the lead passed beside the mask -- pattern rows 1-9 their
   pad clamped to n - 1, rows 0, 10 and 11 zero -- on the one-launch row kernels.  Bars as there: stage A 1e-3 + 1 ulp on live keys,
   dead keys <= -60000 and within 32 of the reference's, stage B 2e-3 + 1 ulp on the kernel's own rows, 9-tuple bit-identical at
   step 0, at the flush, after it and at the end, product instantiation bit-identical to the dumped one.  A clone stepped with the mask
   alone beside it: dumped rows bit-identical from the lead on and exactly -65504 in every whole super-block under it, the state
   bit-identical, the outputs within 1.5e-3 + 1 ulp (section 9's bar for two launch forms of one step: the V walk is divided again,
   which regroups fp32 partial sums).
2. The skip really skips: every word of the whole K and V super-blocks under a row's lead overwritten with a NaN pattern -- the lead
   form gives finite outputs, bit-identical to its outputs over the clean cache (with the mask alone the NaNs reach the output).
3. Forms that ignore the lead ("split", "slices2"): outputs and state bit-identical to the same form without it.
4. Graph: a decode_graphed run with the option on whose mask rows and lead are rewritten in place partway (row 1: lead 0 -> 600)
   equals the eager steps bit for bit, with one capture.
5. Model and scheduler on the tiny test model, prompts of 9 / 600 / 1200 tokens: d1 = max |on - off| over all logits of the prompt
   pass and 16 teacher-forced steps against d0 = max |off - off_split| (the two-launch form the project already ships for the same
   arithmetic): d1 <= 2 d0, both maxima of the same kind of regrouping error over a few thousand logits.  generate_continuous with
   the option on equals its restated policy with the option on, graphed equals eager.
"""
import pytest
import torch

import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from longpad_masks import ROWS, SB, assert_patterns, longpad_mask
from test_extend_gpu import _assert_same_state, _model
from test_longpad_gpu import _lengths, _same_tuple

pytestmark = pytest.mark.gpu
D, G32 = 128, 32
FMIN_BITS = 0xFBFF - 0x10000            # fp16 -65504 as int16
NAN_WORD = 0x7FC07FC0


def longpad_lead(n, Tq, Tv, device="cuda"):
    """(12,) int32: the lead of every pattern row of longpad_mask(n, Tq, Tv) -- rows 1-9 their pad clamped to n - 1, the control row and
    the two rows whose mask is no leading pad (10, 11) zero."""
    pads = {1: SB, 2: SB + 1, 3: SB - 1, 4: (Tq // SB) * SB, 5: Tq, 6: max(Tq, Tv) + 1, 7: n - 2, 8: n - 1, 9: 700}
    lead = [0] * ROWS
    for b, p in pads.items():
        lead[b] = max(0, min(p, n - 1))
    return torch.tensor(lead, dtype=torch.int32, device=device)


def _forced(form):
    from kivi_amd import _lib
    if form.startswith("slices"):
        return _lib.gqa_slices(int(form[6:]))
    return _lib.GQA_FORCE_SPLIT if form == "split" else _lib.GQA_FORCE_ROW


def _step_inputs(s, B, nh, nh_kv, kind):
    return (make_kv(100 + s, B, nh, 1, D).cuda(), make_kv(200 + s, B, nh_kv, 1, D, kind).cuda(), make_kv(300 + s, B, nh_kv, 1, D).cuda())


def _dumped(layer, B, nh, n):
    return layer._native[4][0][:B, :nh, :, :n].clone()


# ------------------------------------------------------------------ 1. stages under a lead
def _longpad_patterns(n, Tq, Tv):
    return longpad_mask(n, Tq, Tv, "cuda"), longpad_lead(n, Tq, Tv)


def _longpad_check(pre, ref, n, Tq, lead, s):
    count = assert_patterns(pre, ref, Tq, what=("lead", s))
    assert bool((count[5] == n - Tq).all()), (s, "row 5: the fp16 residual and the new token")


def _cuda_kv(seed, heads, T, kind="randn"):
    return make_kv(seed, ROWS, heads, T, D, kind).cuda()


def _poison_under(layer, lead, Tq, Tv):
    """Every word of the whole K and V super-blocks under each row's lead overwritten with a NaN pattern, through the cache's own
    stores.  Returns the number of words written."""
    words = 0
    for b, p in enumerate(lead.tolist()):
        for store, T in ((layer.kt, Tq), (layer.vt, Tv)):
            nsb = min(p, T) // SB
            store[b, :, :nsb] = NAN_WORD
            words += store[b, :, :nsb].numel()
    return words


def _template_args(name):
    """("mf_row_kernel", ["8", "8", "8", "false", "true", "2", "2", "true"]) of the launch probe's "(mf_row_kernel<8, 8, ...>)"."""
    name = name.strip("() ")
    kernel, _, rest = name.partition("<")
    return kernel.strip(), [a.strip() for a in rest.rstrip("> ").split(",")] if rest else []


def lead_stages(nh, nh_kv, T0, R, kind, bits, patterns=_longpad_patterns, check=_longpad_check, draw=_cuda_kv, what="decode lead row",
                split_control=False, poison=False, expect=None):
    """The stage loop under a lead, every step across one K flush (the module's docstring, 1.).  `patterns(n, Tq, Tv)` -> (mask, lead)
    of a step, `check(pre, ref, n, Tq, lead, s)` the patterns' own assertions on the reference's rows, `draw(seed, heads, T, kind)` the
    inputs (on the GPU; the reference is built from the same tensors).  On top of it, for tests/test_decode_lead_long_gpu.py:
    `split_control` -- the two-launch form with the mask alone against the row form with the mask alone, inside the bar the lead is held
    to against the mask alone (two forms that shipped before the lead: an input where they miss it is a badly chosen input);
    `poison` -- at step 0 a clone whose whole super-blocks under each lead hold NaNs gives finite, bit-identical outputs;
    `expect` -- (kernel, template arguments with None for "any") of the instantiation the launch probe must name at every step.
    Returns the worst ratios (stage A, stage B, against the mask alone, split against row)."""
    from kivi_amd import _lib
    from kivi_amd.attention import KiviConfig, KiviLayerCacheMF, kivi_attention_decode, make_layer_cache
    B = ROWS
    steps = (R - T0 % R) + 3                    # exactly one K flush (at step index steps - 4) and three steps after it
    flush = steps - 4
    cfg = KiviConfig(bits, bits, G32, R)
    k0, v0 = draw(1, nh_kv, T0, kind), draw(2, nh_kv, T0)
    layer = make_layer_cache(cfg, B, nh_kv, D, T0 + 8, "cuda", num_heads=nh)     # small capacity: the cache must grow
    assert isinstance(layer, KiviLayerCacheMF)
    forced = _forced("row")
    layer.flags = forced | _lib.GQA_DUMP_SCORES
    layer.prefill(k0, v0)
    assert _lib.load().kivi_mf_launch_plan(B, nh, nh_kv, layer.k_quant_len, layer.k_res_len, R, layer.flags, bits, 0) == 1
    product, plain = layer.clone(), layer.clone()        # the lead without the dump flag; the mask alone (dumped)
    product.flags = forced
    split = None
    if split_control:
        split = layer.clone()
        split.flags = _forced("split")
    probe = None
    if expect is not None:
        from test_fullsize_gpu import LaunchProbe
        probe = LaunchProbe()
    past = T64.prefill_cache(k0, v0, bits, bits, G32, R)
    del k0, v0
    _same_tuple(layer, past, "after the prompt pass")
    worst_a = worst_b = worst_m = worst_c = 0.0
    keys = torch.arange(T0 + steps + 1, device="cuda")
    for s in range(steps):
        q, kn, vn = draw(100 + s, nh, 1), draw(200 + s, nh_kv, 1, kind), draw(300 + s, nh_kv, 1)
        n = T0 + s + 1
        Tq, Tv = _lengths(past, bits)
        mask, lead = patterns(n, Tq, Tv)
        for c in (layer, plain):
            c.ensure_room(1)
        poisoned = None
        if poison and s == 0:
            poisoned = product.clone()
            assert _poison_under(poisoned, lead, Tq, Tv) > 0
        layer._desc(nh, q.device)[4][0].fill_(float("nan"))          # the scratch rows of this step (a stale row must not pass)
        out = kivi_attention_decode(q, kn, vn, layer, attention_mask=mask, lead=lead)
        x_gpu = _dumped(layer, B, nh, n)                              # the rows the softmax consumed
        if probe is not None:
            probe.arm()
        out_p = kivi_attention_decode(q, kn, vn, product, attention_mask=mask, lead=lead)
        if probe is not None:
            kernel, args = _template_args(probe.kernel())
            want = [None if a is None else str(a).lower() for a in expect[1]]
            assert kernel == expect[0] and len(args) == len(want) and all(w is None or w == a for w, a in zip(want, args)), \
                ("the instantiation that ran", s, kernel, args, expect)
        assert torch.isfinite(out).all(), s
        assert same_bits(out, out_p), ("the product instantiation differs from the dumped one", s)
        if poisoned is not None:
            out_n = kivi_attention_decode(q, kn, vn, poisoned, attention_mask=mask, lead=lead)
            assert bool(torch.isfinite(out_n).all()), "a poisoned super-block under the lead reached the output"
            assert same_bits(out_n, out_p), "the poisoned cache's output differs from the clean one's"
            del poisoned, out_n
        plain._desc(nh, q.device)[4][0].fill_(float("nan"))
        out_m = kivi_attention_decode(q, kn, vn, plain, attention_mask=mask)
        x_m = _dumped(plain, B, nh, n)
        # ---- against the mask alone
        at_or_after = (keys[:n][None] >= lead[:, None].long())[:, None, None, :].expand_as(x_gpu)
        assert torch.equal(x_gpu.view(torch.int16)[at_or_after], x_m.view(torch.int16)[at_or_after]), ("rows from the lead on", s)
        whole = (torch.minimum(lead.long(), torch.tensor(Tq, device="cuda")) // SB) * SB         # whole K super-blocks under the lead
        under = (keys[:n][None] < whole[:, None])[:, None, None, :].expand_as(x_gpu)
        assert bool(under.any()) and bool((x_gpu.view(torch.int16)[under] == FMIN_BITS).all()), ("skipped slots hold -65504", s)
        ok, rm = gemv_close(out, out_m, rtol=1.5e-3, ulps=1)
        assert ok, ("lead against the mask alone", s, rm)
        if split is not None:                                         # the control of that bar: two forms that shipped before the lead
            out_s = kivi_attention_decode(q, kn, vn, split, attention_mask=mask)
            ok, rc = gemv_close(out_s, out_m, rtol=1.5e-3, ulps=1)
            assert ok, ("control: split against row, the mask alone", s, rc)
            worst_c = max(worst_c, rc)
            del out_s
        del x_m, at_or_after, under
        # ---- against the reference, as in _longpad_stages
        ref, new_past, pre = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, attention_mask=mask)
        _, _, pre0 = T64.decode_step(q, kn, vn, past, bits, bits, G32, R)
        check(pre, ref, n, Tq, lead, s)
        assert not torch.isnan(x_gpu).any(), ("a key of the row was not written", s)
        live = pre.float() > -60000
        ok, ra = gemv_close(torch.where(live, x_gpu, pre0), torch.where(live, pre, pre0), rtol=1e-3, ulps=1)
        assert ok, ("stage A", s, ra)
        xd, pd = x_gpu.float()[~live], pre.float()[~live]
        assert bool((xd <= -60000).all()) and bool(((xd - pd).abs() <= 32).all()), ("masked keys", s)
        del xd, pd, pre0, live
        ref_b, _, _ = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, attention_mask=mask, scores_override=x_gpu)
        ok, rb = gemv_close(out, ref_b, rtol=2e-3, ulps=1)
        assert ok, ("stage B", s, rb)
        worst_a, worst_b, worst_m = max(worst_a, ra), max(worst_b, rb), max(worst_m, rm)
        past = new_past
        del ref, ref_b, pre, x_gpu, new_past                          # (the fp64 reference's step: gigabytes at the many-unit shapes)
        if s == flush:
            assert _lengths(past, bits)[0] == Tq + R, "the K flush"
        if s in (0, flush, flush + 1, steps - 1):
            _same_tuple(layer, past, ("step", s))
    assert layer.k_res_len == 3
    _assert_same_state(layer, product)
    _assert_same_state(layer, plain)
    if split is not None:
        _same_tuple(split, past, "split, last step")
    print(f"{what} {nh}/{nh_kv} T0={T0} R={R} {kind} {bits}-bit: worst ratio: scores {worst_a:.3f} of 1e-3+1ulp, "
          f"attend {worst_b:.3f} of 2e-3+1ulp, against the mask alone {worst_m:.3f} of 1.5e-3+1ulp over {steps} steps"
          + (f", control split against row {worst_c:.3f} of 1.5e-3+1ulp" if split is not None else ""))
    return worst_a, worst_b, worst_m, worst_c


@pytest.mark.parametrize("nh,nh_kv,T0,R,kind,bits", [(4, 4, 1100, 32, "randn", 2), (4, 4, 1100, 32, "randn", 4),
                                                      (8, 2, 1100, 128, "outlier", 2), (16, 2, 1100, 32, "randn", 2),
                                                      (8, 2, 1100, 32, "outlier", 4)])
def test_row_kernels_under_a_lead_match_reference_and_the_mask_alone(nh, nh_kv, T0, R, kind, bits):
    lead_stages(nh, nh_kv, T0, R, kind, bits)


# ------------------------------------------------------------------ 2. the skip really skips
@pytest.mark.parametrize("nh,nh_kv", [(4, 4), (8, 2), (32, 32), (48, 48)],
                         ids=["mf_row_kernel", "mf_row4_kernel", "mf_row_kernel_384_rows", "mf_row_kernel_576_rows"])
def test_whole_super_blocks_under_the_lead_are_never_read(nh, nh_kv):
    """(4, 4) and (8, 2): one shape per kernel.  12 x 32 and 12 x 48 rows: mf_row_kernel's other two instantiations -- eight waves per
    row (257 to 512 rows) and the headline's four (more) -- which the 48 rows of the small shapes never launch."""
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    B, T0, R, bits = ROWS, 1100, 32, 2
    k0, v0 = make_kv(1, B, nh_kv, T0, D).cuda(), make_kv(2, B, nh_kv, T0, D).cuda()
    clean = make_layer_cache(KiviConfig(bits, bits, G32, R), B, nh_kv, D, T0 + 64, "cuda", num_heads=nh)
    clean.flags = _forced("row")
    clean.prefill(k0, v0)
    poisoned, plain = clean.clone(), clean.clone()
    n = T0 + 1
    Tq, Tv = clean.k_quant_len, clean.v_quant_len
    mask, lead = longpad_mask(n, Tq, Tv, "cuda"), longpad_lead(n, Tq, Tv)
    words = 0
    for b, p in enumerate(lead.tolist()):                 # only super-blocks WHOLLY under the lead, through the cache's own stores
        for store, T in ((poisoned.kt, Tq), (poisoned.vt, Tv)):
            nsb = min(p, T) // SB
            store[b, :, :nsb] = NAN_WORD
            words += store[b, :, :nsb].numel()
    assert words > 0 and lead.tolist()[4] == 1024 and Tq == 1088
    q, kn, vn = _step_inputs(0, B, nh, nh_kv, "randn")
    want = kivi_attention_decode(q, kn, vn, clean, attention_mask=mask, lead=lead)
    got = kivi_attention_decode(q, kn, vn, poisoned, attention_mask=mask, lead=lead)
    assert bool(torch.isfinite(got).all()), "a poisoned super-block under the lead reached the output"
    assert same_bits(got, want)
    # the mask alone over the clean cache: the same step, the V walk divided differently (section 9's bar for two forms of one step)
    ok, worst = gemv_close(want, kivi_attention_decode(q, kn, vn, plain, attention_mask=mask), rtol=1.5e-3, ulps=1)
    assert ok, worst
    # ... and so do the step's own writes: the K append, the V ring
    assert same_bits(clean.k_res[:, :, : clean.k_res_len], poisoned.k_res[:, :, : poisoned.k_res_len]) and same_bits(clean.v_res, poisoned.v_res)


# ------------------------------------------------------------------ 3. forms that ignore it
@pytest.mark.parametrize("nh,nh_kv,T0,R,form", [(4, 4, 1100, 32, "split"), (8, 2, 1100, 128, "slices2")])
def test_forms_that_ignore_the_lead_are_bit_identical(nh, nh_kv, T0, R, form):
    from kivi_amd import _lib
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    B, bits, steps = ROWS, 2, 4
    k0, v0 = make_kv(1, B, nh_kv, T0, D).cuda(), make_kv(2, B, nh_kv, T0, D).cuda()
    with_lead = make_layer_cache(KiviConfig(bits, bits, G32, R), B, nh_kv, D, T0 + 64, "cuda", num_heads=nh)
    with_lead.flags = _forced(form)
    with_lead.prefill(k0, v0)
    if form != "split":
        assert _lib.load().kivi_mf_launch_plan(B, nh, nh_kv, with_lead.k_quant_len, with_lead.k_res_len, R, with_lead.flags, bits, 0) == 2
    without = with_lead.clone()
    for s in range(steps):
        q, kn, vn = _step_inputs(s, B, nh, nh_kv, "randn")
        n = T0 + s + 1
        mask, lead = longpad_mask(n, with_lead.k_quant_len, with_lead.v_quant_len, "cuda"), longpad_lead(n, with_lead.k_quant_len, with_lead.v_quant_len)
        a = kivi_attention_decode(q, kn, vn, with_lead, attention_mask=mask, lead=lead)
        b = kivi_attention_decode(q, kn, vn, without, attention_mask=mask)
        assert same_bits(a, b), (form, s)
    _assert_same_state(with_lead, without)


# ------------------------------------------------------------------ 4. graph
def _lead_model(seed, on=True):
    model = _model(4, seed)                          # four heads, four kv heads: the decode steps run mf_row_kernel
    model.config.kivi_decode_lead = on
    return model


def test_graphed_steps_replay_under_a_rewritten_lead(monkeypatch):
    from kivi_amd.generation import leading_pads
    from kivi_amd.llama import left_pad
    from test_admit_gpu import _prompts
    model = _lead_model(81)
    L = 900
    ids, mask = left_pad(_prompts(5, [L, L, 9]), 0, "cuda", length=L)
    lg, past = model(ids, padding_mask=mask)
    twin = [p.layer.clone().as_tuple() for p in past]
    tok0 = lg.argmax(-1)
    seen = []
    dyn = type(past[0].layer).decode_step_dyn
    monkeypatch.setattr(type(past[0].layer), "decode_step_dyn",
                        lambda self, *a, **k: seen.append(k.get("lead")) or dyn(self, *a, **k))
    m = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
    assert leading_pads(m).tolist() == [0, 0, L - 9]
    fed = [model.decode_graphed(tok0, past, L, 4, attention_mask=m)]
    buf = model.graphs.lead
    assert buf is not None and buf.tolist() == [0, 0, L - 9]
    m = torch.cat([m, torch.ones_like(m[:, :4])], 1)
    m[1, :600] = 0                                   # as an admission does: row 1's mask row -- and with it its lead -- rewritten in place
    fed.append(model.decode_graphed(model.graphs.tok.clone(), past, L + 4, 4, attention_mask=m))
    assert model.graphs.lead is buf and buf.tolist() == [0, 600, L - 9]
    last = model.graphs.tok.clone()
    eager_steps, captures, replays = model.graphs.stats
    assert captures == 1 and replays >= 6, model.graphs.stats
    assert seen and all(ld is buf for ld in seen), "the captured step reads the static lead buffer"
    # the eager steps: the same masks, the lead derived from them
    tok, m_e, want = tok0, torch.cat([mask, torch.ones_like(mask[:, :1])], 1), []
    for s in range(8):
        if s == 4:
            m_e[1, :600] = 0
        want.append(tok)
        lg, twin = model(tok, twin, padding_mask=m_e)
        tok = lg.argmax(-1)
        m_e = torch.cat([m_e, torch.ones_like(m_e[:, :1])], 1)
    assert torch.equal(torch.cat(fed, 1), torch.cat(want, 1)) and torch.equal(last, tok)
    for p, t in zip(past, twin):
        _assert_same_state(p.layer, t.layer)


# ------------------------------------------------------------------ 5. model and scheduler
def test_model_logits_move_no_more_than_between_two_shipped_forms():
    from kivi_amd import _lib
    from kivi_amd.llama import left_pad
    from test_admit_gpu import _prompts
    model = _lead_model(82, on=False)
    L, steps = 1200, 16
    ids, mask = left_pad(_prompts(7, [9, 600, L]), 0, "cuda", length=L)
    forced = torch.randint(1, 320, (steps, 3, 1), generator=torch.Generator().manual_seed(8)).cuda()      # teacher-forced tokens

    def run(option, split):
        model.config.kivi_decode_lead = option
        lg, past = model(ids, padding_mask=mask)
        leads = []
        for p in past:
            assert getattr(p.layer, "layout", "") == "mfma"
            p.layer.flags = _lib.GQA_FORCE_SPLIT if split else 0
            step = p.layer.decode_step
            p.layer.decode_step = lambda *a, _step=step, **k: leads.append(k.get("lead")) or _step(*a, **k)
        out, m = [lg.float()], mask
        for s in range(steps):
            m = torch.cat([m, torch.ones_like(m[:, :1])], 1)
            lg, past = model(forced[s], past, padding_mask=m)
            out.append(lg.float())
        assert len(leads) == 2 * steps
        assert all(ld is not None and ld.tolist() == [L - 9, L - 600, 0] for ld in leads) if option else all(ld is None for ld in leads)
        return torch.cat(out, 1)
    on, off, off_split = run(True, False), run(False, False), run(False, True)
    model.config.kivi_decode_lead = False
    assert torch.isfinite(on).all()
    assert torch.equal(on[:, 0], off[:, 0]), "the prompt pass does not know the option"
    d0, d1 = (off - off_split).abs().max().item(), (on - off).abs().max().item()
    line = (f"decode lead parity: tiny model (2 layers, 4/4 heads), prompts 9 / 600 / 1200 left-padded to 1200, {steps} teacher-forced steps: "
            f"d0 = max|off - off_split| = {d0:.6g}, d1 = max|on - off| = {d1:.6g}, d1 / d0 = {d1 / d0 if d0 else float('inf'):.3f}")
    print(line)                                      # (recorded in profiles/decode_lead_parity.log)
    assert d0 > 0, "the two shipped forms agree bit for bit: no yardstick"
    assert d1 <= 2 * d0, (d1, d0)


def test_generate_continuous_with_the_lead_equals_its_restated_policy():
    import test_admit_gpu as A
    import test_admit_offset_gpu as O
    model = _lead_model(83)
    # L-padded admissions
    prompts = A._prompts(4, A.LENS)
    want, landed = A._restate(model, prompts, A.LIMITS, 3)
    assert len(set(landed.values())) > 1 and len(landed) > 3, "no admission happened"
    out = model.generate_continuous(prompts, A.LIMITS, 3)
    assert [o.tolist() for o in out] == want
    graphed = model.generate_continuous(prompts, A.LIMITS, 3, graphed=True)
    assert [o.tolist() for o in graphed] == want
    # offset admissions and compact=
    model.release_graphs()
    prompts = A._prompts(6, O.LENS)
    want, admissions, drops = O._restate(model, prompts, O.LIMITS, 3, compact=32)
    assert admissions and any(off > 0 for _, off, _ in admissions) and drops
    out = model.generate_continuous(prompts, O.LIMITS, 3, compact=32, short_admissions=True)
    assert [o.tolist() for o in out] == want
    graphed = model.generate_continuous(prompts, O.LIMITS, 3, compact=32, short_admissions=True, graphed=True)
    assert [o.tolist() for o in graphed] == want
    model.release_graphs()
