"""GPU: the prompt pass's attention kernel -- kivi_prefill_attention, kivi_attention_prefill(kernel=True), the attention modules
and the model with config.kivi_prefill_kernel.

1. Kernel.  Against attention in float64 on the same fp16 inputs (computed on the GPU, probabilities not rounded) at the attend bar
   2e-3 + 1 ulp of the decode kernels, which hold fp16 probabilities too.  In the same test the parent's form -- repeat_interleave +
   SDPA, causal or with the (B, 1, T, T) mask -- has to sit inside that bar as well: an input where it does not is a badly chosen
   input.  Pad rows exactly zero, nothing non-finite, canaries around `out` untouched, two runs bit-identical.  T = 1 .. 515 (one
   key tile, 16 / 17 / 33: the matrix tile and its neighbours, 130: a second query tile of two rows, 515: five query tiles and
   every wave's own diagonal), nh / nh_kv = 1, 4, 8, leads none / [0, 5, T - 1] / [32, 64, 0] / [T, 0, 1] (a row of pads only).
2. One layer: kernel=True against kernel=False on the same q, k, v -- the cache afterwards bit for bit, the outputs of live rows
   within the 1.5e-3 + 1 ulp bar of two forms of one step.
3. Model: the flash class with the option on a padded batch against the eager class without it, both against every prompt alone,
   d1 <= 2 d0 (the method of DESIGN.md section 19).
4. Serving: generate_continuous on the flash class equals the restatement that calls admit_ by hand; admit_ leaves the other rows
   byte for byte.

Measured on an MI355X (profiles/prefill_attn_ratios.log, profiles/prefill_attn_parity.log): kernel against fp64 at most 0.53 of
2e-3 + 1 ulp (the parent's SDPA form at most 0.50); one layer, kernel against SDPA form, at most 0.65 of 1.5e-3 + 1 ulp;
model d0 = 2.614258, d1 = 2.621582.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import gemv_close, make_kv, same_bits
from test_admit_gpu import _check_outputs, _held, _prompts, _range_words, _restate, _same_member
from test_sample_gpu import _layouts

pytestmark = pytest.mark.gpu
D = 128
SCALE = 1.0 / math.sqrt(D)


def _leads(T):
    out = [None, [0, 5, T - 1], [T, 0, 1]]
    if T > 64:
        out.append([32, 64, 0])
    return out


def _ref64(q, k, v, lead):
    """float64 attention over the live key range of every row; (out (B, nh, T, D) float64 with zero pad rows, live (B, T) bool)."""
    B, nh, T, _ = q.shape
    G = nh // k.shape[1]
    k64, v64 = k.double().repeat_interleave(G, 1), v.double().repeat_interleave(G, 1)
    s = q.double() @ k64.transpose(-1, -2) * SCALE
    pos = torch.arange(T, device=q.device)
    ld = torch.zeros(B, dtype=torch.long, device=q.device) if lead is None else lead.long().clamp(0, T)
    live = pos[None] >= ld[:, None]
    allowed = (pos[None, :, None] >= pos[None, None, :]) & live[:, None, :]
    s = s.masked_fill(~allowed[:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)                  # a pad row has no live key: all -inf -> nan -> 0
    return (p @ v64) * live[:, None, :, None], live


def _parent(q, k, v, lead):
    """What the parent commit runs for the same call: K / V repeated per query head, SDPA causal or with the 4D additive mask."""
    from kivi_amd.generation import padding_prompt_mask
    B, nh, T, _ = q.shape
    G = nh // k.shape[1]
    kr, vr = (k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)) if G > 1 else (k, v)
    if lead is None:
        return F.scaled_dot_product_attention(q, kr, vr, is_causal=True)
    mask2d = (torch.arange(T, device=q.device)[None] >= lead.long()[:, None]).long()
    return F.scaled_dot_product_attention(q, kr, vr, attn_mask=padding_prompt_mask(mask2d))


def _run_with_canaries(q, k, v, lead, layout="bhtd"):
    """The kernel into an `out` that sits between two canary runs of one allocation -> (out, canaries untouched)."""
    from kivi_amd import prefill
    B, nh, T, _ = q.shape
    n, pad = B * nh * T * D, 64
    buf = torch.full((n + 2 * pad,), -777.0, dtype=torch.float16, device="cuda")
    body = buf[pad: pad + n]
    out = body.view(B, nh, T, D) if layout == "bhtd" else body.view(B, T, nh, D).transpose(1, 2)
    res = prefill.attention_kernel(q, k, v, lead, out=out)
    assert res is out
    ok = bool((buf[:pad] == -777.0).all()) and bool((buf[pad + n:] == -777.0).all())
    return out, ok


def _check(q, k, v, lead, tag, layout="bhtd"):
    ref, live = _ref64(q, k, v, lead)
    out, canaries = _run_with_canaries(q, k, v, lead, layout)
    again, _ = _run_with_canaries(q, k, v, lead, layout)
    assert canaries, f"{tag}: a canary next to out was written"
    assert same_bits(out, again), f"{tag}: two runs differ"
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    rows = live[:, None, :].expand(-1, q.shape[1], -1)
    assert bool((out[~rows] == 0).all()) and not bool(torch.signbit(out[~rows]).any()), f"{tag}: pad rows are not exact zeros"
    if not bool(rows.any()):
        return
    ok_p, ratio_p = gemv_close(_parent(q, k, v, lead)[rows], ref[rows], rtol=2e-3, ulps=1)
    ok, ratio = gemv_close(out[rows], ref[rows], rtol=2e-3, ulps=1)
    print(f"prefill kernel vs fp64 {tag}: worst ratio {ratio:.4f} of 2e-3+1ulp (parent's SDPA form {ratio_p:.4f})")
    assert ok_p, f"{tag}: the parent's SDPA form misses the bar ({ratio_p:.3f}): a badly chosen input"
    assert ok, f"{tag}: {ratio:.3f} of the bar"


def _lead_tensor(lead):
    return None if lead is None else torch.tensor(lead, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------ 1. the kernel against fp64 attention
@pytest.mark.parametrize("T", [1, 16, 17, 33, 130, 515])
@pytest.mark.parametrize("nh_kv", [8, 2, 1])
def test_kernel_against_fp64(nh_kv, T):
    B, nh = 3, 8
    q, k, v = (make_kv(1000 * T + 10 * nh_kv + i, B, h, T, D).cuda() for i, h in enumerate((nh, nh_kv, nh_kv)))
    for lead in _leads(T):
        _check(q, k, v, _lead_tensor(lead), f"T={T} nh_kv={nh_kv} lead={lead}")


def test_kernel_strided_inputs_and_token_major_out():
    """q, k, v as the modules hold them -- transposed views of (B, T, heads, D) projections -- and out in (B, T, nh * D) order."""
    B, nh, nh_kv, T = 3, 8, 2, 130
    q, k, v = (make_kv(70 + i, B, T, h, D).cuda().transpose(1, 2) for i, h in enumerate((nh, nh_kv, nh_kv)))
    assert not q.is_contiguous() and q.stride(3) == 1
    for lead in (None, [0, 5, T - 1], [32, 64, 0]):
        _check(q, k, v, _lead_tensor(lead), f"strided lead={lead}", layout="bthd")


def test_kernel_outlier_keys():
    """Keys with a few large channels (KIVI paper fig. 2): raw scores spread over a few hundred units, the softmax is peaked."""
    B, nh, nh_kv, T = 3, 8, 2, 130
    q, v = make_kv(81, B, nh, T, D).cuda(), make_kv(83, B, nh_kv, T, D).cuda()
    k = make_kv(82, B, nh_kv, T, D, kind="outlier").cuda()
    raw = (q.float() @ k.float().repeat_interleave(nh // nh_kv, 1).transpose(-1, -2))
    assert raw.max() - raw.min() > 200
    for lead in (None, [0, 5, T - 1], [32, 64, 0]):
        _check(q, k, v, _lead_tensor(lead), f"outlier lead={lead}")


# ------------------------------------------------------------------ 2. one layer
@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("ratio", [1, 4])
def test_layer_kernel_against_sdpa_form(ratio, layout, monkeypatch):
    from kivi_amd.attention import KiviConfig, kivi_attention_prefill, make_layer_cache
    from kivi_amd.generation import padding_prompt_mask
    _layouts(monkeypatch, layout)
    B, nh_kv, T = 3, 2, 77
    nh = nh_kv * ratio
    cfg = KiviConfig(2, 2, 32, 32)
    q, k, v = (make_kv(90 + i, B, h, T, D).cuda() for i, h in enumerate((nh, nh_kv, nh_kv)))

    def run(**kw):
        layer = make_layer_cache(cfg, B, nh_kv, D, T + 64, "cuda", torch.float16, num_heads=nh)
        assert getattr(layer, "layout", "hook") == layout
        return kivi_attention_prefill(q, k, v, layer, **kw), layer
    lead = torch.tensor([0, 5, 40], dtype=torch.int32, device="cuda")
    mask2d = (torch.arange(T, device="cuda")[None] >= lead.long()[:, None]).long()
    for tag, new, old in (("causal", dict(kernel=True), dict()),
                          ("lead", dict(kernel=True, lead=lead), dict(attention_mask=padding_prompt_mask(mask2d)))):
        (o_new, l_new), (o_old, l_old) = run(**new), run(**old)
        assert l_new.as_tuple()[8] == l_old.as_tuple()[8] == T
        for i, (x, y) in enumerate(zip(l_new.as_tuple()[:8], l_old.as_tuple()[:8])):
            assert _same_member(x, y), (tag, i)
        for x, y in zip(_range_words(l_new), _range_words(l_old)):
            assert torch.equal(x, y)
        rows = (mask2d.bool() if tag == "lead" else torch.ones_like(mask2d).bool())[:, None, :].expand(-1, nh, -1)
        ok, ratio_ = gemv_close(o_new[rows], o_old[rows], rtol=1.5e-3, ulps=1)
        print(f"layer {layout} ratio {ratio} {tag}: kernel vs SDPA form, worst ratio {ratio_:.4f} of 1.5e-3+1ulp")
        assert ok, (tag, ratio_)
        if tag == "lead":
            assert bool((o_new[~rows] == 0).all())


# ------------------------------------------------------------------ 3. the model
def _models(seed):
    """(flash class with the option, eager class without) over the same weights: hidden 512, 4 / 2 heads, 2 layers."""
    from kivi_amd.attention import LlamaFlashAttention_KIVI
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    shape = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=1024,
                 vocab_size=320)
    torch.manual_seed(seed)
    eager = LlamaForCausalLM_KIVI(make_config(shape, residual_length=32)).half().cuda()
    for p in eager.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.05)
    flash = LlamaForCausalLM_KIVI(make_config(shape, residual_length=32, prefill_kernel=True), LlamaFlashAttention_KIVI).half().cuda()
    flash.load_state_dict(eager.state_dict())
    return flash, eager


def test_model_padded_prompt_pass_semantic_bar():
    """A = flash class, option on, padded batch; B = eager class, option off, the same batch; C = every prompt alone, unpadded, eager
    class.  d0 = max |B - C| compares two paths of the parent commit that differ by the pads inside the K groups; d1 = max |A - C|
    adds the attention form and has to stay within 2 d0 (each is one draw of a maximum over the same kind of error)."""
    from kivi_amd.llama import left_pad
    flash, eager = _models(31)
    lens = [9, 20, 33]
    prompts = _prompts(12, lens)
    fed = torch.tensor(_prompts(13, [16, 16, 16]), device="cuda")           # (3, 16)
    ids, mask = left_pad(prompts, 0, "cuda")

    def run(model, ids, mask, fed):
        """prompt logits of the real tokens + 16 teacher-forced steps, per row: list of (len + 16, vocab) float tensors"""
        lg, past = model(ids, padding_mask=mask, last_token_only=False)
        n = mask.sum(-1).tolist()
        rows = [[lg[r, ids.shape[1] - n[r]:].float()] for r in range(ids.shape[0])]
        for s in range(16):
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            lg, past = model(fed[:, s: s + 1], past, padding_mask=mask)
            for r in range(ids.shape[0]):
                rows[r].append(lg[r].float())
        return [torch.cat(x) for x in rows]
    a, b = run(flash, ids, mask, fed), run(eager, ids, mask, fed)
    c = []
    for r, p in enumerate(prompts):
        one = torch.tensor([p], device="cuda")
        c += run(eager, one, torch.ones_like(one), fed[r: r + 1])
    assert all(bool(torch.isfinite(x).all()) for x in a)
    d0 = max((x - y).abs().max().item() for x, y in zip(b, c))
    d1 = max((x - y).abs().max().item() for x, y in zip(a, c))
    line = f"prefill kernel parity: d0 = max|B - C| = {d0:.6f}, d1 = max|A - C| = {d1:.6f}, d1 / d0 = {d1 / max(d0, 1e-30):.3f}"
    print(line)
    log = os.environ.get("KIVI_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert d0 > 0, "the bar has collapsed: the two paths of the parent commit agree exactly"
    assert d1 <= 2 * d0, (d0, d1)


# ------------------------------------------------------------------ 4. serving
def test_generate_continuous_on_the_flash_class():
    flash, _ = _models(32)
    prompts = _prompts(14, [21, 5, 33, 12, 8, 26])
    limits = [4, 12, 9, 1, 10, 6]
    out = flash.generate_continuous(prompts, limits, 2)
    _check_outputs(out, limits)
    want, _ = _restate(flash, prompts, limits, 2)
    assert [o.tolist() for o in out] == want


def test_admit_with_the_option_leaves_the_other_rows():
    from kivi_amd.llama import left_pad
    flash, _ = _models(33)
    ids, mask = left_pad(_prompts(15, [40, 33, 17]), 0, "cuda")
    lg, past = flash(ids, padding_mask=mask)
    for _ in range(5):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = flash(lg.argmax(-1), past, padding_mask=mask)
    L = past[0][-1]
    before = [{n: t.clone() for n, t in _held(p.layer).items()} for p in past]
    nids, nmask = left_pad(_prompts(16, [11]), 0, "cuda", length=L)
    lg1, past2 = flash.admit_(past, [1], nids, nmask)
    alone_lg, alone = flash(nids, padding_mask=nmask)
    assert same_bits(lg1, alone_lg)
    for p, old, src in zip(past2, before, alone):
        for n, t in _held(p.layer).items():
            assert torch.equal(t[[0, 2]].view(torch.uint8), old[n][[0, 2]].view(torch.uint8)), n
        for i, (x, y) in enumerate(zip(p.layer.as_tuple()[:8], src.layer.as_tuple()[:8])):
            assert _same_member(None if x is None else x[1:2], y), i
