"""CPU: the prompt pass's attention kernel and its plumbing.

1. The library exports kivi_prefill_attention, its ctypes signature is the header's declaration argument for argument, the ABI
   version is still 3.
2. Every refusal of the entry point with fake pointers that are never dereferenced: nothing is enqueued.
3. tests/prefill_plan_main.cpp: the tile plan (kivi_prefill_plan.h) walked on the host under AddressSanitizer and UBSan, as a child
   process.
4. The torch restatement of the contract on CPU tensors against float64 attention written here: the live key range per row, pad
   rows exactly zero.  fp32 tensors holding fp16 values; the bar is 1e-5 of max(|ref|, rms of the row): fp32 SDPA carries a few
   dozen roundings of 6e-8 per output at T = 37, two orders under it, while a wrong key range moves outputs by percents.
5. The model on CPU (cache objects replaced by a recorder: the packers have no CPU path): with the option the flash class runs a
   padded prompt pass on lead = T - mask.sum(-1) and padding_prompt_mask is never called; a mask with a hole is refused by the flash
   class and served by the eager class through the masked path; without the option the flash class refuses pads as before.
"""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from helpers import gemv_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ 1. symbol and signature
def test_symbol_and_signature_match_the_header(lib):
    from kivi_amd import _lib, build
    assert hasattr(lib, "kivi_prefill_attention") and "kivi_prefill.hip" in build.SOURCES
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert int(re.search(r"#define KIVI_ABI_VERSION (\d+)", src).group(1)) == 3
    decl = re.search(r"\bint\s+kivi_prefill_attention\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
    ctype = {"constvoid*": ctypes.c_void_p, "void*": ctypes.c_void_p, "constint32_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64,
             "int": ctypes.c_int, "float": ctypes.c_float, "kivi_stream_t": ctypes.c_void_p}
    args, names = [], []
    for a in decl.split(","):
        t, n = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", a).groups()
        args.append(ctype[t.replace(" ", "")])
        names.append(n)
    assert names == ["q", "q_sb", "q_sh", "q_st", "k", "k_sb", "k_sh", "k_st", "v", "v_sb", "v_sh", "v_st", "out", "o_sb", "o_sh", "o_st",
                     "lead", "B", "nh", "nh_kv", "T", "D", "scale", "stream"]
    res, sig = _lib.SIGNATURES["kivi_prefill_attention"]
    assert res is ctypes.c_int and sig == args
    assert lib.kivi_prefill_attention.argtypes == args


# ------------------------------------------------------------------ 2. refusals
def _call(lib, **kw):
    """kivi_prefill_attention on a good (B = 2, nh = 8, nh_kv = 2, T = 200) call with fake pointers, one thing changed."""
    a = dict(q=1 << 24, k=1 << 25, v=1 << 26, out=1 << 27, lead=1 << 28, B=2, nh=8, nh_kv=2, T=200, D=128, scale=1.0 / math.sqrt(128))
    a.update({k: v for k, v in kw.items() if k in a})
    st = {}
    for name, heads in (("q", a["nh"]), ("k", a["nh_kv"]), ("v", a["nh_kv"]), ("o", a["nh"])):
        st[name] = [max(heads, 1) * max(a["T"], 1) * 128, max(a["T"], 1) * 128, 128]
    for key, val in kw.items():
        if key not in a:                                   # e.g. q_st=130: the token stride of q
            name, which = key.split("_")
            st[name][("sb", "sh", "st").index(which)] = val
    return lib.kivi_prefill_attention(a["q"], *st["q"], a["k"], *st["k"], a["v"], *st["v"], a["out"], *st["o"], a["lead"], a["B"], a["nh"],
                                      a["nh_kv"], a["T"], a["D"], a["scale"], None)


INVALID = [("D64", dict(D=64)), ("D256", dict(D=256)), ("D0", dict(D=0)),
           ("B0", dict(B=0)), ("B_negative", dict(B=-1)), ("nh0", dict(nh=0)), ("nh_negative", dict(nh=-8)),
           ("nh_kv0", dict(nh_kv=0)), ("nh_kv_negative", dict(nh_kv=-2)), ("T0", dict(T=0)), ("T_negative", dict(T=-5)),
           ("not_a_multiple", dict(nh=7, nh_kv=2)), ("nh_below_nh_kv", dict(nh=2, nh_kv=4)),
           ("ratio3", dict(nh=6, nh_kv=2)), ("ratio16", dict(nh=32, nh_kv=2)), ("ratio5", dict(nh=5, nh_kv=1)),
           ("null_q", dict(q=None)), ("null_k", dict(k=None)), ("null_v", dict(v=None)), ("null_out", dict(out=None)),
           ("scale_nan", dict(scale=float("nan"))), ("scale_inf", dict(scale=float("inf"))), ("scale_zero", dict(scale=0.0)),
           ("scale_negative", dict(scale=-0.1)),
           ("grid_2_31", dict(B=1 << 16, nh=1 << 15, nh_kv=1 << 15, T=1)), ("grid_T", dict(B=1 << 10, nh=1 << 10, nh_kv=1 << 10, T=1 << 18)),
           ("T_2_31", dict(T=(1 << 31) - 1))]
MISALIGNED = [("q_base", dict(q=(1 << 24) + 8)), ("k_base", dict(k=(1 << 25) + 2)), ("v_base", dict(v=(1 << 26) + 4)),
              ("out_base", dict(out=(1 << 27) + 8)), ("lead_base", dict(lead=(1 << 28) + 2)),
              ("q_st", dict(q_st=130)), ("q_sh", dict(q_sh=200 * 128 + 4)), ("q_sb", dict(q_sb=8 * 200 * 128 + 1)),
              ("k_st", dict(k_st=129)), ("k_sh", dict(k_sh=200 * 128 + 2)), ("k_sb", dict(k_sb=2 * 200 * 128 + 4)),
              ("v_st", dict(v_st=132)), ("v_sh", dict(v_sh=200 * 128 + 7)), ("v_sb", dict(v_sb=2 * 200 * 128 + 6)),
              ("o_st", dict(o_st=8 * 128 + 4)), ("o_sh", dict(o_sh=129)), ("o_sb", dict(o_sb=8 * 200 * 128 + 2))]


@pytest.mark.parametrize("case,change", INVALID, ids=[c for c, _ in INVALID])
def test_refuses_bad_arguments(lib, case, change):
    assert _call(lib, **change) == EINVAL
    assert b"kivi_prefill_attention" in lib.kivi_last_error()


@pytest.mark.parametrize("case,change", MISALIGNED, ids=[c for c, _ in MISALIGNED])
def test_refuses_misaligned_arguments(lib, case, change):
    assert _call(lib, **change) == EALIGN
    assert b"kivi_prefill_attention" in lib.kivi_last_error()


def test_shape_refusals_come_before_alignment(lib):
    assert _call(lib, D=64, q=(1 << 24) + 2) == EINVAL
    assert _call(lib, scale=0.0, lead=(1 << 28) + 1) == EINVAL


# ------------------------------------------------------------------ 3. the tile plan on the host, under sanitizers
def test_tile_plan_covers_exactly_the_live_pairs_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "prefill_plan")
    # the sanitizer runtimes are linked into the program (clang's default), so it does not depend on the order libraries load in
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "prefill_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "prefill plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------ 4. the torch restatement against float64 attention
def _ref64(q, k, v, lead):
    """float64 attention, one (row, head, query) at a time over its live keys [lead, i]; pad rows zero."""
    B, nh, T, D = q.shape
    G = nh // k.shape[1]
    out = torch.zeros((B, nh, T, D), dtype=torch.float64)
    for b in range(B):
        for h in range(nh):
            for i in range(lead[b], T):
                kk, vv = k[b, h // G, lead[b]: i + 1].double(), v[b, h // G, lead[b]: i + 1].double()
                p = torch.softmax(kk @ q[b, h, i].double() / math.sqrt(D), 0)
                out[b, h, i] = p @ vv
    return out


@pytest.mark.parametrize("ratio", [1, 4])
def test_torch_restatement_against_fp64(ratio):
    from kivi_amd import prefill
    B, nh_kv, T, D = 3, 2, 37, 128
    g = torch.Generator().manual_seed(5 + ratio)
    q, k, v = (torch.randn((B, h, T, D), generator=g).half().float() for h in (nh_kv * ratio, nh_kv, nh_kv))
    lead = [0, 5, 36]
    ref = _ref64(q, k, v, lead)
    got = prefill.attention(q, k, v, torch.tensor(lead, dtype=torch.int32))          # CPU tensors: the restatement
    ok, worst = gemv_close(got, ref, rtol=1e-5)
    assert ok, worst
    for b in range(B):
        assert bool((got[b, :, : lead[b]] == 0).all())
    assert bool(torch.isfinite(got).all())
    # without a lead it is the causal call
    ok, worst = gemv_close(prefill.attention(q, k, v), _ref64(q, k, v, [0, 0, 0]), rtol=1e-5)
    assert ok, worst
    # clamped like the kernel: a lead past T is a row of pads only, a negative one no pad
    wild = prefill.attention(q, k, v, torch.tensor([-4, T + 9, 5], dtype=torch.int32))
    assert bool((wild[1] == 0).all())
    ok, worst = gemv_close(wild[[0, 2]], _ref64(q, k, v, [0, T, 5])[[0, 2]], rtol=1e-5)
    assert ok, worst


class _Recorder:
    """Stands in for a layer cache on CPU: what prefill() was handed."""

    def __init__(self, nh_kv):
        self.nh_kv, self.calls = nh_kv, []

    def prefill(self, k, v):
        self.calls.append((k, v))

    def as_tuple(self):
        return (None,) * 8 + (self.calls[0][0].shape[2],)


def test_hook_function_forms_on_cpu():
    """kernel=True on CPU tensors is the restatement; an attention_mask given with it takes the masked SDPA path unchanged; `lead`
    without kernel=True is refused; layer.prefill sees the very tensors in every form."""
    from kivi_amd.attention import kivi_attention_prefill
    from kivi_amd.generation import padding_prompt_mask
    B, nh, nh_kv, T, D = 2, 4, 2, 19, 128
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn((B, h, T, D), generator=g) for h in (nh, nh_kv, nh_kv))
    lead = torch.tensor([0, 7], dtype=torch.int32)
    mask4 = padding_prompt_mask((torch.arange(T)[None] >= lead[:, None]).long()).float()
    outs = {}
    for name, kw in (("old", {}), ("old_mask", dict(attention_mask=mask4)), ("new", dict(kernel=True)),
                     ("new_lead", dict(kernel=True, lead=lead)), ("new_mask", dict(kernel=True, attention_mask=mask4))):
        layer = _Recorder(nh_kv)
        outs[name] = kivi_attention_prefill(q, k, v, layer, **kw)
        assert len(layer.calls) == 1 and layer.calls[0][0] is k and layer.calls[0][1] is v, name
    assert torch.equal(outs["new_mask"], outs["old_mask"])
    assert torch.allclose(outs["new"], outs["old"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(outs["new_lead"][1, :, 7:], outs["old_mask"][1, :, 7:], rtol=1e-5, atol=1e-6)
    assert bool((outs["new_lead"][1, :, :7] == 0).all())
    with pytest.raises(ValueError, match="lead"):
        kivi_attention_prefill(q, k, v, _Recorder(nh_kv), lead=lead)
    with pytest.raises(ValueError, match="lead"):
        kivi_attention_prefill(q, k, v, _Recorder(nh_kv), attention_mask=mask4, lead=lead, kernel=True)


# ------------------------------------------------------------------ 5. the model on CPU
def _model(cls, option, monkeypatch, weights=None):
    import kivi_amd.attention as A
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=2,
                           intermediate_size=256, vocab_size=64), residual_length=32, prefill_kernel=option)
    assert cfg.kivi_prefill_kernel is option
    torch.manual_seed(3)
    model = LlamaForCausalLM_KIVI(cfg, getattr(A, cls))
    if weights is not None:
        model.load_state_dict(weights)
    monkeypatch.setattr(A, "make_layer_cache", lambda cfg, B, nh_kv, *a, **k: _Recorder(nh_kv))
    return model


@pytest.fixture
def spies(monkeypatch):
    """(calls of padding_prompt_mask, the `lead` of every prefill.attention call)"""
    import kivi_amd.generation as G
    from kivi_amd import prefill
    built, leads = [], []
    build, attention = G.padding_prompt_mask, prefill.attention
    monkeypatch.setattr(G, "padding_prompt_mask", lambda m: built.append(tuple(m.shape)) or build(m))
    monkeypatch.setattr(prefill, "attention", lambda q, k, v, lead=None: leads.append(lead) or attention(q, k, v, lead))
    return built, leads


IDS = torch.tensor([[0, 0, 0, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7], [0, 9, 8, 7, 6, 5, 4]])
MASK = torch.tensor([[0, 0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1]])


def test_default_config_has_the_option_off():
    from kivi_amd.llama import make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256, vocab_size=64))
    assert cfg.kivi_prefill_kernel is False


@pytest.mark.parametrize("cls", ["LlamaFlashAttention_KIVI", "MistralFlashAttention_KIVI", "LlamaAttention_KIVI", "MistralAttention_KIVI"])
def test_padded_prompt_pass_runs_on_the_lead(cls, monkeypatch, spies):
    built, leads = spies
    model = _model(cls, True, monkeypatch)
    assert all(layer.self_attn.prefill_kernel for layer in model.model.layers)
    logits, past = model(IDS, padding_mask=MASK)
    assert built == [], "the (B, 1, T, T) mask was built"
    assert len(leads) == 2 and all(ld.dtype == torch.int32 and ld.tolist() == (7 - MASK.sum(-1)).tolist() == [3, 0, 1] for ld in leads)
    assert logits.shape == (3, 1, 64) and bool(torch.isfinite(logits).all()) and past[0][-1] == 7
    # the real tokens see what the masked path of the eager class shows them
    eager = _model("LlamaAttention_KIVI", False, monkeypatch, model.state_dict())
    want, _ = eager(IDS, padding_mask=MASK)
    assert built == [(3, 7)] and len(leads) == 2
    assert torch.allclose(logits, want, rtol=1e-4, atol=1e-5)
    # without a pad nothing is derived at all: the kernel's causal form, no lead
    model(IDS, padding_mask=torch.ones_like(MASK))
    assert len(leads) == 4 and leads[2] is None and leads[3] is None and built == [(3, 7)]
    model(IDS)
    assert len(leads) == 6 and leads[5] is None


def test_mask_with_a_hole(monkeypatch, spies):
    built, leads = spies
    holed = MASK.clone()
    holed[0, 4] = 0
    flash = _model("LlamaFlashAttention_KIVI", True, monkeypatch)
    with pytest.raises(ValueError, match="not left-padded.*leading pads only.*eager class"):
        flash(IDS, padding_mask=holed)
    with pytest.raises(ValueError, match="not left-padded"):
        flash.generate(IDS, 2, attention_mask=holed)
    with pytest.raises(ValueError, match="not left-padded"):
        flash.score(IDS, holed)
    assert built == [] and leads == []
    eager = _model("LlamaAttention_KIVI", True, monkeypatch)
    logits, _ = eager(IDS, padding_mask=holed)                                # the masked path, as without the option
    assert built == [(3, 7)] and leads == [] and bool(torch.isfinite(logits).all())
    plain = _model("LlamaAttention_KIVI", False, monkeypatch, eager.state_dict())
    want, _ = plain(IDS, padding_mask=holed)
    assert torch.equal(logits, want)


@pytest.mark.parametrize("cls", ["LlamaFlashAttention_KIVI", "MistralFlashAttention_KIVI"])
def test_without_the_option_the_flash_class_refuses_pads_as_before(cls, monkeypatch, spies):
    built, leads = spies
    model = _model(cls, False, monkeypatch)
    assert not any(layer.self_attn.prefill_kernel for layer in model.model.layers)
    with pytest.raises(ValueError, match=r"ignores masks \(llama_kivi.py:420-423\), so padded prompts cannot be run; use the eager class"):
        model(IDS, padding_mask=MASK)
    logits, _ = model(IDS)                                                    # and its unpadded pass is today's SDPA call
    assert built == [] and leads == [] and logits.shape == (3, 1, 64)
    # ... made the way it always was: a caller's replacement with the five arguments of before still fits
    import kivi_amd.attention as A
    hook, seen = A.kivi_attention_prefill, []

    def five(q, k, v, layer, attention_mask=None):
        seen.append(attention_mask)
        return hook(q, k, v, layer, attention_mask)
    monkeypatch.setattr(A, "kivi_attention_prefill", five)
    again, _ = model(IDS)
    assert seen == [None, None] and torch.equal(again, logits)


def test_score_takes_the_lead_in_its_own_synchronisation(monkeypatch, spies):
    from kivi_amd import scoring
    built, leads = spies
    monkeypatch.setattr(scoring, "token_logprobs", lambda logits, targets, return_rank=False: torch.zeros(targets.shape))
    model = _model("LlamaFlashAttention_KIVI", True, monkeypatch)
    syncs = []
    padded = model._padded
    monkeypatch.setattr(model, "_padded", lambda *a: syncs.append(a[4:]) or padded(*a))
    lp, valid, _ = model.score(IDS, MASK)
    assert syncs == [(True, True)], "score() hands _padded both facts: no second synchronisation"
    assert built == [] and [ld.tolist() for ld in leads] == [[3, 0, 1]] * 2
    assert valid.tolist() == (MASK[:, 1:] & MASK[:, :-1]).bool().tolist() and lp.shape == (3, 6)
