"""CPU: the per-row lead of the decode step -- contract, plan and plumbing.

1. The library exports kivi_gqa_decode_lead, kivi_mf_decode_layer_lead and kivi_mf_decode_layer_dyn_lead; their ctypes signatures
   are the header's declarations argument for argument -- the old entry's arguments with `lead` before the stream --; the ABI
   version is still 3.
2. A lead off 4 bytes is KIVI_EALIGN, with fake pointers that are never dereferenced; every refusal of the old entries comes back
   from the new ones with the same code and message.
3. tests/lead_plan_main.cpp: the walk of a row under a lead (kivi_lead_plan.h) on the host under AddressSanitizer and UBSan, as a
   child process.
4. The model on CPU, the cache objects replaced by a recorder (the kernels have no CPU path): with the option off no decode call
   sees a lead and the key row arrives as the plain tensor it always was; with it on every decode call's lead is the number of
   leading masked keys of the mask it travels with -- a left-padded generate, the same over beams, the scheduler after an L-padded
   admission, after an offset admission and after a rebase.  The hook-state cache takes a lead and hands its step what it always did.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_abi_cpu import _gqa_args, _mf_layer_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
MIN16 = torch.finfo(torch.float16).min


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ 1. symbols and signatures
CTYPE = {"constvoid*": ctypes.c_void_p, "void*": ctypes.c_void_p, "constint32_t*": ctypes.c_void_p, "int64_t*": ctypes.POINTER(ctypes.c_int64),
         "int64_t": ctypes.c_int64, "int": ctypes.c_int, "kivi_stream_t": ctypes.c_void_p}


def _declared(name):
    """(ctypes argument types, argument names) of `int name(...)` in include/kivi_hip.h."""
    from kivi_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kivi_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\(([^)]*)\)\s*;" % name, src).group(1)
    struct = {"constkivi_gqa_decode_args*": ctypes.POINTER(_lib.GqaDecodeArgs), "constkivi_mf_layer_desc*": ctypes.POINTER(_lib.MfLayerDesc),
              "constkivi_mf_step*": ctypes.POINTER(_lib.MfStep)}
    args, names = [], []
    for a in decl.split(","):
        t, n = re.match(r"\s*((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*$", a).groups()
        t = t.replace(" ", "")
        args.append(struct.get(t) or CTYPE[t])
        names.append(n)
    return args, names


@pytest.mark.parametrize("old", ["kivi_gqa_decode", "kivi_mf_decode_layer", "kivi_mf_decode_layer_dyn"])
def test_symbols_and_signatures_match_the_header(lib, old):
    from kivi_amd import _lib
    new = old + "_lead"
    assert hasattr(lib, new)
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert int(re.search(r"#define KIVI_ABI_VERSION (\d+)", src).group(1)) == 3
    (args, names), (old_args, old_names) = _declared(new), _declared(old)
    # the old entry's arguments unchanged, one trailing `const int32_t* lead` before the stream
    assert names == old_names[:-1] + ["lead", "stream"] and args == old_args[:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    res, sig = _lib.SIGNATURES[new]
    assert res is ctypes.c_int and sig == args and getattr(lib, new).argtypes == args
    assert _lib.SIGNATURES[old][1] == old_args, "the old entry keeps its signature"
    # no descriptor grew: the structs the entries share are the ones test_abi_cpu.py pins
    assert "lead" not in [f for f, _ in _lib.GqaDecodeArgs._fields_] + [f for f, _ in _lib.MfLayerDesc._fields_]


# ------------------------------------------------------------------ 2. refusals
LAYER_ARGS = (0x1000, 8 * 128, 128, 8, 0x1000, 2 * 128, 128, 0x1000, 2 * 128, 128, None, 0, 0x1000, 8 * 128, 128)
LEAD = 0x2000


def _step():
    from kivi_amd import _lib
    return _lib.MfStep(Tq=64, Tv=63, k_res_len=31, v_res_len=32, v_win_start=5, v_flush=1)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_misaligned_lead_is_refused_before_anything_is_enqueued(lib, off):
    a = _gqa_args()
    assert lib.kivi_gqa_decode_lead(ctypes.byref(a), LEAD + off, None) == EALIGN
    assert b"lead must be 4-byte aligned" in lib.kivi_last_error()
    d = _mf_layer_desc()
    state = (ctypes.c_int64 * 6)(64, 31, 63, 5, 32, 95)        # (the next step would flush K)
    before = list(state)
    assert lib.kivi_mf_decode_layer_lead(ctypes.byref(d), state, *LAYER_ARGS, LEAD + off, None) == EALIGN
    assert b"lead must be 4-byte aligned" in lib.kivi_last_error() and list(state) == before
    hs = _step()
    assert lib.kivi_mf_decode_layer_dyn_lead(ctypes.byref(_mf_layer_desc(s_pitch=600)), ctypes.byref(hs), 0x1000, *LAYER_ARGS, LEAD + off,
                                             None) == EALIGN
    assert b"lead must be 4-byte aligned" in lib.kivi_last_error()


GQA_BAD = [dict(nh=6), dict(bits=8), dict(bits=4, nh=16), dict(bits=4, kt_ss=6144), dict(Tq=500), dict(Tv=480), dict(s_sh=516),
           dict(stats_bytes=16), dict(workspace_bytes=65536), dict(workspace_bytes=65536 + 4 * 1 * 2 * 4 * 128 * 4), dict(vnew=0x1004),
           dict(kt_range=None), dict(vt_range=0x1002), dict(k_res_len=32, Tq=480, Tv=480), dict(residual_length=16), dict(v_win_start=33),
           dict(v_window_rows=32), dict(vt_superblocks=0), dict(Tq=1024, Tv=999, kt_superblocks=1), dict(v_res_len=31, Tv=488),
           dict(flags=4, v_window_rows=32), dict(flags=4, v_window_rows=33, v_win_start=33), dict(q=0x1008), dict(out=None),
           dict(dyn_step=0x1004)]


@pytest.mark.parametrize("over", GQA_BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in GQA_BAD])
@pytest.mark.parametrize("lead", [None, LEAD], ids=["null_lead", "lead"])
def test_gqa_decode_lead_refuses_what_gqa_decode_refuses(lib, over, lead):
    a = _gqa_args(**over)
    rc_old, msg_old = lib.kivi_gqa_decode(ctypes.byref(a), None), lib.kivi_last_error()
    assert rc_old < 0
    rc_new, msg_new = lib.kivi_gqa_decode_lead(ctypes.byref(a), lead, None), lib.kivi_last_error()
    assert (rc_new, msg_new) == (rc_old, msg_old)
    assert lib.kivi_gqa_decode_lead(None, lead, None) == EINVAL


LAYER_BAD = [dict(bits=8), dict(bits=4, nh_kv=4), dict(residual_length=48), dict(kt=None), dict(vt_range=None), dict(cap=64),
             dict(kt_ss=100), dict(v_window_rows=32), dict(s_pitch=90)]


@pytest.mark.parametrize("over", LAYER_BAD, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in LAYER_BAD])
def test_mf_decode_layer_lead_refuses_what_mf_decode_layer_refuses(lib, over):
    d = _mf_layer_desc(**over)
    got = []
    for call in (lambda st: lib.kivi_mf_decode_layer(ctypes.byref(d), st, *LAYER_ARGS, None),
                 lambda st: lib.kivi_mf_decode_layer_lead(ctypes.byref(d), st, *LAYER_ARGS, None, None),
                 lambda st: lib.kivi_mf_decode_layer_lead(ctypes.byref(d), st, *LAYER_ARGS, LEAD, None)):
        state = (ctypes.c_int64 * 6)(64, 31, 63, 5, 32, 95)
        rc = call(state)
        got.append((rc, lib.kivi_last_error()))
        assert rc < 0 and list(state) == [64, 31, 63, 5, 32, 95]
    assert got[0] == got[1] == got[2]
    bad = (ctypes.c_int64 * 6)(64, 31, 63, 0, 32, 96)              # inconsistent lengths
    assert lib.kivi_mf_decode_layer_lead(ctypes.byref(_mf_layer_desc()), bad, *LAYER_ARGS, LEAD, None) == EINVAL
    assert list(bad) == [64, 31, 63, 0, 32, 96]
    assert lib.kivi_mf_decode_layer_lead(None, None, None, 0, 0, 0, None, 0, 0, None, 0, 0, None, 0, None, 0, 0, LEAD, None) == EINVAL


def test_mf_decode_layer_dyn_lead_refuses_what_the_dyn_entry_refuses(lib):
    from kivi_amd import _lib
    d, ok = _mf_layer_desc(s_pitch=600), _step()
    cases = ((ok, None, d), (_lib.MfStep(Tq=64, Tv=63, k_res_len=31, v_res_len=32, v_win_start=5, v_flush=0), 0x1000, d),
             (ok, 0x1000, _mf_layer_desc(s_pitch=520)), (ok, 0x1000, _mf_layer_desc(flags=0, s_pitch=600)), (ok, 0x1004, d))
    for hs, dev, desc in cases:
        rc_old, msg_old = lib.kivi_mf_decode_layer_dyn(ctypes.byref(desc), ctypes.byref(hs), dev, *LAYER_ARGS, None), lib.kivi_last_error()
        assert rc_old < 0
        for lead in (None, LEAD):
            rc = lib.kivi_mf_decode_layer_dyn_lead(ctypes.byref(desc), ctypes.byref(hs), dev, *LAYER_ARGS, lead, None)
            assert (rc, lib.kivi_last_error()) == (rc_old, msg_old)


# ------------------------------------------------------------------ 3. the plan on the host, under sanitizers
def test_lead_plan_visits_exactly_the_live_units_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "lead_plan")
    # the sanitizer runtimes are linked into the program (clang's default), so it does not depend on the order libraries load in
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "lead_plan_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "lead plan ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------ 4. the model on CPU
class _Cache:
    """Stands in for a living layer cache on CPU: the lengths move as a cache's do, every call that matters is written to `log`.
    `decode_step` has the signature of before the lead: a caller that hands it one raises."""
    rebase_quantum, rebase_limit = 32, 1 << 20

    def __init__(self, cfg, B, nh_kv, log, kv=0):
        self.cfg, self.B, self.nh_kv, self.log, self.kv_seq_len = cfg, B, nh_kv, log, kv
        self.k_res = torch.zeros(1)

    def prefill(self, k, v):
        self.B, self.kv_seq_len = k.shape[0], k.shape[2]

    def as_tuple(self):
        from kivi_amd.cache import KiviCacheTuple
        return KiviCacheTuple(self)

    def ensure_room(self, n):
        pass

    def _step(self, q, mask, lead):
        self.log.append(("decode", mask, lead))
        self.kv_seq_len += 1
        return torch.zeros_like(q)

    def decode_step(self, q, k, v, attention_mask=None, out=None, fused_kernels=True):
        return self._step(q, attention_mask, "not passed")

    def clone(self):
        return type(self)(self.cfg, self.B, self.nh_kv, self.log, self.kv_seq_len)

    def index_select(self, rows):
        return type(self)(self.cfg, len(rows), self.nh_kv, self.log, self.kv_seq_len)

    def reorder_(self, beam_idx, **kw):
        return self

    def admit_(self, rows, src, check=False, offset=0):
        self.log.append(("admit", rows.tolist(), offset))

    def check_rebase(self, drop):
        assert drop % 32 == 0 and 0 < drop < self.kv_seq_len

    def rebase_(self, drop):
        self.log.append(("rebase", drop))
        self.kv_seq_len -= drop
        return self


class _LeadCache(_Cache):
    """The same with today's signature."""

    def decode_step(self, q, k, v, attention_mask=None, out=None, fused_kernels=True, lead=None):
        return self._step(q, attention_mask, lead)


def _model(option, monkeypatch, log, cache=None):
    import kivi_amd.attention as A
    from kivi_amd.attention import KiviConfig
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    kw = {} if option is None else dict(decode_lead=option)
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=2,
                           intermediate_size=256, vocab_size=64), residual_length=32, **kw)
    assert cfg.kivi_decode_lead is bool(option)
    torch.manual_seed(3)
    model = LlamaForCausalLM_KIVI(cfg, A.LlamaAttention_KIVI)
    cls = cache or (_LeadCache if option else _Cache)
    monkeypatch.setattr(A, "make_layer_cache", lambda c, B, nh_kv, *a, **k: cls(KiviConfig(2, 2, 32, 32), B, nh_kv, log))
    return model


def _leading_masked(mask):
    """leading keys at the fp16 minimum of every row of an additive (B, 1, 1, n) key row"""
    return ((mask[:, 0, 0] != MIN16).cumsum(-1) == 0).sum(-1).tolist()


IDS = torch.tensor([[0, 0, 0, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7], [0, 9, 8, 7, 6, 5, 4]])
MASK = torch.tensor([[0, 0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1, 1]])


def test_the_option_is_off_by_default_and_then_nothing_new_runs(monkeypatch):
    import kivi_amd.generation as G
    import kivi_amd.llama  # noqa: F401  (everything that binds the names patched below is imported first)
    monkeypatch.setattr(G, "leading_pads", lambda m: pytest.fail("a lead was derived with the option off"))
    monkeypatch.setattr(G.DecodeLead, "__init__", lambda self, *a: pytest.fail("a DecodeLead was built with the option off"))
    runs = []
    for option in (None, False):
        log = []
        model = _model(option, monkeypatch, log)                  # (_Cache: a lead handed to its decode_step raises)
        out = model.generate(IDS, 3, attention_mask=MASK)
        model.generate(IDS, 2, attention_mask=MASK, num_beams=2)
        model.generate_continuous([list(range(1, 41)), [5, 6, 7], list(range(1, 34)), [9, 8]], 3, batch_size=2, compact=32)
        dec = [e for e in log if e[0] == "decode"]
        assert dec and all(torch.is_tensor(m) and m.dtype == torch.float16 and lead == "not passed" for _, m, lead in dec)
        runs.append((out, [(tuple(m.shape), _leading_masked(m)) for _, m, _ in dec], [e for e in log if e[0] != "decode"]))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]


def test_left_padded_generate_hands_every_step_the_leading_zeros(monkeypatch):
    log = []
    model = _model(True, monkeypatch, log)
    model.generate(IDS, 3, attention_mask=MASK)
    dec = [e for e in log if e[0] == "decode"]
    assert len(dec) == 2 * 3                                       # layers x steps
    for i, (_, mask, lead) in enumerate(dec):
        assert tuple(mask.shape) == (3, 1, 1, 7 + 1 + i // 2) and mask.dtype == torch.float16
        assert lead.dtype == torch.int32 and lead.tolist() == [3, 0, 1] == _leading_masked(mask)
    # over beams: repeated like the rows
    log.clear()
    model.generate(IDS, 2, attention_mask=MASK, num_beams=2)
    dec = [e for e in log if e[0] == "decode"]
    assert dec and all(lead.tolist() == [3, 3, 0, 0, 1, 1] == _leading_masked(mask) and mask.shape[0] == 6 for _, mask, lead in dec)
    # without a pad nothing is derived: the unmasked step
    log.clear()
    model.generate(IDS, 2, attention_mask=torch.ones_like(MASK))
    assert all(mask is None and lead is None for _, mask, lead in log if _ == "decode")


@pytest.mark.parametrize("short", [False, True], ids=["admit_at_L", "admit_at_offset"])
def test_scheduler_rederives_the_lead_from_every_changed_mask(monkeypatch, short):
    log = []
    model = _model(True, monkeypatch, log)
    # row 0: a long request that outlives the others; row 1: short requests that finish and are replaced.  The caches grow past the
    # prompts, so later admissions are padded (or admitted at an offset), and `compact` rebases once the long prompt's pads allow it.
    prompts = [[3] * 40, [5, 6, 7], [4] * 33, [9, 8], [7] * 3]
    limits = [80, 2, 30, 2, 40]
    model.generate_continuous(prompts, limits, batch_size=2, compact=32, short_admissions=short)
    kinds = [e[0] for e in log]
    assert "admit" in kinds and "rebase" in kinds and "decode" in kinds
    offsets = [e[2] for e in log if e[0] == "admit"]
    assert any(o > 0 for o in offsets) if short else all(o == 0 for o in offsets)
    seen_lead_over_quantum = False
    prev, drop, admitted = None, 0, set()
    for e in log:
        if e[0] == "rebase":
            drop += e[1]
        elif e[0] == "admit":
            admitted |= set(e[1])
            last_offset = e[2]
        elif e[0] == "decode":
            _, mask, lead = e
            assert lead.dtype == torch.int32 and lead.tolist() == _leading_masked(mask), "the lead is the mask's leading zeros"
            for b in admitted:                                    # an offset admission: the zeroed lead counts like any pad
                assert lead[b] >= last_offset
            if prev is not None and drop:                          # a rebase: reduced by the drop, floored at 0
                for b in set(range(2)) - admitted:
                    assert lead[b] == max(prev[b] - drop, 0)
            seen_lead_over_quantum |= max(lead.tolist()) >= 32
            prev, drop, admitted = lead.tolist(), 0, set()
    assert seen_lead_over_quantum


def test_a_rebase_reduces_the_lead_by_the_drop(monkeypatch):
    """model.rebase_ between two decode steps of the scheduler's own making: the mask loses its leading columns, so does the lead."""
    from kivi_amd.generation import decode_key_row, leading_pads
    m = torch.ones((3, 101), dtype=torch.long)
    m[0, :70] = 0
    m[1, :40] = 0
    before = decode_key_row(m, True)
    assert before.lead.tolist() == [70, 40, 0] == _leading_masked(before.mask) and before.lead.dtype == torch.int32
    after = decode_key_row(m[:, 64:], True)
    assert after.lead.tolist() == [6, 0, 0] == _leading_masked(after.mask)
    assert torch.is_tensor(decode_key_row(m, False)), "option off: the plain key row"
    assert leading_pads(torch.tensor([[0, 0, 1, 0, 1], [1, 0, 0, 1, 1]])).tolist() == [2, 0], "leading zeros, not all zeros"


def test_graph_owner_keys_on_the_lead_and_keeps_a_static_buffer(monkeypatch):
    from kivi_amd.graph import DecodeGraphs
    log = []
    model = _model(True, monkeypatch, log)
    g = DecodeGraphs(model, 3, "cpu", whole=True, padded=True, sampler=None, lead=True)
    assert g.lead.dtype == torch.int32 and tuple(g.lead.shape) == (3,)
    assert g.matches(3, True, True, None, True) and not g.matches(3, True, True, None, False) and not g.matches(3, True, True, None)
    off = DecodeGraphs(model, 3, "cpu", whole=True, padded=True)
    assert off.lead is None and off.matches(3, True, True, None) and not off.matches(3, True, True, None, True)
    assert DecodeGraphs(model, 3, "cpu", whole=True, padded=False, lead=True).lead is None, "no pads, no lead"
    # begin() refreshes it in place from the 2D mask, beside the mask buffer
    g.whole = False                                                # (no driver: the caches here are recorders)
    ptr = g.lead.data_ptr()
    cache = _LeadCache(None, 3, 2, log, kv=7)
    cache.n_sb, cache.cap = 1, 64
    m2 = torch.cat([MASK, torch.ones_like(MASK[:, :1])], dim=1)
    g.begin(torch.zeros((3, 1), dtype=torch.long), [cache], m2)
    assert g.lead.tolist() == [3, 0, 1] and g.lead.data_ptr() == ptr
    m2[1, :5] = 0                                                  # an admission rewrote row 1
    g.begin(torch.zeros((3, 1), dtype=torch.long), [cache], m2)
    assert g.lead.tolist() == [3, 5, 1] and g.lead.data_ptr() == ptr and _leading_masked(g.mask[..., :8]) == [3, 5, 1]


def test_prepare_graphs_builds_anew_exactly_when_a_key_field_changes(monkeypatch):
    model = _model(True, monkeypatch, [])

    def prepared(batch=3, **kw):
        model.prepare_graphs(batch, "cpu", whole=True, **kw)
        return model.graphs

    held = prepared()
    assert prepared() is held and held.matches(3, True, False, None), "the same arguments keep the object; the 4-argument form finds it"
    seen = [held]
    for kw in (dict(batch=2), dict(), dict(padded=True), dict(), dict(logprobs=0), dict(logprobs=3), dict()):
        new = prepared(**kw)
        assert all(new is not g for g in seen) and prepared(**kw) is new, kw
        assert (new.B, new.padded, new.logprobs) == (kw.get("batch", 3), kw.get("padded", False), kw.get("logprobs")) and new.whole
        assert (new.lp is None) == (new.logprobs is None) and (new.top_ids is None) == (not new.logprobs)
        seen.append(new)
    assert model.graphs.matches(3, True, False, None)
    # the lead is the model's decode_lead option, and only of a padded batch
    assert prepared().lead is None
    with_lead = prepared(padded=True)
    assert with_lead.lead is not None and with_lead.matches(3, True, True, None, True) and prepared(padded=True) is with_lead
    model.config.kivi_decode_lead = False
    without = prepared(padded=True)
    assert without is not with_lead and without.lead is None and without.matches(3, True, True, None) and prepared(padded=True) is without
    model.release_graphs()
    assert model.graphs is None


def test_hook_state_cache_takes_a_lead_and_steps_as_before(monkeypatch):
    from kivi_amd.attention import kivi_attention_decode
    from kivi_amd.cache import KiviLayerCache
    seen = []
    lc = KiviLayerCache.__new__(KiviLayerCache)
    lc._fused_unsupported = lc._attend_unfusable = False
    lc.cfg = None
    monkeypatch.setattr(KiviLayerCache, "ensure_room", lambda self, n: None)
    monkeypatch.setattr(KiviLayerCache, "_decode_native", lambda self, *a: seen.append(a) or a[0])
    monkeypatch.setattr(KiviLayerCache, "_decode_fused", lambda self, *a: seen.append(a + (None,)) or a[0])
    q = torch.zeros((2, 2, 1, 128), dtype=torch.float16)
    mask = torch.zeros((2, 1, 1, 9), dtype=torch.float16)
    kivi_attention_decode(q, q, q, lc, mask)
    kivi_attention_decode(q, q, q, lc, mask, lead=torch.tensor([4, 0], dtype=torch.int32))
    assert len(seen) == 2 and len(seen[0]) == len(seen[1]) == 5
    assert all(x is y for x, y in zip(seen[0], seen[1])), "the step of the hook-state layout gets what it always got"
