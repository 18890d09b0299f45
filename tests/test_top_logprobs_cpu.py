"""No GPU: the ABI entry kivi_token_top_logprobs (symbol, signature, every refusal with pointers that are never dereferenced), the fp64
restatement reference_top_logprobs against a brute-force ordering and against reference_token_logprobs, the ValueErrors of
top_logprobs() / score() / generate() / generate_graphed() / generate_continuous() before any device work, and the return types of
those five with the new arguments at their defaults."""
import ctypes
import functools
import os
import re

import pytest
import torch

from helpers import ROOT
from test_decode_lead_cpu import _model as _cpu_model

INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_symbol_signature_and_abi_version(lib):
    from kivi_amd import _lib
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert re.search(r"#define\s+KIVI_TOP_LOGPROBS_MAX\s+32\b", src) and re.search(r"#define\s+KIVI_ABI_VERSION\s+3\b", src)
    decl = re.search(r"\bint\s+kivi_token_top_logprobs\s*\(([^;]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert decl, "kivi_token_top_logprobs is not declared in include/kivi_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const void* logits", "int logits_bits", "int64_t row_stride", "int64_t N", "int V", "int k",
                      "const int64_t* targets", "int64_t target_stride", "int64_t ignore_index", "int64_t* out_top_ids",
                      "float* out_top_logprobs", "int64_t top_stride", "float* out_logprob", "float* out_lse", "int32_t* out_rank",
                      "kivi_stream_t stream"]
    ctype = {"int": ctypes.c_int32, "int64_t": ctypes.c_int64}
    want = [ctypes.c_void_p if "*" in p or p.startswith("kivi_stream_t") else ctype[p.split()[0]] for p in params]
    res, args = _lib.SIGNATURES["kivi_token_top_logprobs"]
    assert res is ctypes.c_int32 and list(args) == want
    assert hasattr(lib, "kivi_token_top_logprobs") and lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    from kivi_amd.scoring import TOP_LOGPROBS_MAX
    assert TOP_LOGPROBS_MAX == 32


def test_every_refusal_without_device(lib):
    """Every rejected argument returns a negative code before any HIP call (pointers are never dereferenced)."""
    from kivi_amd._lib import KiviHipError, check
    f = lib.kivi_token_top_logprobs
    p = ctypes.c_void_p
    lg, tg, ids, top, out = p(0x10000), p(0x20000), p(0x30000), p(0x40000), p(0x50000)

    def call(logits=lg, bits=16, row_stride=320, N=4, V=320, k=5, targets=tg, target_stride=1, ignore=-100, ids=ids, top=top,
             top_stride=5, o=out, lse=None, rank=None):
        return f(logits, bits, row_stride, N, V, k, targets, target_stride, ignore, ids, top, top_stride, o, lse, rank, None)

    einval = [(dict(bits=8), b"logits_bits"), (dict(bits=64), b"logits_bits"), (dict(N=0), b"N="), (dict(N=-3), b"N="),
              (dict(V=0, k=1), b"V="), (dict(V=(1 << 20) + 1, row_stride=1 << 21), b"V="), (dict(row_stride=319), b"row_stride"),
              (dict(target_stride=0), b"target_stride"), (dict(logits=None), b"null"),
              # what the lists add
              (dict(k=0), b"k="), (dict(k=-1), b"k="), (dict(k=33, top_stride=33), b"k="), (dict(V=4, row_stride=4, k=5), b"k="),
              (dict(top_stride=4), b"top_stride"), (dict(ids=None), b"null"), (dict(top=None), b"null"),
              (dict(o=None), b"targets without out_logprob"), (dict(targets=None), b"without targets"),
              (dict(targets=None, o=None, rank=p(0x60000)), b"without targets")]
    for kw, word in einval:
        assert call(**kw) == -1, kw
        assert word in lib.kivi_last_error(), (kw, lib.kivi_last_error())
    for kw in (dict(logits=p(0x10001)), dict(logits=p(0x10002), bits=32), dict(targets=p(0x20004)), dict(o=p(0x50002)),
               dict(lse=p(0x60001)), dict(rank=p(0x70003)), dict(ids=p(0x30004)), dict(top=p(0x40002))):
        assert call(**kw) == -2, kw
        assert b"misaligned" in lib.kivi_last_error()
    # targets are checked only when given: without them a zero target_stride is not what gets refused
    assert call(targets=None, o=None, target_stride=0, k=0) == -1 and b"k=" in lib.kivi_last_error()
    with pytest.raises(KiviHipError):
        check(call(k=40), "kivi_token_top_logprobs")


def _brute(row, k):
    """Token j comes before j' iff x_j > x_j', or x_j == x_j' and j < j' (Python floats: -0.0 == 0.0)."""
    def before(a, b):
        (ja, xa), (jb, xb) = a, b
        return -1 if (xa > xb or (xa == xb and ja < jb)) else 1
    order = sorted(enumerate(row), key=functools.cmp_to_key(before))
    return [j for j, _ in order[:k]]


def test_reference_against_a_brute_force_ordering():
    from kivi_amd.scoring import reference_top_logprobs
    rows = [[1.0, 3.0, 3.0, 0.5, 3.0, -0.0, 0.0], [0.0, -0.0, -0.0, 0.0, -1.0], [-INF, 2.0, -INF, 2.0, 1.0, -INF],
            [5.0], [-0.0, 0.0], [2.0, 2.0, 2.0, 2.0], [-INF, -INF, 0.25, -INF],
            [0.5, -3.0, 7.0, 7.0, -0.0, 0.0, 1.0, -INF, 7.0, 0.5, 0.5, -2.0]]
    g = torch.Generator().manual_seed(0)
    rows += [torch.randint(-2, 3, (12,), generator=g).float().tolist() for _ in range(20)]
    for row in rows:
        for dtype in (torch.float16, torch.float32):
            x = torch.tensor([row]).to(dtype)
            for k in range(1, len(row) + 1):
                ids, lps = reference_top_logprobs(x, k)
                assert ids.dtype == torch.int64 and lps.dtype == torch.float64 and ids.shape == lps.shape == (1, k)
                want = _brute(row, k)
                assert ids[0].tolist() == want, (row, k)
                full = torch.log_softmax(x.double(), -1)[0]
                for i, j in enumerate(want):
                    if row[j] == -INF:
                        assert lps[0, i].item() == -INF
                    else:
                        assert abs(lps[0, i].item() - full[j].item()) <= 1e-12
    # leading dimensions are kept
    x = torch.randn((2, 3, 9), generator=g)
    ids, lps = reference_top_logprobs(x, 4)
    assert ids.shape == lps.shape == (2, 3, 4) and torch.equal(ids[..., 0], x.argmax(-1))


def test_reference_agrees_with_reference_token_logprobs():
    from kivi_amd.scoring import reference_token_logprobs, reference_top_logprobs
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-3, 4, (40, 12), generator=g).float()          # many ties
    x[::5, 3] = -INF
    x[1::7, 2] = -0.0
    t = torch.randint(0, 12, (40,), generator=g)
    lp, _, rank = reference_token_logprobs(x, t)
    ids, lps = reference_top_logprobs(x, 12)
    rows = torch.arange(40)
    assert torch.equal(ids[rows, rank], t) and torch.equal(lps[rows, rank], lp)
    assert torch.equal(ids.sort(-1).values, torch.arange(12).expand(40, 12))      # k == V: a permutation of the vocabulary


def test_top_logprobs_argument_errors_come_before_device_work():
    """On the CPU any device work raises KiviHipError (no CPU path): a ValueError shows the check came first."""
    from kivi_amd._lib import KiviHipError
    from kivi_amd.scoring import top_logprobs
    x = torch.randn(3, 10)
    for k in (0, -1, 11, 33, 2.0, True, None):
        with pytest.raises(ValueError, match="k="):
            top_logprobs(x, k)
    with pytest.raises(ValueError, match="k="):
        top_logprobs(torch.randn(3, 100), 33)
    with pytest.raises(ValueError, match="return_rank"):
        top_logprobs(x, 3, return_rank=True)
    with pytest.raises(KiviHipError):                            # valid arguments: no CPU fallback
        top_logprobs(x, 3)
    with pytest.raises(KiviHipError):
        top_logprobs(x, 3, torch.zeros(3, dtype=torch.long))


def test_model_paths_refuse_bad_arguments_before_device_work(monkeypatch):
    from kivi_amd.sampling import SamplingParams
    log = []
    m = _cpu_model(None, monkeypatch, log)                       # vocab_size 64; its caches record every call
    ids = torch.randint(0, 64, (2, 12))
    for k in (-1, 33, 1.5, True):
        with pytest.raises(ValueError, match="top_logprobs"):
            m.score(ids, top_logprobs=k)
        for fn in (m.generate, m.generate_graphed):
            with pytest.raises(ValueError, match="top_logprobs"):
                fn(ids, 4, return_logprobs=True, top_logprobs=k)
        with pytest.raises(ValueError, match="top_logprobs"):
            m.generate_continuous([[1, 2, 3]], 4, batch_size=1, return_logprobs=True, top_logprobs=k)
    for fn in (m.generate, m.generate_graphed):
        with pytest.raises(ValueError, match="return_logprobs"):
            fn(ids, 4, top_logprobs=5)
    with pytest.raises(ValueError, match="return_logprobs"):
        m.generate_continuous([[1, 2, 3]], 4, batch_size=1, top_logprobs=5)
    with pytest.raises(ValueError):
        m.generate(ids, 4, num_beams=2, return_logprobs=True, top_logprobs=5)
    with pytest.raises(ValueError):
        m.generate_graphed(ids, 4, num_beams=2, return_logprobs=True, top_logprobs=5)
    with pytest.raises(ValueError, match="top_logprobs"):
        m.generate_graphed(ids, 4, do_sample=True, num_beams=2, return_logprobs=True, top_logprobs=5)
    with pytest.raises(ValueError, match="logprobs"):
        m.decode_graphed(ids[:, :1], [], 0, 1, logprobs=40)
    with pytest.raises(ValueError, match="top_logprobs"):
        m.generate_continuous([[1, 2, 3]], 4, batch_size=1, sampling=SamplingParams(True, seed=1), return_logprobs=True,
                              top_logprobs=65)
    assert log == [], "a refused call reached the caches"
    # a small vocabulary bounds k
    from kivi_amd.scoring import check_top_k, check_top_logprobs
    check_top_k(7, 7)
    with pytest.raises(ValueError):
        check_top_k(8, 7)
    check_top_logprobs(0, False, 4, 7)                           # off: nothing to refuse


def test_defaults_leave_the_return_types_unchanged(monkeypatch):
    import kivi_amd.scoring as S
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    log = []
    m = _cpu_model(None, monkeypatch, log)
    monkeypatch.setattr(S, "top_logprobs", lambda *a, **k: pytest.fail("top_logprobs ran with the option off"))
    monkeypatch.setattr(S, "score_into", lambda *a, **k: pytest.fail("score_into ran with the option off"))
    calls = []

    def fake_token_logprobs(logits, targets, ignore_index=-100, return_lse=False, return_rank=False):
        calls.append(tuple(logits.shape))
        lp = torch.zeros(targets.shape, dtype=torch.float32)
        return (lp, torch.zeros(targets.shape, dtype=torch.int32)) if return_rank else lp

    monkeypatch.setattr(S, "token_logprobs", fake_token_logprobs)
    import kivi_amd.generation  # noqa: F401  (decode_loop imports token_logprobs from kivi_amd.scoring when it runs)
    ids = torch.randint(1, 64, (2, 9))
    res = m.score(ids)
    assert len(res) == 3 and res[0].shape == (2, 8) and len(m.score(ids, return_rank=True)) == 4 and len(calls) == 2
    out = m.generate(ids, 3)
    assert torch.is_tensor(out) and out.shape == (2, 12) and len(calls) == 2
    seqs, lps = m.generate(ids, 3, return_logprobs=True)
    assert seqs.shape == (2, 12) and lps.shape == (2, 3) and len(calls) == 5          # one launch per step, as before
    toks = m.generate_continuous([[1, 2, 3], [4, 5], [6]], 3, batch_size=2)
    assert isinstance(toks, list) and len(toks) == 3 and all(torch.is_tensor(t) and t.shape == (3,) for t in toks) and len(calls) == 5
    # generate_graphed / decode_graphed: the graphed step itself needs a device; what the call hands it and returns does not
    seen = {}

    def fake_decode_graphed(self, tok, pasts, position, steps, attention_mask=None, sampler=None, sampling=None, **kw):
        seen.update(kw)
        self.graphs = type("G", (), {"end": lambda s: None})()
        return tok.expand(-1, steps)

    monkeypatch.setattr(LlamaForCausalLM_KIVI, "decode_graphed", fake_decode_graphed)
    out = m.generate_graphed(ids, 3)
    assert torch.is_tensor(out) and out.shape == (2, 12) and seen == {} and len(calls) == 5
