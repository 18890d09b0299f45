"""CPU: repetition / presence / frequency penalties in the fused row sampler (kivi_sample_rows_pen, kivi_seen_mark;
kivi_amd.sampling).

* The library exports both entries with the signatures of include/kivi_hip.h; the ABI version is still 3.
* Every refusal of both entries, with fake pointers that are never dereferenced: nothing is enqueued.
* The penalty record: 16 bytes, field for field the struct of the header; SamplingParams' ranges; the bytes RowSampler writes.
* reference_penalise against transformers' RepetitionPenaltyLogitsProcessor (bit-equal in fp32) and against an fp64 evaluation of
  the rule.
* The refusals of generate / generate_graphed, raised before any forward pass, and the routing of the keyword arguments in
  resolve_sampler.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "kivi_hip.h")).read()


def _declared_args(name):
    """The parameter names of `name`'s declaration in the header."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src).group(1)
    return [a.split()[-1].lstrip("*") for a in args.split(",")]


def test_symbols_and_signatures(lib):
    from kivi_amd import _lib
    want = {"kivi_sample_rows_pen": ["logits", "logits_bits", "row_stride", "B", "V", "rows", "draw_index", "pen", "seen",
                                     "seen_stride", "out_tokens", "out_stride", "stream"],
            "kivi_seen_mark": ["seen", "seen_stride", "V", "rows", "n", "tokens", "tok_row_stride", "T", "lead", "flags", "stream"]}
    for name, names in want.items():
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and _declared_args(name) == names and len(args) == len(names)
        for a, t in zip(names, args):                            # strides are 64-bit, pointers void*, the rest int
            assert t is (ctypes.c_int64 if a.endswith("stride") else
                         ctypes.c_int if a in ("logits_bits", "B", "V", "n", "T", "flags") else ctypes.c_void_p), (name, a)
    assert _lib.SIGNATURES["kivi_sample_rows"][1] == _lib.SIGNATURES["kivi_sample_rows_pen"][1][:7] + \
        _lib.SIGNATURES["kivi_sample_rows_pen"][1][10:]          # the sibling's arguments around pen, seen, seen_stride
    assert lib.kivi_abi_version() == 3
    src = _header()
    from kivi_amd import sampling as S
    for flag in ("CLEAR", "PROMPT", "OUTPUT"):
        assert int(re.search(r"#define KIVI_SEEN_%s (\d+)" % flag, src).group(1)) == getattr(S, "SEEN_" + flag)


GOOD = dict(logits=1 << 20, bits=16, rs=320, B=2, V=320, rows=1 << 21, idx=1 << 22, pen=1 << 24, seen=1 << 25, ss=320, out=1 << 23,
            os=1)
BAD = {
    "bits": dict(bits=8), "B0": dict(B=0), "B_big": dict(B=65536), "V0": dict(V=0),
    "V_big": dict(V=(1 << 20) + 1, rs=1 << 21, ss=1 << 21), "row_stride": dict(rs=100), "out_stride": dict(os=0),
    "null_logits": dict(logits=None), "null_rows": dict(rows=None), "null_draw_index": dict(idx=None), "null_out": dict(out=None),
    "null_pen": dict(pen=None), "null_seen": dict(seen=None), "seen_stride": dict(ss=312),
}
MISALIGNED = {"logits16": dict(logits=(1 << 20) + 1), "logits32": dict(bits=32, logits=(1 << 20) + 2),
              "rows": dict(rows=(1 << 21) + 4), "draw_index": dict(idx=(1 << 22) + 4), "out": dict(out=(1 << 23) + 4),
              "pen": dict(pen=(1 << 24) + 2), "seen": dict(seen=(1 << 25) + 8), "seen_stride": dict(ss=324)}


def _pen(lib, a):
    return lib.kivi_sample_rows_pen(a["logits"], a["bits"], a["rs"], a["B"], a["V"], a["rows"], a["idx"], a["pen"], a["seen"],
                                    a["ss"], a["out"], a["os"], None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_pen_refuses_bad_arguments(lib, case):
    assert _pen(lib, {**GOOD, **BAD[case]}) == -1               # KIVI_EINVAL
    assert b"kivi_sample_rows_pen" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MISALIGNED))
def test_pen_refuses_misaligned(lib, case):
    assert _pen(lib, {**GOOD, **MISALIGNED[case]}) == -2        # KIVI_EALIGN
    assert b"kivi_sample_rows_pen" in lib.kivi_last_error()


MARK = dict(seen=1 << 25, ss=320, V=320, rows=1 << 21, n=2, tok=1 << 22, ts=7, T=7, lead=1 << 23, flags=2)
MARK_BAD = {
    "flags0": dict(flags=0), "flags_unknown": dict(flags=8), "prompt_and_output": dict(flags=6), "V0": dict(V=0),
    "V_big": dict(V=(1 << 20) + 1, ss=1 << 21), "n0": dict(n=0), "n_big": dict(n=65536), "T_negative": dict(T=-1),
    "null_seen": dict(seen=None), "seen_stride": dict(ss=312), "null_tokens": dict(tok=None), "tok_row_stride": dict(ts=6),
}
MARK_MISALIGNED = {"seen": dict(seen=(1 << 25) + 8), "seen_stride": dict(ss=324), "rows": dict(rows=(1 << 21) + 2),
                   "tokens": dict(tok=(1 << 22) + 4), "lead": dict(lead=(1 << 23) + 2)}


def _mark(lib, a):
    return lib.kivi_seen_mark(a["seen"], a["ss"], a["V"], a["rows"], a["n"], a["tok"], a["ts"], a["T"], a["lead"], a["flags"], None)


@pytest.mark.parametrize("case", sorted(MARK_BAD))
def test_mark_refuses_bad_arguments(lib, case):
    assert _mark(lib, {**MARK, **MARK_BAD[case]}) == -1
    assert b"kivi_seen_mark" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MARK_MISALIGNED))
def test_mark_refuses_misaligned(lib, case):
    assert _mark(lib, {**MARK, **MARK_MISALIGNED[case]}) == -2
    assert b"kivi_seen_mark" in lib.kivi_last_error()


def test_mark_without_work_enqueues_nothing(lib):
    """T == 0 without CLEAR: returns 0 before any HIP call (the fake pointers would fault otherwise)."""
    for flags in (2, 4):
        assert _mark(lib, {**MARK, "T": 0, "tok": None, "flags": flags}) == 0


def test_penalty_record_matches_header():
    from kivi_amd.sampling import SamplePenalty
    body = re.search(r"typedef struct \{([^}]*)\}\s*kivi_sample_penalty;", _header()).group(1)
    fields = re.findall(r"(\w+)\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert [(n, ctype[t]) for t, n in fields] == list(SamplePenalty._fields_)
    assert [n for _, n in fields] == ["repetition", "presence", "frequency", "reserved"]
    assert [getattr(SamplePenalty, n).offset for _, n in fields] == [0, 4, 8, 12]
    assert ctypes.sizeof(SamplePenalty) == 16 and ctypes.alignment(SamplePenalty) == 4
    from kivi_amd.sampling import SampleRow
    assert ctypes.sizeof(SampleRow) == 32                          # the row record does not change


@pytest.mark.parametrize("kw,match", [(dict(repetition_penalty=0.0), "repetition_penalty"),
                                      (dict(repetition_penalty=-1.5), "repetition_penalty"),
                                      (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                                      (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                                      (dict(repetition_penalty="1.2"), "repetition_penalty"),
                                      (dict(repetition_penalty=True), "repetition_penalty"),
                                      (dict(presence_penalty=float("nan")), "presence_penalty"),
                                      (dict(presence_penalty=float("-inf")), "presence_penalty"),
                                      (dict(presence_penalty=None), "presence_penalty"),
                                      (dict(frequency_penalty=float("inf")), "frequency_penalty"),
                                      (dict(frequency_penalty="x"), "frequency_penalty"),
                                      (dict(do_sample=False, frequency_penalty=float("nan")), "frequency_penalty")])
def test_sampling_params_penalty_refusals(kw, match):
    from kivi_amd.sampling import SamplingParams
    with pytest.raises(ValueError, match=match):
        SamplingParams(**kw)


def test_sampling_params_penalties():
    from kivi_amd.sampling import RowSampler, SamplingParams
    p = SamplingParams()
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.0, 0.0, 0.0) and not p.penalised
    q = SamplingParams(repetition_penalty=1.3, presence_penalty=-0.5, frequency_penalty=2, seed=4)
    assert q.penalties == (1.3, -0.5, 2.0) and q.penalised and isinstance(q.frequency_penalty, float)
    assert q != SamplingParams(seed=4) and hash(q) != hash(SamplingParams(seed=4))
    assert q == SamplingParams(repetition_penalty=1.3, presence_penalty=-0.5, frequency_penalty=2.0, seed=4)
    assert "repetition_penalty=1.3" in repr(q) and "frequency_penalty=2.0" in repr(q)
    r = dataclasses.replace(q, seed=9)                              # what binding a seed does: the penalties travel
    assert r.penalties == q.penalties and r.seed == 9
    assert dataclasses.replace(q, presence_penalty=0.25).penalties == (1.3, 0.25, 2.0)
    assert RowSampler._bind(SamplingParams(frequency_penalty=0.5)).penalties == (1.0, 0.0, 0.5)
    with pytest.raises(dataclasses.FrozenInstanceError):
        q.repetition_penalty = 1.0
    assert SamplingParams(do_sample=False, presence_penalty=1.0).penalised     # greedy rows are penalised too


def test_row_sampler_penalty_state_host_side():
    """What needs no GPU: allocation, record bytes, the key, set_row's record, select, reset, the refusals."""
    from kivi_amd.sampling import RowSampler, SamplePenalty, SamplingParams
    a, b = SamplingParams(seed=1), SamplingParams(seed=2, repetition_penalty=1.3, presence_penalty=0.6, frequency_penalty=0.25)
    with pytest.raises(ValueError, match="vocab_size="):
        RowSampler([a, b], "cpu")
    for bad in (0, -3, (1 << 20) + 1, 2.5, True):
        with pytest.raises(ValueError, match="vocab_size"):
            RowSampler([a], "cpu", vocab_size=bad)
    plain = RowSampler([a, a], "cpu")
    assert plain.seen is None and plain.penalties is None and len(plain.key()) == 4
    with pytest.raises(ValueError, match="vocab_size="):
        plain.set_row(0, b)
    plain.observe_prompt(torch.zeros((2, 3), dtype=torch.long))        # nothing to mark: a no-op
    rs = RowSampler([a, b], "cpu", vocab_size=13)
    assert rs.seen.shape == (2, 16) and rs.seen.dtype == torch.int16 and not rs.seen.any() and rs.seen.data_ptr() % 16 == 0
    assert rs.penalties.shape == (2, 4) and rs.penalties.dtype == torch.float32
    assert rs.key() == ("rows", 2, rs.records.data_ptr(), rs.draw_index.data_ptr(), rs.penalties.data_ptr(), rs.seen.data_ptr())
    rec = SamplePenalty.from_buffer_copy(rs.penalties[1].numpy().tobytes())
    f32 = lambda v: float(np.float32(v))                                # noqa: E731
    assert (rec.repetition, rec.presence, rec.frequency, rec.reserved) == (f32(1.3), f32(0.6), 0.25, 0)
    assert rs.penalties[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert RowSampler([a], "cpu", vocab_size=16).seen.shape == (1, 16)  # neutral rows with vocab_size=: the table exists
    rs.seen[0, 3], rs.seen[1, 5] = 7, -32768
    sel = rs.select([1, 1, 0])
    assert sel.seen.shape == (3, 16) and sel.seen[:, 5].tolist() == [-32768, -32768, 0] and sel.seen[2, 3] == 7
    assert torch.equal(sel.penalties[0], rs.penalties[1]) and torch.equal(sel.penalties[2], rs.penalties[0])
    assert sel.seen.data_ptr() != rs.seen.data_ptr() and sel.vocab_size == 13
    rs.draw_index += 2
    rs.reset()
    assert not rs.seen.any() and rs.draw_index.tolist() == [0, 0]
    with pytest.raises(Exception, match="GPU"):                        # marking is a kernel: no CPU path
        rs.observe_prompt(torch.zeros((2, 3), dtype=torch.long))
    for bad in (lambda: rs.observe_prompt(torch.zeros((3, 3), dtype=torch.long)),
                lambda: rs.observe_prompt(torch.zeros((2, 3), dtype=torch.long), attention_mask=torch.ones((2, 4))),
                lambda: rs.observe_prompt(torch.zeros((2, 3), dtype=torch.long), attention_mask=torch.ones((2, 3)),
                                          lead=torch.zeros(2, dtype=torch.int32)),
                lambda: rs.observe_prompt(torch.zeros((2, 3), dtype=torch.long), lead=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ reference_penalise
def _case(B=3, V=97, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((B, V), generator=g) * 4).half()
    x[:, ::7] = 0.0
    x[:, 1::13] = -0.0
    prompt = torch.rand((B, V), generator=g) < 0.3
    counts = torch.randint(0, 4, (B, V), generator=g) * (torch.rand((B, V), generator=g) < 0.4)
    counts[0, 5], counts[1, 6] = 32767, 5
    return x, prompt, counts


def test_reference_penalise_equals_hf_repetition_penalty():
    transformers = pytest.importorskip("transformers")
    from kivi_amd.sampling import reference_penalise
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float16, torch.float32):
        for theta in (0.5, 1.3, 1.0):
            x = (torch.randn((4, 211), generator=g) * 5).to(dtype)
            x[:, ::9] = 0.0
            ids = torch.randint(0, 211, (4, 37), generator=g)             # unpadded ids, duplicates among them
            want = transformers.RepetitionPenaltyLogitsProcessor(penalty=theta)(ids, x.float().clone())
            prompt = torch.zeros((4, 211), dtype=torch.bool).scatter_(1, ids, True)
            got = reference_penalise(x, prompt, torch.zeros((4, 211), dtype=torch.long), theta, 0.0, 0.0)
            assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), (dtype, theta)
            # HF's processor sees generated tokens exactly as prompt tokens: a count without a prompt bit gives the same
            counts = torch.zeros((4, 211), dtype=torch.long).scatter_add_(1, ids, torch.ones_like(ids))
            again = reference_penalise(x, torch.zeros_like(prompt), counts, theta, 0.0, 0.0)
            assert torch.equal(again.view(torch.int32), want.view(torch.int32))


def test_reference_penalise_against_fp64_rule():
    """Every step of the rule is one fp32 operation: evaluated in fp64 and rounded step by step it has to give the same bits
    (a product or quotient of two fp32 values, and a difference, round once from fp64 exactly as in fp32: 2 * 24 + 2 <= 53)."""
    from kivi_amd.sampling import reference_penalise
    x, prompt, counts = _case()
    theta = torch.tensor([0.5, 1.3, 1.0])
    pres = torch.tensor([-0.7, 0.6, 0.0])
    freq = torch.tensor([0.25, 0.0, 1e4])
    got = reference_penalise(x, prompt, counts, theta, pres, freq)
    f32 = lambda t: t.float().double()                                  # noqa: E731  (one rounding to fp32)
    X, th, pr, fr = x.double(), theta.double()[:, None], pres.double()[:, None], freq.double()[:, None]
    seen = prompt | (counts > 0)
    X = torch.where(seen, torch.where(X > 0, f32(X / th), f32(X * th)), X)
    X = f32(X - f32(fr * counts.double()))
    X = torch.where(counts > 0, f32(X - pr), X)
    assert torch.equal(got.double(), X) and torch.equal(torch.signbit(got), torch.signbit(X))
    # neutral records change nothing, whatever the history; scalars broadcast like one value per row
    assert torch.equal(reference_penalise(x, prompt, counts, 1.0, 0.0, 0.0).view(torch.int32), x.float().view(torch.int32))
    assert torch.equal(reference_penalise(x, prompt, counts, 1.3, 0.6, 0.25),
                       reference_penalise(x, prompt, counts, [1.3] * 3, [0.6] * 3, [0.25] * 3))
    # the pieces: presence once per emitted token, frequency per occurrence, repetition over prompt or output, sign-aware
    one = torch.tensor([[2.0, -2.0, 2.0, -2.0, 2.0, 0.0]])
    pm = torch.tensor([[True, True, False, False, False, True]])
    ct = torch.tensor([[0, 0, 3, 3, 0, 2]])
    assert reference_penalise(one, pm, ct, 2.0, 0.5, 0.25).tolist() == [[1.0, -4.0, 1.0 - 0.75 - 0.5, -4.0 - 0.75 - 0.5, 2.0,
                                                                         0.0 - 0.5 - 0.5]]


def test_seen_words():
    from kivi_amd.sampling import seen_words
    t = torch.tensor([[0, 1, -32768, -32767, 32767, -1, 5, 9]], dtype=torch.int16)
    prompt, counts = seen_words(t, 7)
    assert prompt.tolist() == [[False, False, True, True, False, True, False]]
    assert counts.tolist() == [[0, 1, 0, 1, 32767, 32767, 5]]


# ------------------------------------------------------------------ generate: refusals and routing
def _kivi_model():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_generate_penalty_refusals(monkeypatch):
    from kivi_amd.sampling import SamplingParams
    model = _kivi_model()
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    ids = torch.zeros((2, 5), dtype=torch.long)
    p = SamplingParams(seed=1, repetition_penalty=1.2)
    for fn in (model.generate, model.generate_graphed):
        for kw, match in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
                          (dict(presence_penalty=float("inf")), "presence_penalty"), (dict(frequency_penalty="1"), "frequency_penalty")):
            with pytest.raises(ValueError, match=match):
                fn(ids, 3, **kw)
        for kw in (dict(repetition_penalty=1.3), dict(presence_penalty=0.5), dict(frequency_penalty=-0.5)):
            with pytest.raises(ValueError, match="cannot be combined"):
                fn(ids, 3, sampling=p, **kw)                        # with sampling= the penalties come from the SamplingParams
            with pytest.raises(ValueError, match="beam"):
                fn(ids, 3, num_beams=2, **kw)
        with pytest.raises(ValueError, match="temperature"):        # the other arguments are validated as before
            fn(ids, 3, repetition_penalty=1.3, do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match="num_return_sequences"):   # n samples per prompt stay a feature of sampling=
        model.generate(ids, 3, repetition_penalty=1.3, num_return_sequences=2)


def test_resolve_sampler_routes_the_penalties():
    from kivi_amd.generation import resolve_sampler
    from kivi_amd.sampling import RowSampler, Sampler, SamplingParams
    base = ("cpu", 3, 1, 1)
    hf = (1.0, 50, 1.0, None)
    # neutral values: what the call did before
    assert resolve_sampler(*base, False, *hf, None, None) == (None, 1)
    assert resolve_sampler(*base, False, *hf, None, None, 1.0, 0.0, 0.0, 64) == (None, 1)
    assert isinstance(resolve_sampler(*base, True, *hf, 7, None, 1, 0, 0, 64)[0], Sampler)
    # a penalty without sampling=: identical rows, streams 0..B-1, the call's seed, greedy rows without do_sample
    pick, fan = resolve_sampler(*base, False, *hf, None, None, 1.3, 0.0, 0.2, 64)
    assert isinstance(pick, RowSampler) and fan == 1 and pick.B == 3 and pick.streams == [0, 1, 2] and pick.vocab_size == 64
    assert len(set(pick.params)) == 1 and not pick.params[0].do_sample and pick.params[0].penalties == (1.3, 0.0, 0.2)
    assert pick.seen.shape == (3, 64) and torch.equal(pick.penalties[:, :3], torch.tensor([[1.3, 0.0, 0.2]] * 3))
    pick, _ = resolve_sampler(*base, True, 0.7, 12, 0.9, 0.05, 11, None, presence_penalty=0.5, vocab_size=64)
    p = pick.params[0]
    assert (p.do_sample, p.temperature, p.top_k, p.top_p, p.min_p, p.seed, p.penalties) == (True, 0.7, 12, 0.9, 0.05, 11, (1.0, 0.5, 0.0))
    torch.manual_seed(5)
    drawn = resolve_sampler(*base, True, *hf, None, None, frequency_penalty=1.0, vocab_size=64)[0]
    assert len({q.seed for q in drawn.params}) == 1                     # seed=None: ONE seed drawn for the call, as Sampler does
    with pytest.raises(ValueError, match="vocab_size="):
        resolve_sampler(*base, False, *hf, None, None, 1.3)
    # sampling=: the table exists exactly when a request is penalised; fan rows repeat the request's record
    plain, pen = SamplingParams(seed=1), SamplingParams(seed=2, repetition_penalty=1.5)
    rs, fan = resolve_sampler("cpu", 3, 2, 1, False, *hf, None, [plain, pen, plain], vocab_size=64)
    assert fan == 2 and rs.B == 6 and rs.seen.shape == (6, 64) and rs.penalties[:, 0].tolist() == [1.0, 1.0, 1.5, 1.5, 1.0, 1.0]
    rs, _ = resolve_sampler("cpu", 3, 1, 1, False, *hf, None, plain, vocab_size=64)
    assert rs.seen is None and len(rs.key()) == 4
    mine = RowSampler([pen] * 3, "cpu", vocab_size=64)
    assert resolve_sampler("cpu", 3, 1, 1, False, *hf, None, mine, vocab_size=64)[0] is mine
    for kw in (dict(repetition_penalty=1.1), dict(presence_penalty=0.1), dict(frequency_penalty=0.1)):
        with pytest.raises(ValueError, match="cannot be combined"):
            resolve_sampler("cpu", 3, 1, 1, False, *hf, None, plain, vocab_size=64, **kw)


def test_continuous_arguments_keep_the_penalties():
    from kivi_amd.sampling import SamplingParams
    from kivi_amd.serving import check_arguments
    req = [SamplingParams(frequency_penalty=1e4), SamplingParams(seed=3)]
    _, _, params = check_arguments([[1, 2], [3]], 4, 2, None, 0, req, 64)
    assert params[0].penalties == (1.0, 0.0, 1e4) and params[0].seed is not None and not params[1].penalised
