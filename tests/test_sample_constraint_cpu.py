"""CPU: constrained decoding in the fused row sampler (kivi_sample_rows_con, kivi_allow_mark; kivi_amd.sampling; DESIGN.md
section 25).

* The library exports both entries with the signatures of include/kivi_hip.h; the ABI version is still 3.
* Every refusal of both entries, with fake pointers that are never dereferenced: nothing is enqueued.
* The constraint record and the list entry: field for field the structs of the header; SamplingParams' ranges, ==, hash, replace;
  the bytes RowSampler writes, the list sorted and merged, the suppress_until arithmetic, key() unchanged without constraints.
* reference_constrain against an fp64 evaluation of the rule rounded step by step, and -- on finite rows without a negative zero,
  which HF's dense additions turn into +0 where the rule leaves an unlisted token alone -- bit-equal to transformers' single-token
  SequenceBiasLogitsProcessor, MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor and PrefixConstrainedLogitsProcessor
  (all four exist in the transformers these tests were written against; one that a version lacks is skipped by name).
* The refusals and routing of generate / generate_graphed / resolve_sampler / generate_continuous' argument checks.
"""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "kivi_hip.h")).read()


def _declared_args(name):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    args = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src).group(1)
    return [a.split()[-1].lstrip("*") for a in args.split(",")]


def test_symbols_and_signatures(lib):
    from kivi_amd import _lib
    from kivi_amd import sampling as S
    want = {"kivi_sample_rows_con": ["logits", "logits_bits", "row_stride", "B", "V", "rows", "draw_index", "pen", "seen",
                                     "seen_stride", "con", "allow", "allow_stride", "list", "list_stride", "out_tokens", "out_stride",
                                     "stream"],
            "kivi_allow_mark": ["allow", "allow_stride", "V", "rows", "n", "tokens", "tok_row_stride", "T", "len", "flags", "stream"]}
    for name, names in want.items():
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and _declared_args(name) == names and len(args) == len(names)
        for a, t in zip(names, args):
            assert t is (ctypes.c_int64 if a.endswith("stride") else
                         ctypes.c_int if a in ("logits_bits", "B", "V", "n", "T", "flags") else ctypes.c_void_p), (name, a)
    pen, con = _lib.SIGNATURES["kivi_sample_rows_pen"][1], _lib.SIGNATURES["kivi_sample_rows_con"][1]
    assert con[:10] + con[15:] == pen                              # the sibling's arguments around con ... list_stride
    assert _lib.SIGNATURES["kivi_allow_mark"][1] == _lib.SIGNATURES["kivi_seen_mark"][1]
    assert lib.kivi_abi_version() == 3 and re.search(r"#define KIVI_ABI_VERSION 3\b", _header())
    src = _header()
    for flag in ("NONE", "ALL", "SET", "UNSET"):
        assert int(re.search(r"#define KIVI_ALLOW_%s (\d+)" % flag, src).group(1)) == getattr(S, "ALLOW_" + flag)
    assert int(re.search(r"#define KIVI_SAMPLE_MAX_LIST (\d+)", src).group(1)) == S.MAX_LIST == _lib.SAMPLE_MAX_LIST == 1024
    assert int(re.search(r"#define KIVI_CONSTRAINT_MASK (\d+)u", src).group(1)) == S.CONSTRAINT_MASK
    assert int(re.search(r"#define KIVI_LIST_TOKEN (0x[0-9A-Fa-f]+)u", src).group(1), 16) == S.LIST_TOKEN == S.MAX_TOKEN_ID
    assert int(re.search(r"#define KIVI_LIST_SUPPRESS (0x[0-9A-Fa-f]+)u", src).group(1), 16) == S.LIST_SUPPRESS


GOOD = dict(logits=1 << 20, bits=16, rs=320, B=2, V=320, rows=1 << 21, idx=1 << 22, pen=1 << 24, seen=1 << 25, ss=320, con=1 << 26,
            allow=1 << 27, as_=12, list=1 << 28, ls=1024, out=1 << 23, os=1)
BAD = {
    "bits": dict(bits=8), "B0": dict(B=0), "B_big": dict(B=65536), "V0": dict(V=0),
    "V_big": dict(V=(1 << 20) + 1, rs=1 << 21, ss=1 << 21, as_=1 << 16), "row_stride": dict(rs=100), "out_stride": dict(os=0),
    "null_logits": dict(logits=None), "null_rows": dict(rows=None), "null_draw_index": dict(idx=None), "null_out": dict(out=None),
    "null_pen_alone": dict(pen=None), "null_seen_alone": dict(seen=None), "seen_stride": dict(ss=312), "null_con": dict(con=None),
    "allow_stride": dict(as_=8), "list_stride_negative": dict(ls=-1), "list_stride_big": dict(ls=1025),
}
MISALIGNED = {"logits16": dict(logits=(1 << 20) + 1), "logits32": dict(bits=32, logits=(1 << 20) + 2),
              "rows": dict(rows=(1 << 21) + 4), "draw_index": dict(idx=(1 << 22) + 4), "out": dict(out=(1 << 23) + 4),
              "pen": dict(pen=(1 << 24) + 2), "seen": dict(seen=(1 << 25) + 8), "seen_stride": dict(ss=324),
              "con": dict(con=(1 << 26) + 4), "allow": dict(allow=(1 << 27) + 8), "allow_stride": dict(as_=14),
              "list": dict(list=(1 << 28) + 4)}


def _con(lib, a):
    return lib.kivi_sample_rows_con(a["logits"], a["bits"], a["rs"], a["B"], a["V"], a["rows"], a["idx"], a["pen"], a["seen"], a["ss"],
                                    a["con"], a["allow"], a["as_"], a["list"], a["ls"], a["out"], a["os"], None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_con_refuses_bad_arguments(lib, case):
    assert _con(lib, {**GOOD, **BAD[case]}) == -1                 # KIVI_EINVAL
    assert b"kivi_sample_rows_con" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MISALIGNED))
def test_con_refuses_misaligned(lib, case):
    assert _con(lib, {**GOOD, **MISALIGNED[case]}) == -2          # KIVI_EALIGN
    assert b"kivi_sample_rows_con" in lib.kivi_last_error()


MARK = dict(allow=1 << 25, as_=12, V=320, rows=1 << 21, n=2, tok=1 << 22, ts=7, T=7, len=1 << 23, flags=5)
MARK_BAD = {
    "flags0": dict(flags=0), "flags_unknown": dict(flags=16), "none_and_all": dict(flags=3), "set_and_unset": dict(flags=12),
    "all_four": dict(flags=15), "V0": dict(V=0), "V_big": dict(V=(1 << 20) + 1, as_=1 << 16), "n0": dict(n=0), "n_big": dict(n=65536),
    "T_negative": dict(T=-1), "null_allow": dict(allow=None), "allow_stride": dict(as_=8), "null_tokens": dict(tok=None),
    "tok_row_stride": dict(ts=6),
}
MARK_MISALIGNED = {"allow": dict(allow=(1 << 25) + 8), "allow_stride": dict(as_=14), "rows": dict(rows=(1 << 21) + 2),
                   "tokens": dict(tok=(1 << 22) + 4), "len": dict(len=(1 << 23) + 2)}


def _mark(lib, a):
    return lib.kivi_allow_mark(a["allow"], a["as_"], a["V"], a["rows"], a["n"], a["tok"], a["ts"], a["T"], a["len"], a["flags"], None)


@pytest.mark.parametrize("case", sorted(MARK_BAD))
def test_mark_refuses_bad_arguments(lib, case):
    assert _mark(lib, {**MARK, **MARK_BAD[case]}) == -1
    assert b"kivi_allow_mark" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MARK_MISALIGNED))
def test_mark_refuses_misaligned(lib, case):
    assert _mark(lib, {**MARK, **MARK_MISALIGNED[case]}) == -2
    assert b"kivi_allow_mark" in lib.kivi_last_error()


def test_mark_without_work_enqueues_nothing(lib):
    """T == 0 without a fill: returns 0 before any HIP call (the fake pointers would fault otherwise)."""
    for flags in (4, 8):
        assert _mark(lib, {**MARK, "T": 0, "tok": None, "flags": flags}) == 0


def _struct_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header()).group(1)
    return re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_records_match_header():
    from kivi_amd.sampling import SampleConstraint, SampleListEntry, SamplePenalty, SampleRow
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    fields = _struct_fields("kivi_sample_constraint")
    assert [n for _, n, _ in fields] == ["flags", "n_list", "suppress_until", "reserved"] == [n for n, _ in SampleConstraint._fields_]
    for (t, n, dim), (_, ct) in zip(fields, SampleConstraint._fields_):
        assert ctypes.sizeof(ct) == ctypes.sizeof(ctype[t]) * int(dim or 1), n
    assert [getattr(SampleConstraint, n).offset for _, n, _ in fields] == [0, 4, 8, 16]
    assert ctypes.sizeof(SampleConstraint) == 32 and ctypes.alignment(SampleConstraint) == 8
    fields = _struct_fields("kivi_sample_list_entry")
    assert [(n, ctype[t]) for t, n, _ in fields] == list(SampleListEntry._fields_) == [("word", ctypes.c_uint32), ("value", ctypes.c_float)]
    assert ctypes.sizeof(SampleListEntry) == 8
    assert ctypes.sizeof(SampleRow) == 32 and ctypes.sizeof(SamplePenalty) == 16      # the other records do not change


@pytest.mark.parametrize("kw,match", [(dict(logit_bias={3: float("nan")}), "logit_bias"), (dict(logit_bias={-1: 1.0}), "logit_bias"),
                                      (dict(logit_bias={1 << 20: 1.0}), "logit_bias"), (dict(logit_bias={2.5: 1.0}), "logit_bias"),
                                      (dict(logit_bias={True: 1.0}), "logit_bias"), (dict(logit_bias={3: "1"}), "logit_bias"),
                                      (dict(logit_bias=[(3, 1.0)]), "logit_bias"),
                                      (dict(logit_bias={t: 1.0 for t in range(1025)}), "logit_bias"),
                                      (dict(allowed_token_ids=[]), "allowed_token_ids"), (dict(allowed_token_ids=[3, 3]), "allowed_token_ids"),
                                      (dict(allowed_token_ids=[-1]), "allowed_token_ids"), (dict(allowed_token_ids=7), "allowed_token_ids"),
                                      (dict(allowed_token_ids=[1.5]), "allowed_token_ids"),
                                      (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=1.0), "min_new_tokens"),
                                      (dict(min_new_tokens=True), "min_new_tokens"), (dict(do_sample=False, min_new_tokens=None), "min_new_tokens")])
def test_sampling_params_constraint_refusals(kw, match):
    from kivi_amd.sampling import SamplingParams
    with pytest.raises(ValueError, match=match):
        SamplingParams(**kw)


def test_sampling_params_constraints():
    from kivi_amd.sampling import RowSampler, SamplingParams
    p = SamplingParams()
    assert (p.logit_bias, p.allowed_token_ids, p.min_new_tokens) == (None, None, 0) and not p.constrained
    assert SamplingParams(logit_bias={}).logit_bias is None and not SamplingParams(logit_bias={}).constrained
    assert len(dataclasses.fields(p)) == 6 and len(dataclasses.astuple(p)) == 6
    assert "logit_bias" not in repr(p)                              # an unconstrained request prints as before
    q = SamplingParams(seed=4, logit_bias={9: -INF, 2: 1, 5: INF}, allowed_token_ids=torch.tensor([7, 3]), min_new_tokens=2)
    assert dict(q.logit_bias) == {2: 1.0, 5: INF, 9: -INF} and list(q.logit_bias) == [2, 5, 9] and isinstance(q.logit_bias[2], float)
    assert q.allowed_token_ids == (3, 7) and q.min_new_tokens == 2 and q.constrained
    assert q == SamplingParams(seed=4, logit_bias={2: 1.0, 5: INF, 9: -INF}, allowed_token_ids=(3, 7), min_new_tokens=2)
    assert hash(q) == hash(SamplingParams(seed=4, logit_bias={5: INF, 9: -INF, 2: 1.0}, allowed_token_ids=[7, 3], min_new_tokens=2))
    assert q != SamplingParams(seed=4) and q != dataclasses.replace(q, min_new_tokens=3) and hash(q) != hash(SamplingParams(seed=4))
    assert q != dataclasses.replace(q, logit_bias={2: 1.0}) and q != dataclasses.replace(q, allowed_token_ids=None)
    r = dataclasses.replace(q, seed=9)                              # what binding a seed does: the constraints travel
    assert r.constraints == q.constraints and r.seed == 9 and RowSampler._bind(dataclasses.replace(q, seed=None)).constraints == q.constraints
    assert "min_new_tokens=2" in repr(q) and "allowed_token_ids=(3, 7)" in repr(q) and "logit_bias={2: 1.0" in repr(q)
    with pytest.raises(dataclasses.FrozenInstanceError):
        q.min_new_tokens = 0
    with pytest.raises(TypeError):
        q.logit_bias[2] = 0.0                                       # a read-only mapping
    for each in (dict(logit_bias={1: 0.0}), dict(allowed_token_ids=[0]), dict(min_new_tokens=1)):
        assert SamplingParams(**each).constrained and SamplingParams(do_sample=False, **each).constrained
    q.check_vocab(None)
    q.check_vocab(10)
    with pytest.raises(ValueError, match="logit_bias"):
        q.check_vocab(9)
    with pytest.raises(ValueError, match="allowed_token_ids"):
        SamplingParams(allowed_token_ids=[3, 64]).check_vocab(64)


def _rec(t):
    from kivi_amd.sampling import SampleConstraint
    r = SampleConstraint.from_buffer_copy(t.numpy().tobytes())
    return r.flags, r.n_list, r.suppress_until, list(r.reserved)


def _entries(t, n):
    from kivi_amd.sampling import SampleListEntry
    raw = t[:n].numpy().tobytes()
    return [(e.word, e.value) for e in (SampleListEntry.from_buffer_copy(raw[8 * i: 8 * i + 8]) for i in range(n))]


def test_row_sampler_constraint_state_host_side():
    """What needs no GPU: allocation, the bytes of records, lists and masks, the key, set_allowed, select, reset, the refusals."""
    from kivi_amd.sampling import RowSampler, SamplingParams, allow_bitmask, allow_words, constraint_list
    a = SamplingParams(seed=1)
    b = SamplingParams(seed=2, logit_bias={40: 1.5, 3: -INF, 7: 0.25}, min_new_tokens=4)
    c = SamplingParams(seed=3, allowed_token_ids=[69, 0, 32], repetition_penalty=1.2)
    with pytest.raises(ValueError, match="vocab_size="):
        RowSampler([a, b], "cpu")
    with pytest.raises(ValueError, match="vocab_size="):
        RowSampler([a], "cpu", constraints=True)
    with pytest.raises(ValueError, match="constraints"):
        RowSampler([a, b], "cpu", vocab_size=70, constraints=False)
    with pytest.raises(ValueError, match="constraints"):
        RowSampler([a], "cpu", vocab_size=70, constraints=1)
    with pytest.raises(ValueError, match="logit_bias"):
        RowSampler([b], "cpu", vocab_size=40)                        # id 40 outside the vocabulary
    with pytest.raises(ValueError, match="suppress"):
        RowSampler([b], "cpu", vocab_size=70, suppress=[-2])
    # without constrained rows nothing changes
    for plain in (RowSampler([a, a], "cpu"), RowSampler([a, a], "cpu", vocab_size=70), RowSampler([a], "cpu", vocab_size=70, constraints=False)):
        assert plain.constraint is None and plain.allowed is None and plain.bias_list is None
        assert plain.key() == ("rows", plain.B, plain.records.data_ptr(), plain.draw_index.data_ptr()) + \
            (() if plain.seen is None else (plain.penalties.data_ptr(), plain.seen.data_ptr()))
        with pytest.raises(ValueError, match="constraint"):
            plain.set_allowed(0, [1])
        with pytest.raises(ValueError, match="constraint"):
            plain.set_row(0, b)
    rs = RowSampler([a, b, c], "cpu", vocab_size=70, suppress=[[1], [7, 2, 69], [5]])
    assert allow_words(70) == 4 and allow_words(1) == 4 and allow_words(129) == 8 and allow_words(128256) == 4008
    assert rs.constraint.shape == (3, 4) and rs.constraint.dtype == torch.int64
    assert rs.allowed.shape == (3, 4) and rs.allowed.dtype == torch.int32 and rs.allowed.data_ptr() % 16 == 0
    assert rs.bias_list.shape == (3, 1024, 2) and rs.bias_list.dtype == torch.int32 and rs.seen.shape == (3, 72)
    assert rs.key() == ("rows", 3, rs.records.data_ptr(), rs.draw_index.data_ptr(), rs.penalties.data_ptr(), rs.seen.data_ptr(),
                        rs.constraint.data_ptr(), rs.allowed.data_ptr(), rs.bias_list.data_ptr())
    assert [_rec(r) for r in rs.constraint] == [(0, 0, 0, [0] * 4), (0, 5, 4, [0] * 4), (1, 0, 0, [0] * 4)]
    S = 1 << 31                                                     # sorted and merged: 7 is biased AND suppressed
    assert _entries(rs.bias_list[1], 5) == [(2 | S, 0.0), (3, -INF), (7 | S, 0.25), (40, 1.5), (69 | S, 0.0)]
    assert constraint_list(b, [7, 2, 69]) == [(2, 0.0, True), (3, -INF, False), (7, 0.25, True), (40, 1.5, False), (69, 0.0, True)]
    assert constraint_list(c, [5]) == [] and constraint_list(a, [5]) == []          # no min_new_tokens: nothing is suppressed
    with pytest.raises(ValueError, match="1024"):
        constraint_list(dataclasses.replace(b, logit_bias={t: 1.0 for t in range(1024)}), [2000])
    assert bool((rs.allowed[:2] == -1).all())
    bits = allow_bitmask([0, 32, 69], 70)
    assert torch.equal(rs.allowed[2], bits) and bits.tolist() == [1, 1, 1 << 5, 0]
    assert allow_bitmask([31, 70, -1, 200], 70).tolist() == [-(1 << 31), 0, 0, 0]   # ids outside the vocabulary are ignored
    # set_allowed: ids, a bitmask, None
    key = rs.key()
    rs.set_allowed(0, [64, 1])
    assert rs.allowed[0].tolist() == [2, 0, 1, 0] and _rec(rs.constraint[0])[0] == 1
    rs.set_allowed(0, torch.tensor([5, 6, 7, 8], dtype=torch.int32))
    assert rs.allowed[0].tolist() == [5, 6, 7, 0] and _rec(rs.constraint[0])[0] == 1      # ceil(70 / 32) = 3 words are copied
    rs.set_allowed(0, [])
    assert rs.allowed[0].tolist() == [0] * 4 and _rec(rs.constraint[0])[0] == 1
    rs.set_allowed(0, None)
    assert rs.allowed[0].tolist() == [-1] * 4 and _rec(rs.constraint[0])[:3] == (0, 0, 0) and rs.key() == key
    for bad in (lambda: rs.set_allowed(3, [1]), lambda: rs.set_allowed(0, torch.zeros(2, dtype=torch.int32)),
                lambda: rs.set_row(0, SamplingParams(logit_bias={70: 1.0}))):
        with pytest.raises(ValueError):
            bad()
    # select and reset
    rs.set_allowed(1, [9])
    sel = rs.select([1, 1, 2])
    assert torch.equal(sel.constraint, rs.constraint[[1, 1, 2]]) and torch.equal(sel.allowed, rs.allowed[[1, 1, 2]])
    assert torch.equal(sel.bias_list, rs.bias_list[[1, 1, 2]]) and sel.bias_list.data_ptr() != rs.bias_list.data_ptr()
    assert _rec(sel.constraint[0])[:3] == (1, 5, 4) and len(sel.key()) == 9
    rs.draw_index += 2
    rs.reset()
    assert rs.draw_index.tolist() == [0, 0, 0] and _rec(rs.constraint[1])[:3] == (1, 5, 4) and rs.allowed[1].tolist() == [1 << 9, 0, 0, 0]
    rs.bind_suppress([[1], [11], [5]])
    assert _entries(rs.bias_list[1], 4) == [(3, -INF), (7, 0.25), (11 | S, 0.0), (40, 1.5)] and _rec(rs.constraint[1])[:3] == (1, 4, 4)


# ------------------------------------------------------------------ reference_constrain
def _case(B=3, V=97, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((B, V), generator=g) * 4).half()
    x[:, ::7] = 0.0
    x[:, 1::13] = -0.0
    prompt = torch.rand((B, V), generator=g) < 0.3
    counts = torch.randint(0, 4, (B, V), generator=g) * (torch.rand((B, V), generator=g) < 0.4)
    return x, prompt, counts


def test_reference_constrain_against_fp64_rule():
    """Every step of the rule is one fp32 operation: evaluated in fp64 and rounded step by step it gives the same bits (a sum, a
    product, a quotient or a difference of two fp32 values rounds once from fp64 exactly as in fp32: 2 * 24 + 2 <= 53)."""
    from kivi_amd.sampling import allow_bitmask, reference_constrain
    x, prompt, counts = _case()
    V = x.shape[1]
    lists = [[(0, 1.1, False), (5, -INF, False), (13, 0.0, False), (14, -0.0, True), (96, 1e-3, True), (97, 9.0, False), (300, 1.0, True)],
             None, [(t, 0.3 * t - 7.0, t % 5 == 0) for t in range(0, V, 2)]]
    active = [True, True, False]
    allow_ids = sorted(set(range(0, V, 3)) | {96, 14})
    allow = [None, torch.arange(V) % 2 == 0, allow_bitmask(allow_ids, V)]
    theta, pres, freq = torch.tensor([0.5, 1.3, 1.0]), torch.tensor([-0.7, 0.6, 0.0]), torch.tensor([0.25, 0.0, 1e4])
    got = reference_constrain(x, lists, active, allow, (prompt, counts, theta, pres, freq))
    f32 = lambda t: t.float().double()                                  # noqa: E731  (one rounding to fp32)
    X = x.double()
    masked = torch.zeros_like(prompt)
    for b, ls in enumerate(lists):
        for t, v, sup in ls or ():
            if t >= V:
                continue
            if sup and active[b]:
                masked[b, t] = True
            else:
                X[b, t] = f32(X[b, t] + torch.tensor(v, dtype=torch.float32).double())
    th, pr, fr = theta.double()[:, None], pres.double()[:, None], freq.double()[:, None]
    seen = prompt | (counts > 0)
    X = torch.where(seen, torch.where(X > 0, f32(X / th), f32(X * th)), X)
    X = f32(X - f32(fr * counts.double()))
    X = torch.where(counts > 0, f32(X - pr), X)
    masked[1] |= torch.arange(V) % 2 != 0
    masked[2, [t for t in range(V) if t not in allow_ids]] = True
    X = X.masked_fill(masked, -INF)
    assert got.dtype == torch.float32 and torch.equal(got.double(), X) and torch.equal(torch.signbit(got), torch.signbit(X))
    assert bool((got[0, [14, 96]] == -INF).all()) and bool(got[2, ::10].isfinite().any())
    # neutral input changes nothing; a NaN value reads as 0; bool and bitmask rows agree; one bool for every row
    assert torch.equal(reference_constrain(x).view(torch.int32), x.float().view(torch.int32))
    assert torch.equal(reference_constrain(x, [[(1, float("nan"), False)], None, None])[0, 1], x.float()[0, 1] + 0.0)
    m = torch.arange(V) % 3 == 0
    assert torch.equal(reference_constrain(x, allow=[m] * 3), reference_constrain(x, allow=[allow_bitmask(m.nonzero().view(-1).tolist(), V)] * 3))
    assert torch.equal(reference_constrain(x, [[(4, 1.0, True)]] * 3, True)[:, 4], torch.full((3,), -INF))
    assert torch.equal(reference_constrain(x, [[(4, 1.0, True)]] * 3, False)[:, 4], x.float()[:, 4] + 1.0)
    assert torch.equal(reference_constrain(x, penalties=(prompt, counts, theta, pres, freq)),
                       __import__("kivi_amd.sampling", fromlist=["x"]).reference_penalise(x, prompt, counts, theta, pres, freq))


def _finite_rows(dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((4, 211), generator=g) * 5).to(dtype)
    x[:, ::9] = 0.0                                                     # exact +0 among them; no -0 (see the module docstring)
    return x


def _hf(name):
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, name):
        pytest.skip(f"the installed transformers has no {name}")
    return getattr(transformers, name)


def _bits_equal(got, want):
    return got.dtype == want.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_reference_constrain_equals_hf_sequence_bias():
    from kivi_amd.sampling import SamplingParams, constraint_list, reference_constrain
    cls = _hf("SequenceBiasLogitsProcessor")
    bias = {3: 2.5, 0: -4.0, 210: -INF, 17: 0.125, 99: 1e-3}
    try:
        proc = cls(sequence_bias={(t,): v for t, v in bias.items()})
    except (TypeError, ValueError):
        proc = cls(sequence_bias=[[[t], v] for t, v in bias.items()])
    ids = torch.zeros((4, 5), dtype=torch.long)
    for dtype in (torch.float16, torch.float32):
        x = _finite_rows(dtype, 3)
        want = proc(ids, x.float().clone())
        got = reference_constrain(x, [constraint_list(SamplingParams(logit_bias=bias))] * 4)
        assert _bits_equal(got, want), dtype


def test_reference_constrain_equals_hf_min_new_tokens():
    from kivi_amd.sampling import SamplingParams, constraint_list, reference_constrain
    cls = _hf("MinNewTokensLengthLogitsProcessor")
    eos, prompt_len, min_new = [7, 200], 5, 3
    proc = cls(prompt_length_to_skip=prompt_len, min_new_tokens=min_new, eos_token_id=eos, device="cpu")
    lists = [constraint_list(SamplingParams(min_new_tokens=min_new), eos)] * 4
    x = _finite_rows(torch.float16, 4)
    for generated in range(6):                                          # draw index = tokens generated so far; suppress_until = min_new
        ids = torch.zeros((4, prompt_len + generated), dtype=torch.long)
        want = proc(ids, x.float().clone())
        got = reference_constrain(x, lists, generated < min_new)
        assert _bits_equal(got, want), generated
        assert bool((got[:, eos] == -INF).all()) == (generated < min_new)


def test_reference_constrain_equals_hf_suppress_tokens():
    from kivi_amd.sampling import SamplingParams, constraint_list, reference_constrain
    cls = _hf("SuppressTokensLogitsProcessor")
    banned = [0, 5, 64, 210]
    proc = cls(suppress_tokens=banned, device="cpu")
    x = _finite_rows(torch.float32, 5)
    want = proc(torch.zeros((4, 3), dtype=torch.long), x.clone())
    got = reference_constrain(x, [constraint_list(SamplingParams(logit_bias={t: -INF for t in banned}))] * 4)
    assert _bits_equal(got, want)


def test_reference_constrain_equals_hf_prefix_allowed():
    from kivi_amd.sampling import allow_bitmask, reference_constrain
    cls = _hf("PrefixConstrainedLogitsProcessor")
    allowed = [[1, 2, 3], [0, 210], list(range(0, 211, 2)), [64]]
    proc = cls(lambda batch_id, sent: allowed[batch_id], num_beams=1)
    x = _finite_rows(torch.float16, 6)
    want = proc(torch.zeros((4, 3), dtype=torch.long), x.float().clone())
    got = reference_constrain(x, allow=[allow_bitmask(a, 211) for a in allowed])
    assert _bits_equal(got, want)


# ------------------------------------------------------------------ generate: refusals and routing
def _kivi_model():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_generate_constraint_refusals(monkeypatch):
    from kivi_amd.sampling import SamplingParams
    model = _kivi_model()
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    ids = torch.zeros((2, 5), dtype=torch.long)
    p = SamplingParams(seed=1, min_new_tokens=2)
    for fn in (model.generate, model.generate_graphed):
        for kw, match in ((dict(logit_bias={3: float("nan")}), "logit_bias"), (dict(logit_bias={64: 1.0}), "logit_bias"),
                          (dict(allowed_token_ids=[]), "allowed_token_ids"), (dict(allowed_token_ids=[64]), "allowed_token_ids"),
                          (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens="2"), "min_new_tokens")):
            with pytest.raises(ValueError, match=match):
                fn(ids, 3, **kw)
        for kw in (dict(logit_bias={3: 1.0}), dict(allowed_token_ids=[1, 2]), dict(min_new_tokens=2)):
            with pytest.raises(ValueError, match="cannot be combined"):
                fn(ids, 3, sampling=p, **kw)                        # with sampling= the constraints come from the SamplingParams
            with pytest.raises(ValueError, match="beam"):
                fn(ids, 3, num_beams=2, **kw)
        with pytest.raises(ValueError, match="temperature"):        # the other arguments are validated as before
            fn(ids, 3, min_new_tokens=2, do_sample=True, temperature=0.0)
        with pytest.raises(ValueError, match="allowed_token_ids"):  # ids of per-request params against the vocabulary
            fn(ids, 3, sampling=SamplingParams(seed=1, allowed_token_ids=[70]))
    with pytest.raises(ValueError, match="num_return_sequences"):   # n samples per prompt stay a feature of sampling=
        model.generate(ids, 3, min_new_tokens=2, num_return_sequences=2)


def test_resolve_sampler_routes_the_constraints():
    from kivi_amd.generation import bind_suppress, resolve_sampler
    from kivi_amd.sampling import RowSampler, Sampler, SamplingParams
    from kivi_amd.stopping import StopParams
    base = ("cpu", 3, 1, 1)
    hf = (1.0, 50, 1.0, None)
    # neutral values: what the call did before
    assert resolve_sampler(*base, False, *hf, None, None, 1.0, 0.0, 0.0, 64, None, None, 0) == (None, 1)
    assert resolve_sampler(*base, False, *hf, None, None, vocab_size=64, logit_bias={}) == (None, 1)
    assert isinstance(resolve_sampler(*base, True, *hf, 7, None, vocab_size=64, min_new_tokens=0)[0], Sampler)
    pen_only = resolve_sampler(*base, False, *hf, None, None, 1.3, vocab_size=64)[0]
    assert pen_only.constraint is None and len(pen_only.key()) == 6
    # a constraint without sampling=: identical rows, streams 0..B-1, greedy rows without do_sample
    pick, fan = resolve_sampler(*base, False, *hf, None, None, vocab_size=64, logit_bias={5: -INF}, min_new_tokens=2)
    assert isinstance(pick, RowSampler) and fan == 1 and pick.B == 3 and pick.streams == [0, 1, 2] and pick.vocab_size == 64
    assert len(set(pick.params)) == 1 and not pick.params[0].do_sample and pick.params[0].constraints == (((5, -INF),), None, 2)
    assert [_rec(r)[:3] for r in pick.constraint] == [(0, 1, 2)] * 3 and pick.allowed.shape == (3, 4)
    # the suppressed ids arrive once the finish conditions are known: eos ids and stop token ids, never stop sequences
    bind_suppress(pick, None, None, 9)
    assert [_rec(r)[:3] for r in pick.constraint] == [(0, 2, 2)] * 3 and _entries(pick.bias_list[2], 2) == [(5, -INF), (9 | 1 << 31, 0.0)]
    bind_suppress(pick, None, [StopParams((9, 4), ((7, 8),))] * 2 + [StopParams((6,))], None)
    assert [_rec(r)[1] for r in pick.constraint] == [3, 3, 2] and _entries(pick.bias_list[0], 3)[0] == (4 | 1 << 31, 0.0)
    bind_suppress(None, None, None, 9)
    bind_suppress(pen_only, None, None, 9)                              # no constraint state: nothing to bind
    mine = RowSampler([SamplingParams(seed=1, min_new_tokens=1)] * 3, "cpu", vocab_size=64, suppress=[3])
    bind_suppress(mine, mine, None, 9)                                  # a caller's sampler is used as it is
    assert _entries(mine.bias_list[0], 1) == [(3 | 1 << 31, 0.0)]
    pick, _ = resolve_sampler(*base, True, 0.7, 12, 0.9, 0.05, 11, None, vocab_size=64, allowed_token_ids=[3, 1], presence_penalty=0.5)
    q = pick.params[0]
    assert (q.do_sample, q.temperature, q.seed, q.penalties, q.allowed_token_ids) == (True, 0.7, 11, (1.0, 0.5, 0.0), (1, 3))
    assert [_rec(r)[0] for r in pick.constraint] == [1] * 3 and pick.allowed[0].tolist() == [0b1010, 0, 0, 0]
    with pytest.raises(ValueError, match="vocab_size="):
        resolve_sampler(*base, False, *hf, None, None, min_new_tokens=1)
    # sampling=: the state exists exactly when a request is constrained; fan rows repeat the request's record
    plain, con = SamplingParams(seed=1), SamplingParams(seed=2, allowed_token_ids=[5])
    rs, fan = resolve_sampler("cpu", 3, 2, 1, False, *hf, None, [plain, con, plain], vocab_size=64)
    assert fan == 2 and rs.B == 6 and [_rec(r)[0] for r in rs.constraint] == [0, 0, 1, 1, 0, 0] and rs.seen.shape == (6, 64)
    rs, _ = resolve_sampler("cpu", 3, 1, 1, False, *hf, None, plain, vocab_size=64)
    assert rs.seen is None and rs.constraint is None and len(rs.key()) == 4
    for kw in (dict(logit_bias={1: 0.1}), dict(allowed_token_ids=[1]), dict(min_new_tokens=1)):
        with pytest.raises(ValueError, match="cannot be combined"):
            resolve_sampler("cpu", 3, 1, 1, False, *hf, None, plain, vocab_size=64, **kw)


def test_continuous_arguments_keep_the_constraints():
    from kivi_amd.sampling import SamplingParams
    from kivi_amd.serving import check_arguments
    req = [SamplingParams(min_new_tokens=3, logit_bias={2: 1.0}), SamplingParams(seed=3)]
    _, _, params = check_arguments([[1, 2], [3]], 4, 2, None, 0, req, 64)
    assert params[0].constraints == (((2, 1.0),), None, 3) and params[0].seed is not None and not params[1].constrained
    with pytest.raises(ValueError, match="logit_bias"):
        check_arguments([[1, 2], [3]], 4, 2, None, 0, [SamplingParams(logit_bias={64: 1.0})] * 2, 64)
    fn = lambda toks: [1]                                               # noqa: E731
    for bad in (3, [fn], [fn, 3], "x"):
        with pytest.raises(ValueError, match="allowed_fn"):
            check_arguments([[1, 2], [3]], 4, 2, None, 0, req, 64, allowed_fn=bad)
    check_arguments([[1, 2], [3]], 4, 2, None, 0, req, 64, allowed_fn=[fn, None])
    _, _, params = check_arguments([[1, 2], [3]], 4, 2, None, 0, None, 64, allowed_fn=fn)     # greedy requests get greedy rows
    assert len(params) == 2 and not any(p.do_sample for p in params)
    assert check_arguments([[1, 2], [3]], 4, 2, None, 0, None, 64)[2] is None
