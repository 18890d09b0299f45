"""CPU: per-request sampling (kivi_sample_rows, kivi_amd.sampling.SamplingParams / RowSampler, generate(sampling=)).

* The library exports kivi_sample_rows with a ctypes signature; the ABI version is still 3.
* Every refusal of the entry point, with fake pointers that are never dereferenced (as in tests/test_sample_cpu.py): nothing is
  enqueued.
* The record layout: ctypes.sizeof 32 and the field offsets, against the struct in include/kivi_hip.h.
* SamplingParams, RowSampler and generate / generate_graphed / decode_graphed refusals, raised before any forward pass.
* draw_u_rows against draw_u: (seed, stream = b, n) is row b of draw_u(seed, rows, n).
* no_gc_in_capture (kivi_amd/graph.py): dead cycles are collected before the block, the collector is off inside it.
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


def test_symbol_and_signature(lib):
    from kivi_amd import _lib
    assert hasattr(lib, "kivi_sample_rows")
    res, args = _lib.SIGNATURES["kivi_sample_rows"]
    assert res is ctypes.c_int32 and len(args) == 10
    assert lib.kivi_abi_version() == 3


GOOD = dict(logits=1 << 20, bits=16, rs=320, B=2, V=320, rows=1 << 21, idx=1 << 22, out=1 << 23, os=1)
BAD = {
    "bits": dict(bits=8), "B0": dict(B=0), "B_big": dict(B=65536), "V0": dict(V=0), "V_big": dict(V=(1 << 20) + 1, rs=1 << 21),
    "row_stride": dict(rs=100), "out_stride": dict(os=0), "null_logits": dict(logits=None), "null_rows": dict(rows=None),
    "null_draw_index": dict(idx=None), "null_out": dict(out=None),
}
MISALIGNED = {"logits16": dict(logits=(1 << 20) + 1), "logits32": dict(bits=32, logits=(1 << 20) + 2),
              "rows": dict(rows=(1 << 21) + 4), "draw_index": dict(idx=(1 << 22) + 4), "out": dict(out=(1 << 23) + 4)}


def _call(lib, a):
    return lib.kivi_sample_rows(a["logits"], a["bits"], a["rs"], a["B"], a["V"], a["rows"], a["idx"], a["out"], a["os"], None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_rows_refuses_bad_arguments(lib, case):
    assert _call(lib, {**GOOD, **BAD[case]}) == -1            # KIVI_EINVAL
    assert b"kivi_sample_rows" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MISALIGNED))
def test_rows_refuses_misaligned(lib, case):
    assert _call(lib, {**GOOD, **MISALIGNED[case]}) == -2     # KIVI_EALIGN
    assert b"kivi_sample_rows" in lib.kivi_last_error()


def test_record_layout_matches_header():
    from kivi_amd.sampling import GREEDY, SampleRow
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*kivi_sample_row;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    size = {"float": 4, "int32_t": 4, "uint32_t": 4, "int64_t": 8}
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
    assert [n for _, n in fields] == ["temperature", "top_k", "top_p", "min_p", "seed", "stream", "flags"]
    assert [(n, ctype[t]) for t, n in fields] == list(SampleRow._fields_)
    off = 0
    for t, n in fields:
        off = (off + size[t] - 1) // size[t] * size[t]          # C's natural alignment
        assert getattr(SampleRow, n).offset == off, n
        off += size[t]
    assert off == 32 and ctypes.sizeof(SampleRow) == 32 and ctypes.alignment(SampleRow) == 8
    assert int(re.search(r"#define KIVI_SAMPLE_ROW_GREEDY (\d+)u", src).group(1)) == GREEDY == 1


def test_record_bytes():
    from kivi_amd.sampling import SampleRow, SamplingParams, _record
    rec = _record(SamplingParams(True, 0.5, 7, 0.25, 0.125, seed=2 ** 64 - 2), 9)
    assert rec.dtype == torch.int64 and rec.shape == (4,)
    r = SampleRow.from_buffer_copy(rec.numpy().tobytes())
    assert (r.temperature, r.top_k, r.top_p, r.min_p, r.seed, r.stream, r.flags) == (0.5, 7, 0.25, 0.125, -2, 9, 0)
    r = SampleRow.from_buffer_copy(_record(SamplingParams(do_sample=False, seed=3), 0).numpy().tobytes())
    assert (r.flags, r.seed, r.min_p) == (1, 3, 0.0)


@pytest.mark.parametrize("kw,match", [(dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
                                      (dict(temperature=-2.0), "temperature"), (dict(top_k=-1), "top_k"),
                                      (dict(top_k=2.5), "top_k"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.01), "top_p"),
                                      (dict(min_p=1.0), "min_p"), (dict(min_p=-0.5), "min_p"), (dict(seed=-1), "seed"),
                                      (dict(seed=2 ** 64), "seed"), (dict(seed=1.5), "seed"), (dict(do_sample=1), "do_sample"),
                                      (dict(do_sample=False, top_k=-1), "top_k")])
def test_sampling_params_refusals(kw, match):
    from kivi_amd.sampling import SamplingParams
    with pytest.raises(ValueError, match=match):
        SamplingParams(**kw)


def test_sampling_params_frozen_with_hf_defaults():
    from kivi_amd.sampling import SamplingParams
    p = SamplingParams()
    assert dataclasses.astuple(p) == (True, 1.0, 50, 1.0, None, None)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.temperature = 2.0


def test_row_sampler_refusals():
    from kivi_amd.sampling import RowSampler, SamplingParams
    p, dev = SamplingParams(seed=1), "cpu-never-touched"
    for args, kw, match in (((dict(temperature=1.0),), {}, "SamplingParams"), (([],), {}, "SamplingParams"),
                            (([p, "x"],), {}, "SamplingParams"), (([p, p],), dict(streams=[0]), "streams"),
                            (([p],), dict(streams=[-1]), "stream"), (([p],), dict(streams=[2 ** 32]), "stream"),
                            (([p],), dict(streams=[0.5]), "stream"), ((p,), dict(B=0), "B"), (([p, p],), dict(B=3), "B=3")):
        with pytest.raises(ValueError, match=match):
            RowSampler(*args, device=dev, **kw)


def test_row_sampler_host_side():
    """What needs no GPU: binding of seeds, the key, set_row / select / reset on CPU buffers."""
    from kivi_amd.sampling import RowSampler, Sampler, SampleRow, SamplingParams
    torch.manual_seed(4)
    rs = RowSampler([SamplingParams(seed=5), SamplingParams(do_sample=False), SamplingParams(top_k=0)], "cpu", streams=[0, 1, 2])
    assert rs.B == 3 and rs.records.shape == (3, 4) and rs.draw_index.tolist() == [0, 0, 0]
    assert rs.params[0].seed == 5 and all(p.seed is not None for p in rs.params)
    assert rs.params[1].seed != rs.params[2].seed                         # drawn per row
    key = rs.key()
    assert key == ("rows", 3, rs.records.data_ptr(), rs.draw_index.data_ptr())
    assert not any(isinstance(k, float) for k in key) and len(key) != 5   # no parameter value; not the shape of a Sampler.key()
    rs.draw_index += 3
    rs.set_row(1, SamplingParams(temperature=0.5, seed=8), stream=6)
    assert rs.key() == key and rs.draw_index.tolist() == [3, 0, 3]
    r = SampleRow.from_buffer_copy(rs.records[1].numpy().tobytes())
    assert (r.temperature, r.seed, r.stream, r.flags) == (0.5, 8, 6, 0)
    sel = rs.select([2, 2, 0], streams=[0, 1, 0])
    assert sel.B == 3 and sel.draw_index.tolist() == [3, 3, 3] and sel.key() != key
    assert [p.seed for p in sel.params] == [rs.params[2].seed, rs.params[2].seed, 5] and sel.streams == [0, 1, 0]
    assert torch.equal(rs.select(torch.tensor([1])).records[0], rs.records[1])
    rs.reset()
    assert rs.draw_index.tolist() == [0, 0, 0]
    for bad in (lambda: rs.set_row(3, SamplingParams()), lambda: rs.set_row(0, "p"), lambda: rs.set_row(0, SamplingParams(), -1),
                lambda: rs.select([]), lambda: rs.select([3])):
        with pytest.raises(ValueError):
            bad()
    one = RowSampler(SamplingParams(seed=1), "cpu", B=4)
    assert one.B == 4 and one.streams == [0] * 4 and bool((one.records == one.records[0]).all())


def _kivi_model():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_generate_sampling_argument_refusals(monkeypatch):
    from kivi_amd.sampling import RowSampler, SamplingParams
    model = _kivi_model()
    # nothing may run: a forward pass would fail the test before the refusal
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    ids = torch.zeros((2, 5), dtype=torch.long)
    p = SamplingParams(seed=1)
    for fn in (model.generate, model.generate_graphed):
        for kw in (dict(do_sample=True), dict(temperature=0.7), dict(top_k=0), dict(top_p=0.9), dict(min_p=0.1), dict(seed=3)):
            with pytest.raises(ValueError, match="cannot be combined"):
                fn(ids, 3, sampling=p, **kw)
        with pytest.raises(ValueError, match="beam"):
            fn(ids, 3, sampling=p, num_beams=2)
        with pytest.raises(ValueError, match="batch of 2"):
            fn(ids, 3, sampling=[p, p, p])
        with pytest.raises(ValueError, match="SamplingParams"):
            fn(ids, 3, sampling=[p, dict(top_k=1)])
        with pytest.raises(ValueError, match="SamplingParams"):
            fn(ids, 3, sampling="greedy")
        with pytest.raises(ValueError, match="holds 3 rows"):
            fn(ids, 3, sampling=RowSampler([p, p, p], "cpu"))
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, 3, sampling=p, num_return_sequences=0)
    with pytest.raises(ValueError, match="holds 2 rows"):                   # 2 requests x 3 samples need 6 rows
        model.generate(ids, 3, sampling=RowSampler([p, p], "cpu"), num_return_sequences=3)
    with pytest.raises(ValueError, match="pad_token_id"):
        model.generate(ids, 3, sampling=p, eos_token_id=1)
    with pytest.raises(ValueError, match="return_scores"):
        model.generate(ids, 3, sampling=p, return_scores=True)
    # without sampling= the old rule stands
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, 3, num_return_sequences=2)
    with pytest.raises(ValueError, match="not both"):
        model.decode_graphed(ids[:, :1], [], 5, 1, sampler=object(), sampling=RowSampler([p, p], "cpu"))
    with pytest.raises(ValueError, match="holds 3 rows"):
        model.decode_graphed(ids[:, :1], [], 5, 1, sampling=RowSampler([p, p, p], "cpu"))


def test_draw_u_rows_against_draw_u():
    from kivi_amd.sampling import draw_u, draw_u_rows, philox4x32
    rows = np.arange(37)
    for seed, n in ((0x0123456789ABCDEF, 0), (7, 1), (2 ** 64 - 1, (1 << 32) + 3), (2 ** 63 + 5, 2 ** 40)):
        assert np.array_equal(draw_u_rows([seed] * 37, rows, [n] * 37), draw_u(seed, rows, n))
    # mixed rows: each entry is the batch-of-one draw of its own (seed, stream, n)
    seeds, streams, ns = [3, 2 ** 64 - 9, 3, 11], [0, 5, 2 ** 32 - 1, 0], [0, (7 << 32) + 1, 4, 2 ** 33]
    u = draw_u_rows(seeds, streams, ns)
    for i in range(4):
        assert u[i] == draw_u(seeds[i], [streams[i]], ns[i])[0]
    want = philox4x32(np.array([5, 0, 1, 7], dtype=np.uint32), np.array([(2 ** 64 - 9) & 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32))[0]
    assert u[1] == float(want >> 8) * 2.0 ** -24
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()


def test_no_gc_in_capture():
    import gc
    import weakref
    from kivi_amd.graph import no_gc_in_capture

    class Node:
        pass

    a, b = Node(), Node()
    a.other, b.other = b, a
    dead = weakref.ref(a)
    del a, b
    assert gc.isenabled()
    with no_gc_in_capture():
        assert dead() is None and not gc.isenabled()            # collected before the block; no pass can start inside it
    assert gc.isenabled()
    gc.disable()
    try:
        with no_gc_in_capture():
            pass
        assert not gc.isenabled()                               # a caller's own setting is kept
    finally:
        gc.enable()
