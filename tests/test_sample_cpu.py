"""CPU: sampling (kivi_sample, kivi_amd.sampling, generate(do_sample=True)).

* The library exports kivi_sample and refuses bad arguments before anything is enqueued (fake pointers that are never
  dereferenced, as in tests/test_beam_cpu.py); the ABI version is still 3.
* The Sampler and generate / generate_graphed refusals, raised before anything runs on a device.
* The numpy Philox4x32-10 reproduces Random123's known-answer vectors.
* The fp64 reference of the contract against transformers' own Temperature -> TopK -> TopP -> MinP warper chain: identical kept
  sets on tie-free rows; on rows with ties the reference keeps HF's set plus whole tie classes.
"""
import itertools

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def test_sample_symbol_exported(lib):
    assert hasattr(lib, "kivi_sample")
    assert lib.kivi_abi_version() == 3


GOOD = dict(logits=1 << 20, bits=16, rs=320, B=2, V=320, temp=1.0, top_k=50, top_p=1.0, min_p=0.0, state=1 << 21, out=1 << 22,
            os=1)
BAD = {
    "bits": dict(bits=8), "B0": dict(B=0), "B_big": dict(B=65536), "V0": dict(V=0), "V_big": dict(V=(1 << 20) + 1, rs=1 << 21),
    "row_stride": dict(rs=100), "out_stride": dict(os=0), "temp0": dict(temp=0.0), "temp_neg": dict(temp=-1.0),
    "temp_inf": dict(temp=float("inf")), "temp_nan": dict(temp=float("nan")), "top_k": dict(top_k=-1), "top_p0": dict(top_p=0.0),
    "top_p_big": dict(top_p=1.5), "top_p_nan": dict(top_p=float("nan")), "min_p_neg": dict(min_p=-0.1), "min_p1": dict(min_p=1.0),
    "null_logits": dict(logits=None), "null_state": dict(state=None), "null_out": dict(out=None),
}
MISALIGNED = {"logits16": dict(logits=(1 << 20) + 1), "logits32": dict(bits=32, logits=(1 << 20) + 2),
              "state": dict(state=(1 << 21) + 4), "out": dict(out=(1 << 22) + 4)}


def _call(lib, a):
    return lib.kivi_sample(a["logits"], a["bits"], a["rs"], a["B"], a["V"], a["temp"], a["top_k"], a["top_p"], a["min_p"],
                           a["state"], a["out"], a["os"], None)


@pytest.mark.parametrize("case", sorted(BAD))
def test_sample_refuses_bad_arguments(lib, case):
    assert _call(lib, {**GOOD, **BAD[case]}) == -1            # KIVI_EINVAL
    assert b"kivi_sample" in lib.kivi_last_error()


@pytest.mark.parametrize("case", sorted(MISALIGNED))
def test_sample_refuses_misaligned(lib, case):
    assert _call(lib, {**GOOD, **MISALIGNED[case]}) == -2     # KIVI_EALIGN
    assert b"kivi_sample" in lib.kivi_last_error()


@pytest.mark.parametrize("kw,match", [(dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
                                      (dict(temperature=-2.0), "temperature"), (dict(top_k=-1), "top_k"),
                                      (dict(top_k=2.5), "top_k"), (dict(top_p=0.0), "top_p"), (dict(top_p=1.01), "top_p"),
                                      (dict(min_p=1.0), "min_p"), (dict(min_p=-0.5), "min_p"), (dict(seed=-1), "seed")])
def test_sampler_refusals(kw, match):
    from kivi_amd.sampling import Sampler
    with pytest.raises(ValueError, match=match):
        Sampler(device="cpu-never-touched", **kw)


def _kivi_model():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_generate_sampling_refusals(monkeypatch):
    model = _kivi_model()
    # nothing may run: a forward pass would fail the test before the refusal
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    ids = torch.zeros((2, 5), dtype=torch.long)
    for fn in (model.generate, model.generate_graphed):
        with pytest.raises(ValueError, match="beam sampling"):
            fn(ids, 3, do_sample=True, num_beams=2)
        for kw, match in ((dict(temperature=0.0), "temperature"), (dict(top_k=-3), "top_k"), (dict(top_p=2.0), "top_p"),
                          (dict(min_p=1.5), "min_p")):
            with pytest.raises(ValueError, match=match):
                fn(ids, 3, do_sample=True, **kw)


# ------------------------------------------------------------------ Philox4x32-10
def test_philox_known_answers():
    from kivi_amd.sampling import philox4x32
    cases = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
             ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
             ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in cases:
        assert philox4x32(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32)).tolist() == want


def test_philox_counter_mapping():
    from kivi_amd.sampling import draw_u, philox4x32, philox_x0
    seed, n = 0x0123456789ABCDEF, (5 << 32) + 7
    x = philox_x0(seed, [0, 3], n)
    for i, b in enumerate([0, 3]):
        want = philox4x32(np.array([b, 0, 7, 5], dtype=np.uint32), np.array([0x89ABCDEF, 0x01234567], dtype=np.uint32))[0]
        assert x[i] == want
    u = draw_u(seed, np.arange(1000), 0)
    assert (u >= 0).all() and (u < 1).all() and np.all(u * 2 ** 24 == np.floor(u * 2 ** 24))


# ------------------------------------------------------------------ the fp64 reference against transformers' warpers
def _hf_kept(logits, temperature, top_k, top_p, min_p):
    from transformers.generation.logits_process import (LogitsProcessorList, MinPLogitsWarper, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    procs = LogitsProcessorList()
    if temperature != 1.0:
        procs.append(TemperatureLogitsWarper(temperature))
    if top_k:
        procs.append(TopKLogitsWarper(top_k))
    if top_p < 1.0:
        procs.append(TopPLogitsWarper(top_p))
    if min_p:
        procs.append(MinPLogitsWarper(min_p))
    ids = torch.zeros((logits.shape[0], 1), dtype=torch.long)
    return procs(ids, logits.float().clone()) > -float("inf")


GRID = list(itertools.product([0.7, 1.0, 1.3], [0, 1, 5, 50, 400], [1.0, 0.9, 0.5, 0.2], [None, 0.05]))


def test_reference_matches_hf_tie_free():
    from kivi_amd.sampling import reference_kept
    g = torch.Generator().manual_seed(0)
    V = 300
    logits = torch.randn((6, V), generator=g) * 3
    logits[1] = torch.linspace(-5, 5, V)[torch.randperm(V, generator=g)]           # no ties by construction
    for t, k, p, mp in GRID:
        s = logits / t
        assert all(len(set(r.tolist())) == V for r in s)
        ours, _ = reference_kept(logits, t, k, p, mp)
        assert torch.equal(ours, _hf_kept(logits, t, k, p, mp)), (t, k, p, mp)


def test_reference_with_ties_adds_whole_classes():
    from kivi_amd.sampling import reference_kept
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn((8, 200), generator=g) * 2).half().float()                 # fp16 values: many ties
    logits[0, :50] = 1.0                                                            # one large tie class
    logits = (logits * 4).round() / 4
    split = 0
    for t, k, p, mp in GRID:
        ours, _ = reference_kept(logits, t, k, p, mp)
        hf = _hf_kept(logits, t, k, p, mp)
        split += int((ours & ~hf).any())
        assert (ours | ~hf).all(), (t, k, p, mp)                                     # HF's set is a subset
        s = logits / t
        extra = ours & ~hf
        for r in range(logits.shape[0]):
            for v in s[r][extra[r]].unique():
                cls = s[r] == v
                assert (ours[r] | ~cls).all()                                        # a whole class is kept ...
                assert (hf[r] & cls).any(), (t, k, p, mp)                            # ... that HF split at its boundary
    assert split > 0                                                                # the case is exercised


def test_reference_draw_is_inverse_cdf():
    from kivi_amd.sampling import reference_sample
    logits = torch.tensor([[0.0, -float("inf"), 0.0, 0.0, 0.0]])
    # kept mass 4 (the -inf token weighs 0): u in [0, 1/4) -> 0, [1/4, 1/2) -> 2, [1/2, 3/4) -> 3, [3/4, 1) -> 4
    for u, want in ((0.0, 0), (0.2499, 0), (0.25, 2), (0.5, 3), (0.9999, 4)):
        assert int(reference_sample(logits, [u], top_k=0)[0]) == want
