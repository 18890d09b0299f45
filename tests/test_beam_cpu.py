"""CPU: beam search (kivi_cache_reorder, kivi_amd.beam, LlamaForCausalLM_KIVI.generate(num_beams=...)).

* The library exports kivi_cache_reorder and refuses bad arguments with KIVI_EINVAL before anything is enqueued (fake pointers
  that are never dereferenced, as in tests/test_extend_cpu.py); the ABI version is still 3.
* The refusals of generate / generate_graphed, raised before anything runs on a device.
* kivi_amd.beam.beam_search against Hugging Face's own beam search: a tiny random fp32 LlamaForCausalLM on the CPU, driven through
  the step callback with DynamicCache.reorder_cache.  Same sequences, sequences_scores within 1e-5.
"""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def test_reorder_symbol_exported(lib):
    assert hasattr(lib, "kivi_cache_reorder")
    assert lib.kivi_abi_version() == 3


def _slabs(n=1, base=1 << 20, run=4096, rs=1 << 16):
    from kivi_amd import _lib
    arr = (_lib.ReorderSlab * max(n, 1))()
    for d in arr:
        d.base, d.row_stride, d.run = base, rs, run
        for k in range(3):
            d.n[k], d.stride[k] = 1, 0
    return arr


@pytest.mark.parametrize("case", ["group0", "group_not_dividing", "group_too_big", "idx_null", "idx_misaligned", "idx_bytes",
                                  "too_many_slabs", "negative_count", "slab_misaligned", "null_base"])
def test_reorder_refuses_bad_arguments(lib, case):
    from kivi_amd import _lib
    B, group, idx, idx_bytes, n = 8, 4, 1 << 20, 8, 1
    slabs = _slabs()
    if case == "group0":
        group = 0
    elif case == "group_not_dividing":
        group = 3
    elif case == "group_too_big":
        B = group = _lib.REORDER_MAX_GROUP + 1
    elif case == "idx_null":
        idx = None
    elif case == "idx_misaligned":
        idx = (1 << 20) + 4
    elif case == "idx_bytes":
        idx_bytes = 2
    elif case == "too_many_slabs":
        n = _lib.REORDER_MAX_SLABS + 1
        slabs = _slabs(n)
    elif case == "negative_count":
        slabs[0].n[1] = -1
    elif case == "slab_misaligned":
        slabs = _slabs(base=(1 << 20) + 2)
    elif case == "null_base":
        slabs = _slabs(base=0)
    assert lib.kivi_cache_reorder(slabs, n, B, group, idx, idx_bytes, None) == -1          # KIVI_EINVAL
    assert b"kivi_cache_reorder" in lib.kivi_last_error()


def test_reorder_empty_slabs_enqueue_nothing(lib):
    slabs = _slabs(run=0)
    assert lib.kivi_cache_reorder(slabs, 1, 8, 4, 1 << 20, 8, None) == 0
    assert lib.kivi_cache_reorder(slabs, 0, 8, 8, 1 << 20, 4, None) == 0


def test_reorder_index_checks():
    from kivi_amd.reorder import check_idx
    assert check_idx(torch.tensor([1, 0, 3, 3]), 4, 2, "cpu").tolist() == [1, 0, 3, 3]
    with pytest.raises(ValueError, match="group"):
        check_idx(torch.tensor([2, 0, 3, 3]), 4, 2, "cpu")          # idx[0] outside its group
    with pytest.raises(ValueError, match="shape"):
        check_idx(torch.tensor([0, 1, 2]), 4, 2, "cpu")
    with pytest.raises(ValueError, match="int32 or int64"):
        check_idx(torch.tensor([0.0, 1.0]), 2, 2, "cpu")
    with pytest.raises(ValueError, match="divide"):
        check_idx(torch.tensor([0, 1, 2, 3]), 4, 3, "cpu")


# ------------------------------------------------------------------ refusals of the model layer
def _kivi_model():
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_generate_beam_refusals():
    model = _kivi_model()
    ids = torch.zeros((2, 5), dtype=torch.long)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, 3, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, 3, num_return_sequences=2)
    with pytest.raises(ValueError, match="pad_token_id"):
        model.generate(ids, 3, num_beams=4, eos_token_id=1)
    with pytest.raises(ValueError, match="return_scores"):
        model.generate(ids, 3, return_scores=True)
    with pytest.raises(ValueError, match="greedy only"):
        model.generate_graphed(ids, 3, num_beams=4)


def test_beam_search_refusals():
    from kivi_amd.beam import beam_search
    ids, logits = torch.zeros((1, 3), dtype=torch.long), torch.zeros((1, 10))
    with pytest.raises(ValueError, match="num_return_sequences"):
        beam_search(None, ids, logits, 2, 4, num_return_sequences=3)
    with pytest.raises(ValueError, match="early_stopping"):
        beam_search(None, ids, logits, 2, 4, early_stopping="sometimes")


# ------------------------------------------------------------------ against transformers' own beam search
def _hf_model():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = transformers.LlamaConfig(vocab_size=50, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=128, bos_token_id=None, eos_token_id=None,
                                   pad_token_id=None)
    model = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0.0, 0.3)      # peaked logits: beams diverge, some reach EOS
    return transformers, model


@pytest.mark.parametrize("B,eos,early_stopping,length_penalty,nrs", [
    (1, None, False, 1.0, 1),
    (1, None, False, 1.0, 4),
    (2, None, True, 0.0, 4),
    (1, 25, False, 1.0, 4),
    (1, 25, True, 1.0, 2),
    (1, 25, "never", 2.0, 4),
    (1, 25, "never", 0.0, 1),
    (2, 25, False, 2.0, 4),
    (2, 48, True, 0.0, 1),
    (2, 48, "never", 1.0, 4),
])
def test_beam_search_matches_transformers(B, eos, early_stopping, length_penalty, nrs):
    transformers, model = _hf_model()
    from kivi_amd.beam import beam_search
    nb, new = 4, 12
    g = torch.Generator().manual_seed(B * 100 + (eos or 0))
    ids = torch.randint(0, 50, (B, 6), generator=g)
    kw = dict(num_beams=nb, max_new_tokens=new, do_sample=False, early_stopping=early_stopping, length_penalty=length_penalty,
              num_return_sequences=nrs)
    if eos is not None:
        kw.update(eos_token_id=eos, pad_token_id=0)
    with torch.no_grad():
        ref = model.generate(ids, attention_mask=torch.ones_like(ids), return_dict_in_generate=True, output_scores=True, **kw)
        cache = transformers.DynamicCache(config=model.config)
        first = model(ids.repeat_interleave(nb, 0), past_key_values=cache, use_cache=True).logits[:, -1].float()

        def step(tok, beam_idx):
            cache.reorder_cache(beam_idx)
            return model(tok, past_key_values=cache, use_cache=True).logits[:, -1].float()

        seqs, scores = beam_search(step, ids, first, nb, new, eos, 0 if eos is not None else None, length_penalty, early_stopping,
                                   nrs)
    assert torch.equal(seqs, ref.sequences)
    assert torch.allclose(scores, ref.sequences_scores, rtol=0, atol=1e-5)
    if (B, eos, early_stopping) == (1, 25, False):
        assert bool((seqs[:, 6:] == eos).any()), "this case returns finished beams (EOS, then padding)"
