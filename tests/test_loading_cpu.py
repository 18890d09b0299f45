"""No GPU: the checkpoint loader (kivi_amd/loading.py) driven with plain dicts, and from_pretrained over
safetensors files on the CPU, in fp32.  The models are the E = 4, 2-layer Mixtral of tests/test_moe_cpu.py and the tiny Qwen2 of
tests/test_qwen_cpu.py.  (The translation of the three spellings itself is tests/test_moe_cpu.py.)

1. A dense-expert checkpoint that repeats one piece and lacks another is refused, by the stack's name: the ledger holds the set of
   pieces, not their number.
2. The files of a checkpoint in either order fill the model with the same bits; a tensor in two files ends as the later one.
3. Tied embeddings: lm_head.weight owes nothing, model.embed_tokens.weight does.
4. Nothing of a file is reachable from the loader once take() has returned."""
import gc
import json
import weakref

import pytest
import torch

from test_moe_cpu import _cfg, _spell
from test_qwen_cpu import _d, _hf_names

MIXTRAL = dict(model_type="mixtral", num_local_experts=4, num_experts_per_tok=2, num_hidden_layers=2, intermediate_size=32)
TWICE, LACKING = "model.layers.1.block_sparse_moe.experts.2.w3.weight", "model.layers.1.block_sparse_moe.experts.3.w3.weight"


def _mixtral(seed):
    from kivi_amd.llama import MixtralForCausalLM_KIVI, make_config
    torch.manual_seed(seed)
    return MixtralForCausalLM_KIVI(make_config(_cfg(**MIXTRAL)))


def _mixtral_files(src, spelling="mixtral"):
    """The source model's state under a checkpoint spelling, as two "files": the pieces of one parameter come apart."""
    state = _spell({k: v.detach().clone() for k, v in src.state_dict().items()}, spelling)
    names = list(state)
    half = len(names) // 2
    return {k: state[k] for k in names[:half]}, {k: state[k] for k in names[half:]}


def _repeat_and_lack(files):
    """The same piece count as a whole checkpoint: one up matrix of layer 1 in both files, another in neither."""
    a, b = (dict(f) for f in files)
    piece = (a if TWICE in a else b)[TWICE]
    a[TWICE], b[TWICE] = piece, piece.clone()
    assert a.pop(LACKING, None) is not None or b.pop(LACKING, None) is not None
    return a, b


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_a_dense_stack_that_repeats_one_piece_and_lacks_another_is_refused():
    from kivi_amd.loading import CheckpointLoader
    files = _mixtral_files(_mixtral(1))
    whole = CheckpointLoader(_mixtral(2), torch.float32)
    for part in files:
        whole.take(part)
    whole.finish()                                              # the checkpoint as it is loads
    loader = CheckpointLoader(_mixtral(2), torch.float32)
    for part in _repeat_and_lack(files):
        loader.take(part)
    with pytest.raises(KeyError, match="layers.1.mlp.experts.gate_up_proj"):
        loader.finish()
    assert not loader.unexpected


def test_from_pretrained_refuses_the_repeat_and_lack_checkpoint(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI, MixtralForCausalLM_KIVI
    src = _mixtral(1)
    files = _mixtral_files(src)
    (tmp_path / "config.json").write_text(json.dumps(_cfg(**MIXTRAL)))
    for i, part in enumerate(files):
        st.save_file({k: v.contiguous() for k, v in part.items()}, str(tmp_path / f"model-0000{i + 1}-of-00002.safetensors"))
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", dtype=torch.float32)
    assert type(loaded) is MixtralForCausalLM_KIVI
    _same_state(loaded, src)
    for i, part in enumerate(_repeat_and_lack(files)):
        st.save_file({k: v.contiguous() for k, v in part.items()}, str(tmp_path / f"model-0000{i + 1}-of-00002.safetensors"))
    with pytest.raises(KeyError, match="layers.1.mlp.experts.gate_up_proj"):
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", dtype=torch.float32)


@pytest.mark.parametrize("spelling", ["mixtral", "fused"])
def test_the_files_fill_the_model_in_either_order(spelling):
    from kivi_amd.loading import CheckpointLoader
    src = _mixtral(1)
    files = _mixtral_files(src, spelling)
    for seed, order in ((2, files), (3, files[::-1])):
        dst = _mixtral(seed)
        loader = CheckpointLoader(dst, torch.float32)
        for part in order:
            loader.take(part)
        loader.finish()
        assert not loader.unexpected
        _same_state(dst, src)


def test_a_tensor_in_two_files_ends_as_the_later_one():
    from kivi_amd.loading import CheckpointLoader
    src = _mixtral(1)
    first, second = _mixtral_files(src)
    name = "model.layers.0.input_layernorm.weight"
    assert name in first and name not in second
    early, late = torch.full_like(first[name], 3.0), torch.full_like(first[name], 5.0)
    dst = _mixtral(2)
    loader = CheckpointLoader(dst, torch.float32)
    loader.take({**first, name: early})
    assert torch.equal(dst.state_dict()[name], early)
    loader.take({**second, name: late, "model.layers.0.block_sparse_moe.unheard_of": late})
    loader.finish()
    assert torch.equal(dst.state_dict()[name], late)
    assert loader.unexpected == ["model.layers.0.mlp.unheard_of"]       # collected under the module's spelling, otherwise ignored
    with pytest.raises(RuntimeError, match=name):                       # a shape that does not fit names its parameter
        loader.take({name: late[:-1]})


def test_tied_embeddings_owe_no_lm_head(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI
    g = torch.Generator().manual_seed(4)
    state = {k: torch.randn(s, generator=g) for k, s in _hf_names(6, True, False, tied=True).items()}
    assert "lm_head.weight" not in state
    (tmp_path / "config.json").write_text(json.dumps(_d(6, model_type="qwen2", tie_word_embeddings=True)))
    st.save_file(state, str(tmp_path / "model.safetensors"))
    m = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", dtype=torch.float32)
    assert type(m) is Qwen2ForCausalLM_KIVI and m.lm_head.weight is m.model.embed_tokens.weight
    assert torch.equal(m.lm_head.weight, state["model.embed_tokens.weight"])
    del state["model.embed_tokens.weight"]
    st.save_file(state, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="model.embed_tokens.weight"):
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), device="cpu", dtype=torch.float32)


def test_nothing_of_a_file_outlives_take():
    from kivi_amd.loading import CheckpointLoader
    first, second = _mixtral_files(_mixtral(1))
    loader = CheckpointLoader(_mixtral(2), torch.float32)
    part = {k: v.clone() for k, v in first.items()}
    plain = [weakref.ref(part[k]) for k in ("model.embed_tokens.weight", "model.layers.0.input_layernorm.weight")]
    piece = weakref.ref(part["model.layers.0.block_sparse_moe.experts.0.w1.weight"])
    loader.take(part)
    del part
    gc.collect()
    assert all(r() is None for r in plain) and piece() is None
    loader.take(second)
    loader.finish()
