"""GPU: what the checkpoint loader (kivi_amd/loading.py) changes for a load onto the device, on the tiny
models of tests/tiny_w4_models.py.

1. A Qwen2 checkpoint without one k_proj.bias, loaded with weight_bits=4: the bias is a state_dict key of its own in the ledger,
   so packing the layer's weight does not forgive it.
2. Peak device memory of a dense fp16 load from 8 files: the model plus one file, with room for a cast copy of that file --
   max_memory_allocated() - before <= model_bytes + 2 * largest_file_bytes.  The bound is the design's (one file alive at a time),
   not a measurement; a loader that keeps every file until the end sits near 2 * model_bytes."""
import json

import pytest
import torch

import tiny_w4_models as M

pytestmark = pytest.mark.gpu


def _cpu_state(family, seed):
    return {k: v.detach().cpu().contiguous() for k, v in M.build_dense(family, seed, torch.float16).state_dict().items()}


def test_a_missing_bias_of_a_packed_layer_is_refused(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    state = _cpu_state("qwen2", 61)
    (tmp_path / "config.json").write_text(json.dumps(M.config_dict("qwen2")))
    st.save_file(state, str(tmp_path / "model.safetensors"))
    kw = dict(dtype=torch.float16, residual_length=32, weight_bits=4, weight_group=128)
    whole = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), **kw)            # the checkpoint as it is loads
    assert torch.equal(whole.model.layers[1].self_attn.k_proj.bias.cpu(), state["model.layers.1.self_attn.k_proj.bias"])
    del state["model.layers.1.self_attn.k_proj.bias"]
    st.save_file(state, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="layers.1.self_attn.k_proj.bias"):
        LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), **kw)


def test_peak_memory_of_a_load_is_the_model_and_one_file(tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    state = _cpu_state("llama", 62)
    names = sorted(state)
    files = [{k: state[k] for k in names[i::8]} for i in range(8)]              # the sorted names dealt round-robin
    for i, part in enumerate(files):
        st.save_file(part, str(tmp_path / f"model-{i + 1:05d}-of-00008.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(M.config_dict("llama")))
    largest = max(sum(t.numel() * t.element_size() for t in part.values()) for part in files)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    model = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), residual_length=32)
    peak = torch.cuda.max_memory_allocated() - before
    model_bytes = sum(t.numel() * t.element_size() for t in list(model.parameters()) + list(model.buffers()))
    print(f"peak of the load {peak} B, model {model_bytes} B, largest file {largest} B, checkpoint "
          f"{sum(t.numel() * t.element_size() for t in state.values())} B: peak - model = {(peak - model_bytes) / largest:.2f} files, "
          f"bound model + 2 files = {model_bytes + 2 * largest} B")
    for k, v in model.state_dict().items():
        assert torch.equal(v.cpu(), state[k]), k
    assert peak <= model_bytes + 2 * largest, (peak, model_bytes, largest)
