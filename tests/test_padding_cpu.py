"""CPU: batches of prompts with different lengths (left padding).

* kivi_mf_extend_layer takes one broadcast key-mask row per batch row (mask_sq == 0, mask_sb >= P0 + Q) and still refuses a row
  too short for P0 + Q keys (fake pointers that are never dereferenced, the pattern of tests/test_extend_cpu.py: an accepted mask
  is shown by a refusal at the later alignment check, so nothing is ever launched);
* the HF conventions of kivi_amd.llama: left_pad, position ids, the 4D prompt mask, the additive key row;
* the refusals of the model layer, raised before anything runs on a device.
"""
import ctypes

import pytest
import torch

from test_extend_cpu import _fake_desc

MIN16 = torch.finfo(torch.float16).min
LENGTHS = [64, 10, 42, 0, 32, 74]     # Tq, k_res_len, Tv, v_win_start, v_res_len, kv_seq_len


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def _extend(lib, st, Q, mask_sb, mask_sq, out=1 << 20):
    fake = 1 << 20
    nh = 4
    return lib.kivi_mf_extend_layer(ctypes.byref(_fake_desc()), st, Q, fake, nh * Q * 128, Q * 128, 128, nh, fake, 2 * Q * 128,
                                    Q * 128, 128, fake, 2 * Q * 128, Q * 128, 128, fake, mask_sb, mask_sq, out, nh * Q * 128,
                                    Q * 128, 128, None)


@pytest.mark.parametrize("mask_sb,mask_sq,rc", [
    (74 + 8, 0, -2),          # broadcast row of exactly P0 + Q halves: past the mask check (refused later: misaligned out)
    (4096, 0, -2),            # a row of a wider per-request buffer
    (74 + 8 - 1, 0, -1),      # broadcast row too short for P0 + Q keys
    (0, 0, -1),               # broadcast over the batch too: not a row per batch row
    (8 * 82, 82, -2),         # a fully built mask, as before
    (8 * 81, 81, -1),         # its pitch below P0 + Q, as before
])
def test_extend_layer_broadcast_mask_rows(lib, mask_sb, mask_sq, rc):
    st = (ctypes.c_int64 * 6)(*LENGTHS)
    assert _extend(lib, st, 8, mask_sb, mask_sq, out=(1 << 20) + 2) == rc      # KIVI_EALIGN (-2) / KIVI_EINVAL (-1)
    assert list(st) == LENGTHS, "a refused call leaves the caller's lengths alone"
    if rc == -1:
        assert b"mask rows" in lib.kivi_last_error()


def test_abi_version_unchanged(lib):
    assert lib.kivi_abi_version() == 3


# ------------------------------------------------------------------ HF conventions
def test_left_pad():
    from kivi_amd.llama import left_pad
    ids, mask = left_pad([[5, 6, 7], [8], torch.tensor([1, 2])], pad_token_id=9)
    assert ids.tolist() == [[5, 6, 7], [9, 9, 8], [9, 1, 2]]
    assert mask.tolist() == [[1, 1, 1], [0, 0, 1], [0, 1, 1]]
    assert ids.dtype == mask.dtype == torch.long


def test_position_ids_and_masks():
    from kivi_amd.llama import padding_key_row, padding_position_ids, padding_prompt_mask
    mask = torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]])
    assert padding_position_ids(mask, 4).tolist() == [[0, 1, 2, 3], [1, 1, 0, 1], [1, 0, 1, 2]]
    assert padding_position_ids(mask, 2).tolist() == [[2, 3], [0, 1], [1, 2]]
    m4 = padding_prompt_mask(mask)
    assert m4.shape == (3, 1, 4, 4) and m4.dtype == torch.float16
    for b in range(3):
        for i in range(4):
            for j in range(4):
                want = 0.0 if j <= i and mask[b, j] else MIN16
                assert m4[b, 0, i, j].item() == want
    row = padding_key_row(mask, 6)
    assert row.shape == (3, 1, 1, 6) and row.dtype == torch.float16
    assert row[:, 0, 0].tolist() == [[0, 0, 0, 0, 0, 0], [MIN16, MIN16, 0, 0, 0, 0], [MIN16, 0, 0, 0, 0, 0]]


# ------------------------------------------------------------------ refusals of the model layer
def _model(attention_cls=None):
    from kivi_amd.attention import LlamaAttention_KIVI
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=1,
                           intermediate_size=256, vocab_size=64), residual_length=32)
    return LlamaForCausalLM_KIVI(cfg, attention_cls or LlamaAttention_KIVI)


def test_forward_refuses_both_masks():
    model = _model()
    ids = torch.zeros((2, 5), dtype=torch.long)
    with pytest.raises(ValueError, match="not both"):
        model(ids, attention_mask=torch.zeros((2, 1, 5, 5), dtype=torch.float16), padding_mask=torch.ones((2, 5)))


@pytest.mark.parametrize("cls", ["LlamaFlashAttention_KIVI", "MistralFlashAttention_KIVI"])
def test_flash_class_refuses_padded_prompts(cls):
    import kivi_amd.attention as A
    model = _model(getattr(A, cls))
    ids, mask = torch.zeros((2, 5), dtype=torch.long), torch.ones((2, 5), dtype=torch.long)
    mask[1, :2] = 0
    with pytest.raises(ValueError, match="ignores"):
        model(ids, padding_mask=mask)
    with pytest.raises(ValueError, match="ignores"):
        model.generate(ids, 3, attention_mask=mask)
    with pytest.raises(ValueError, match="ignores"):
        model.generate_graphed(ids, 3, attention_mask=mask)


def test_mask_shape_and_eos_refusals():
    model = _model()
    ids = torch.zeros((2, 5), dtype=torch.long)
    with pytest.raises(ValueError, match="size"):
        model.generate(ids, 3, attention_mask=torch.ones((2, 4), dtype=torch.long))
    with pytest.raises(ValueError, match="size"):
        model(ids, padding_mask=torch.ones((2, 1, 1, 5)))
    with pytest.raises(ValueError, match="pad_token_id"):
        model.generate(ids, 3, eos_token_id=1)
