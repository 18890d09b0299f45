"""No GPU: which query-group ratios run padded on the matrix-pipe layout (mfma.padded_ratio, cache_mf.padded_heads; DESIGN.md section
27), and that nothing changes for anybody who does not ask: make_config leaves `qk_kernel` off and a module built without it keeps
its own head count."""
import pytest

from kivi_amd.attention import KiviConfig, LlamaAttention_KIVI
from kivi_amd.cache_mf import padded_heads
from kivi_amd.llama import make_config
from kivi_amd.quant import mfma

TABLE = [(2, 2, 4), (2, 3, 4), (2, 5, 8), (2, 6, 8), (2, 7, 8), (4, 2, 4), (4, 3, 4), (4, 5, None), (4, 6, None), (4, 7, None),
         (4, 8, None)]


@pytest.mark.parametrize("bits,ratio,want", TABLE)
def test_padded_ratio_table(bits, ratio, want):
    assert mfma.padded_ratio(bits, bits, ratio) == want


def test_padded_ratio_edges():
    for bits, served in ((2, (1, 4, 8)), (4, (1, 4))):
        for r in served:                                        # a ratio the layout serves pads to itself
            assert mfma.padded_ratio(bits, bits, r) == r
            assert mfma.supported(bits, bits, 32, 128, 32, r)
    assert mfma.padded_ratio(2, 2, 9) is None and mfma.padded_ratio(2, 2, 16) is None
    assert mfma.padded_ratio(2, 4, 3) is None and mfma.padded_ratio(3, 3, 2) is None and mfma.padded_ratio(2, 2, 0) is None
    for bits, ratio, want in TABLE:                             # whatever it answers is a ratio the layout serves
        if want is not None:
            assert want >= ratio and mfma.supported(bits, bits, 32, 128, 32, want) and not mfma.supported(bits, bits, 32, 128, 32, ratio)


@pytest.mark.parametrize("bits,ratio,want", TABLE)
def test_padded_heads(bits, ratio, want):
    cfg = KiviConfig(bits, bits, 32, 32)
    assert padded_heads(cfg, 128, 2 * ratio, 2) == (None if want is None else 2 * want)
    assert padded_heads(cfg, 64, 2 * ratio, 2) is None                           # the layout's head size only
    assert padded_heads(KiviConfig(bits, bits, 64, 64), 128, 2 * ratio, 2) is None   # ... and its group size


def test_padded_heads_leaves_served_ratios_alone():
    cfg = KiviConfig(2, 2, 32, 32)
    for ratio in (1, 4, 8):
        assert padded_heads(cfg, 128, 2 * ratio, 2) is None


def _cfg(ratio, **kw):
    d = dict(hidden_size=256, num_attention_heads=2 * ratio, num_key_value_heads=2, num_hidden_layers=2, intermediate_size=512,
             vocab_size=64, head_dim=128)
    return make_config(d, **kw)


def test_make_config_leaves_the_option_off():
    assert _cfg(2).kivi_qk_kernel is False
    assert _cfg(2, qk_kernel=True).kivi_qk_kernel is True
    with pytest.raises(TypeError):
        _cfg(2, qk_kernl=True)


@pytest.mark.parametrize("ratio,on", [(2, 4), (3, 4), (5, 8), (7, 8), (4, 4), (8, 8), (1, 1)])
def test_attention_cache_heads(ratio, on):
    off = LlamaAttention_KIVI(_cfg(ratio), 0)
    assert not off.qk_kernel and off.cache_heads == 2 * ratio       # the option off: the hook-state layout for ratio 2, as ever
    assert LlamaAttention_KIVI(_cfg(ratio, qk_kernel=True), 0).cache_heads == 2 * on
    assert LlamaAttention_KIVI(_cfg(ratio, qk_kernel=True, k_bits=4, v_bits=4), 0).cache_heads == 2 * (on if on <= 4 else ratio)
