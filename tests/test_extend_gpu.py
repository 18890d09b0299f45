"""GPU: the multi-token extend of a KIVI cache (kivi_attention_extend; matrix-pipe layout: kivi_mf_extend_layer, the HIP kernel
mf_extend_kernel + the flushes; hook-state layout: the untuned torch composition).

1. outputs of every unit against the fp64 contract (tests/test_extend_cpu.py: extend64) at the hook bar 3e-3 + 1 ulp;
2. the cache after an extend is bit-identical (9-tuple, range words of both stores) to Q decode steps on a clone, and so is the
   next decode step's output;
3. Q = 1 against the decode step (1.5e-3 + 1 ulp, the bar for two forms of one step);
4. a left-padding mask: the masked keys do not change the output;
5. a 2-layer random-weight model: forward(turn 2, pasts) on both layouts, generate(past_key_values=...), decode_graphed after it.
Shapes are small: the full-size shapes are timed by tools/extend_time.py."""
import pytest
import torch

import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from test_extend_cpu import extend64

pytestmark = pytest.mark.gpu
D, G32 = 128, 32


def _kv(seed, B, h, T, kind):
    if kind == "x30":
        return (make_kv(seed, B, h, T, D).float() * 30).half()
    return make_kv(seed, B, h, T, D, kind)


def _setup(bits, ratio, R, T0, kind, B=2, nh_kv=2):
    from kivi_amd.attention import KiviConfig, make_layer_cache
    cfg = KiviConfig(bits, bits, G32, R)
    k0, v0 = _kv(1, B, nh_kv, T0, kind).cuda(), _kv(2, B, nh_kv, T0, kind).cuda()
    layer = make_layer_cache(cfg, B, nh_kv, D, T0 + 8, "cuda", num_heads=nh_kv * ratio)
    assert layer.layout == "mfma"
    layer.prefill(k0, v0)
    past = T64.prefill_cache(k0, v0, bits, bits, G32, R)
    return layer, past


def _chunk(Q, B, nh, nh_kv, kind, seed=10):
    return (make_kv(seed, B, nh, Q, D).cuda(), _kv(seed + 1, B, nh_kv, Q, kind).cuda(), _kv(seed + 2, B, nh_kv, Q, kind).cuda())


def _assert_same_state(a, b):
    from kivi_amd.quant import mfma
    ta, tb = a.as_tuple(), b.as_tuple()
    for x, y in zip(ta[:8], tb[:8]):
        assert (x is None and y is None) or (x is not None and y is not None and same_bits(x, y))
    assert ta[8] == tb[8]
    assert torch.equal(mfma.range_flags(a.kt), mfma.range_flags(b.kt)) and torch.equal(mfma.range_flags(a.vt), mfma.range_flags(b.vt))


# (bits, nh / nh_kv, R, P0, Q, inputs): ratio 1 / 4 / 8 at 2 bits, 1 / 4 at 4 bits; P0 + Q crossing a 512-token super-block;
# Q = 37 crosses a K flush, Q = 300 runs several.  tests/test_extend_stages_gpu.py runs these cases stage by stage, with the
# 4-bit nh / nh_kv = 4 cases on outlier and x30 inputs.
CASES = [(2, 1, 32, 500, 37, "randn"), (2, 4, 32, 70, 5, "outlier"), (2, 8, 128, 200, 300, "randn"), (2, 1, 128, 480, 1, "x30"),
         (4, 1, 32, 130, 37, "tiny"), (4, 4, 64, 300, 37, "randn"), (2, 4, 32, 1000, 37, "tiny")]


@pytest.mark.parametrize("bits,ratio,R,T0,Q,kind", CASES)
def test_extend_outputs_and_state(bits, ratio, R, T0, Q, kind):
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend
    B, nh_kv = 2, 2
    nh = nh_kv * ratio
    layer, past = _setup(bits, ratio, R, T0, kind, B, nh_kv)
    steps = layer.clone()
    q, kn, vn = _chunk(Q, B, nh, nh_kv, kind)
    out = kivi_attention_extend(q, kn, vn, layer)
    ref, ref_past = extend64(q, kn, vn, past, bits, bits, G32, R)
    ok, ratio_ = gemv_close(out, ref, rtol=3e-3, ulps=1)
    assert ok, ratio_
    assert layer.kv_seq_len == T0 + Q
    for x, y in zip(layer.as_tuple()[:8], ref_past[:8]):       # the contract's cache, bit for bit
        assert (x is None and y is None) or same_bits(x, y)
    for i in range(Q):                                        # Q decode steps on a clone
        kivi_attention_decode(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], steps)
    _assert_same_state(layer, steps)
    qn, kk, vv = _chunk(1, B, nh, nh_kv, kind, seed=50)       # the next step gives the same bits whichever way the cache got there
    assert same_bits(kivi_attention_decode(qn, kk, vv, layer), kivi_attention_decode(qn, kk, vv, steps))
    _assert_same_state(layer, steps)


# ((2, 4, 64, 700): both forms against the contract, stage by stage, in tests/test_extend_stages_gpu.py)
@pytest.mark.parametrize("bits,ratio,R,T0", [(2, 1, 32, 300), (2, 4, 32, 300), (2, 8, 32, 100), (4, 1, 32, 520), (4, 4, 128, 260)])
def test_extend_q1_matches_decode_step(bits, ratio, R, T0):
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend
    B, nh_kv = 2, 2
    layer, _ = _setup(bits, ratio, R, T0, "randn", B, nh_kv)
    other = layer.clone()
    q, kn, vn = _chunk(1, B, nh_kv * ratio, nh_kv, "randn")
    a = kivi_attention_extend(q, kn, vn, layer)
    b = kivi_attention_decode(q, kn, vn, other)
    ok, r = gemv_close(a, b, rtol=1.5e-3, ulps=1)
    assert ok, r
    _assert_same_state(layer, other)


@pytest.mark.parametrize("bits,ratio", [(2, 4), (4, 1)])
def test_extend_left_padding_mask(bits, ratio):
    """Row 0 is left-padded by 32 tokens (a whole K group; V is per token): two caches whose prompts differ only there give the
    same bits under an HF-style 4D mask, and both hold the fp64 contract with that mask."""
    from kivi_amd.attention import kivi_attention_extend
    B, nh_kv, R, T0, Q, pad = 2, 2, 32, 130, 9, 32
    nh = nh_kv * ratio
    from kivi_amd.attention import KiviConfig, make_layer_cache
    cfg = KiviConfig(bits, bits, G32, R)
    k0, v0 = make_kv(1, B, nh_kv, T0, D).cuda(), make_kv(2, B, nh_kv, T0, D).cuda()
    k1, v1 = k0.clone(), v0.clone()
    k1[0, :, :pad] = make_kv(3, 1, nh_kv, pad, D, "outlier")[0].cuda() * 7
    v1[0, :, :pad] = make_kv(4, 1, nh_kv, pad, D, "outlier")[0].cuda() * 7
    mask = torch.zeros((B, 1, Q, T0 + Q), dtype=torch.float16, device="cuda")
    mask[0, :, :, :pad] = torch.finfo(torch.float16).min
    q, kn, vn = _chunk(Q, B, nh, nh_kv, "randn")
    outs = []
    for kk, vv in ((k0, v0), (k1, v1)):
        layer = make_layer_cache(cfg, B, nh_kv, D, T0 + 8, "cuda", num_heads=nh)
        layer.prefill(kk, vv)
        out = kivi_attention_extend(q, kn, vn, layer, attention_mask=mask)
        ref, _ = extend64(q, kn, vn, T64.prefill_cache(kk, vv, bits, bits, G32, R), bits, bits, G32, R, attention_mask=mask)
        ok, r = gemv_close(out, ref, rtol=3e-3, ulps=1)
        assert ok, r
        outs.append(out)
    assert same_bits(outs[0], outs[1])


def _model(nkv, seed):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    torch.manual_seed(seed)
    cfg = make_config(dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=nkv, num_hidden_layers=2,
                           intermediate_size=1024, vocab_size=320), residual_length=32)
    model = LlamaForCausalLM_KIVI(cfg).half().cuda()
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.05)
    return model


@pytest.mark.parametrize("nkv", [1, 4])
def test_model_turn2_both_layouts_then_graphed_decode(nkv, monkeypatch):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM
    model = _model(nkv, 3)
    ids1 = torch.randint(0, 320, (2, 45), device="cuda")
    ids2 = torch.randint(0, 320, (2, 23), device="cuda")
    # matrix-pipe layout
    _, p_mf = model(ids1)
    assert p_mf[0].layer.layout == "mfma"
    lg_mf, p_mf = model(ids2, p_mf, last_token_only=False)
    # hook-state layout (the untuned path)
    with monkeypatch.context() as m:
        m.setattr(CM, "supported", lambda *a, **k: False)
        m.setattr(A, "_mf_supported", lambda *a, **k: False)
        _, p_hs = model(ids1)
        assert getattr(p_hs[0].layer, "layout", "") != "mfma"
        lg_hs, p_hs = model(ids2, p_hs, last_token_only=False)
    assert lg_mf.shape == lg_hs.shape == (2, 23, 320)
    rms = lg_hs.float().pow(2).mean().sqrt().item()
    assert (lg_mf.float() - lg_hs.float()).abs().max().item() <= 1e-2 * rms
    assert p_mf[0][-1] == p_hs[0][-1] == 68
    # then decoding: graphed over the extended caches vs eager forward() over a clone
    tok = lg_mf[:, -1:].argmax(-1)
    clones = [p.layer.clone().as_tuple() for p in p_mf]
    eager, t, pe = [], tok, clones
    for _ in range(12):
        eager.append(t)
        lg, pe = model(t, pe)
        t = lg.argmax(-1)
    graphed = model.decode_graphed(tok, p_mf, 68, 12)
    assert torch.equal(graphed, torch.cat(eager, 1))
    # generate(past_key_values=...) continues a conversation from the caches
    _, p3 = model(ids1)
    gen = model.generate(ids2, 4, past_key_values=p3)
    assert gen.shape == (2, 27) and torch.equal(gen[:, 23:24], tok)
