"""GPU: checkpoint and exact rollback of the quantised KV cache (kivi_cache_snapshot, KiviCacheBase.checkpoint / restore_,
LlamaForCausalLM_KIVI.checkpoint / restore_).

The scheme of the layer tests: prefill P0, decode `a` steps, checkpoint at F = P0 + a, decode `n` steps of stream A, restore, decode
`m` steps of stream B.  The oracle is an independent cache fed the prefill, the `a` steps and stream B, never rolled back.  After
the restore the 9-tuple and the range words, the output of every step of B, and the 9-tuple and range words at the end are
bit-identical to the oracle's.  B = 3 rows, 2 kv heads, fixed-seed inputs as in tests/test_beam_gpu.py.

The cuts, in units of the residual length R (32; the g = 64 hook cache needs R = 64, a multiple of its group): F with 0, 1 and
R - 1 residual keys, F < R (window not full, nothing of V packed), n = 1 (from R - 1 residual keys: the one step flushes K) and
n = R + 2 (a K flush, V flushes, the ring wraps), F = 500 with n = 40 (a 512-token super-block, the hook layout's window
compaction, and the stores grow between checkpoint and restore), and a cache of capacity 64 that stream A forces to grow.
"""
import warnings

import pytest
import torch

from helpers import make_kv, same_bits
from test_extend_gpu import _model

pytestmark = pytest.mark.gpu
B, NH_KV = 3, 2

# (layout, bits, nh / nh_kv, g, R, D)
LAYOUTS = [("mfma", 2, 1, 32, 32, 128), ("mfma", 2, 4, 32, 32, 128), ("mfma", 2, 8, 32, 32, 128), ("mfma", 4, 1, 32, 32, 128),
           ("mfma", 4, 4, 32, 32, 128), ("hook", 2, 1, 32, 32, 128), ("hook", 2, 1, 64, 64, 64)]
IDS = ["mf2x1", "mf2x4", "mf2x8", "mf4x1", "mf4x4", "hook_g32_D128", "hook_g64_D64"]


def _cuts(R):
    """(P0, a, n, m, capacity or None)"""
    return [(2 * R - 4, 4, 1, 3, None),            # F = 2R: the residual is empty
            (2 * R - 4, 5, R + 2, R + 4, None),    # one residual key; A and B both flush K, the ring wraps
            (3 * R - 6, 5, R + 2, 5, None),        # R - 1 residual keys
            (3 * R - 6, 5, 1, 2, None),            # ... and the single step of A is the K flush
            (10, 10, R + 2, R + 2, None),          # F = 20 < R: the window is not full, nothing of V is packed
            (490, 10, 40, 40, None),               # F = 500: across 512, the stores are reallocated under the checkpoint
            (R + 8, 5, R + 2, 6, 64)]              # capacity 64: stream A forces reserve()


def _layer(layout, bits, ratio, g, R, D, cap):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, make_layer_cache
    cfg = KiviConfig(bits, bits, g, R)
    if layout == "hook":
        return KiviLayerCache(cfg, B, NH_KV, D, cap, "cuda")
    layer = make_layer_cache(cfg, B, NH_KV, D, cap, "cuda", num_heads=NH_KV * ratio)
    assert layer.layout == "mfma"
    return layer


def _same_state(a, b):
    ta, tb = a.as_tuple(), b.as_tuple()
    for x, y in zip(ta[:8], tb[:8]):
        assert (x is None and y is None) or (x is not None and y is not None and same_bits(x, y))
    assert ta[8] == tb[8]
    if getattr(a, "layout", "") == "mfma":
        from kivi_amd.quant import mfma
        for sa, sb in ((a.kt, b.kt), (a.vt, b.vt)):
            assert torch.equal(mfma.range_flags(sa), mfma.range_flags(sb))


def _qkv(seed, s, nh, D, Q=1, scale=1.0):
    q = make_kv(seed + 3 * s, B, nh, Q, D).cuda()
    k = (make_kv(seed + 3 * s + 1, B, NH_KV, Q, D) * scale).half().cuda()
    v = (make_kv(seed + 3 * s + 2, B, NH_KV, Q, D) * scale).half().cuda()
    return q, k, v


def _steps(layer, n, nh, D, seed, scale=1.0):
    """n decode steps of the stream `seed`; the outputs of all of them."""
    from kivi_amd.attention import kivi_attention_decode
    return [kivi_attention_decode(*_qkv(seed, s, nh, D, scale=scale), layer) for s in range(n)]


def _start(shape, P0, a, cap=None):
    """A cache fed the prefill and the `a` steps every case starts with."""
    layout, bits, ratio, g, R, D = shape
    layer = _layer(layout, bits, ratio, g, R, D, cap or P0 + 8)
    layer.prefill(make_kv(1, B, NH_KV, P0, D).cuda(), make_kv(2, B, NH_KV, P0, D).cuda())
    _steps(layer, a, NH_KV * ratio, D, 500)
    return layer


STREAM_A, STREAM_B, A_SCALE = 1000, 2000, 200.0


@pytest.mark.parametrize("cut", range(7))
@pytest.mark.parametrize("shape", LAYOUTS, ids=IDS)
def test_rollback_is_exact(shape, cut):
    ratio, R, D = shape[2], shape[4], shape[5]
    P0, a, n, m, cap = _cuts(R)[cut]
    nh = NH_KV * ratio
    layer = _start(shape, P0, a, cap)
    ck = layer.checkpoint()
    assert ck.kv_seq_len == P0 + a and ck.nbytes() == ck.buf.numel() > 0
    ptrs = (layer.k_res.data_ptr(), layer.v_res.data_ptr())
    # stream A is 200 x larger: its scales mark the range words, and whatever it leaves behind would show in B's outputs
    _steps(layer, n, nh, D, STREAM_A, scale=A_SCALE)
    grew = layer.cap
    assert layer.restore_(ck) is layer
    assert layer.cap == grew and ptrs == (layer.k_res.data_ptr(), layer.v_res.data_ptr())     # nothing shrunk or reallocated
    oracle = _start(shape, P0, a, cap)
    _same_state(layer, oracle)
    for got, ref in zip(_steps(layer, m, nh, D, STREAM_B), _steps(oracle, m, nh, D, STREAM_B)):
        assert same_bits(got, ref)
    _same_state(layer, oracle)


@pytest.mark.parametrize("shape", [LAYOUTS[1], LAYOUTS[3], LAYOUTS[5], LAYOUTS[6]], ids=[IDS[1], IDS[3], IDS[5], IDS[6]])
def test_restore_then_extend(shape):
    from kivi_amd.attention import kivi_attention_extend
    ratio, R, D = shape[2], shape[4], shape[5]
    nh = NH_KV * ratio
    layer = _start(shape, 3 * R - 6, 5)                    # R - 1 residual keys
    ck = layer.checkpoint()
    _steps(layer, R + 2, nh, D, STREAM_A, scale=A_SCALE)
    layer.restore_(ck)
    oracle = _start(shape, 3 * R - 6, 5)
    q, k, v = _qkv(STREAM_B, 0, nh, D, Q=37)
    assert same_bits(kivi_attention_extend(q, k, v, layer), kivi_attention_extend(q, k, v, oracle))
    _same_state(layer, oracle)
    assert same_bits(_steps(layer, 1, nh, D, 3000)[0], _steps(oracle, 1, nh, D, 3000)[0])


def _flat(t):
    """Byte copy of the whole allocation behind `t` (a matrix-pipe store: the super-blocks and the range words behind them)."""
    stg = t.untyped_storage()
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(stg, 0, (stg.nbytes(),), (1,)).clone()


@pytest.mark.parametrize("shape", [LAYOUTS[1], LAYOUTS[4], LAYOUTS[5]], ids=[IDS[1], IDS[4], IDS[5]])
def test_restore_leaves_the_packed_stores_alone(shape):
    """Byte copies of the packed stores before and after restore_ differ in the range words and nowhere else."""
    from kivi_amd.quant import mfma
    layout, ratio, R, D = shape[0], shape[2], shape[4], shape[5]
    nh = NH_KV * ratio
    layer = _start(shape, 10, 10)                          # F = 20: nothing is packed yet, the range words are still zero
    ck = layer.checkpoint()
    _steps(layer, 2 * R + 2, nh, D, STREAM_A, scale=A_SCALE)   # K flushes and V flushes of large values
    names = ("kt", "vt") if layout == "mfma" else ("k_code", "k_scale", "k_mn", "v_code", "v_scale", "v_mn")
    before = [_flat(getattr(layer, n)) for n in names]
    if layout == "mfma":
        marked = [mfma.range_flags(getattr(layer, n)).clone() for n in names]
        assert all(bool(x.any()) for x in marked)
    layer.restore_(ck)
    for i, n in enumerate(names):
        after = _flat(getattr(layer, n))
        if layout != "mfma":
            assert torch.equal(after, before[i])
            continue
        st = getattr(layer, n)
        main = st.shape[0] * st.shape[1] * st.shape[2] * st.shape[3] * 4
        assert torch.equal(after[:main], before[i][:main])
        assert not mfma.range_flags(st).any() and not torch.equal(after[main:], before[i][main:])


def _slab_views(layer, slabs, rows):
    """Byte copies of the layer's allocations, and torch views (rows, n0, n1, n2, run) into them of what the slabs name."""
    mems = [(t.untyped_storage().data_ptr(), _flat(t)) for t in (layer.kt, layer.vt, layer.k_res, layer.v_res)]
    views = []
    for base, rs, levels, run in slabs:
        p0, mem = next((p, m) for p, m in mems if p <= base < p + m.numel())
        views.append(torch.as_strided(mem, (rows, *[n for n, _ in levels], run), (rs, *[st for _, st in levels], 1), base - p0))
    return [m for _, m in mems], views


@pytest.mark.parametrize("from_token", [200, 0])
def test_snapshot_of_levelled_slabs(from_token):
    """checkpoint() hands kivi_cache_snapshot flat slabs only (residual, window, range words).  Here the entry point gets what a
    reorder of a matrix-pipe cache of 530 tokens moves (B = 2, 2 kv heads).  From token 200: the 3-level K scale pieces, the
    2-level V scale runs, the range words (word-wide), flat slabs of a full chunk and a partial one (codes, window).  From token 0:
    the whole super-blocks under a head level, full chunks of a slab that is not flat.  The gathered buffer is what torch reads at
    the slabs' addresses, in the buffer-row format; scattered into a cache with other strides, the cache's allocations change in
    those bytes and nowhere else."""
    from kivi_amd import checkpoint
    from kivi_amd.attention import KiviConfig, make_layer_cache
    rows, T = 2, 530

    def cache(cap, seed):
        lc = make_layer_cache(KiviConfig(2, 2, 32, 32), rows, NH_KV, 128, cap, "cuda", num_heads=NH_KV)
        lc.prefill(make_kv(seed, rows, NH_KV, T, 128).cuda(), make_kv(seed + 1, rows, NH_KV, T, 128).cuda())
        return lc
    src, dst = cache(T + 8, 1), cache(2100, 3)
    slabs, into = src._reorder_slabs(from_token), dst._reorder_slabs(from_token)
    shape = [([n for n, _ in s[2]], s[3]) for s in slabs]
    assert shape == [([n for n, _ in s[2]], s[3]) for s in into] and src.kt.stride(0) != dst.kt.stride(0)
    units = [(n, n[0] * n[1] * n[2] * run // 16) for n, run in shape if run % 16 == 0]
    assert any(run % 16 for _, run in shape) and any(n[1:] == [1, 1] and 1024 < u < 2048 for n, u in units)      # word-wide; flat
    assert any(min(n) > 1 for n, _ in units) if from_token else any(n[1] > 1 and u >= 1024 for n, u in units)
    before, views = _slab_views(src, slabs, rows)
    pieces = [v.reshape(rows, -1) for v in views]
    buf = torch.zeros((rows, checkpoint.row_bytes(slabs)), dtype=torch.uint8, device="cuda")
    checkpoint.run(slabs, rows, buf, 0)
    assert torch.equal(buf, torch.cat([torch.nn.functional.pad(x, (0, -x.shape[1] % 16)) for x in pieces], 1))
    want, views = _slab_views(dst, into, rows)                 # copies from before the scatter: the slabs' bytes are replaced
    off = 0
    for v, x in zip(views, pieces):
        v.copy_(x.reshape(v.shape))
        assert torch.equal(buf[:, off: off + x.shape[1]], x)
        off += -(-x.shape[1] // 16) * 16
    checkpoint.run(into, rows, buf, 1)
    for t, w in zip((dst.kt, dst.vt, dst.k_res, dst.v_res), want):
        assert torch.equal(_flat(t), w)
    for t, b in zip((src.kt, src.vt, src.k_res, src.v_res), before):
        assert torch.equal(_flat(t), b)                        # the source was only read


@pytest.mark.parametrize("shape", [LAYOUTS[1], LAYOUTS[5]], ids=[IDS[1], IDS[5]])
def test_two_checkpoints_and_staleness(shape):
    ratio, R, D = shape[2], shape[4], shape[5]
    nh = NH_KV * ratio
    P0, a1, a2 = 2 * R + 5, 5, R + 9                       # F1 = 2R + 10, F2 = 3R + 14
    layer = _start(shape, P0, a1)
    ck1 = layer.checkpoint()
    _steps(layer, a2 - a1, nh, D, 700)
    ck2 = layer.checkpoint()
    o2 = _start(shape, P0, a1)
    _steps(o2, a2 - a1, nh, D, 700)
    _steps(layer, R + 2, nh, D, STREAM_A, scale=A_SCALE)
    layer.restore_(ck2)
    _same_state(layer, o2)
    _steps(layer, 7, nh, D, STREAM_B)
    layer.restore_(ck2)                                    # the same checkpoint twice: fine
    _same_state(layer, o2)
    layer.restore_(ck1)
    _same_state(layer, _start(shape, P0, a1))
    _steps(layer, a2 - a1 + 3, nh, D, STREAM_A)            # past F2 again, with other tokens
    with pytest.raises(ValueError, match="stale"):
        layer.restore_(ck2)
    ck3 = layer.checkpoint()
    layer.reorder_(torch.tensor([1, 0, 2], device="cuda"))
    for ck in (ck1, ck3):
        with pytest.raises(ValueError, match="stale"):
            layer.restore_(ck)


def test_hook_state_flags_are_restored():
    """Hook state, R = 256: past 136 residual keys a layer leaves the fused attend launch for good (its rows no longer fit); the
    checkpoint at 100 residual keys brings that fusion level back, so the steps after the restore run -- bit for bit -- as the
    oracle's, which never went that far."""
    shape = ("hook", 2, 1, 32, 256, 128)
    layer = _start(shape, 90, 10)
    assert layer.k_res_len == 100 and not layer._attend_unfusable
    ck = layer.checkpoint()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _steps(layer, 60, NH_KV, 128, STREAM_A)
    dropped = (layer._attend_unfusable, layer._softmax_unfusable, layer._fused_unsupported)
    assert any(dropped), "stream A was meant to push the layer off a fusion level"
    layer.restore_(ck)
    oracle = _start(shape, 90, 10)
    assert (layer._attend_unfusable, layer._softmax_unfusable, layer._fused_unsupported) == (False, False, False)
    _same_state(layer, oracle)
    for got, ref in zip(_steps(layer, 10, NH_KV, 128, STREAM_B), _steps(oracle, 10, NH_KV, 128, STREAM_B)):
        assert same_bits(got, ref)
    _same_state(layer, oracle)


# ------------------------------------------------------------------ the model
def _on_layout(layout, monkeypatch):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM
    if layout == "hook":
        monkeypatch.setattr(CM, "supported", lambda *a, **k: False)
        monkeypatch.setattr(A, "_mf_supported", lambda *a, **k: False)


def _greedy(model, logits, pasts, steps, mask=None, pick=None):
    """`steps` decode steps from the logits of the pass before: (tokens fed, their logits, pasts)."""
    toks, lgs = [], []
    pick = pick or (lambda lg: lg.argmax(-1))
    tok = pick(logits)
    for _ in range(steps):
        toks.append(tok)
        if mask is not None:
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        logits, pasts = model(tok, pasts, padding_mask=mask)
        lgs.append(logits)
        tok = pick(logits)
    return torch.cat(toks, 1), torch.cat(lgs, 1), pasts


@pytest.mark.parametrize("padded", [False, True], ids=["equal", "left_padded"])
@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_rollback_repeats_the_run(layout, padded, monkeypatch):
    from kivi_amd.llama import left_pad
    _on_layout(layout, monkeypatch)
    model = _model(4, 21)
    if padded:
        ids, mask = left_pad([list(range(3, 48)), list(range(50, 71))], pad_token_id=0, device="cuda")
    else:
        ids, mask = torch.randint(0, 320, (2, 45), device="cuda", generator=torch.Generator("cuda").manual_seed(9)), None
    logits, pasts = model(ids, padding_mask=mask)
    assert getattr(pasts[0].layer, "layout", "hook") == layout
    ck = model.checkpoint(pasts)
    assert ck.kv_seq_len == 45 and len(ck.layers) == 2
    t1, l1, end = _greedy(model, logits, pasts, 40, mask)
    assert end[0][-1] == 85
    fresh = model.restore_(end, ck)
    assert [p[-1] for p in fresh] == [45, 45]
    t2, l2, _ = _greedy(model, logits, fresh, 40, mask)
    assert torch.equal(t1, t2) and same_bits(l1, l2)
    # the tuples of the prompt pass are stale by length but still name their caches
    t3, l3, _ = _greedy(model, logits, model.restore_(pasts, ck), 40, mask)
    assert torch.equal(t1, t3) and same_bits(l1, l3)
    with pytest.raises(ValueError, match="in-place cache"):
        model.restore_([(None,) * 8 + (45,)] * 2, ck)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_rollback_then_graphed_decode(layout, monkeypatch):
    _on_layout(layout, monkeypatch)
    model = _model(4, 22)
    ids = torch.randint(0, 320, (2, 45), device="cuda", generator=torch.Generator("cuda").manual_seed(10))
    logits, pasts = model(ids)
    ck = model.checkpoint(pasts)
    eager, _, _ = _greedy(model, logits, pasts, 40)
    tok = logits.argmax(-1)
    stats = []
    for _ in range(2):                                     # the second pass replays the graph the first one captured
        pasts = model.restore_(pasts, ck)
        assert torch.equal(model.decode_graphed(tok, pasts, 45, 40), eager)
        stats.append(model.graphs.stats)
    if layout == "mfma":                                   # (eager steps, captures, replays) of the whole-step graph, cumulative
        assert stats[1][1] == stats[0][1] and stats[1][2] == stats[0][2] + 40
    model.release_graphs()


def test_model_rollback_and_sampler_reset():
    from kivi_amd.sampling import Sampler
    model = _model(4, 23)
    ids = torch.randint(0, 320, (2, 45), device="cuda", generator=torch.Generator("cuda").manual_seed(11))
    logits, pasts = model(ids)
    ck = model.checkpoint(pasts)
    sampler = Sampler(0.9, 40, 0.95, None, 7, "cuda")
    t1, l1, end = _greedy(model, logits, pasts, 40, pick=sampler)
    sampler.reset(7)
    t2, l2, _ = _greedy(model, logits, model.restore_(end, ck), 40, pick=sampler)
    assert torch.equal(t1, t2) and same_bits(l1, l2)
