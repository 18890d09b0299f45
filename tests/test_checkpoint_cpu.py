"""CPU: checkpoint / rollback of the KIVI cache (kivi_cache_snapshot, KiviCacheBase.checkpoint / restore_, the model methods).

* The library exports kivi_cache_snapshot and refuses bad arguments before anything is enqueued (fake pointers that are never
  dereferenced, as in tests/test_beam_cpu.py): KIVI_EINVAL for counts, null pointers, the buffer stride and the direction,
  KIVI_EALIGN for misaligned bases, runs and buffers; the ABI version is still 3.
* The slab lists of both layouts and the bytes a checkpoint takes, on CPU-allocated caches (no kernel involved).
* The ValueErrors of restore_ and of the model methods, raised before anything runs on a device: the launch itself
  (kivi_amd.checkpoint.run) is replaced by a recorder, so the host-side record of what is stale is what is tested.
"""
import pytest
import torch

EINVAL, EALIGN = -1, -2


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def test_snapshot_symbol_exported(lib):
    from kivi_amd import _lib
    assert hasattr(lib, "kivi_cache_snapshot") and "kivi_cache_snapshot" in _lib.SIGNATURES
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3


def _slabs(n=1, base=1 << 20, run=4096, rs=1 << 16):
    from kivi_amd import _lib
    arr = (_lib.ReorderSlab * max(n, 1))()
    for d in arr:
        d.base, d.row_stride, d.run = base, rs, run
        for k in range(3):
            d.n[k], d.stride[k] = 1, 0
    return arr


@pytest.mark.parametrize("case,rc", [
    ("no_slabs", EINVAL), ("negative_slabs", EINVAL), ("too_many_slabs", EINVAL), ("B0", EINVAL), ("B_negative", EINVAL),
    ("null_slabs", EINVAL), ("null_buf", EINVAL), ("null_base", EINVAL), ("negative_count", EINVAL), ("stride0", EINVAL),
    ("stride_too_small", EINVAL), ("stride_too_small_two_slabs", EINVAL), ("direction2", EINVAL), ("direction_negative", EINVAL),
    ("base_misaligned", EALIGN), ("run_misaligned", EALIGN), ("row_stride_misaligned", EALIGN), ("level_stride_misaligned", EALIGN),
    ("buf_misaligned", EALIGN), ("buf_stride_misaligned", EALIGN)])
def test_snapshot_refuses_bad_arguments(lib, case, rc):
    from kivi_amd import _lib
    B, buf, stride, direction, n = 8, 1 << 24, 4096, 0, 1
    slabs = _slabs()
    if case == "no_slabs":
        n = 0
    elif case == "negative_slabs":
        n = -1
    elif case == "too_many_slabs":
        n = _lib.REORDER_MAX_SLABS + 1
        slabs, stride = _slabs(n, run=16), 16 * n
    elif case == "B0":
        B = 0
    elif case == "B_negative":
        B = -3
    elif case == "null_slabs":
        slabs = None
    elif case == "null_buf":
        buf = None
    elif case == "null_base":
        slabs = _slabs(base=0)
    elif case == "negative_count":
        slabs[0].n[2] = -1
    elif case == "stride0":
        stride = 0
    elif case == "stride_too_small":
        stride = 4096 - 16
    elif case == "stride_too_small_two_slabs":      # a word slab of 8 bytes takes 16 in the buffer row
        n = 2
        slabs, stride = _slabs(2, run=8), 16
    elif case == "direction2":
        direction = 2
    elif case == "direction_negative":
        direction = -1
    elif case == "base_misaligned":
        slabs = _slabs(base=(1 << 20) + 2)
    elif case == "run_misaligned":
        slabs = _slabs(run=4094)
    elif case == "row_stride_misaligned":
        slabs = _slabs(rs=(1 << 16) + 1)
    elif case == "level_stride_misaligned":
        slabs[0].n[0], slabs[0].stride[0] = 2, 8190
    elif case == "buf_misaligned":
        buf += 8
    elif case == "buf_stride_misaligned":
        stride = 4096 + 8
    assert lib.kivi_cache_snapshot(slabs, n, B, buf, stride, direction, None) == rc
    assert b"kivi_cache_snapshot" in lib.kivi_last_error()


def test_snapshot_empty_slabs_enqueue_nothing(lib):
    """Slabs with a zero count or run move nothing and take no room in the buffer row."""
    assert lib.kivi_cache_snapshot(_slabs(run=0), 1, 8, 1 << 24, 16, 0, None) == 0
    s = _slabs(2, run=0)
    s[1].n[1] = 0
    assert lib.kivi_cache_snapshot(s, 2, 8, 1 << 24, 16, 1, None) == 0


# ------------------------------------------------------------------ the slab lists and what a checkpoint holds
def _cache(layout, B=3, nh_kv=2, R=32, cap=200, bits=2, ratio=1, g=32, D=128):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, make_layer_cache
    cfg = KiviConfig(bits, bits, g, R)
    if layout == "hook":
        return KiviLayerCache(cfg, B, nh_kv, D, cap, "cpu")
    lc = make_layer_cache(cfg, B, nh_kv, D, cap, "cpu", num_heads=nh_kv * ratio)
    assert lc.layout == "mfma"
    return lc


def _set_len(lc, kv):
    """The lengths of the state machine at kv tokens (cache.py: K flushes whole residuals, V keeps a window of R)."""
    R = lc.cfg.residual_length
    lc.k_quant_len, lc.k_res_len = kv // R * R, kv % R
    lc.v_quant_len, lc.v_res_len = max(kv - R, 0), min(kv, R)
    lc.v_res_start = lc.v_quant_len % lc.v_res.shape[2]
    lc.kv_seq_len = kv


def test_checkpoint_slabs_of_both_layouts():
    from kivi_amd import checkpoint
    from kivi_amd.quant import mfma
    hook = _cache("hook", D=64, g=64, R=64)
    assert hook._checkpoint_slabs() == [] and checkpoint.row_bytes([]) == 0
    _set_len(hook, 100)                  # residual 36 keys, window 64 values from row 36
    (kb, krs, klv, krun), (vb, vrs, vlv, vrun) = hook._checkpoint_slabs()
    assert (kb, krs, klv[0], krun) == (hook.k_res.data_ptr(), 2 * 64 * 64 * 2, (2, 64 * 64 * 2), 36 * 128)
    assert (vb, vrs, vlv[0], vrun) == (hook.v_res.data_ptr() + 36 * 128, 2 * 129 * 64 * 2, (2, 129 * 64 * 2), 64 * 128)
    assert checkpoint.row_bytes(hook._checkpoint_slabs()) == 2 * (36 + 64) * 128
    # the lengths of a checkpoint, not the current ones, when restoring
    assert hook._checkpoint_slabs(dict(k_res_len=0, v_res_start=5, v_res_len=7)) == [
        (hook.v_res.data_ptr() + 5 * 128, 2 * 129 * 128, [(2, 129 * 128), (1, 0), (1, 0)], 7 * 128)]
    mf = _cache("mfma")
    _set_len(mf, 37)
    sl = mf._checkpoint_slabs()
    assert [s[0] for s in sl] == [mf.k_res.data_ptr(), mf.v_res.data_ptr(), mfma.range_flags(mf.kt).data_ptr(),
                                  mfma.range_flags(mf.vt).data_ptr()]
    assert [s[3] for s in sl] == [5 * 256, 33 * 256, 8, 8] and sl[2][1] == 8        # the range words: word moves, 8 bytes a row
    assert checkpoint.row_bytes(sl) == 2 * 5 * 256 + 2 * 33 * 256 + 16 + 16          # every slab starts on a 16-byte boundary
    _set_len(mf, 64)
    assert len(mf._checkpoint_slabs()) == 3                                          # an empty residual is left out


def test_checkpoint_size_at_the_llama2_7b_shape():
    """B = 32, 32 / 32 heads, R = 32, the residual as full as it gets -- 16.8 MB, against the 400 MB of the layer's
    cache at 4127 tokens."""
    from kivi_amd import checkpoint
    mf = _cache("mfma", B=32, nh_kv=32, cap=64)
    _set_len(mf, 63)
    per_row = checkpoint.row_bytes(mf._checkpoint_slabs())
    assert per_row == 32 * (31 + 33) * 256 + 2 * 128
    assert 32 * per_row < 17e6


# ------------------------------------------------------------------ restore_ refuses before anything runs on a device
@pytest.fixture
def launches(monkeypatch):
    """kivi_amd.checkpoint.run replaced by a recorder: (number of slabs, direction) per call."""
    from kivi_amd import checkpoint
    calls = []
    monkeypatch.setattr(checkpoint, "run", lambda slabs, B, buf, direction: calls.append((len(slabs), direction)))
    return calls


@pytest.mark.parametrize("layout", ["hook", "mfma"])
def test_restore_puts_lengths_and_flags_back(layout, launches):
    from kivi_amd import checkpoint
    lc = _cache(layout)
    _set_len(lc, 70)
    nat = lc._native = ("descriptor",)
    ck = lc.checkpoint()
    assert launches == [(len(lc._checkpoint_slabs()), 0)]
    assert ck.kv_seq_len == 70 and ck.state == (64, 6, 38, 38 % lc.v_res.shape[2], 32, 70) and ck.flags == (False, False, False)
    assert ck.nbytes() == 3 * checkpoint.row_bytes(lc._checkpoint_slabs()) == ck.buf.numel()
    assert ck.buf.data_ptr() not in (lc.k_res.data_ptr(), lc.v_res.data_ptr())      # a buffer of its own
    _set_len(lc, 111)
    lc._attend_unfusable = lc._fused_unsupported = True
    old = lc.as_tuple()
    assert lc.restore_(ck) is lc
    assert launches[-1][1] == 1 and len(launches) == 2                               # one scatter launch
    assert tuple(getattr(lc, n) for n in checkpoint.LENGTHS) == ck.state
    assert not (lc._attend_unfusable or lc._softmax_unfusable or lc._fused_unsupported)
    assert lc._native is nat                                                         # descriptors stay valid
    assert old[-1] == 111 and lc.as_tuple()[-1] == 70
    with pytest.raises(RuntimeError, match="stale"):                                 # tuples issued before stay stale
        old[1]


@pytest.mark.parametrize("layout", ["hook", "mfma"])
def test_restore_refuses_stale_and_foreign_checkpoints(layout, launches):
    lc = _cache(layout)
    _set_len(lc, 40)
    ck1 = lc.checkpoint()
    _set_len(lc, 50)
    ck2 = lc.checkpoint()
    _set_len(lc, 45)
    with pytest.raises(ValueError, match="beyond"):       # never mind how the cache got shorter: the checkpoint is ahead of it
        lc.restore_(ck2)
    _set_len(lc, 90)
    n = len(launches)
    lc.restore_(ck2)
    _set_len(lc, 60)
    lc.restore_(ck2)                                      # the same checkpoint again
    ck3 = lc.checkpoint()                                 # at 50, after the restores
    lc.restore_(ck1)
    assert len(launches) == n + 4
    _set_len(lc, 95)
    for ck in (ck2, ck3):                                 # the cache has been below them since they were taken
        with pytest.raises(ValueError, match="stale checkpoint.*restored to kv length 40"):
            lc.restore_(ck)
    ck4 = lc.checkpoint()                                 # taken after that restore: fine, and so is ck1
    _set_len(lc, 99)
    lc.restore_(ck4)
    lc.restore_(ck1)
    assert lc.kv_seq_len == 40
    n = len(launches)
    # another geometry, another layout, another cache
    other = _cache(layout, B=4)
    _set_len(other, 90)
    with pytest.raises(ValueError, match="another geometry or layout"):
        other.restore_(ck1)
    other = _cache("mfma" if layout == "hook" else "hook")
    _set_len(other, 90)
    with pytest.raises(ValueError, match="another geometry or layout"):
        other.restore_(ck1)
    twin = _cache(layout)
    _set_len(twin, 90)
    with pytest.raises(ValueError, match="another cache"):
        twin.restore_(ck1)
    with pytest.raises(ValueError, match="KiviCheckpoint"):
        lc.restore_(lc.as_tuple())
    assert len(launches) == n and lc.kv_seq_len == 40     # the refusals launched nothing and changed nothing


def test_reorder_and_prefill_make_checkpoints_stale(launches, monkeypatch):
    from kivi_amd import reorder
    monkeypatch.setattr(reorder, "run", lambda *a, **k: None)
    lc = _cache("mfma")
    _set_len(lc, 40)
    ck = lc.checkpoint()
    _set_len(lc, 44)
    lc.reorder_(torch.tensor([1, 0, 2]), check=False)
    with pytest.raises(ValueError, match="stale checkpoint.*reordered"):
        lc.restore_(ck)
    after = lc.checkpoint()
    _set_len(lc, 50)
    lc.restore_(after)                                    # a checkpoint taken after the reorder is fine
    assert lc.kv_seq_len == 44
    lc._void_checkpoints()                                # what a new prompt pass (prefill) does
    with pytest.raises(ValueError, match="stale"):
        lc.restore_(after)


# ------------------------------------------------------------------ the model methods
def test_model_checkpoint_refusals(launches):
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    plain = [(None,) * 8 + (5,)]
    with pytest.raises(ValueError, match="in-place cache"):
        LlamaForCausalLM_KIVI.checkpoint(plain)
    with pytest.raises(ValueError, match="in-place cache"):
        LlamaForCausalLM_KIVI.checkpoint(None)
    caches = [_cache("mfma"), _cache("mfma")]
    for c in caches:
        _set_len(c, 40)
    past = [c.as_tuple() for c in caches]
    ck = LlamaForCausalLM_KIVI.checkpoint(past)
    assert ck.kv_seq_len == 40 and len(ck.layers) == 2 and ck.nbytes() == sum(c.nbytes() for c in ck.layers)
    for c in caches:
        _set_len(c, 47)
    with pytest.raises(ValueError, match="in-place cache"):
        LlamaForCausalLM_KIVI.restore_(plain, ck)
    with pytest.raises(ValueError, match="layers"):
        LlamaForCausalLM_KIVI.restore_(past[:1], ck)
    fresh = LlamaForCausalLM_KIVI.restore_(past, ck)        # tuples whose length is stale still name their caches
    assert [t[-1] for t in fresh] == [40, 40] and all(t.layer is c for t, c in zip(fresh, caches))
    # one layer refuses: no layer is touched
    for c in caches:
        _set_len(c, 47)
    caches[1]._void_checkpoints()
    n = len(launches)
    with pytest.raises(ValueError, match="stale"):
        LlamaForCausalLM_KIVI.restore_(fresh, ck)
    assert len(launches) == n and [c.kv_seq_len for c in caches] == [47, 47]
