"""CPU: continuous batching -- kivi_cache_admit, KiviCacheBase.admit_, LlamaForCausalLM_KIVI.admit_, generate_continuous
(DESIGN.md section 16).

1. The library exports kivi_cache_admit with a ctypes signature; kivi_admit_slab against the struct in include/kivi_hip.h (size,
   field offsets); the ABI version is still 3.
2. Every refusal of the entry point with fake pointers that are never dereferenced: nothing is enqueued.  Empty slabs return 0.
3. The slab lists of both layouts on CPU-allocated caches, run through a small interpreter of the slab semantics (a byte copy per
   (i, level indices) from the source address to the destination address; every destination run has to lie inside row rows[i] of
   one of the destination's buffers): the admitted rows read like the source rows through every reader that works on CPU tensors,
   every byte of every other row is unchanged.  Every pair of ring phases at window lengths 1, R - 1 and R (matrix-pipe layout),
   v_res_start 0 and R (hook-state layout), lengths 20 / 32 / 33 / 512 / 530, a destination with more super-blocks / pages than
   the source, several K pages (page_tokens = 64).
4. The ValueErrors of admit_, model.admit_, generate_continuous, left_pad(length=) and set_row(draw_index=), raised before
   anything runs on a device.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_checkpoint_cpu import _cache, _set_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
R = 32


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ 1. symbol, signature, struct layout
def test_symbol_signature_and_struct_layout(lib):
    from kivi_amd import _lib
    assert hasattr(lib, "kivi_cache_admit")
    res, args = _lib.SIGNATURES["kivi_cache_admit"]
    assert res is ctypes.c_int32 and len(args) == 7 and args[0] == ctypes.POINTER(_lib.AdmitSlab)
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    body = re.search(r"typedef struct kivi_admit_slab \{([^}]*)\}\s*kivi_admit_slab;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"((?:const\s+)?\w+\s*\*?)\s*(\w+)(?:\[(\d+)\])?;", body)
    assert [n for _, n, _ in fields] == ["dst_base", "dst_row_stride", "dst_stride", "src_base", "src_row_stride", "src_stride",
                                         "n", "run"]
    assert [n for n, _ in _lib.AdmitSlab._fields_] == [n for _, n, _ in fields]
    off = 0
    for t, n, count in fields:
        t = t.replace(" ", "")
        assert t in ("void*", "constvoid*", "int64_t"), t              # every member is 8 bytes wide
        assert getattr(_lib.AdmitSlab, n).offset == off, n
        assert getattr(_lib.AdmitSlab, n).size == 8 * int(count or 1), n
        off += 8 * int(count or 1)
    assert off == ctypes.sizeof(_lib.AdmitSlab) == 112 and ctypes.alignment(_lib.AdmitSlab) == 8
    assert int(re.search(r"#define KIVI_REORDER_MAX_SLABS (\d+)", src).group(1)) == _lib.REORDER_MAX_SLABS


# ------------------------------------------------------------------ 2. refusals of the entry point
def _slabs(n=1, dst=1 << 20, src=1 << 24, run=4096, drs=1 << 16, srs=1 << 15):
    from kivi_amd import _lib
    arr = (_lib.AdmitSlab * max(n, 1))()
    for d in arr:
        d.dst_base, d.dst_row_stride, d.src_base, d.src_row_stride, d.run = dst, drs, src, srs, run
        for k in range(3):
            d.n[k], d.dst_stride[k], d.src_stride[k] = 1, 0, 0
    return arr


CASES = ["n_rows0", "n_rows_negative", "n_rows_above_B", "B0", "B_negative", "B_65536", "rows_bytes2", "rows_bytes16", "null_rows",
         "rows_misaligned4", "rows_misaligned8", "negative_slabs", "too_many_slabs", "null_slabs", "negative_count", "negative_run",
         "null_dst_base", "null_src_base", "dst_base_misaligned", "src_base_misaligned", "dst_row_stride_misaligned",
         "src_row_stride_misaligned", "dst_level_stride_misaligned", "src_level_stride_misaligned", "run_misaligned",
         "units_2_31", "units_product_2_31"]
# (the grid bound of 2^31 chunks cannot be reached from outside: 32 slabs of < 2^31 units are at most 2^26 chunks of 1024 units)


@pytest.mark.parametrize("case", CASES)
def test_admit_refuses_bad_arguments(lib, case):
    from kivi_amd import _lib
    n_slabs, n_rows, rows, rows_bytes, B = 1, 2, 1 << 28, 8, 8
    slabs = _slabs()
    if case == "n_rows0":
        n_rows = 0
    elif case == "n_rows_negative":
        n_rows = -1
    elif case == "n_rows_above_B":
        n_rows = 9
    elif case == "B0":
        B = 0
    elif case == "B_negative":
        B = -4
    elif case == "B_65536":
        B = 65536
    elif case == "rows_bytes2":
        rows_bytes = 2
    elif case == "rows_bytes16":
        rows_bytes = 16
    elif case == "null_rows":
        rows = None
    elif case == "rows_misaligned4":
        rows, rows_bytes = (1 << 28) + 2, 4
    elif case == "rows_misaligned8":
        rows = (1 << 28) + 4
    elif case == "negative_slabs":
        n_slabs = -1
    elif case == "too_many_slabs":
        n_slabs = _lib.REORDER_MAX_SLABS + 1
        slabs = _slabs(n_slabs)
    elif case == "null_slabs":
        slabs = None
    elif case == "negative_count":
        slabs[0].n[1] = -1
    elif case == "negative_run":
        slabs[0].run = -16
    elif case == "null_dst_base":
        slabs = _slabs(dst=0)
    elif case == "null_src_base":
        slabs = _slabs(src=0)
    elif case == "dst_base_misaligned":
        slabs = _slabs(dst=(1 << 20) + 2)
    elif case == "src_base_misaligned":
        slabs = _slabs(src=(1 << 24) + 1)
    elif case == "dst_row_stride_misaligned":
        slabs = _slabs(drs=(1 << 16) + 2)
    elif case == "src_row_stride_misaligned":
        slabs = _slabs(srs=(1 << 15) + 3)
    elif case == "dst_level_stride_misaligned":
        slabs[0].n[0], slabs[0].dst_stride[0], slabs[0].src_stride[0] = 2, 8190, 8192
    elif case == "src_level_stride_misaligned":
        slabs[0].n[2], slabs[0].dst_stride[2], slabs[0].src_stride[2] = 2, 8192, 8190
    elif case == "run_misaligned":
        slabs = _slabs(run=4094)
    elif case == "units_2_31":
        slabs[0].n[0] = 1 << 31
    elif case == "units_product_2_31":
        slabs[0].n[0], slabs[0].n[1], slabs[0].run = 1 << 16, 1 << 15, 16
    assert lib.kivi_cache_admit(slabs, n_slabs, n_rows, rows, rows_bytes, B, None) == EINVAL
    assert b"kivi_cache_admit" in lib.kivi_last_error()


def test_admit_empty_slabs_enqueue_nothing(lib):
    assert lib.kivi_cache_admit(None, 0, 1, 1 << 28, 4, 1, None) == 0
    assert lib.kivi_cache_admit(_slabs(run=0), 1, 2, 1 << 28, 8, 8, None) == 0
    s = _slabs(2, run=0)
    s[1].run, s[1].n[1] = 64, 0
    assert lib.kivi_cache_admit(s, 2, 8, 1 << 28, 4, 8, None) == 0
    s = _slabs(dst=0, src=0, run=0)                      # an empty slab is not looked at any further
    assert lib.kivi_cache_admit(s, 1, 1, 1 << 28, 4, 8, None) == 0


# ------------------------------------------------------------------ 3. the slab lists, interpreted
def _buffers(lc):
    """name -> tensor of every buffer a cache object holds (the range words of the matrix-pipe stores included)."""
    from kivi_amd.quant import mfma
    out = {n: getattr(lc, n) for n in lc._BUFFERS}
    if hasattr(lc, "kt"):
        out["kt_range"], out["vt_range"] = mfma.range_flags(lc.kt), mfma.range_flags(lc.vt)
    return out


def _fill(lc, seed):
    g = torch.Generator().manual_seed(seed)
    for t in _buffers(lc).values():
        raw = torch.randint(0, 256, (t.numel() * t.element_size(),), generator=g, dtype=torch.uint8)
        flat = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), t.storage_offset() * t.element_size(),
                                                      (t.numel() * t.element_size(),), (1,))
        assert t.permute(*np.argsort([-s for s in t.stride()]).tolist()).is_contiguous()     # dense: the flat view is the tensor
        flat.copy_(raw)


def _bytes_of(t):
    """(address, uint8 numpy view) of the dense memory of tensor `t`."""
    n = t.numel() * t.element_size()
    flat = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage(), t.storage_offset() * t.element_size(), (n,), (1,))
    return t.data_ptr(), flat.numpy()


def _interpret(slabs, rows, dst, src):
    """The semantics of kivi_cache_admit in Python.  Every source run has to lie inside row i of a buffer of `src`, every
    destination run inside row rows[i] of a buffer of `dst`; returns the bytes written."""
    def regions(lc):
        out = []
        for t in _buffers(lc).values():
            addr, mem = _bytes_of(t)
            out.append((addr, t.stride(0) * t.element_size(), mem))
        return out
    dreg, sreg = regions(dst), regions(src)

    def find(reg, addr, run, row):
        for base, rs, mem in reg:
            if base + row * rs <= addr and addr + run <= base + (row + 1) * rs:
                return mem, addr - base
        raise AssertionError(f"a run of {run} bytes at {addr:#x} lies outside row {row} of every buffer")
    written = 0
    for db, drs, dst_st, sb, srs, src_st, cnt, run in slabs:
        assert run % 4 == 0 and all(x % 4 == 0 for x in (db, drs, sb, srs, *dst_st, *src_st))
        for i, r in enumerate(rows):
            for i0 in range(cnt[0]):
                for i1 in range(cnt[1]):
                    for i2 in range(cnt[2]):
                        sa = sb + i * srs + i0 * src_st[0] + i1 * src_st[1] + i2 * src_st[2]
                        da = db + r * drs + i0 * dst_st[0] + i1 * dst_st[1] + i2 * dst_st[2]
                        smem, so = find(sreg, sa, run, i)
                        dmem, do = find(dreg, da, run, r)
                        dmem[do: do + run] = smem[so: so + run]
                        written += run
    return written


def _mf_used(store, n_tok, is_k, bits):
    """The bytes in use of every (row, head) of a matrix-pipe store holding n_tok tokens, by the index arithmetic of
    kivi_mfma_layout.h: codes of block j at words [j BW, (j + 1) BW) of its super-block; V scales / zero points of block j at
    halves j * 128 of their regions; K scales / zero points of group j at halves (j >> 3) * 1024 + q * 64 + (j & 7) * 8, q < 16."""
    from kivi_amd.quant import mfma
    W = mfma.sb_words(bits)
    S0, BW = (W - 2048) * 4, (W - 2048) // 16 * 4
    B, h = store.shape[:2]
    out = []
    for j in range(-(-n_tok // 32)):
        s, jj = divmod(j, 16)
        sb = store[:, :, s].contiguous().view(torch.uint8).reshape(B, h, W * 4)
        out.append(sb[..., jj * BW: (jj + 1) * BW])
        for region in (0, 1):
            if is_k:
                for q in range(16):
                    o = S0 + region * 4096 + (jj >> 3) * 2048 + q * 128 + (jj & 7) * 16
                    out.append(sb[..., o: o + 16])
            else:
                o = S0 + region * 4096 + jj * 256
                out.append(sb[..., o: o + 256])
    return torch.cat(out, -1) if out else torch.empty((B, h, 0), dtype=torch.uint8)


def _readers(lc):
    """Everything of a cache that reads on CPU tensors, as a list of (B, ...) tensors (None members left out)."""
    from kivi_amd.quant import mfma
    out = [lc.k_res_view(), lc.v_res_view()]
    if hasattr(lc, "kt"):
        out += [_mf_used(lc.kt, lc.k_quant_len, True, lc.cfg.k_bits), _mf_used(lc.vt, lc.v_quant_len, False, lc.cfg.v_bits),
                mfma.range_flags(lc.kt), mfma.range_flags(lc.vt)]
    else:
        out += list(lc.k_quant_reference_layout()) + list(lc.v_quant_views())
    return [t for t in out if t is not None]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _admit_and_check(dst, src, rows):
    before = {n: t.clone() for n, t in _buffers(dst).items()}
    lengths = tuple(getattr(dst, n) for n in ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len"))
    ptrs = {n: t.data_ptr() for n, t in _buffers(dst).items()}
    want = [t.clone() for t in _readers(src)]
    slabs = dst._admit_slabs(src)
    from kivi_amd import admit
    assert admit.moved_bytes(slabs, len(rows)) == 2 * _interpret(admit.live(slabs), rows, dst, src)
    got = _readers(dst)
    assert len(got) == len(want) and len(got) >= 2
    for g, w in zip(got, want):
        for i, r in enumerate(rows):
            assert _same(g[r], w[i]), (r, i, g.shape)
    others = [b for b in range(dst.B) if b not in rows]
    for n, t in _buffers(dst).items():
        assert t.data_ptr() == ptrs[n]
        for b in others:
            assert _same(t[b], before[n][b]), (n, b)
    assert lengths == tuple(getattr(dst, n) for n in ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len"))
    for g, w in zip(_readers(src), want):                # the source is only read
        assert _same(g, w)
    return slabs


def _pair(layout, kv, dst_cap, src_cap, rows, B=3, nh_kv=2, bits=2, page_tokens=None):
    if layout == "hook" and page_tokens:
        from kivi_amd.attention import KiviConfig, KiviLayerCache
        cfg = KiviConfig(bits, bits, 32, R)
        dst = KiviLayerCache(cfg, B, nh_kv, 128, dst_cap, "cpu", page_tokens=page_tokens)
        src = KiviLayerCache(cfg, len(rows), nh_kv, 128, src_cap, "cpu", page_tokens=page_tokens)
    else:
        dst = _cache(layout, B=B, nh_kv=nh_kv, cap=dst_cap, bits=bits)
        src = _cache(layout, B=len(rows), nh_kv=nh_kv, cap=src_cap, bits=bits)
    _fill(dst, 1)
    _fill(src, 2)
    _set_len(dst, kv)
    _set_len(src, kv)
    return dst, src


@pytest.mark.parametrize("kv", [20, 32, 33, 512, 530])
@pytest.mark.parametrize("layout,bits", [("mfma", 2), ("mfma", 4), ("hook", 2)])
def test_admit_slabs_move_the_rows(layout, bits, kv):
    """The destination has grown (more super-blocks / pages, longer V rows), the source is as small as its prompt."""
    for rows in ([1], [2, 0]):
        dst, src = _pair(layout, kv, 2100, kv + 8, rows, bits=bits)
        if layout == "mfma":
            assert dst.n_sb > src.n_sb and dst.kt.stride(2) == src.kt.stride(2) and dst.kt.stride(0) != src.kt.stride(0)
            src.v_res_start = 0                          # a fresh prompt pass; the destination's ring stands where decoding left it
        else:
            assert dst.n_pages > src.n_pages and dst.v_code.stride(1) != src.v_code.stride(1)
            src.v_res_start = 0
            dst.v_res_start = min(kv, R)                 # the window buffer of this layout is linear: 2R + 1 rows
        slabs = _admit_and_check(dst, src, rows)
        assert len(slabs) <= 32


@pytest.mark.parametrize("kv", [20, 64, 530])
def test_admit_slabs_hook_pages_and_window_starts(kv):
    """page_tokens = 64: several K pages move, each side with its own page stride; v_res_start 0 and R on either side."""
    for s_dst, s_src in ((0, 0), (R, 0), (0, R), (R, R)):
        dst, src = _pair("hook", kv, 1000, kv + 8, [2, 0], page_tokens=64)
        assert dst.n_pages > src.n_pages and dst.k_code.stride(0) != src.k_code.stride(0)      # (pages lie outside the heads in memory)
        dst.v_res_start, src.v_res_start = s_dst, s_src
        slabs = _admit_and_check(dst, src, [2, 0])
        full, part = divmod(dst.k_quant_len, 64)
        assert len(slabs) == 3 * (bool(full) + bool(part)) + bool(dst.k_res_len) + 3 * bool(dst.v_quant_len) + 1


@pytest.mark.parametrize("kv", [1, R - 1, 40])
def test_admit_slabs_every_pair_of_ring_phases(kv):
    """Window lengths 1, R - 1 and R: token t goes from source ring row (s_src + t) mod (R + 1) to destination row (s_dst + t)
    mod (R + 1), in at most three segments, and the destination's dead ring row is not written."""
    dst, src = _pair("mfma", kv, 100, 100, [1], B=2, nh_kv=1)
    n = min(kv, R)
    fixed = len([s for s in dst._admit_slabs(src)]) - len(_ring_slabs(dst, src))
    for s_src in range(R + 1):
        for s_dst in range(R + 1):
            _fill(dst, 3 + s_dst)
            dst.v_res_start, src.v_res_start = s_dst, s_src
            before = dst.v_res.clone()
            slabs = _admit_and_check(dst, src, [1])
            ring = _ring_slabs(dst, src)
            assert 1 <= len(ring) <= 3 and len(slabs) == fixed + len(ring)
            assert sum(s[7] for s in ring) == n * 256
            dead = [r for r in range(R + 1) if (r - s_dst) % (R + 1) >= n]
            assert len(dead) == R + 1 - n and _same(dst.v_res[:, :, dead], before[:, :, dead])


def _ring_slabs(dst, src):
    lo, hi = dst.v_res.data_ptr(), dst.v_res.data_ptr() + dst.v_res.numel() * 2
    return [s for s in dst._admit_slabs(src) if lo <= s[0] < hi]


# ------------------------------------------------------------------ 4. refusals before any device work
@pytest.fixture
def launches(monkeypatch):
    """kivi_amd.admit.run replaced by a recorder: (number of slabs, rows, B) per call."""
    from kivi_amd import admit
    calls = []
    monkeypatch.setattr(admit, "run", lambda slabs, rows, B: calls.append((len(slabs), rows.tolist(), B)))
    return calls


@pytest.mark.parametrize("layout", ["hook", "mfma"])
def test_admit_refusals_and_what_stays(layout, launches):
    dst = _cache(layout)
    _set_len(dst, 70)
    nat = dst._native = ("descriptor",)
    dst._attend_unfusable = True

    def source(B=1, kv=70, **kw):
        s = _cache(layout, B=B, **kw)
        _set_len(s, kv)
        return s
    for reason, call, match in (
            ("self", lambda: dst.admit_([0, 1, 2], dst), "itself"),
            ("class", lambda: dst.admit_([0], _other_layout(layout)), "another class or geometry.*KiviLayerCache"),
            ("heads", lambda: dst.admit_([0], source(nh_kv=4)), "another class or geometry"),
            ("bits", lambda: dst.admit_([0], source(bits=4)), "another class or geometry"),
            ("not a cache", lambda: dst.admit_([0], dst.as_tuple()), "another class or geometry"),
            ("kv_seq_len", lambda: dst.admit_([0], source(kv=71)), "kv_seq_len differs.*71.*70"),
            ("k_res_len", lambda: dst.admit_([0], _with(source(), k_res_len=5)), "k_res_len differs.*5.*6"),
            ("k_quant_len", lambda: dst.admit_([0], _with(source(), k_quant_len=32)), "k_quant_len differs.*32.*64"),
            ("v_quant_len", lambda: dst.admit_([0], _with(source(), v_quant_len=37)), "v_quant_len differs.*37.*38"),
            ("v_res_len", lambda: dst.admit_([0], _with(source(), v_res_len=31)), "v_res_len differs.*31.*32"),
            ("row count", lambda: dst.admit_([0, 1], source()), "holds 1 rows, 2 rows"),
            ("too many", lambda: dst.admit_([0, 1, 2, 0], source(B=4), check=False), "4 rows cannot be admitted into a cache of 3"),
            ("duplicate", lambda: dst.admit_([1, 1], source(B=2)), "duplicate"),
            ("range", lambda: dst.admit_(torch.tensor([3]), source()), "out of range"),
            ("negative", lambda: dst.admit_(torch.tensor([-1], dtype=torch.int32), source()), "out of range"),
            ("dtype", lambda: dst.admit_(torch.tensor([1.0]), source()), "int32 or int64"),
            ("shape", lambda: dst.admit_(torch.tensor([[1]]), source()), "1-D"),
            ("shared", lambda: dst.admit_([0], _sharing(dst, source())), "shares a buffer")):
        with pytest.raises(ValueError, match=match):
            call()
    assert launches == []
    # a good one: another capacity and window start are fine; lengths, pointers, descriptor and flags stay, checkpoints go stale
    ck = _checkpoint(dst)
    src = source(B=2, cap=900)
    src.v_res_start = 0
    ptrs = [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    assert dst.admit_(torch.tensor([2, 0], dtype=torch.int32), src) is dst
    assert launches == [(len(dst._admit_slabs(src)), [2, 0], 3)]
    assert dst.kv_seq_len == 70 and dst._native is nat and dst._attend_unfusable
    assert ptrs == [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    with pytest.raises(ValueError, match="stale"):
        dst.restore_(ck)
    dst.admit_([5, 1], src, check=False)                 # check=False: the values are the kernel's business
    assert launches[-1][1] == [5, 1]


def _checkpoint(lc):
    from kivi_amd import checkpoint
    run = checkpoint.run
    checkpoint.run = lambda *a, **k: None
    try:
        return lc.checkpoint()
    finally:
        checkpoint.run = run


def _other_layout(layout):
    o = _cache("mfma" if layout == "hook" else "hook", B=1)
    _set_len(o, 70)
    return o


def _with(lc, **kw):
    for k, v in kw.items():
        setattr(lc, k, v)
    return lc


def _sharing(dst, src):
    src.k_res = dst.k_res[:1]
    return src


def _kivi_model(layers=2):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    cfg = make_config(dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=2, num_hidden_layers=layers,
                           intermediate_size=256, vocab_size=64))
    return LlamaForCausalLM_KIVI(cfg)


def test_model_admit_refusals(launches, monkeypatch):
    model = _kivi_model()
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    caches = [_cache("mfma"), _cache("mfma")]
    for c in caches:
        _set_len(c, 40)
    past = [c.as_tuple() for c in caches]
    ids, mask = torch.zeros((2, 40), dtype=torch.long), torch.ones((2, 40), dtype=torch.long)
    with pytest.raises(ValueError, match="in-place cache"):
        model.admit_([(None,) * 8 + (40,)] * 2, [0, 1], ids, mask)
    with pytest.raises(ValueError, match="L = 40"):
        model.admit_(past, [0, 1], ids[:, :39], mask[:, :39])
    with pytest.raises(ValueError, match="L = 40"):
        model.admit_(past, [0, 1], ids[0], mask)
    with pytest.raises(ValueError, match=r"size \(2, 40\)"):
        model.admit_(past, [0, 1], ids, mask[:1])
    with pytest.raises(ValueError, match=r"size \(2, 40\)"):
        model.admit_(past, [0, 1], ids, None)
    with pytest.raises(ValueError, match="4 prompts for living caches of 3 rows"):
        model.admit_(past, [0, 1, 2, 0], ids.repeat(2, 1), mask.repeat(2, 1))
    for rows, match in (([0, 0], "duplicate"), ([0, 3], "out of range"), ([0], "1 rows were named for 2"), ([0.5, 1.0], "int32 or int64")):
        with pytest.raises(ValueError, match=match):
            model.admit_(past, rows, ids, mask)
    assert launches == []


def test_generate_continuous_refusals(monkeypatch):
    from kivi_amd.sampling import RowSampler, SamplingParams
    model = _kivi_model(1)
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    prompts = [[1, 2, 3], [4, 5], [6]]
    p = SamplingParams(seed=1)
    for kw, match in ((dict(max_new_tokens=[3, 4]), "2 max_new_tokens for 3 requests"), (dict(max_new_tokens=0), "max_new_tokens"),
                      (dict(max_new_tokens=[3, 0, 1]), "max_new_tokens"), (dict(max_new_tokens=2.5), "max_new_tokens"),
                      (dict(batch_size=0), "batch_size"), (dict(batch_size=True), "batch_size"), (dict(batch_size=1.5), "batch_size"),
                      (dict(eos_token_id=2, pad_token_id=None), "pad_token_id"),
                      (dict(sampling=[p, p]), "2 SamplingParams for 3 requests"), (dict(sampling=[p, p, "greedy"]), "SamplingParams"),
                      (dict(sampling=dict(top_k=1)), "SamplingParams"), (dict(sampling=RowSampler([p, p, p], "cpu")), "SamplingParams"),
                      (dict(prompts=[]), "non-empty"), (dict(prompts=[[1], []]), "prompt 1 is empty"),
                      (dict(prompts=[[1], [64]]), "outside the vocabulary"), (dict(prompts=torch.zeros(3, 4)), "non-empty list")):
        args = dict(prompts=prompts, max_new_tokens=4, batch_size=2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            model.generate_continuous(**args)
    with pytest.raises(ValueError, match="temperature"):                  # bad sampling parameters never reach the call
        model.generate_continuous(prompts, 4, 2, sampling=SamplingParams(temperature=0.0))


def test_check_arguments_binds_one_seed_per_request():
    from kivi_amd.sampling import SamplingParams
    from kivi_amd.serving import check_arguments
    torch.manual_seed(3)
    seqs, limits, params = check_arguments([[1, 2], (3,), torch.tensor([4, 5, 6])], 7, 2, None, 0, SamplingParams(), 10)
    assert [s.tolist() for s in seqs] == [[1, 2], [3], [4, 5, 6]] and limits == [7, 7, 7]
    assert all(p.seed is not None for p in params) and len({p.seed for p in params}) == 3
    _, limits, params = check_arguments([[1], [2]], [3, 1], 5, 9, 0, None)
    assert limits == [3, 1] and params is None
    given = [SamplingParams(seed=5), SamplingParams(do_sample=False)]
    assert check_arguments([[1], [2]], 1, 1, None, None, given)[2][0] is given[0]


def test_left_pad_to_a_length():
    from kivi_amd.llama import left_pad
    ids, mask = left_pad([[1, 2, 3], [4]], pad_token_id=9, length=5)
    assert ids.tolist() == [[9, 9, 1, 2, 3], [9, 9, 9, 9, 4]] and mask.tolist() == [[0, 0, 1, 1, 1], [0, 0, 0, 0, 1]]
    same = left_pad([[1, 2, 3], [4]], pad_token_id=9, length=3)
    assert all(torch.equal(a, b) for a, b in zip(same, left_pad([[1, 2, 3], [4]], pad_token_id=9)))
    for bad in (2, 0, -1, 3.0, True):
        with pytest.raises(ValueError, match="length"):
            left_pad([[1, 2, 3], [4]], length=bad)


def test_set_row_draw_index():
    from kivi_amd.sampling import RowSampler, SamplingParams
    rs = RowSampler([SamplingParams(seed=5), SamplingParams(seed=6), SamplingParams(seed=7)], "cpu")
    rs.draw_index += 4
    rs.set_row(1, SamplingParams(seed=8), draw_index=1)
    assert rs.draw_index.tolist() == [4, 1, 4]
    rs.set_row(2, SamplingParams(seed=9), stream=3, draw_index=2 ** 40)
    assert rs.draw_index.tolist() == [4, 1, 2 ** 40] and rs.streams == [0, 0, 3]
    rs.set_row(0, SamplingParams(seed=8))                                # the default: as before
    assert rs.draw_index.tolist() == [0, 1, 2 ** 40]
    for bad in (-1, 1.0, True, 2 ** 63):
        with pytest.raises(ValueError, match="draw_index"):
            rs.set_row(0, SamplingParams(seed=1), draw_index=bad)
    assert rs.draw_index.tolist() == [0, 1, 2 ** 40]
