"""CPU: admission at an offset -- kivi_mf_store_admit, KiviCacheBase.admit_(offset=), LlamaForCausalLM_KIVI.admit_(offset=),
generate_continuous(short_admissions=).

1. The library exports kivi_mf_store_admit with a ctypes signature, the header declares it, the ABI version is still 3.
2. Every refusal of the entry point with fake pointers that are never dereferenced: nothing is enqueued.  The nothing-to-do call
   returns 0.
3. tests/admit_walk_main.cpp: the kernel's grid walked on host buffers under AddressSanitizer and UBSan, as a child process.
4. The hook-state layout's torch path run for real on CPU tensors: the admitted rows sliced at the offset are the source, the lead is
   zero, every other row keeps its bytes.
5. The ValueErrors of admit_, model.admit_ and short_admissions=, raised before anything runs on a device; what a good offset
   admission launches on the matrix-pipe layout.
6. admission_offset against a restatement.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_admit_cpu import _checkpoint, _fill, _kivi_model, _with
from test_checkpoint_cpu import _cache, _set_len
from test_rebase_cpu import _same_member, _sliced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len")


@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ 1. symbol, signature
def test_symbol_and_signature(lib):
    from kivi_amd import _lib
    assert hasattr(lib, "kivi_mf_store_admit")
    res, args = _lib.SIGNATURES["kivi_mf_store_admit"]
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert res is i32 and args == [vp, i64, i64, i64, vp, vp, i64, i64, i64, vp, i32, i32, i32, vp, i32, i32, i32, i64, i64, vp]
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert "#define KIVI_ABI_VERSION 3" in src
    decl = re.search(r"int kivi_mf_store_admit\(([^)]*)\);", src).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["dst", "dst_sb", "dst_sh", "dst_ss", "dst_range", "src", "src_sb", "src_sh", "src_ss", "src_range", "bits", "is_k",
                     "n_rows", "rows", "rows_bytes", "B", "nh_kv", "n_blocks", "shift_blocks", "stream"]
    ctype = {"void*": vp, "const void*": vp, "int64_t": i64, "int": i32, "kivi_stream_t": vp}
    assert [ctype[" ".join(a.split()[:-1])] for a in decl.split(",")] == args
    assert "kivi_admit_shift.hip" in __import__("kivi_amd.build", fromlist=["SOURCES"]).SOURCES


# ------------------------------------------------------------------ 2. refusals of the entry point
W2, W4 = 6144, 10240
# destination: 3 rows of 4 super-blocks, the super-block index outside the head index; source: 2 rows of 2 super-blocks
GOOD = dict(dst=1 << 20, dsb=4 * 2 * W2, dsh=W2, dss=2 * W2, drange=1 << 28, src=1 << 24, ssb=2 * 2 * W2, ssh=W2, sss=2 * W2,
            srange=1 << 29, bits=2, is_k=1, n_rows=2, rows=1 << 30, rows_bytes=8, B=3, nh_kv=2, n_blocks=19, shift=14)
CASES = {
    "bits3": (dict(bits=3), EINVAL), "bits0": (dict(bits=0), EINVAL), "bits8": (dict(bits=8), EINVAL),
    "B0": (dict(B=0), EINVAL), "B_negative": (dict(B=-1), EINVAL), "B_65536": (dict(B=65536), EINVAL),
    "n_rows0": (dict(n_rows=0), EINVAL), "n_rows_negative": (dict(n_rows=-1), EINVAL), "n_rows_above_B": (dict(n_rows=4), EINVAL),
    "rows_bytes2": (dict(rows_bytes=2), EINVAL), "rows_bytes16": (dict(rows_bytes=16), EINVAL), "null_rows": (dict(rows=None), EINVAL),
    "rows_misaligned4": (dict(rows=(1 << 30) + 2, rows_bytes=4), EINVAL), "rows_misaligned8": (dict(rows=(1 << 30) + 4), EINVAL),
    "heads0": (dict(nh_kv=0), EINVAL), "heads_negative": (dict(nh_kv=-2), EINVAL),
    "n_blocks_negative": (dict(n_blocks=-1), EINVAL), "shift_negative": (dict(shift=-1), EINVAL),
    "blocks_2_31": (dict(n_blocks=1 << 30, shift=1 << 30), EINVAL), "n_blocks_2_31": (dict(n_blocks=1 << 31, shift=0), EINVAL),
    "null_dst": (dict(dst=None), EINVAL), "null_dst_range": (dict(drange=None), EINVAL),
    "null_src": (dict(src=None), EINVAL), "null_src_range": (dict(srange=None), EINVAL),
    "dst_row_stride_too_small": (dict(shift=46), EINVAL),                       # 65 blocks: five super-blocks, the rows hold four
    "src_row_stride_too_small": (dict(n_blocks=33, shift=0), EINVAL),           # three super-blocks, the source's rows hold two
    "dst_sb_stride_below_a_super_block": (dict(dss=W2 - 4), EINVAL), "src_sb_stride_below_a_super_block": (dict(sss=W2 - 4), EINVAL),
    "dst_head_stride_below_a_super_block": (dict(dsh=W2 - 4), EINVAL), "src_head_stride_below_a_super_block": (dict(ssh=W2 - 4), EINVAL),
    "dst_heads_overlap_super_blocks": (dict(dsh=W2, dss=W2, dsb=64 * W2), EINVAL),
    "src_heads_overlap_super_blocks": (dict(ssh=W2, sss=W2, ssb=64 * W2), EINVAL),
    "four_bit_super_blocks_in_two_bit_strides": (dict(bits=4), EINVAL),
    "negative_dst_stride": (dict(dss=-2 * W2), EINVAL), "negative_src_stride": (dict(sss=-2 * W2), EINVAL),
    "grid_2_31": (dict(B=65535, n_rows=60000, nh_kv=8, dsb=1 << 39, dsh=1 << 30, dss=W2, ssb=1 << 39, ssh=1 << 30, sss=W2,
                       n_blocks=40, shift=8), EINVAL),                          # 60000 * 8 * 48 * 96 units
    "dst_misaligned": (dict(dst=(1 << 20) + 8), EALIGN), "src_misaligned": (dict(src=(1 << 24) + 4), EALIGN),
    "dst_row_stride_misaligned": (dict(dsb=4 * 2 * W2 + 2), EALIGN), "src_row_stride_misaligned": (dict(ssb=2 * 2 * W2 + 2), EALIGN),
    "dst_head_stride_misaligned": (dict(dsh=W2 + 1, dss=2 * W2 + 4, dsb=64 * W2), EALIGN),
    "src_head_stride_misaligned": (dict(ssh=W2 + 1, sss=2 * W2 + 4, ssb=64 * W2), EALIGN),
    "dst_sb_stride_misaligned": (dict(dss=2 * W2 + 2, dsb=64 * W2), EALIGN), "src_sb_stride_misaligned": (dict(sss=2 * W2 + 2, ssb=64 * W2), EALIGN),
    "dst_range_misaligned": (dict(drange=(1 << 28) + 2), EALIGN), "src_range_misaligned": (dict(srange=(1 << 29) + 1), EALIGN),
}


def _call(lib, **kw):
    a = dict(GOOD)
    a.update(kw)
    return lib.kivi_mf_store_admit(a["dst"], a["dsb"], a["dsh"], a["dss"], a["drange"], a["src"], a["ssb"], a["ssh"], a["sss"], a["srange"],
                                   a["bits"], a["is_k"], a["n_rows"], a["rows"], a["rows_bytes"], a["B"], a["nh_kv"], a["n_blocks"],
                                   a["shift"], None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_store_admit_refuses_bad_arguments(lib, case):
    kw, rc = CASES[case]
    assert _call(lib, **kw) == rc
    assert b"kivi_mf_store_admit" in lib.kivi_last_error()


def test_store_admit_nothing_to_do_enqueues_nothing(lib):
    """No block on either side: 0 without a launch (the pointers are fake: a launch would not return 0 on a machine without a GPU,
    and would fault on one with)."""
    assert _call(lib, n_blocks=0, shift=0) == 0
    assert _call(lib, n_blocks=0, shift=0, dsb=0, dsh=0, dss=0, ssb=0, ssh=0, sss=0, B=1, n_rows=1, nh_kv=1) == 0
    assert _call(lib, n_blocks=0, shift=0, bits=4, is_k=0, rows_bytes=4) == 0


# ------------------------------------------------------------------ 3. the kernel's walk on the host, under sanitizers
def test_admit_walk_matches_a_per_block_copy_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "admit_walk")
    # the sanitizer runtimes are linked into the program (clang's default), so it does not depend on the order libraries load in
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "admit_walk_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "admit walk ok" and run.stderr == "", run.stdout + run.stderr


# ------------------------------------------------------------------ 4. the hook-state layout on CPU tensors
def _hook(B, kv, page_tokens, seed, start):
    from kivi_amd.attention import KiviConfig, KiviLayerCache
    lc = KiviLayerCache(KiviConfig(2, 2, 32, 32), B, 2, 128, kv + 8, "cpu", page_tokens=page_tokens)
    _fill(lc, seed)
    _set_len(lc, kv)
    lc.v_res_start = start                               # (this layout's window is linear: 32 live rows inside 65)
    return lc


def _raw(lc):
    return {n: getattr(lc, n).clone() for n in lc._BUFFERS}


@pytest.mark.parametrize("rows", [[1], [2, 0]])
@pytest.mark.parametrize("L,S,page_tokens", [(110, 46, 64), (530, 82, 64), (1100, 76, 128), (530, 82, None)])
def test_hook_state_offset_admission_on_cpu_tensors(L, S, page_tokens, rows):
    off = L - S
    dst, src = _hook(3, L, page_tokens, 1, 5), _hook(len(rows), S, page_tokens, 2, 11)
    before, src_before = _raw(dst), _raw(src)
    lengths, ptrs = [getattr(dst, n) for n in LENGTHS], [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    want = tuple(None if x is None else x.clone() for x in src.as_tuple()[:8])
    ck = _checkpoint(dst)
    idx = torch.tensor(rows, dtype=torch.int32 if len(rows) == 1 else torch.int64)
    assert dst.admit_(idx, src, offset=off) is dst
    got = dst.as_tuple()
    mine = tuple(None if x is None else x[rows] for x in got[:8]) + (L,)
    for i, (x, y) in enumerate(zip(_sliced(mine, off)[:8], want)):
        assert _same_member(x, y), i
    kc, _, ks, km, vc, _, vs, vm, _ = mine
    assert not kc[..., : off // 16].any() and not ks[..., : off // 32].any() and not km[..., : off // 32].any()
    assert not vc[:, :, :off].any() and not vs[:, :, :off].any() and not vm[:, :, :off].any()
    others = [b for b in range(3) if b not in rows]
    after = _raw(dst)
    for n in dst._BUFFERS:
        assert torch.equal(after[n][others].view(torch.uint8), before[n][others].view(torch.uint8)), n
        assert torch.equal(getattr(src, n).view(torch.uint8), src_before[n].view(torch.uint8)), n      # the source is only read
    assert lengths == [getattr(dst, n) for n in LENGTHS] and ptrs == [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    with pytest.raises(ValueError, match="stale"):
        dst.check_restore(ck)


def test_hook_state_offset_admission_leaves_a_stray_row_unused():
    """check=False and a row index outside [0, B): that source row is not used, on the device and without a host read."""
    dst, src = _hook(3, 110, 64, 1, 5), _hook(3, 46, 64, 2, 0)
    before = _raw(dst)
    want = tuple(None if x is None else x.clone() for x in src.as_tuple()[:8])
    dst.admit_(torch.tensor([7, 2, -1]), src, check=False, offset=64)
    mine = tuple(None if x is None else x[[2]] for x in dst.as_tuple()[:8]) + (110,)
    for i, (x, y) in enumerate(zip(_sliced(mine, 64)[:8], want)):
        assert _same_member(x, None if y is None else y[[1]]), i
    for n in dst._BUFFERS:
        assert torch.equal(getattr(dst, n)[:2].view(torch.uint8), before[n][:2].view(torch.uint8)), n
    twin = _hook(3, 110, 64, 1, 5)
    twin.admit_(torch.tensor([3, 9, -4]), src, check=False, offset=64)          # no good row at all: nothing changes
    for n in twin._BUFFERS:
        assert torch.equal(getattr(twin, n).view(torch.uint8), before[n].view(torch.uint8)), n


# ------------------------------------------------------------------ 5. refusals and bookkeeping
@pytest.fixture
def launches(monkeypatch):
    """kivi_amd.admit.run and admit_store replaced by recorders."""
    from kivi_amd import admit
    calls = []
    monkeypatch.setattr(admit, "run", lambda slabs, rows, B: calls.append(("run", len(slabs), rows.tolist(), B)))
    monkeypatch.setattr(admit, "admit_store", lambda dst, src, rows, bits, is_k, n, s: calls.append(
        ("store", dst.data_ptr(), src.data_ptr(), rows.tolist(), bits, is_k, n, s)))
    return calls


@pytest.mark.parametrize("layout", ["hook", "mfma"])
def test_offset_admission_refusals_and_what_stays(layout, launches, monkeypatch):
    from kivi_amd.attention import KiviLayerCache
    monkeypatch.setattr(KiviLayerCache, "_admit_offset", lambda self, rows, src, offset: launches.append(("hook", rows.tolist(), offset)))
    dst = _cache(layout, cap=700)
    _set_len(dst, 330)                                   # K 320 + 10, V 298 + 32
    state = (ctypes.c_int64 * 6)()
    nat = dst._native = ("descriptor", state)
    dst._attend_unfusable = True

    def source(kv=74, B=1):                              # offset 256: K 64 + 10, V 42 + 32
        s = _cache(layout, B=B, cap=100)
        _set_len(s, kv)
        return s
    for off, match in ((256.0, "offset has to be an int.*256.0"), ("256", "offset has to be an int"), (True, "offset has to be an int"),
                       (False, "offset has to be an int"), (None, "offset has to be an int"), (torch.tensor(256), "offset has to be an int"),
                       (-32, "offset=-32 is negative"), (16, "offset=16 is not a multiple.*32"), (250, "offset=250 is not a multiple.*32"),
                       (320, "offset=320 leaves 10 .* 330 tokens.*residual_length = 32")):
        with pytest.raises(ValueError, match=match):
            dst.admit_([0], source(), offset=off)
    for name, src, match in (
            ("kv_seq_len", source(kv=106), "kv_seq_len does not fit offset=256: the source is at 106, this cache at 330.*at 74"),
            ("k_quant_len", _with(source(), k_quant_len=32), "k_quant_len does not fit offset=256: the source is at 32.*at 320.*at 64"),
            ("v_quant_len", _with(source(), v_quant_len=41), "v_quant_len does not fit offset=256: the source is at 41.*at 298.*at 42"),
            ("k_res_len", _with(source(), k_res_len=9), "k_res_len does not fit offset=256: the source is at 9.*at 10.*at 10"),
            ("v_res_len", _with(source(), v_res_len=31), "v_res_len does not fit offset=256: the source is at 31.*at 32.*at 32")):
        with pytest.raises(ValueError, match=match):
            dst.admit_([0], src, offset=256)
    with pytest.raises(ValueError, match="kv_seq_len differs: the source is at 74, this cache at 330 .a prompt is admitted left-padded"):
        dst.admit_([0], source())                        # offset 0: the old message
    with pytest.raises(ValueError, match="the source holds 2 rows, 1 rows were named"):
        dst.admit_([0], source(B=2), offset=256)
    with pytest.raises(ValueError, match="duplicate"):
        dst.admit_([1, 1], source(B=2), offset=256)
    ck = _checkpoint(dst)
    assert launches == []
    before = [getattr(dst, n) for n in LENGTHS]
    ptrs = [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    src = source(B=2)
    assert dst.admit_([2, 0], src, offset=256) is dst
    if layout == "mfma":        # V: 42 tokens, the last block partial; then the fp16 residual and the ring (phases 1 <- 9: two segments)
        assert launches == [("store", dst.kt.data_ptr(), src.kt.data_ptr(), [2, 0], 2, True, 2, 8),
                            ("store", dst.vt.data_ptr(), src.vt.data_ptr(), [2, 0], 2, False, 2, 8), ("run", 3, [2, 0], 3)]
    else:
        assert launches == [("hook", [2, 0], 256)]
    assert before == [getattr(dst, n) for n in LENGTHS] and ptrs == [getattr(dst, n).data_ptr() for n in dst._BUFFERS]
    assert dst._native is nat and dst._attend_unfusable and dst.cap == 704
    with pytest.raises(ValueError, match="stale"):
        dst.check_restore(ck)


def test_admit_store_checks_before_it_launches():
    from kivi_amd import admit
    from kivi_amd.quant import mfma
    dst, src, rows = mfma.alloc_store(3, 2, 2, "cpu"), mfma.alloc_store(2, 2, 1, "cpu"), torch.tensor([2, 0])
    for n, s in ((17, 0), (16, 17), (4, -1), (-1, 4)):
        with pytest.raises(ValueError, match="admit_store"):
            admit.admit_store(dst, src, rows, 2, True, n, s)
    with pytest.raises(ValueError, match="admit_store"):
        admit.admit_store(dst, src, torch.tensor([2, 0, 1]), 2, True, 4, 4)
    admit.admit_store(dst, src, rows, 2, True, 0, 0)     # nothing to do: no device is needed
    assert admit.store_moved_bytes(dst, 2, 10, 4) == 2 * 2 * 1536 * (2 * 10 + 4)
    assert admit.store_moved_bytes(mfma.alloc_store(1, 1, 1, "cpu", 4), 1, 3, 3) == 2560 * 9


def test_model_offset_admission_refusals(launches, monkeypatch):
    model = _kivi_model()
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    caches = [_cache("mfma", cap=300), _cache("mfma", cap=300)]
    for c in caches:
        _set_len(c, 200)
    past = [c.as_tuple() for c in caches]
    ids, mask = torch.zeros((2, 72), dtype=torch.long), torch.ones((2, 72), dtype=torch.long)
    for off, match in ((128.0, "offset has to be an int"), (True, "offset has to be an int"), (False, "offset has to be an int"),
                       (-32, "negative"), (48, "not a multiple of the rebase quantum 32"), (192, "leaves 8 .*residual_length = 32")):
        with pytest.raises(ValueError, match=match):
            model.admit_(past, [0, 1], ids, mask, offset=off)
    with pytest.raises(ValueError, match=r"input_ids must be \(n, L - offset\) with L = 200 .* offset = 128 .*to 72.*\(2, 71\)"):
        model.admit_(past, [0, 1], ids[:, :71], mask[:, :71], offset=128)
    with pytest.raises(ValueError, match=r"L - offset"):
        model.admit_(past, [0, 1], torch.zeros((2, 200), dtype=torch.long), torch.ones((2, 200), dtype=torch.long), offset=128)
    with pytest.raises(ValueError, match=r"size \(2, 72\)"):
        model.admit_(past, [0, 1], ids, mask[:1], offset=128)
    with pytest.raises(ValueError, match=r"size \(2, 72\)"):
        model.admit_(past, [0, 1], ids, torch.ones((2, 200), dtype=torch.long), offset=128)
    with pytest.raises(ValueError, match="duplicate"):
        model.admit_(past, [1, 1], ids, mask, offset=128)
    with pytest.raises(ValueError, match="L = 200"):      # offset 0: the old message
        model.admit_(past, [0, 1], ids, mask)
    assert launches == []


def test_short_admissions_refusals(monkeypatch):
    from kivi_amd.serving import check_arguments
    model = _kivi_model(1)
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    for bad in (0, 1, None, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="short_admissions has to be a bool"):
            model.generate_continuous([[1, 2, 3], [4, 5]], 4, 2, short_admissions=bad)
    for ok in (False, True):
        check_arguments([[1, 2, 3], [4, 5]], 4, 2, None, 0, None, 64, short_admissions=ok)


# ------------------------------------------------------------------ 6. the offset, restated
def _restated_offset(L, P, R, quantum):
    """the prompt pass needs room for the longest prompt and for one residual; the rest of L, in whole quanta,
    stays under the offset."""
    short = P if P > R else R
    off = 0
    while off + quantum + short <= L:
        off += quantum
    return off


def test_admission_offset_against_a_restatement():
    from kivi_amd.serving import admission_offset
    seen = set()
    for R, quantum in ((32, 32), (64, 64), (96, 96), (128, 128)):
        for L in (R, R + 1, 47, 84, 160, 161, 530, 700, 1100, 4096, 4097):
            for P in (1, 7, R - 1, R, R + 1, 100, L - quantum - 1, L - quantum, L - quantum + 1, L - 1, L):
                if P < 1 or P > L or L < R:
                    continue
                want = _restated_offset(L, P, R, quantum)
                assert admission_offset(L, P, R, quantum) == want, (L, P, R, quantum)
                assert want % quantum == 0 and L - want >= max(P, R) and L - want - quantum < max(P, R)
                seen.add((P < R, P > L - quantum, want == 0, R))
    assert {(True, False, False, 128), (False, True, True, 32), (False, True, True, 128)} <= seen
    assert admission_offset(4096, 100, 32, 32) == 3968 and admission_offset(4096, 20, 128, 128) == 3968
    assert admission_offset(110, 46, 32, 32) == 64 and admission_offset(84, 20, 32, 32) == 32 and admission_offset(84, 60, 32, 32) == 0
