"""CPU: rebase of a living cache -- kivi_mf_store_shift, KiviCacheBase.rebase_, LlamaForCausalLM_KIVI.rebase_,
generate_continuous(compact=).

1. The library exports kivi_mf_store_shift with a ctypes signature, the header declares it, the ABI version is still 3.
2. Every refusal of the entry point with fake pointers that are never dereferenced: nothing is enqueued.  A zero shift and an empty
   store return 0.
3. The ValueErrors of rebase_, model.rebase_ and compact=, raised before anything runs on a device; what a good rebase_ launches and
   what it leaves alone (matrix-pipe layout, the launch recorded); the hook-state layout's torch path run for real on CPU tensors
   against its own earlier 9-tuple with every token axis sliced.
4. The scheduler's drop computation against a restatement, on hand-made cases.
5. tests/shift_walk_main.cpp: the kernel's grid walked on host buffers under AddressSanitizer and UBSan, as a child process.
"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_admit_cpu import _checkpoint, _fill, _kivi_model
from test_checkpoint_cpu import _cache, _set_len

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
    assert hasattr(lib, "kivi_mf_store_shift")
    res, args = _lib.SIGNATURES["kivi_mf_store_shift"]
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert res is i32 and args == [vp, i64, i64, i64, vp, i32, i32, i32, i32, i64, i64, vp]
    assert lib.kivi_abi_version() == _lib.ABI_VERSION == 3
    src = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert "#define KIVI_ABI_VERSION 3" in src
    decl = re.search(r"int kivi_mf_store_shift\(([^)]*)\);", src).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["store", "st_sb", "st_sh", "st_ss", "range", "bits", "is_k", "B", "nh_kv",
                                                                   "n_blocks", "shift_blocks", "stream"]
    assert "kivi_shift.hip" in __import__("kivi_amd.build", fromlist=["SOURCES"]).SOURCES


# ------------------------------------------------------------------ 2. refusals of the entry point
W2, W4 = 6144, 10240
GOOD = dict(store=1 << 20, sb=4 * 2 * W2, sh=W2, ss=2 * W2, range=1 << 28, bits=2, is_k=1, B=3, nh_kv=2, n_blocks=40, shift=8)
CASES = {
    "bits3": (dict(bits=3), EINVAL), "bits0": (dict(bits=0), EINVAL), "bits8": (dict(bits=8), EINVAL),
    "B0": (dict(B=0), EINVAL), "B_negative": (dict(B=-1), EINVAL), "B_65536": (dict(B=65536), EINVAL),
    "heads0": (dict(nh_kv=0), EINVAL), "heads_negative": (dict(nh_kv=-2), EINVAL),
    "n_blocks_negative": (dict(n_blocks=-1, shift=0), EINVAL),
    "shift_negative": (dict(shift=-1), EINVAL), "shift_above_n_blocks": (dict(shift=41), EINVAL),
    "null_store": (dict(store=None), EINVAL), "null_range": (dict(range=None), EINVAL),
    "row_stride_too_small": (dict(n_blocks=65), EINVAL),                       # five super-blocks, the rows hold four
    "sb_stride_below_a_super_block": (dict(ss=W2 - 4), EINVAL),
    "head_stride_below_a_super_block": (dict(sh=W2 - 4), EINVAL),
    "heads_overlap_super_blocks": (dict(sh=W2, ss=W2, sb=64 * W2), EINVAL),
    "four_bit_super_blocks_in_two_bit_strides": (dict(bits=4), EINVAL),
    "negative_stride": (dict(ss=-2 * W2), EINVAL),
    "store_misaligned": (dict(store=(1 << 20) + 8), EALIGN), "store_misaligned4": (dict(store=(1 << 20) + 4), EALIGN),
    "row_stride_misaligned": (dict(sb=4 * 2 * W2 + 2), EALIGN), "head_stride_misaligned": (dict(sh=W2 + 1, ss=2 * W2 + 4, sb=64 * W2), EALIGN),
    "sb_stride_misaligned": (dict(ss=2 * W2 + 2, sb=64 * W2), EALIGN), "range_misaligned": (dict(range=(1 << 28) + 2), EALIGN),
}


def _call(lib, **kw):
    a = dict(GOOD)
    a.update(kw)
    return lib.kivi_mf_store_shift(a["store"], a["sb"], a["sh"], a["ss"], a["range"], a["bits"], a["is_k"], a["B"], a["nh_kv"],
                                   a["n_blocks"], a["shift"], None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_store_shift_refuses_bad_arguments(lib, case):
    kw, rc = CASES[case]
    assert _call(lib, **kw) == rc
    assert b"kivi_mf_store_shift" in lib.kivi_last_error()


def test_store_shift_nothing_to_do_enqueues_nothing(lib):
    assert _call(lib, shift=0) == 0
    assert _call(lib, n_blocks=0, shift=0) == 0
    assert _call(lib, n_blocks=0, shift=0, sb=0, sh=0, ss=0, B=1, nh_kv=1) == 0       # an empty store needs no room
    assert _call(lib, bits=4, sb=4 * 2 * W4, sh=W4, ss=2 * W4, is_k=0, shift=0) == 0
    assert _call(lib, shift=0, n_blocks=64) == 0                                       # exactly the four super-blocks of a row
    assert _call(lib, shift=0, B=1, sb=0, n_blocks=64) == 0                            # one row: its stride is not looked at
    assert _call(lib, shift=0, sh=4 * W2, ss=W2, sb=8 * W2) == 0                       # the head index outside the super-block index


# ------------------------------------------------------------------ 3. refusals and bookkeeping of rebase_
@pytest.fixture
def launches(monkeypatch):
    """kivi_amd.rebase.shift_store replaced by a recorder: (store data pointer, bits, is_k, n_blocks, shift_blocks) per call."""
    from kivi_amd import rebase
    calls = []
    monkeypatch.setattr(rebase, "shift_store", lambda st, bits, is_k, n, s: calls.append((st.data_ptr(), bits, is_k, n, s)))
    return calls


def test_quantum():
    from kivi_amd import rebase
    assert [rebase.quantum(r) for r in (32, 64, 96, 128, 16, 48)] == [32, 64, 96, 128, 32, 96]
    for layout, R in (("mfma", 32), ("mfma", 64), ("mfma", 128), ("hook", 32), ("hook", 128)):
        assert _cache(layout, R=R).rebase_quantum == R


@pytest.mark.parametrize("layout", ["hook", "mfma"])
def test_rebase_refusals_and_what_stays(layout, launches):
    lc = _cache(layout, cap=700)
    _set_len(lc, 330)                                    # K 320 + 10, V 298 + 32
    assert lc.rebase_limit == 298 and lc.rebase_quantum == 32
    before = [getattr(lc, n) for n in LENGTHS]
    for drop, match in ((32.0, "has to be an int.*32.0"), ("32", "has to be an int"), (True, "has to be an int"), (None, "has to be an int"),
                        (torch.tensor(32), "has to be an int"), (-32, "drop=-32 is negative"), (16, "drop=16 is not a multiple.*32"),
                        (33, "drop=33 is not a multiple.*32"), (320, "drop=320 lies above rebase_limit = 298")):
        with pytest.raises(ValueError, match=match):
            lc.rebase_(drop)
    ck = _checkpoint(lc)
    assert lc.rebase_(0) is lc                           # nothing to do: nothing launched, nothing voided
    lc.check_restore(ck)
    assert launches == [] and before == [getattr(lc, n) for n in LENGTHS]
    if layout == "hook":
        return                                           # its torch path runs for real below
    state = (ctypes.c_int64 * 6)()
    nat = lc._native = ("descriptor", state)
    lc._attend_unfusable = True
    ptrs = [getattr(lc, n).data_ptr() for n in lc._BUFFERS]
    assert lc.rebase_(256) is lc
    assert launches == [(lc.kt.data_ptr(), 2, True, 10, 8), (lc.vt.data_ptr(), 2, False, 10, 8)]     # V: 298 tokens, the last block partial
    assert [getattr(lc, n) for n in LENGTHS] == [64, 10, 42, before[3], 32, 74] == list(state)
    assert ptrs == [getattr(lc, n).data_ptr() for n in lc._BUFFERS] and lc._native is nat and lc._attend_unfusable and lc.cap == 704
    with pytest.raises(ValueError, match="stale"):
        lc.check_restore(ck)
    assert lc.rebase_limit == 42
    with pytest.raises(ValueError, match="drop=64 lies above rebase_limit = 42"):
        lc.rebase_(64)
    lc.rebase_(32)
    assert launches[2:] == [(lc.kt.data_ptr(), 2, True, 2, 1), (lc.vt.data_ptr(), 2, False, 2, 1)] and lc.kv_seq_len == 42


def test_rebase_quantum_of_longer_residuals(launches):
    lc = _cache("mfma", R=64, cap=700)
    _set_len(lc, 400)
    with pytest.raises(ValueError, match="not a multiple of the rebase quantum 64"):
        lc.rebase_(32)
    lc.rebase_(192)
    assert launches == [(lc.kt.data_ptr(), 2, True, 12, 6), (lc.vt.data_ptr(), 2, False, 11, 6)]
    assert (lc.k_quant_len, lc.v_quant_len, lc.kv_seq_len) == (192, 144, 208)


def test_shift_store_checks_before_it_launches():
    from kivi_amd import rebase
    from kivi_amd.quant import mfma
    st = mfma.alloc_store(2, 2, 2, "cpu")
    for n, s in ((33, 1), (4, 5), (4, -1)):
        with pytest.raises(ValueError, match="shift_store"):
            rebase.shift_store(st, 2, True, n, s)
    rebase.shift_store(st, 2, True, 4, 0)                # nothing to do: no device is needed
    rebase.shift_store(st, 2, True, 0, 0)
    assert rebase.moved_bytes(st, 2, 10, 4) == 2 * 2 * 1536 * (2 * 6 + 4)
    assert rebase.moved_bytes(mfma.alloc_store(1, 1, 1, "cpu", 4), 4, 3, 3) == 2560 * 3


def _sliced(t, drop, kf=16, g=32):
    """A 9-tuple with every token axis cut by `drop` tokens from the front."""
    kc, kfull, ks, km, vc, vfull, vs, vm, n = t
    if kc is not None and kc.shape[-1] * kf == drop:
        kc = ks = km = None
    elif kc is not None:
        kc, ks, km = kc[..., drop // kf:], ks[..., drop // g:], km[..., drop // g:]
    if vc is not None and vc.shape[2] == drop:
        vc = vs = vm = None
    elif vc is not None:
        vc, vs, vm = vc[:, :, drop:], vs[:, :, drop:], vm[:, :, drop:]
    return (kc, kfull, ks, km, vc, vfull, vs, vm, n - drop)


def _same_member(x, y):
    if x is None or y is None:
        return x is None and y is None
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


@pytest.mark.parametrize("kv,drop,page_tokens", [(64, 32, None), (110, 32, None), (330, 256, 64), (330, 288, 64), (650, 512, 128),
                                                 (2100, 32, None), (2100, 2048, None), (4200, 2080, None)])
def test_hook_state_rebase_equals_its_sliced_tuple(kv, drop, page_tokens):
    """The untuned torch path on CPU tensors: several pages (page_tokens = 64 / 128 and the default 2048), a drop of whole pages, a
    drop that leaves no packed V, one block."""
    from kivi_amd.attention import KiviConfig, KiviLayerCache
    lc = KiviLayerCache(KiviConfig(2, 2, 32, 32), 3, 2, 128, kv + 8, "cpu", page_tokens=page_tokens)
    _fill(lc, kv)
    _set_len(lc, kv)
    lc.v_res_start = 5                                   # (this layout's window is linear: 32 live rows inside 65)
    want = _sliced(tuple(None if x is None else x.clone() for x in lc.as_tuple()[:8]) + (kv,), drop)
    ptrs = [getattr(lc, n).data_ptr() for n in lc._BUFFERS]
    start = lc.v_res_start
    ck = _checkpoint(lc)
    assert lc.rebase_(drop) is lc
    got = lc.as_tuple()
    assert got[8] == kv - drop == lc.kv_seq_len
    for i, (x, y) in enumerate(zip(got[:8], want[:8])):
        assert _same_member(x, y), i
    assert ptrs == [getattr(lc, n).data_ptr() for n in lc._BUFFERS] and lc.v_res_start == start
    assert (lc.k_quant_len, lc.k_res_len, lc.v_quant_len, lc.v_res_len) == (kv // 32 * 32 - drop, kv % 32, kv - 32 - drop, 32)
    with pytest.raises(ValueError, match="stale"):
        lc.check_restore(ck)


def test_model_rebase_refusals(launches):
    model = _kivi_model()
    caches = [_cache("mfma", cap=300), _cache("mfma", cap=300)]
    for c in caches:
        _set_len(c, 200)
    past = [c.as_tuple() for c in caches]
    assert model.rebase_quantum(past) == 32 and model.rebase_limit(past) == 168
    for fn in (model.rebase_quantum, model.rebase_limit, lambda p: model.rebase_(p, 32)):
        with pytest.raises(ValueError, match="in-place cache"):
            fn([(None,) * 8 + (200,)] * 2)
    for drop, match in ((1.0, "has to be an int"), (-32, "negative"), (48, "not a multiple"), (192, "above rebase_limit = 168")):
        with pytest.raises(ValueError, match=match):
            model.rebase_(past, drop)
    caches[1].v_quant_len = 100                          # the LAST layer refuses: the first one must not have been touched
    assert model.rebase_limit(past) == 100
    with pytest.raises(ValueError, match="above rebase_limit = 100"):
        model.rebase_(past, 128)
    assert launches == [] and caches[0].kv_seq_len == 200
    caches[1].v_quant_len = 168
    fresh = model.rebase_(past, 64)
    assert [p.layer for p in fresh] == caches and [p[-1] for p in fresh] == [136, 136] and len(launches) == 4
    with pytest.raises(RuntimeError, match="stale KIVI cache tuple"):
        past[0][0]


def test_compact_refusals(monkeypatch):
    from kivi_amd.serving import check_arguments
    model = _kivi_model(1)
    monkeypatch.setattr(model, "_forward", lambda *a, **k: pytest.fail("forward ran before the refusal"))
    for bad in (0, -32, 32.0, True, "32", [32]):
        with pytest.raises(ValueError, match="compact has to be None or a positive integer"):
            model.generate_continuous([[1, 2, 3], [4, 5]], 4, 2, compact=bad)
    for ok in (None, 1, 32, 1000):
        check_arguments([[1, 2, 3], [4, 5]], 4, 2, None, 0, None, 64, compact=ok)


# ------------------------------------------------------------------ 4. the policy, restated
def _restated_drop(lead, live, L, waiting_lengths, limit, quantum):
    """DESIGN.md section 17, "The scheduler": lead[b] leading pads of row b, live[b] whether it serves a request."""
    leads = [n for n, a in zip(lead, live) if a]
    room = min(leads) if leads else L
    room = min(room, L - (max(waiting_lengths) if waiting_lengths else 0), limit)
    return room // quantum * quantum


@pytest.mark.parametrize("lead,live,L,waiting,limit,quantum,want", [
    ([100, 70, 90], [True, True, True], 200, [], 168, 32, 64),                  # the least lead of the live rows
    ([100, 10, 90], [True, False, True], 200, [], 168, 32, 64),                 # a dead row does not count
    ([150, 140, 160], [True, True, True], 200, [120], 168, 32, 64),             # a waiting prompt longer than L - lead
    ([150, 140, 160], [True, True, True], 200, [30, 199], 168, 32, 0),
    ([150, 140, 160], [True, True, True], 200, [30, 40], 168, 32, 128),
    ([5, 5, 5], [False, False, False], 200, [90], 168, 32, 96),                 # no live row: the whole length counts
    ([5, 5, 5], [False, False, False], 200, [], 168, 32, 160),                  # ... up to the limit
    ([31, 40, 50], [True, True, True], 200, [], 168, 32, 0),                    # just below one quantum
    ([32, 40, 50], [True, True, True], 200, [], 168, 32, 32),                   # exactly one
    ([63, 200, 200], [True, True, True], 300, [], 268, 64, 0),
    ([64, 200, 200], [True, True, True], 300, [], 268, 64, 64),
    ([100, 100, 100], [True, True, True], 120, [], 88, 32, 64),                 # the limit binds
    ([100, 100, 100], [True, True, True], 40, [], 8, 32, 0),
])
def test_compact_drop_against_a_restatement(lead, live, L, waiting, limit, quantum, want):
    from kivi_amd.serving import compact_drop
    assert _restated_drop(lead, live, L, waiting, limit, quantum) == want
    assert compact_drop([n for n, a in zip(lead, live) if a], L, max(waiting, default=0), limit, quantum) == want


# ------------------------------------------------------------------ 5. the kernel's walk on the host, under sanitizers
def test_shift_walk_matches_an_out_of_place_shift_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "shift_walk")
    # the sanitizer runtimes are linked into the program (clang's default), so it does not depend on the order libraries load in
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static, "-o", exe, os.path.join(ROOT, "tests", "shift_walk_main.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "shift walk ok" and run.stderr == "", run.stdout + run.stderr
