"""CPU: the multi-token extend (kivi_attention_extend, kivi_mf_extend_layer, kivi_vt_pack_at).

* The library exports both entry points and refuses bad arguments with KIVI_EINVAL before anything is enqueued (fake pointers
  that are never dereferenced, as in tests/test_abi_cpu.py), leaving the caller's lengths untouched.
* `extend64`, the fp64 reference of an extend that tests/test_extend_gpu.py and tests/test_extend_stages_gpu.py hold the kernels to,
  is itself pinned here: at Q = 1 it IS torch_ref64.decode_step (bit for bit), its bulk cache update equals Q chained decode steps
  (bit for bit) -- at g = 32 / D = 128 and at the hook-state layout's own shapes -- and its own rows fed back through
  `scores_override` change nothing.
"""
import ctypes
import math

import pytest
import torch

import torch_ref64 as T64
from helpers import make_kv


def _h(x):
    return x.to(torch.float32).to(torch.float16)


def extend64(q, kn, vn, past, k_bits, v_bits, g, R, attention_mask=None, scores_override=None, return_scores=False):
    """The extend contract in fp64 (include/kivi_hip.h, kivi_mf_extend_layer): q (B, nh, Q, D), kn / vn (B, nh_kv, Q, D).
    Row i attends to the cache as it stands (packed K / V, K residual, V window) and chunk tokens 0..i, with the rounding sequence
    of torch_ref64.decode_step.  Returns (out (B, nh, Q, D) fp16, the 9-tuple after the call) and, with `return_scores`, the
    (B, nh, Q, P0 + Q) fp16 rows fed to the softmax (scaled, mask added and clamped; before the causal mask).
    `scores_override`: rows of that shape to feed the softmax instead (stage B of the extend stage checks,
    tests/test_extend_stages_gpu.py); the causal mask is applied to them as to the reference's own, so the keys a row does not
    see may hold anything."""
    B, nh, Q, D = q.shape
    ratio = nh // kn.shape[1]
    kc, k_full, ks, km, vc, v_full, vs, vm, P0 = past
    att_q = T64.scores64(q, kc, ks, km, g, k_bits) if kc is not None else None
    k_all = torch.cat([k_full, kn], 2) if k_full is not None else kn
    att_f = _h(torch.matmul(q.double(), T64._expand_heads(k_all, ratio).transpose(2, 3).double()))
    w = (torch.cat([att_q, att_f], -1) if att_q is not None else att_f) / math.sqrt(D)
    if attention_mask is not None:
        w = w + attention_mask
        w = torch.max(w, torch.tensor(torch.finfo(w.dtype).min, device=w.device, dtype=w.dtype))
    pre = w
    if scores_override is not None:
        assert scores_override.shape == w.shape and scores_override.dtype == torch.float16
        w = scores_override.to(w.device)
    causal = torch.ones((Q, Q), dtype=torch.bool, device=w.device).triu(1)
    w = w.clone()
    w[..., P0:] = w[..., P0:].masked_fill(causal, float("-inf"))
    p = torch.softmax(w, dim=-1, dtype=torch.float32).to(torch.float16)
    v_all = torch.cat([v_full, vn], 2)
    Lv = v_all.shape[2]
    out = _h(torch.matmul(p[..., -Lv:].double(), T64._expand_heads(v_all, ratio).double()))
    if vc is not None:
        out = T64.output64(p[..., :-Lv], vc, vs, vm, g, v_bits) + out
    # the cache: whole R-runs of the K residual + chunk quantised per channel, the values that leave the window per token
    nk = (k_all.shape[2] // R) * R
    if nk:
        c, s, m = T64.quant_pack_lastdim(k_all[:, :, :nk].transpose(2, 3).contiguous(), g, k_bits)
        kc, ks, km = (c, s, m) if kc is None else (torch.cat([kc, c], 3), torch.cat([ks, s], 3), torch.cat([km, m], 3))
    k_full = k_all[:, :, nk:].contiguous() if k_all.shape[2] > nk else None
    nv = max(Lv - R, 0)
    if nv:
        c, s, m = T64.quant_pack_lastdim(v_all[:, :, :nv].contiguous(), g, v_bits)
        vc, vs, vm = (c, s, m) if vc is None else (torch.cat([vc, c], 2), torch.cat([vs, s], 2), torch.cat([vm, m], 2))
    v_full = v_all[:, :, nv:].contiguous()
    new_past = (kc, k_full, ks, km, vc, v_full, vs, vm, P0 + Q)
    return (out, new_past, pre) if return_scores else (out, new_past)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16) if a.dtype == torch.float16 else a,
                                              b.contiguous().view(torch.int16) if b.dtype == torch.float16 else b)


@pytest.mark.parametrize("bits,ratio,T0,R", [(2, 1, 70, 32), (2, 4, 45, 32), (4, 2, 150, 64)])
def test_extend64_q1_is_decode_step(bits, ratio, T0, R):
    B, nh_kv, D, g = 1, 2, 128, 32
    past = T64.prefill_cache(make_kv(1, B, nh_kv, T0, D), make_kv(2, B, nh_kv, T0, D), bits, bits, g, R)
    q, kn, vn = make_kv(3, B, nh_kv * ratio, 1, D), make_kv(4, B, nh_kv, 1, D), make_kv(5, B, nh_kv, 1, D)
    mask = torch.zeros((B, 1, 1, T0 + 1), dtype=torch.float16)
    mask[..., :3] = torch.finfo(torch.float16).min
    for m in (None, mask):
        o1, t1 = extend64(q, kn, vn, past, bits, bits, g, R, m)
        o2, t2, _ = T64.decode_step(q, kn, vn, past, bits, bits, g, R, m)
        assert _same(o1, o2)
        assert all(_same(x, y) for x, y in zip(t1[:8], t2[:8])) and t1[8] == t2[8]


@pytest.mark.parametrize("bits,T0,R,Q", [(2, 70, 32, 5), (2, 40, 32, 37), (4, 100, 64, 150), (2, 31, 32, 1)])
def test_extend64_cache_is_q_decode_steps(bits, T0, R, Q):
    B, nh_kv, D, g = 1, 2, 128, 32
    past = T64.prefill_cache(make_kv(1, B, nh_kv, T0, D), make_kv(2, B, nh_kv, T0, D), bits, bits, g, R)
    q, kn, vn = make_kv(3, B, nh_kv, Q, D), make_kv(4, B, nh_kv, Q, D, "outlier"), make_kv(5, B, nh_kv, Q, D)
    _, bulk = extend64(q, kn, vn, past, bits, bits, g, R)
    chained = past
    for i in range(Q):
        _, chained, _ = T64.decode_step(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], chained, bits, bits, g, R)
    for x, y in zip(bulk[:8], chained[:8]):
        assert _same(x, y)
    assert bulk[8] == chained[8] == T0 + Q


@pytest.mark.parametrize("bits,ratio,T0,R,Q,masked", [(2, 4, 70, 32, 9, False), (4, 1, 100, 64, 40, True), (2, 8, 45, 32, 1, True)])
def test_extend64_scores_override_with_its_own_rows_is_identity(bits, ratio, T0, R, Q, masked):
    """Stage B's reference: fed the rows it consumed itself, extend64 gives the same output and cache bit for bit -- whatever the keys a
    row does not see hold (the causal mask is applied to the override)."""
    B, nh_kv, D, g = 2, 2, 128, 32
    past = T64.prefill_cache(make_kv(1, B, nh_kv, T0, D, "outlier"), make_kv(2, B, nh_kv, T0, D), bits, bits, g, R)
    q, kn, vn = make_kv(3, B, nh_kv * ratio, Q, D), make_kv(4, B, nh_kv, Q, D, "outlier"), make_kv(5, B, nh_kv, Q, D)
    mask = None
    if masked:
        mask = torch.zeros((B, 1, Q, T0 + Q), dtype=torch.float16)
        mask[0, ..., :5] = torch.finfo(torch.float16).min
        mask[1, ..., T0 + Q - 1] = -2.5                              # a chunk key too
    out, past1, pre = extend64(q, kn, vn, past, bits, bits, g, R, mask, return_scores=True)
    assert pre.shape == (B, nh_kv * ratio, Q, T0 + Q) and pre.dtype == torch.float16
    rows = pre.clone()
    rows[..., T0:] = rows[..., T0:].masked_fill(torch.ones((Q, Q), dtype=torch.bool).triu(1), float("nan"))
    out2, past2 = extend64(q, kn, vn, past, bits, bits, g, R, mask, scores_override=rows)
    assert _same(out, out2)
    assert all(_same(x, y) for x, y in zip(past1[:8], past2[:8])) and past1[8] == past2[8]


# the shapes of the hook-state layout (tests/test_extend_stages_gpu.py): groups of 64 / 128, head_dim 64, K and V bits apart, R = 256
OTHER_SHAPES = [(2, 2, 64, 128, 1, 64, 150, 70), (2, 2, 128, 128, 2, 128, 300, 131), (4, 4, 32, 64, 1, 32, 100, 40),
                (2, 4, 32, 128, 1, 32, 70, 33), (4, 4, 64, 64, 8, 64, 200, 67), (2, 4, 32, 128, 4, 256, 300, 259)]


@pytest.mark.parametrize("kb,vb,g,D,ratio,R,T0,Q", OTHER_SHAPES)
def test_extend64_other_shapes(kb, vb, g, D, ratio, R, T0, Q):
    """extend64 off the g = 32 / D = 128 shape: at Q = 1 it is decode_step bit for bit (with and without a mask), and its bulk
    cache update over Q tokens (K and V flushes) equals Q chained decode steps bit for bit."""
    B, nh_kv = 1, 2
    past = T64.prefill_cache(make_kv(1, B, nh_kv, T0, D), make_kv(2, B, nh_kv, T0, D), kb, vb, g, R)
    q, kn, vn = make_kv(3, B, nh_kv * ratio, Q, D), make_kv(4, B, nh_kv, Q, D, "outlier"), make_kv(5, B, nh_kv, Q, D)
    mask = torch.zeros((B, 1, 1, T0 + 1), dtype=torch.float16)
    mask[..., :3] = torch.finfo(torch.float16).min
    for m in (None, mask):
        o1, t1 = extend64(q[:, :, :1], kn[:, :, :1], vn[:, :, :1], past, kb, vb, g, R, m)
        o2, t2, _ = T64.decode_step(q[:, :, :1], kn[:, :, :1], vn[:, :, :1], past, kb, vb, g, R, m)
        assert _same(o1, o2)
        assert all(_same(x, y) for x, y in zip(t1[:8], t2[:8])) and t1[8] == t2[8]
    _, bulk = extend64(q, kn, vn, past, kb, vb, g, R)
    chained = past
    for i in range(Q):
        _, chained, _ = T64.decode_step(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], chained, kb, vb, g, R)
    for x, y in zip(bulk[:8], chained[:8]):
        assert _same(x, y)
    assert bulk[8] == chained[8] == T0 + Q


# ------------------------------------------------------------------ the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    from kivi_amd import _lib, build
    build.build()
    return _lib.load()


def _fake_desc(cap=1024, R=32):
    from kivi_amd import _lib
    fake = 1 << 20                      # never dereferenced: every case below fails validation first
    return _lib.MfLayerDesc(B=2, nh_kv=2, D=128, bits=2, group_size=32, residual_length=R, inv_scale=1.0 / math.sqrt(128), cap=cap,
                            v_window_rows=R + 1, s_pitch=cap + 64, kt=fake, kt_sb=4 * 6144, kt_sh=2 * 6144, kt_ss=6144,
                            vt=fake, vt_sb=4 * 6144, vt_sh=2 * 6144, vt_ss=6144, k_res=fake, kr_sb=2 * R * 128, kr_sh=R * 128,
                            kr_st=128, v_res=fake, vr_sb=2 * (R + 1) * 128, vr_sh=(R + 1) * 128, vr_st=128, scores=fake, s_sb=0,
                            s_sh=0, stats=fake, stats_bytes=0, workspace=fake, workspace_bytes=0, flags=_lib.GQA_WINDOW_RING,
                            kt_range=fake, vt_range=fake)


def _extend(lib, d, st, Q, mask=None, mask_sq=0):
    fake = 1 << 20
    nh = 4
    return lib.kivi_mf_extend_layer(ctypes.byref(d), st, Q, fake, nh * Q * 128, Q * 128, 128, nh, fake, 2 * Q * 128, Q * 128, 128,
                                    fake, 2 * Q * 128, Q * 128, 128, mask, Q * mask_sq, mask_sq, fake, nh * Q * 128, Q * 128, 128, None)


def test_extend_symbols_exported(lib):
    assert hasattr(lib, "kivi_mf_extend_layer") and hasattr(lib, "kivi_vt_pack_at")
    assert lib.kivi_abi_version() == 3


@pytest.mark.parametrize("case", ["q0", "mask_pitch", "capacity", "lengths", "no_ring", "dump_null", "dump_pitch", "dump_head",
                                  "dump_batch"])
def test_extend_layer_refuses_bad_arguments(lib, case):
    d = _fake_desc()
    lengths = [64, 10, 42, 0, 32, 74]     # Tq, k_res_len, Tv, v_win_start, v_res_len, kv_seq_len
    Q, mask, mask_sq = 8, None, 0
    if case == "q0":
        Q = 0
    elif case == "mask_pitch":
        mask, mask_sq = 1 << 20, 74 + 8 - 1
    elif case == "capacity":
        Q = 1024 - 74 + 1
    elif case == "lengths":
        lengths[2] = 41
    elif case == "no_ring":
        d.flags = 0
    elif case.startswith("dump"):                           # KIVI_GQA_DUMP_SCORES: rows of P0 + Q = 82 halves, Q rows per head
        from kivi_amd import _lib
        d.flags |= _lib.GQA_DUMP_SCORES
        d.s_pitch, d.s_sh, d.s_sb = 82, 8 * 82, 4 * 8 * 82
        if case == "dump_null":
            d.scores = None
        elif case == "dump_pitch":
            d.s_pitch, d.s_sh, d.s_sb = 81, 8 * 82, 4 * 8 * 82
        elif case == "dump_head":
            d.s_sh = 8 * 82 - 1
        else:
            d.s_sb = 4 * 8 * 82 - 1
    st = (ctypes.c_int64 * 6)(*lengths)
    assert _extend(lib, d, st, Q, mask, mask_sq) == -1          # KIVI_EINVAL
    assert list(st) == lengths, "a refused call leaves the caller's lengths alone"
    assert b"kivi_mf_extend_layer" in lib.kivi_last_error()
    if case.startswith("dump"):
        assert b"score dump" in lib.kivi_last_error()


def test_vt_pack_at_refuses_bad_arguments(lib):
    fake = 1 << 20
    args = (fake, 128 * 64, 128 * 32, 128, fake, 4 * 6144, 2 * 6144, 6144, fake)
    assert lib.kivi_vt_pack_at(*args, -1, 2, 2, 8, 128, 32, 2, None) == -1          # negative token offset
    assert lib.kivi_vt_pack_at(*args, 5, 2, 2, -3, 128, 32, 2, None) == -1          # negative length
    assert lib.kivi_vt_pack_at(*args, 5, 0, 2, 8, 128, 32, 2, None) == -1           # empty batch
    assert lib.kivi_vt_pack_at(*args, 5, 2, 2, 8, 128, 32, 3, None) == -3           # 3-bit codes: not on the matrix pipe
    assert lib.kivi_vt_pack_at(*args[:8], None, 5, 2, 2, 8, 128, 32, 2, None) == -1  # no range words
    assert lib.kivi_vt_pack_at(*args, 5, 2, 2, 0, 128, 32, 2, None) == 0            # nothing to do
