"""GPU: kivi_qkv_rope_bf16 alone (kivi_amd/csrc/kivi_qkrope.hip).

The kernel against the fp64 evaluation of its contract, rounded once (tests/bf16_ref.py, which tests/test_bf16_cpu.py holds the torch
statement to): every element within half an fp16 ulp of the exact value, which is bit equality with the once-rounded value.
B = 2, Q in {1, 5}, nh_kv = 2, (R, Rp) in {(1, 1), (4, 4), (3, 4), (5, 8), (7, 8)}, head norm on and off, one table for all rows or one
per row at positions up to 1e5, inputs contiguous or three views into one fused (B, Q, (nh + 2 nh_kv) D) buffer.  The outputs start as
NaN bit patterns inside a guarded buffer: afterwards the pad heads are exact zeros and nothing outside the outputs has changed.
v_out equals torch's own cast of v_in.  Saturation at +-65504, NaN kept.  D = 64 is KIVI_EINVAL and writes nothing.
kivi_qk_rope, whose file this kernel shares, still gives fp16 inputs the bits of the torch expression."""
import pytest
import torch

import bf16_ref as R
from helpers import same_bits

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7E01
GUARD = 512


def _guarded(shapes):
    """Contiguous fp16 tensors of `shapes` inside one buffer of NaN bit patterns, `GUARD` elements before, between and after."""
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    buf = torch.full((sum(sizes) + GUARD * (len(sizes) + 1),), NAN_BITS, dtype=torch.int16, device="cuda")
    views, at, inside = [], GUARD, torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    for s, n in zip(shapes, sizes):
        views.append(buf[at: at + n].view(torch.float16).view(s))
        inside[at: at + n] = True
        at += n + GUARD
    return buf, views, inside


def _positions(Bc, Q):
    pos = torch.tensor([[100000, 1, 77, 4095, 0], [3, 99999, 65536, 12345, 31]])
    return pos[:Bc, :Q]


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "headnorm"])
@pytest.mark.parametrize("R_,Rp", [(1, 1), (4, 4), (3, 4), (5, 8), (7, 8)])
@pytest.mark.parametrize("Bc", [1, 2])
@pytest.mark.parametrize("Q", [1, 5])
def test_kernel_equals_the_once_rounded_fp64_value(Q, Bc, R_, Rp, norm):
    from kivi_amd.qkrope import qkv_rope_bf16
    B, nkv = 2, 2
    cos, sin = R.tables(_positions(Bc, Q))
    for fused in (False, True):
        q, k, v, qw, kw = R.inputs(100 + 10 * R_ + Q, B, Q, nkv, R_, fused=fused)
        assert q.is_contiguous() != fused and q.stride(3) == 1
        w = (qw, kw, R.EPS) if norm else (None, None, 0.0)
        want = R.exact(q, k, v, cos, sin, *w, ratio_padded=Rp)
        dev = R.on_gpu(q, k, v)                                     # the views keep their strides, in one buffer, on the device
        assert not fused or dev[1].data_ptr() - dev[0].data_ptr() == 2 * nkv * R_ * R.D
        assert all(d.stride() == t.stride() and same_bits(d, t) for d, t in zip(dev, (q, k, v)))
        keep = [t.clone() for t in dev]
        wd = tuple(t.cuda() if torch.is_tensor(t) else t for t in w)
        buf, outs, inside = _guarded([(B, nkv * Rp, Q, R.D), (B, nkv, Q, R.D), (B, nkv, Q, R.D)])
        got = qkv_rope_bf16(*dev, cos.cuda(), sin.cuda(), Rp, *wd, q_out=outs[0], k_out=outs[1], v_out=outs[2])
        assert all(g is o for g, o in zip(got, outs))
        for name, g, x in zip("qkv", got, want):
            assert same_bits(g.cpu(), x), (name, fused, int((g.cpu().view(torch.int16) != x.view(torch.int16)).sum()))
        pads = outs[0].view(B, nkv, Rp, Q, R.D)[:, :, R_:]
        assert not bool(pads.view(torch.int16).any())               # exact +0, every call
        assert bool((buf[~inside] == NAN_BITS).all())               # nothing outside the outputs was written
        assert same_bits(outs[2], dev[2].transpose(1, 2).to(torch.float16))
        assert all(same_bits(a, b) for a, b in zip(dev, keep))
    fresh = qkv_rope_bf16(*dev, cos.cuda(), sin.cuda(), Rp, *wd)    # without buffers: new tensors of the same content
    assert all(same_bits(a, b) and a.is_contiguous() for a, b in zip(fresh, outs))
    if R_ == Rp:                                                    # no padding asked for: the default
        assert same_bits(qkv_rope_bf16(*dev, cos.cuda(), sin.cuda(), None, *wd)[0], outs[0])


def test_saturation_and_nan():
    from kivi_amd.qkrope import qkv_rope_bf16
    q, k, v, qw, kw = R.inputs(5, 1, 2, 1, 1)
    q[0, 0, 0, :4] = torch.tensor([1e6, -1e6, float("nan"), 7e4]).bfloat16()
    q[0, 0, 0, 64:68] = 0.0
    k[0, 1, 0, :2] = torch.tensor([-1e6, float("nan")]).bfloat16()
    k[0, 1, 0, 64:66] = 0.0
    v[0, 0, 0, :4] = torch.tensor([1e6, -1e6, float("nan"), 65504.0]).bfloat16()
    cos, sin = torch.ones(1, 2, R.D), torch.zeros(1, 2, R.D)
    want = R.exact(q, k, v, cos, sin)
    gq, gk, gv = (t.cpu() for t in qkv_rope_bf16(q.cuda(), k.cuda(), v.cuda(), cos.cuda(), sin.cuda()))
    assert gq[0, 0, 0, :2].tolist() == [65504.0, -65504.0] and gq[0, 0, 0, 2].isnan() and gq[0, 0, 0, 3].item() == 65504.0
    assert gk[0, 0, 1, 0].item() == -65504.0 and gk[0, 0, 1, 1].isnan()
    assert gv[0, 0, 0, :2].tolist() == [65504.0, -65504.0] and gv[0, 0, 0, 2].isnan() and gv[0, 0, 0, 3].item() == 65504.0
    for g, x in zip((gq, gk, gv), want):                            # everywhere else, and the NaNs as NaNs
        assert torch.equal(g.isnan(), x.isnan()) and torch.equal(g.nan_to_num(0.0), x.nan_to_num(0.0))
    # through the rotation: 1e6 * cos + 1e6 * sin at a real position saturates too, the sign the exact value's
    q2, k2, v2, _, _ = R.inputs(6, 1, 1, 1, 1)
    q2[0, 0, 0, :] = torch.tensor(1e6).bfloat16()
    cos, sin = R.tables(torch.tensor([[12345]]))
    want = R.exact(q2, k2, v2, cos, sin)[0]
    got = qkv_rope_bf16(q2.cuda(), k2.cuda(), v2.cuda(), cos.cuda(), sin.cuda())[0].cpu()
    assert same_bits(got, want) and torch.isfinite(got).all() and (got.abs() == 65504.0).sum() > 64


def test_q_and_k_take_their_own_weights():
    from kivi_amd.qkrope import qkv_rope_bf16
    q, k, v, qw, kw = (t.cuda() for t in R.inputs(7, 2, 3, 1, 2))
    cos, sin = (t.cuda() for t in R.tables(torch.tensor([[5, 6, 7]])))
    a = qkv_rope_bf16(q, k, v, cos, sin, None, qw, kw, R.EPS)
    b = qkv_rope_bf16(q, k, v, cos, sin, None, kw, qw, R.EPS)
    assert not same_bits(a[0], b[0]) and not same_bits(a[1], b[1]) and same_bits(a[2], b[2])
    same = qkv_rope_bf16(q, q[:, :, :1], v, cos, sin, None, qw, qw, R.EPS)   # one head through both sides of the kernel
    assert same_bits(same[0][:, :1], same[1])


def test_other_head_sizes_are_einval_and_write_nothing():
    from kivi_amd import _lib
    from kivi_amd.qkrope import boundary_usable, qkv_rope_bf16
    q, k, v, _, _ = (t.cuda() for t in R.inputs(8, 2, 3, 2, 2, head_dim=64))
    cos, sin = (t.cuda() for t in R.tables(torch.arange(3)[None], 64))
    assert not boundary_usable(q, 64) and boundary_usable(q, 128) and not boundary_usable(q.half(), 128)
    buf, outs, _ = _guarded([(2, 4, 3, 64), (2, 2, 3, 64), (2, 2, 3, 64)])
    with pytest.raises(_lib.KiviHipError) as e:
        qkv_rope_bf16(q, k, v, cos, sin, None, q_out=outs[0], k_out=outs[1], v_out=outs[2])
    assert e.value.rc == -1                                                  # KIVI_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == NAN_BITS).all())


def test_torch_restatement_on_the_gpu_equals_the_kernel():
    """head_dim != 128 runs the torch statement on the device: the same fp64 operations there, so the same bits as the kernel."""
    from kivi_amd.qkrope import qkv_rope_bf16, qkv_rope_bf16_torch
    q, k, v, qw, kw = (t.cuda() for t in R.inputs(9, 2, 5, 2, 3))
    cos, sin = (t.cuda() for t in R.tables(_positions(2, 5)))
    for w in ((None, None, 0.0), (qw, kw, R.EPS)):
        a = qkv_rope_bf16(q, k, v, cos, sin, None, *w)
        b = qkv_rope_bf16_torch(q, k, v, cos, sin, *w)
        assert all(same_bits(x, y) for x, y in zip(a, b))


def test_the_fp16_sibling_gives_the_bits_it_gave():
    """kivi_qk_rope shares the file: one case of tests/test_qkrope_gpu.py, the torch expression on fp16 tensors bit for bit."""
    import qkrope_ref as F
    from kivi_amd.qkrope import qk_rope
    B, Q, nkv, R_, Rp = 2, 37, 2, 5, 8
    g = torch.Generator(device="cuda").manual_seed(11 + Q + R_)
    q_in = torch.randn((B, Q, nkv * R_ * F.D), device="cuda", generator=g).half().view(B, Q, nkv * R_, F.D)
    k_in = torch.randn((B, Q, nkv * F.D), device="cuda", generator=g).half().view(B, Q, nkv, F.D)
    cos, sin = (t.cuda() for t in F.tables(3 * Q + 2, 2, Q))
    q_out, k_out = qk_rope(q_in, k_in, cos, sin, Rp)
    want_q, want_k = F.rope_torch(q_in, k_in, cos, sin)
    assert same_bits(q_out, F.place(want_q, R_, Rp)) and same_bits(k_out, want_k)
