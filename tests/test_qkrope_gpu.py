"""GPU: kivi_qk_rope alone (kivi_amd/csrc/kivi_qkrope.hip).

1. Without a head norm the kernel IS the torch expression `x * cos + rotate_half(x) * sin` on fp16 tensors, bit for bit, placed into
   the padded head layout: Q in {1, 37}, one table for all rows or one per row, inputs that are views of the projections' outputs
   and views with other strides, (R, Rp) in {(4, 4), (3, 4), (2, 4), (5, 8), (7, 8)}; the outputs start as NaN bit patterns inside
   a guarded buffer: afterwards the pad heads are exact zeros and no byte outside the outputs has changed.
2. The head norm alone (cos = 1, sin = 0) and norm + RoPE against the fp64 evaluation of the rounding sequence (tests/qkrope_ref.py):
   every element within 1 fp16 ulp, at most 1 % not bit-equal -- on the inputs tests/test_qkrope_ref_cpu.py holds the torch path to
   the same two conditions on.
3. D = 64 is KIVI_EINVAL and writes nothing."""
import pytest
import torch

import qkrope_ref as R
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


def _inputs(seed, B, Q, nh, nh_kv, strided):
    """q_in (B, Q, nh, D), k_in (B, Q, nh_kv, D): views of (B, Q, heads * D) `projection outputs`, or -- strided -- slices of wider
    buffers with other batch, token and head strides."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if not strided:
        q = torch.randn((B, Q, nh * R.D), device="cuda", generator=g).half().view(B, Q, nh, R.D)
        k = torch.randn((B, Q, nh_kv * R.D), device="cuda", generator=g).half().view(B, Q, nh_kv, R.D)
        return q, k
    q = torch.randn((B + 1, Q + 2, nh + 1, R.D + 8), device="cuda", generator=g).half()[1:, 1: Q + 1, 1:, : R.D]
    k = torch.randn((B, nh_kv, Q, 2 * R.D), device="cuda", generator=g).half()[..., R.D:].transpose(1, 2)
    assert q.stride(3) == 1 and k.stride(3) == 1 and not q.is_contiguous() and not k.is_contiguous()
    return q, k


@pytest.mark.parametrize("R_,Rp", [(4, 4), (3, 4), (2, 4), (5, 8), (7, 8)])
@pytest.mark.parametrize("Bc", [1, 2])
@pytest.mark.parametrize("Q", [1, 37])
def test_rope_and_placement_bit_identical_to_torch(Q, Bc, R_, Rp):
    from kivi_amd.qkrope import qk_rope
    B, nh_kv = 2, 2
    nh = nh_kv * R_
    cos, sin = (t.cuda() for t in R.tables(3 * Q + Bc, Bc, Q))
    for strided in (False, True):
        q_in, k_in = _inputs(11 + Q + R_, B, Q, nh, nh_kv, strided)
        keep = q_in.clone(), k_in.clone()
        buf, (q_out, k_out), inside = _guarded([(B, nh_kv * Rp, Q, R.D), (B, nh_kv, Q, R.D)])
        rq, rk = qk_rope(q_in, k_in, cos, sin, Rp, q_out=q_out, k_out=k_out)
        assert rq is q_out and rk is k_out
        want_q, want_k = R.rope_torch(q_in, k_in, cos, sin)
        assert same_bits(q_out, R.place(want_q, R_, Rp)), strided
        assert same_bits(k_out, want_k), strided
        pads = q_out.view(B, nh_kv, Rp, Q, R.D)[:, :, R_:]
        assert not bool(pads.view(torch.int16).any())                       # exact +0, every call
        assert bool((buf[~inside] == NAN_BITS).all())                       # nothing outside the outputs was written
        assert same_bits(q_in, keep[0]) and same_bits(k_in, keep[1])
    # without buffers: fresh tensors of the same content
    nq, nk = qk_rope(q_in, k_in, cos, sin, Rp)
    assert same_bits(nq, q_out) and same_bits(nk, k_out) and nq.is_contiguous()
    if R_ == Rp:                                                            # no padding asked for: the default
        assert same_bits(qk_rope(q_in, k_in, cos, sin)[0], q_out)


def _norm_case(with_rope):
    from kivi_amd.qkrope import qk_rope
    q_in, k_in, qw, kw = R.norm_inputs(0)
    B, Q = q_in.shape[:2]
    if with_rope:
        cos, sin = R.tables(50, B, Q)
    else:
        cos, sin = torch.ones((1, Q, R.D), dtype=torch.float16), torch.zeros((1, Q, R.D), dtype=torch.float16)
    got_q, got_k = qk_rope(q_in.cuda(), k_in.cuda(), cos.cuda(), sin.cuda(), 8, qw.cuda(), kw.cuda(), R.EPS)
    ref_q, ref_k = R.rope64(R.norm64(q_in, qw), R.norm64(k_in, kw), cos, sin)
    assert not bool(got_q.view(B, 1, 8, Q, R.D)[:, :, 5:].view(torch.int16).any())
    for name, got, ref in (("q", got_q.view(B, 1, 8, Q, R.D)[:, 0, :5], ref_q), ("k", got_k, ref_k)):
        assert torch.isfinite(got).all()
        ok, worst, off = R.within_norm_bars(got, ref)
        print(f"{name}: worst ulp distance {worst}, share not bit-equal {off:.2e}")
        assert ok, (name, worst, off)


def test_head_norm_alone_against_the_fp64_sequence():
    """cos = 1, sin = 0: the rotation is the identity (x * 1 + rot(x) * 0, every rounding exact)."""
    _norm_case(False)


def test_head_norm_then_rope_against_the_fp64_sequence():
    _norm_case(True)


def test_q_and_k_take_their_own_weights():
    from kivi_amd.qkrope import qk_rope
    q_in, k_in, qw, kw = (t.cuda() for t in R.norm_inputs(0))
    Q = q_in.shape[1]
    cos, sin = torch.ones((1, Q, R.D), dtype=torch.float16, device="cuda"), torch.zeros((1, Q, R.D), dtype=torch.float16, device="cuda")
    a = qk_rope(q_in, k_in, cos, sin, None, qw, kw, R.EPS)
    b = qk_rope(q_in, k_in, cos, sin, None, kw, qw, R.EPS)
    assert not same_bits(a[0], b[0]) and not same_bits(a[1], b[1])
    same = qk_rope(q_in, q_in[:, :, :1], cos, sin, None, qw, qw, R.EPS)       # one head through both sides of the kernel
    assert same_bits(same[0][:, :1], same[1])


def test_other_head_sizes_are_einval_and_write_nothing():
    from kivi_amd import _lib
    from kivi_amd.qkrope import qk_rope
    B, Q, nh, nh_kv, D = 2, 3, 4, 2, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    q_in = torch.randn((B, Q, nh, D), device="cuda", generator=g).half()
    k_in = torch.randn((B, Q, nh_kv, D), device="cuda", generator=g).half()
    cos = torch.ones((1, Q, D), dtype=torch.float16, device="cuda")
    buf, (q_out, k_out), _ = _guarded([(B, nh, Q, D), (B, nh_kv, Q, D)])
    with pytest.raises(_lib.KiviHipError) as e:
        qk_rope(q_in, k_in, cos, torch.zeros_like(cos), None, q_out=q_out, k_out=k_out)
    assert e.value.rc == -1                                                  # KIVI_EINVAL
    torch.cuda.synchronize()
    assert bool((buf == NAN_BITS).all())
