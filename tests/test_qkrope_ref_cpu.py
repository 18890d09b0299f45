"""No GPU: the references and inputs of tests/test_qkrope_gpu.py hold on their own.  The torch path of the head norm (HF's fp32
formula, kivi_amd.qkrope.head_norm / qk_rope_torch) stays inside the two conditions of the kernel tests on the inputs those tests
use, norm alone and norm + RoPE; the fp64 RoPE sequence equals the torch expression bit for bit; the helpers do what they say."""
import torch

import qkrope_ref as R
from kivi_amd.qkrope import head_norm, qk_rope_torch

SEED = 0        # the inputs of tests/test_qkrope_gpu.py


def test_ulp_distance_and_single_rounding():
    a = torch.tensor([1.0, 1.0, -1.0, 0.0, 6.1e-5, 65504.0], dtype=torch.float16)
    b = torch.tensor([1.0, 1.0009765625, -0.99951171875, -0.0, -6.1e-5, 65472.0], dtype=torch.float16)
    assert R.ulp_distance(a, b).tolist() == [0, 1, 1, 0, 2 * int(a[4].view(torch.int16)), 1]
    # 1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10: one rounding goes up, two (through fp32: onto the tie, then to even) down
    x = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)
    assert float(R.h16(x)) == 1.0 + 2.0 ** -10 and float(x.float().half()) == 1.0


def test_rope64_is_the_torch_expression():
    q, k, _, _ = R.norm_inputs(SEED)
    for Bc in (1, 2):
        cos, sin = R.tables(7, Bc, q.shape[1])
        for a, b in zip(R.rope_torch(q, k, cos, sin), R.rope64(q, k, cos, sin)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_place_pads_with_zero_heads():
    q = torch.arange(2 * 6 * 1 * R.D, dtype=torch.float32).view(2, 6, 1, R.D).half() + 1
    p = R.place(q, 3, 4)
    assert p.shape == (2, 8, 1, R.D)
    for kv in range(2):
        assert torch.equal(p[:, 4 * kv: 4 * kv + 3], q[:, 3 * kv: 3 * kv + 3]) and not p[:, 4 * kv + 3].any()


def test_torch_path_stays_inside_the_bars_on_the_test_inputs():
    q, k, qw, kw = R.norm_inputs(SEED)
    assert float(q[:, 1].abs().max()) > 60 and float(q[:, 2].abs().max()) < 6e-3 and float(q[:, 3].abs().max()) == 200.0
    for x, w in ((q, qw), (k, kw)):
        ok, worst, off = R.within_norm_bars(head_norm(x, w, R.EPS), R.norm64(x, w))
        assert ok, (worst, off)
    cos, sin = R.tables(SEED + 50, 2, q.shape[1])
    got = qk_rope_torch(q, k, cos, sin, qw, kw, R.EPS)
    ref = R.rope64(R.norm64(q, qw), R.norm64(k, kw), cos, sin)
    for a, b in zip(got, ref):
        ok, worst, off = R.within_norm_bars(a, b)
        assert ok, (worst, off)
