"""GPU: kivi_w4_pack / kivi_w4_dequant / kivi_w4_linear / kivi_w4_gate_up and the modules over them.

Pack     (O, K) in {(16, 128), (48, 384), (32, 896)}, G in {64, 128}, fp16 and bf16 input; normal weights, one outlier per group, a
         constant group, a group whose range is one fp16-subnormal ulp: codes / scale / mn bit-identical to the oracle's last-dim
         quantiser on the fp16 image, through wquant.to_ref.
Dequant  bit-identical to round_to_dtype(fma(code, scale, mn)) evaluated in torch from the triple.
Linear   K in {128, 384, 896, 1152} (1 tile; fewer tiles than waves; 7 and 9 tiles dealt unevenly over the 8 waves), O in {16, 48},
         N in {1, 5, 16, 17, 64, 65, 130}, bias on and off, both dtypes and groups, x a strided slice.  The bar is the one of the
         sparse block's tests: the worst |y - y64| / rms(y64) of the kernel must not exceed 2 x the same figure of
         F.linear(x, w^) in the model dtype on the same inputs, y64 the fp64 product with the represented weight (tests/w4_ref.py);
         both accumulate in fp32 and round once, only the order of summation differs, which the factor covers.  Both are printed.
Gate/up  (I, K) in {(128, 384), (384, 896)} against fp64 silu(g) * u, the same bar with the torch statement as the yardstick.
Bits     a token alone has the bits it has in a batch of 7, of 64 and of 65; permuting the tokens permutes the bits; two calls
         agree; torch.cuda.graph captures of QuantLinear.forward and QuantMLP.forward replayed on new inputs equal the eager calls;
         above kernel_max_tokens the module equals F.linear(x, module.dequant()) bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

import w4_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NS = [1, 5, 16, 17, 64, 65, 130]


def _wq():
    from kivi_amd import wquant
    return wquant


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------------- pack / dequant
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G", [64, 128])
@pytest.mark.parametrize("O,K", [(16, 128), (48, 384), (32, 896)])
@pytest.mark.parametrize("kind", ["normal", "outlier", "constant", "ulp"])
def test_pack_is_the_oracles_quantiser_bit_for_bit(kind, O, K, G, dtype):
    wq = _wq()
    w = R.weights(kind, O, K, G, dtype, O + K + G)
    code, scale, mn = R.oracle_triple(w, G)
    q, s, m = wq.pack(w.cuda(), G)
    assert (tuple(q.shape), tuple(s.shape), tuple(m.shape)) == wq.shapes(O, K, G)
    c2, s2, m2 = (t.cpu() for t in wq.to_ref(q, s, m))
    assert torch.equal(s2.view(torch.int16), scale.view(torch.int16)) and torch.equal(m2.view(torch.int16), mn.view(torch.int16))
    assert torch.equal(c2, code)
    if kind == "constant":
        assert int(R.codes_of(code)[1, :G].max()) == 0 and float(scale[1, 0]) == 0.0
    if kind == "ulp":
        assert float(scale[:, 0].abs().max()) == 0.0 and set(R.codes_of(code)[:, :G].reshape(-1).tolist()) == {0, 15}
    # a strided view of a wider tensor is read as it is
    wide = torch.zeros((O, K + 16), dtype=dtype, device="cuda")
    wide[:, 8:8 + K] = w.cuda()
    for a, b in zip(wq.pack(wide[:, 8:8 + K], G), (q, s, m)):
        assert torch.equal(a, b)
    # dequant: the formula from the triple, in both dtypes
    want = R.represented(code, scale, mn, G)
    for out_dtype in DTYPES:
        got = wq.dequant(q, s, m, out_dtype)
        assert got.dtype == out_dtype and _same(got.cpu(), want.float().to(out_dtype))
        assert _same(wq.dequant_torch(q, s, m, out_dtype), got)


def test_pack_refuses_an_infinite_fp16_image_by_name():
    wq = _wq()
    w = torch.randn((16, 128), generator=torch.Generator().manual_seed(1)).bfloat16()
    w[3, 7] = 70000.0                                               # finite in bf16, infinite in fp16
    with pytest.raises(ValueError, match="layers.3.q_proj"):
        wq.pack(w.cuda(), 64, "layers.3.q_proj.weight")
    h = torch.randn((16, 128), generator=torch.Generator().manual_seed(1)).half()
    h[0, 0] = float("inf")
    with pytest.raises(ValueError, match="down_proj"):
        wq.pack(h.cuda(), 128, "down_proj.weight")


# ------------------------------------------------------------------------------------------------------------- linear
@functools.lru_cache(maxsize=None)
def _layer(O, K, G, dtype, seed=0):
    """The packed weight on the GPU, its dequantised image in the dtype, the represented weight in fp64 (computed once, shared)."""
    wq = _wq()
    w = R.weights("normal", O, K, G, dtype, 1000 + O + K + G + seed)
    triple = wq.pack(w.cuda(), G)
    wt = R.represented(*(t.cpu() for t in wq.to_ref(*triple)), G)
    return triple, wq.dequant(*triple, dtype), wt


@functools.lru_cache(maxsize=None)
def _x(N, K, dtype, seed=0):
    """x (N, K) as a slice of a wider tensor: row stride K + 16, the first row 16 bytes in."""
    g = torch.Generator().manual_seed(N * 7 + K + seed)
    wide = torch.randn((N, K + 16), generator=g).to(dtype).cuda()
    return wide[:, 8:8 + K]


def _figure(y, ref):
    return (y.double().cpu() - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G", [64, 128])
@pytest.mark.parametrize("O", [16, 48])
@pytest.mark.parametrize("K", [128, 384, 896, 1152])
def test_linear_within_twice_the_error_of_f_linear_on_the_dequantised_weight(K, O, G, dtype):
    wq = _wq()
    triple, what, wt = _layer(O, K, G, dtype)
    bias = (torch.randn(O, generator=torch.Generator().manual_seed(K + O)) * 0.5).to(dtype).cuda()
    for N in NS:
        x = _x(N, K, dtype)
        assert x.stride(0) == K + 16 and not x.is_contiguous() or N == 1
        for b in (None, bias):
            ref = R.linear_ref(x, wt, b)
            got = wq.linear(x, *triple, b)
            torch_y = F.linear(x, what, b)
            assert got.dtype == dtype and tuple(got.shape) == (N, O) and torch.isfinite(got).all()
            d_kernel, d_torch = _figure(got, ref), _figure(torch_y, ref)
            print(f"linear K={K} O={O} G={G} {dtype} N={N} bias={b is not None}: worst |y - y64| / rms: kernel {d_kernel:.4g}, "
                  f"F.linear {d_torch:.4g}")
            assert d_kernel <= 2.0 * d_torch, (N, b is not None, d_kernel, d_torch)
            assert _same(wq.linear(x.contiguous(), *triple, b), got)            # the stride of x does not matter


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G", [64, 128])
@pytest.mark.parametrize("I,K", [(128, 384), (384, 896)])
def test_gate_up_within_twice_the_error_of_the_torch_statement(I, K, G, dtype):
    wq = _wq()
    gate, gate_hat, gate_t = _layer(I, K, G, dtype, 1)
    up, up_hat, up_t = _layer(I, K, G, dtype, 2)
    for N in (1, 5, 16, 17, 33, 64, 65):
        x = _x(N, K, dtype, 3)
        ref = R.gate_up_ref(x, gate_t, up_t)
        got = wq.gate_up(x, gate, up)
        torch_y = F.silu(F.linear(x, gate_hat)) * F.linear(x, up_hat)
        assert got.dtype == dtype and tuple(got.shape) == (N, I) and torch.isfinite(got).all()
        d_kernel, d_torch = _figure(got, ref), _figure(torch_y, ref)
        print(f"gate_up I={I} K={K} G={G} {dtype} N={N}: worst |y - y64| / rms: kernel {d_kernel:.4g}, torch {d_torch:.4g}")
        assert d_kernel <= 2.0 * d_torch, (N, d_kernel, d_torch)


# --------------------------------------------------------------------------------------------------------- bit relations
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,G", [(384, 64), (1152, 128)])
def test_a_tokens_bits_do_not_depend_on_the_batch(K, G, dtype):
    wq = _wq()
    O = 48
    triple, _, _ = _layer(O, K, G, dtype)
    gate, _, _ = _layer(128, K, G, dtype, 1)
    up, _, _ = _layer(128, K, G, dtype, 2)
    bias = (torch.randn(O, generator=torch.Generator().manual_seed(5)) * 0.5).to(dtype).cuda()
    x = _x(65, K, dtype, 9).contiguous()
    for fn in (lambda t: wq.linear(t, *triple, bias), lambda t: wq.gate_up(t, gate, up)):
        full = fn(x)                                                           # 65 tokens: two passes
        assert _same(fn(x), full)                                              # two calls agree
        for n, batch in ((0, 7), (5, 7), (0, 64), (17, 64), (63, 64), (64, 65), (40, 65)):
            got = fn(x[:batch])
            assert _same(got, full[:batch]), batch
            assert _same(fn(x[n:n + 1])[0], full[n]), (n, batch)               # alone
        perm = torch.randperm(65, generator=torch.Generator().manual_seed(3)).cuda()
        assert _same(fn(x[perm].contiguous()), full[perm])
        assert _same(fn(x[3:33]), full[3:33])                                  # another N, other columns, two token tiles


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_modules_replayed_from_a_graph_equal_the_eager_calls(dtype):
    wq = _wq()
    H, I = 384, 896
    torch.manual_seed(21)
    lin = torch.nn.Linear(H, 48, bias=True).to(dtype).cuda()
    qlin = wq.QuantLinear.from_linear(lin, 64).eval()
    mlp = wq.QuantMLP(H, I, 128).cuda().eval()
    for name in ("gate_proj", "up_proj", "down_proj"):
        m = getattr(mlp, name)
        m.pack_((torch.randn((m.out_features, m.in_features), device="cuda") * 0.05).to(dtype), name)
    assert qlin.bias is not None and qlin.bias.dtype == dtype and tuple(qlin.qweight.shape) == (3, 3, 256)
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn((3, 1, H), generator=g).to(dtype).cuda() for _ in range(3)]
    with torch.no_grad():
        for module in (qlin, mlp):
            static = xs[0].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                module(static)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = module(static)
            for x in xs[1:] + xs[:1]:
                static.copy_(x)
                graph.replay()
                assert _same(out, module(x))
            # under capture the kernel runs whatever kernel_max_tokens says
            eager = module(xs[1])
            for m in module.modules():
                if isinstance(m, wq.QuantLinear):
                    m.kernel_max_tokens = 2
            static.copy_(xs[1])
            graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph2):
                out2 = module(static)
            graph2.replay()
            assert _same(out2, eager)
        # the MLP is the two launches: gate_up, then the down projection
        x2 = xs[2].view(3, H)
        a = wq.gate_up(x2, mlp.gate_proj.triple, mlp.up_proj.triple)
        for m in mlp.modules():
            if isinstance(m, wq.QuantLinear):
                m.kernel_max_tokens = 64
        assert _same(mlp(xs[2]).view(3, H), wq.linear(a, *mlp.down_proj.triple))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_above_kernel_max_tokens_the_module_is_f_linear_on_its_dequantised_weight(dtype):
    wq = _wq()
    torch.manual_seed(31)
    lin = torch.nn.Linear(384, 48, bias=True).to(dtype).cuda()
    big = torch.nn.Linear(896, 64, bias=False).to(dtype).cuda()
    qlin, qbig = wq.QuantLinear.from_linear(lin, 128, kernel_max_tokens=8), wq.QuantLinear.from_linear(big, 64, kernel_max_tokens=8)
    x = torch.randn((3, 5, 384), device="cuda").to(dtype)
    xb = torch.randn((15, 896), device="cuda").to(dtype)
    with torch.no_grad():
        assert not qlin.uses_kernel(15) and qlin.uses_kernel(8)
        w_hat = qlin.dequant(dtype)
        assert w_hat.dtype == dtype and _same(w_hat, wq.dequant_torch(*qlin.triple, dtype))
        y = qlin(x)                                                            # the scratch is shared: the larger weight goes through it next
        yb = qbig(xb)
        assert tuple(y.shape) == (3, 5, 48) and _same(y, F.linear(x, w_hat, qlin.bias))
        assert _same(yb, F.linear(xb, qbig.dequant(dtype)))
        assert _same(qlin(x), y)                                               # ... and the smaller one again
        few = qlin(x[:1])                                                      # 5 tokens: the kernel
        assert _same(few, wq.linear(x[:1].reshape(5, 384), *qlin.triple, qlin.bias).view(1, 5, 48))
        mlp = wq.QuantMLP(384, 896, 64, kernel_max_tokens=8).cuda()
        for name in ("gate_proj", "up_proj", "down_proj"):
            m = getattr(mlp, name)
            m.pack_((torch.randn((m.out_features, m.in_features), device="cuda") * 0.05).to(dtype), name)
        hat = {n: getattr(mlp, n).dequant(dtype) for n in ("gate_proj", "up_proj", "down_proj")}
        want = F.linear(F.silu(F.linear(x, hat["gate_proj"])) * F.linear(x, hat["up_proj"]), hat["down_proj"])
        assert _same(mlp(x), want)
