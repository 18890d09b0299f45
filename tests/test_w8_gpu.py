"""GPU: kivi_w8_dequant / kivi_w8_linear / kivi_w8_gate_up, the load-time quantiser and the modules over them.

Dequant    a (16, 256) weight holding every byte value except the two NaNs, each at 16 positions, under scales log-uniform over
           [2^-30, 2^8] and a zero scale: bit-identical to torch's (w8.float() * s).to(dtype) in fp16 and bf16.  This is the test
           that says what v_cvt_scalef32_pk_{f16,bf16}_fp8 return on the card.
Linear     K in {128, 384, 896, 1152} (1 tile; fewer tiles than waves; 7 and 9 tiles dealt unevenly over the 8 waves), O in
           {16, 48, 144} (144 crosses a scale block-row at row 128), N in {1, 5, 16, 17, 64, 65, 130}, bias on and off, both dtypes,
           x a strided slice.  Bytes uniform over the 254 finite codes, block scales 2^-6 * u with u distinct per block in [0.5, 2):
           a wrong block index moves an output by order one.  The bar is the one of tests/test_w4_gpu.py: the worst
           |y - y64| / rms(y64) of the kernel must not exceed 2 x the same figure of F.linear(x, W^) in the model dtype on the same
           inputs, y64 the fp64 product with the represented weight (tests/w8_ref.py).  Both are printed.
Gate/up    (I, K) in {(128, 384), (144, 896)} against fp64 silu(g) * u, the same bar with the torch statement as the yardstick.
Bits       a token alone has the bits it has in a batch of 7, of 64 and of 65; permuting the tokens permutes the bits; two calls
           agree; torch.cuda.graph captures of Fp8Linear.forward and Fp8MLP.forward replayed on new inputs equal the eager calls;
           above kernel_max_tokens the module equals F.linear(x, module.dequant()) bit for bit.
Quantiser  wfp8.quantize on the device equals tests/w8_ref.py's CPU restatement bit for bit: normal weights, an all-zero block, a
           block with one outlier, a partial block-row, bf16 and fp16 input."""
import functools

import pytest
import torch
import torch.nn.functional as F

import w8_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NS = [1, 5, 16, 17, 64, 65, 130]


def _w8():
    from kivi_amd import wfp8
    return wfp8


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _bits(scale: torch.Tensor) -> torch.Tensor:
    return scale.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ dequant
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dequant_of_every_byte_is_the_torch_statement_bit_for_bit(dtype):
    w8 = _w8()
    g = torch.Generator().manual_seed(8)
    # 254 codes x 16 positions, shuffled: every code meets both scale blocks, every lane, both halves of a pair and of a word
    weight = R.FINITE_BYTES.repeat(16)[:16 * 256 - 32]
    weight = torch.cat([weight, R.FINITE_BYTES[:32]])[torch.randperm(4096, generator=g)].reshape(16, 256)
    assert all(int((weight == b).sum()) >= 16 for b in R.FINITE_BYTES.tolist()) and not bool(((weight & 0x7F) == 0x7F).any())
    exps = -30.0 + 38.0 * torch.rand(47, generator=g, dtype=torch.float64)
    values = torch.cat([torch.pow(2.0, exps), torch.tensor([0.0, 2.0 ** -30, 2.0 ** 8], dtype=torch.float64)]).float()
    dev = weight.cuda()
    for i in range(0, values.numel(), 2):
        scale = values[i:i + 2].reshape(1, 2)
        want = (weight.view(torch.float8_e4m3fn).float() * R.expand(scale, 16, 256)).to(dtype)
        assert _same(want, R.represented(weight, scale).float().to(dtype))                 # ... which is the contract's weight, rounded
        got = w8.dequant(dev, _bits(scale).cuda(), dtype)
        assert got.dtype == dtype and _same(got.cpu(), want), (i, scale)
    assert float(values.min()) == 0.0
    # into a buffer, and the torch form of the module agrees
    out = torch.empty((16, 256), dtype=dtype, device="cuda")
    assert w8.dequant(dev, _bits(scale).cuda(), dtype, out=out) is out and _same(out.cpu(), want)
    assert _same(w8.dequant_torch(dev, scale.cuda(), dtype), out)


# ------------------------------------------------------------------------------------------------------------------- linear
@functools.lru_cache(maxsize=None)
def _layer(O, K, dtype, seed=0):
    """The pair on the GPU, its dequantised image in the dtype, the represented weight in fp64 (computed once, shared)."""
    w8 = _w8()
    weight, scale = R.random_bytes((O, K), 1000 + O + K + seed), R.block_scales(O, K, O + K + seed)
    assert scale.unique().numel() == scale.numel()
    pair = (weight.cuda(), _bits(scale).cuda())
    return pair, w8.dequant(*pair, dtype), R.represented(weight, scale)


@functools.lru_cache(maxsize=None)
def _x(N, K, dtype, seed=0):
    """x (N, K) as a slice of a wider tensor: row stride K + 16, the first row 16 bytes in."""
    g = torch.Generator().manual_seed(N * 7 + K + seed)
    wide = torch.randn((N, K + 16), generator=g).to(dtype).cuda()
    return wide[:, 8:8 + K]


def _figure(y, ref):
    return (y.double().cpu() - ref).abs().max().item() / ref.pow(2).mean().sqrt().item()


def _linear_ref(x, wt, bias=None):
    y = x.double().cpu() @ wt.t()
    return y if bias is None else y + bias.double().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("O", [16, 48, 144])
@pytest.mark.parametrize("K", [128, 384, 896, 1152])
def test_linear_within_twice_the_error_of_f_linear_on_the_dequantised_weight(K, O, dtype):
    w8 = _w8()
    pair, what, wt = _layer(O, K, dtype)
    bias = (torch.randn(O, generator=torch.Generator().manual_seed(K + O)) * 0.5).to(dtype).cuda()
    for N in NS:
        x = _x(N, K, dtype)
        assert x.stride(0) == K + 16 and not x.is_contiguous() or N == 1
        for b in (None, bias):
            ref = _linear_ref(x, wt, b)
            got = w8.linear(x, *pair, b)
            torch_y = F.linear(x, what, b)
            assert got.dtype == dtype and tuple(got.shape) == (N, O) and torch.isfinite(got).all()
            d_kernel, d_torch = _figure(got, ref), _figure(torch_y, ref)
            print(f"linear K={K} O={O} {dtype} N={N} bias={b is not None}: worst |y - y64| / rms: kernel {d_kernel:.4g}, "
                  f"F.linear {d_torch:.4g}")
            assert d_kernel <= 2.0 * d_torch, (N, b is not None, d_kernel, d_torch)
            assert _same(w8.linear(x.contiguous(), *pair, b), got)              # the stride of x does not matter


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("I,K", [(128, 384), (144, 896)])
def test_gate_up_within_twice_the_error_of_the_torch_statement(I, K, dtype):
    w8 = _w8()
    gate, gate_hat, gate_t = _layer(I, K, dtype, 1)
    up, up_hat, up_t = _layer(I, K, dtype, 2)
    for N in (1, 5, 16, 17, 33, 64, 65):
        x = (_x(N, K, dtype, 3) * 0.125).contiguous()           # g ~ 15 rms: silu is neither the identity nor zero on most of it
        g64, u64 = _linear_ref(x, gate_t), _linear_ref(x, up_t)
        ref = g64 * torch.sigmoid(g64) * u64
        got = w8.gate_up(x, gate, up)
        torch_y = F.silu(F.linear(x, gate_hat)) * F.linear(x, up_hat)
        assert got.dtype == dtype and tuple(got.shape) == (N, I) and torch.isfinite(got).all()
        d_kernel, d_torch = _figure(got, ref), _figure(torch_y, ref)
        print(f"gate_up I={I} K={K} {dtype} N={N}: worst |y - y64| / rms: kernel {d_kernel:.4g}, torch {d_torch:.4g}")
        assert d_kernel <= 2.0 * d_torch, (N, d_kernel, d_torch)


# ------------------------------------------------------------------------------------------------------------ bit relations
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [384, 1152])
def test_a_tokens_bits_do_not_depend_on_the_batch(K, dtype):
    w8 = _w8()
    O = 144
    pair, _, _ = _layer(O, K, dtype)
    gate, _, _ = _layer(128, K, dtype, 1)
    up, _, _ = _layer(128, K, dtype, 2)
    bias = (torch.randn(O, generator=torch.Generator().manual_seed(5)) * 0.5).to(dtype).cuda()
    x = (_x(65, K, dtype, 9) * 0.125).contiguous()
    for fn in (lambda t: w8.linear(t, *pair, bias), lambda t: w8.gate_up(t, gate, up)):
        full = fn(x)                                                           # 65 tokens: two passes
        assert _same(fn(x), full)                                              # two calls agree
        for n, batch in ((0, 7), (5, 7), (0, 64), (17, 64), (63, 64), (64, 65), (40, 65)):
            got = fn(x[:batch])
            assert _same(got, full[:batch]), batch
            assert _same(fn(x[n:n + 1])[0], full[n]), (n, batch)               # alone
        perm = torch.randperm(65, generator=torch.Generator().manual_seed(3)).cuda()
        assert _same(fn(x[perm].contiguous()), full[perm])
        assert _same(fn(x[3:33]), full[3:33])                                  # another N, other columns, two token tiles


def _from_linear(w8, linear, **kw):
    """The Fp8Linear of an nn.Linear on the GPU: its weight quantised on the device, its bias taken over."""
    with torch.device("cuda"):
        m = w8.Fp8Linear(linear.in_features, linear.out_features, linear.bias is not None, **kw)
    m.quantize_(linear.weight.data)
    if linear.bias is not None:
        m.bias.data = linear.bias.data.clone()
    return m


def _random_mlp(w8, H, I, dtype, **kw):
    mlp = w8.Fp8MLP(H, I, **kw).cuda().eval()
    for name in ("gate_proj", "up_proj", "down_proj"):
        m = getattr(mlp, name)
        m.quantize_((torch.randn((m.out_features, m.in_features), device="cuda") * 0.05).to(dtype), name)
    return mlp


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_modules_replayed_from_a_graph_equal_the_eager_calls(dtype):
    w8 = _w8()
    H, I = 384, 896
    torch.manual_seed(21)
    lin = torch.nn.Linear(H, 48, bias=True).to(dtype).cuda()
    qlin = _from_linear(w8, lin).eval()
    mlp = _random_mlp(w8, H, I, dtype)
    assert qlin.bias is not None and qlin.bias.dtype == dtype and tuple(qlin.weight.shape) == (48, 384)
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
                if isinstance(m, w8.Fp8Linear):
                    m.kernel_max_tokens = 2
            static.copy_(xs[1])
            graph2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph2):
                out2 = module(static)
            graph2.replay()
            assert _same(out2, eager)
        # the MLP is the two launches: gate_up, then the down projection
        x2 = xs[2].view(3, H)
        a = w8.gate_up(x2, mlp.gate_proj.pair, mlp.up_proj.pair)
        for m in mlp.modules():
            if isinstance(m, w8.Fp8Linear):
                m.kernel_max_tokens = 64
        assert _same(mlp(xs[2]).view(3, H), w8.linear(a, *mlp.down_proj.pair))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_above_kernel_max_tokens_the_module_is_f_linear_on_its_dequantised_weight(dtype):
    w8 = _w8()
    torch.manual_seed(31)
    lin = torch.nn.Linear(384, 48, bias=True).to(dtype).cuda()
    big = torch.nn.Linear(896, 144, bias=False).to(dtype).cuda()
    qlin, qbig = _from_linear(w8, lin, kernel_max_tokens=8), _from_linear(w8, big, kernel_max_tokens=8)
    x = torch.randn((3, 5, 384), device="cuda").to(dtype)
    xb = torch.randn((15, 896), device="cuda").to(dtype)
    with torch.no_grad():
        assert not qlin.uses_kernel(15) and qlin.uses_kernel(8)
        w_hat = qlin.dequant(dtype)
        assert w_hat.dtype == dtype and _same(w_hat, w8.dequant_torch(qlin.weight, qlin.scale, dtype))
        y = qlin(x)                                                            # the scratch is shared: the larger weight goes through it next
        yb = qbig(xb)
        assert tuple(y.shape) == (3, 5, 48) and _same(y, F.linear(x, w_hat, qlin.bias))
        assert _same(yb, F.linear(xb, qbig.dequant(dtype)))
        assert _same(qlin(x), y)                                               # ... and the smaller one again
        few = qlin(x[:1])                                                      # 5 tokens: the kernel
        assert _same(few, w8.linear(x[:1].reshape(5, 384), *qlin.pair, qlin.bias).view(1, 5, 48))
        mlp = _random_mlp(w8, 384, 896, dtype, kernel_max_tokens=8)
        hat = {n: getattr(mlp, n).dequant(dtype) for n in ("gate_proj", "up_proj", "down_proj")}
        want = F.linear(F.silu(F.linear(x, hat["gate_proj"])) * F.linear(x, hat["up_proj"]), hat["down_proj"])
        assert _same(mlp(x), want)


# ---------------------------------------------------------------------------------------------------------------- quantiser
def _weights(kind, O, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((O, K), generator=g) * 0.05
    if kind == "zero_block":
        w[:128, 128:256] = 0
    elif kind == "outlier":
        w[130 % O, 200] = 5.0
    return w.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("kind,O,K", [("normal", 256, 384), ("zero_block", 256, 384), ("outlier", 256, 256), ("normal", 144, 384),
                                      ("outlier", 48, 256)])
def test_the_device_quantiser_is_the_cpu_restatement_bit_for_bit(kind, O, K, dtype):
    w8 = _w8()
    w = _weights(kind, O, K, dtype, O + K)
    codes, inv = w8.quantize(w.cuda())
    rc, ri = R.quantize_ref(w)
    assert codes.is_cuda and codes.dtype == torch.uint8 and inv.dtype == torch.float32
    assert torch.equal(inv.cpu().view(torch.int32), ri.view(torch.int32))
    assert torch.equal(codes.cpu(), rc)
    lin = w8.Fp8Linear(K, O).cuda().quantize_(w.cuda(), "w")
    assert torch.equal(lin.weight.cpu(), rc) and torch.equal(lin.weight_scale_inv.cpu(), ri.view(torch.int32))
    if kind == "zero_block":
        assert float(ri[0, 1]) == 1.0 and int(rc[:128, 128:256].max()) == 0
