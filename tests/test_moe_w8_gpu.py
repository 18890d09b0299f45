"""GPU: kivi_moe_experts_w8 and SparseMoeBlock(expert_fp8=True).

Shapes   the smallest at which an index can go wrong: H in {256, 640} (640: five stretches, wave 0 takes two and the tree sees uneven
         partials; five block-rows of `down`), I in {128, 384} (128: one stretch of `down`, three waves idle; 384: three stretches,
         three block-rows of gate and three of up offset by them), E / K in {8 / 2, 128 / 8}, fp16 and bf16, moe_ref's crafted
         plans (`tied` N = 5; `counts` N = 64 with per-expert counts 0 / 1 / 16 / 17 / 33; `one` N = 64).
Inputs   bytes uniform over the 254 finite codes, block scales distinct per block (a wrong block index moves an output by order
         one), scaled by moe_w8_ref.SCALE_FACTOR so that the fp64 reference's intermediate and output stay below 1 / 16 of the
         fp16 maximum (asserted here on the reference, and finiteness on the result).
Error    tests/test_moe_gpu.py's bar, measured and not fixed: the worst |y - y64| / rms(y64) of experts_w8 against the fp64
         restatement on the represented weights (tests/moe_w8_ref.py) must not exceed 2 x the same figure of the torch loop in the
         model dtype on the same inputs -- experts_torch over `dequant` of the same buffers.  Both figures are printed.
Bits     two calls agree; a token alone has the bits it has in the batch; permuting tokens permutes bits; another N gives the same
         bits for the shared tokens; `out=` is honoured; a torch.cuda.graph capture of SparseMoeBlock(expert_fp8=True).forward at
         E 128 / K 8 / H 256 / I 128, N = 3, replayed on three inputs equals the eager call bit for bit; the policy switches."""
import functools

import pytest
import torch

import moe_ref as R
import moe_w8_ref as W

pytestmark = pytest.mark.gpu
EK = [(8, 2), (128, 8)]
DTYPES = [torch.float16, torch.bfloat16]
FP16_MAX = 65504.0


def _moe():
    from kivi_amd import moe
    return moe


def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@functools.lru_cache(maxsize=2)
def _buffers(E, H, I):
    """The four buffers on the CPU (the reference reads them there)."""
    return W.random_experts(E, H, I, 7 + H + I + E)


@functools.lru_cache(maxsize=2)
def _experts(E, H, I):
    moe = _moe()
    gu, gus, dn, dns = _buffers(E, H, I)
    m = moe.Fp8Experts(E, H, I)
    for e in range(E):
        m.load_expert_(e, "gate_up", gu[e].view(torch.float8_e4m3fn), gus[e], name=f"gate_up[{e}]")
        m.load_expert_(e, "down", dn[e].view(torch.float8_e4m3fn), dns[e], name=f"down[{e}]")
    return m.cuda()


@functools.lru_cache(maxsize=2)
def _dense(E, H, I, dtype):
    """`dequant` of the same buffers in the model dtype: the baseline's weights."""
    return _experts(E, H, I).dequant(dtype)


def _logits(kind, N, E, K, dtype):
    if kind == "tied":
        return R.tied_logits(N, E, 100 + N + E, dtype).cuda()
    return R.crafted_logits(R.crafted_assignment(N, E, K, kind, _moe().TOKEN_TILE), E, 200 + N + E, dtype).cuda()


@functools.lru_cache(maxsize=None)
def _case(kind, N, E, K, H, I, dtype):
    """x, logits, the kernels' plan and the fp64 reference, computed once per case."""
    moe = _moe()
    logits = _logits(kind, N, E, K, dtype)
    x = torch.randn((N, H), generator=torch.Generator().manual_seed(N + E + I)).to(dtype).cuda()
    plan = moe.route(logits, K, True, False)
    ref, a_max = W.experts_w8_ref(x, plan.idx.long(), plan.w, *_buffers(E, H, I))
    return x, logits, plan, ref, a_max


EXPERT_CASES = [("tied", 5), ("counts", 64), ("one", 64)]


# (the shape is the outer parameter: the buffers of one shape are built once and serve its twelve cases)
@pytest.mark.parametrize("kind,N", EXPERT_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,K", EK)
@pytest.mark.parametrize("I", [128, 384])
@pytest.mark.parametrize("H", [256, 640])
def test_experts_w8_within_twice_the_torch_loops_error(H, I, E, K, dtype, kind, N):
    moe = _moe()
    x, logits, plan, ref, a_max = _case(kind, N, E, K, H, I, dtype)
    assert a_max < FP16_MAX / 16 and ref.abs().max().item() < FP16_MAX / 16, (a_max, ref.abs().max().item())
    fp8 = _experts(E, H, I)
    got = moe.experts_w8(x, plan, fp8)
    loop = moe.experts_torch(x, plan, *_dense(E, H, I, dtype))
    assert got.dtype == dtype and tuple(got.shape) == (N, H) and bool(torch.isfinite(got).all()) and bool(torch.isfinite(loop).all())
    rms = ref.pow(2).mean().sqrt().item()
    d_kernel = (got.double().cpu() - ref).abs().max().item() / rms
    d_loop = (loop.double().cpu() - ref).abs().max().item() / rms
    print(f"{kind} N={N} E={E} K={K} H={H} I={I} {dtype}: worst |y - y64| / rms: experts_w8 {d_kernel:.4g}, torch loop on dequant "
          f"{d_loop:.4g}")
    assert d_kernel <= 2.0 * d_loop, (d_kernel, d_loop)
    out = torch.full((N, H), float("nan"), dtype=dtype, device="cuda")
    assert moe.experts_w8(x, plan, fp8, out=out) is out and _same(out, got)                # two calls, and `out=`
    assert _same(moe.experts_w8_torch(x, plan, fp8), loop)            # the dequantising loop on the same plan: the baseline's bits


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,K,H,I", [(8, 2, 640, 384), (128, 8, 256, 128)])
def test_a_tokens_bits_do_not_depend_on_the_batch(E, K, H, I, dtype):
    moe = _moe()
    N = 64
    x, logits, _, _, _ = _case("counts", N, E, K, H, I, dtype)
    fp8 = _experts(E, H, I)
    run = lambda xs, lg: moe.experts_w8(xs, moe.route(lg, K, True, False), fp8)            # noqa: E731
    got = run(x, logits)
    assert _same(run(x, logits), got)                                                       # two calls
    for n in (0, 1, 16, 17, 40, 63):                                                        # alone: N = 1, one row per tile
        assert _same(run(x[n:n + 1], logits[n:n + 1])[0], got[n]), n
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).cuda()
    assert _same(run(x[perm].contiguous(), logits[perm].contiguous()), got[perm])
    assert _same(run(x[8:13], logits[8:13]), got[8:13])                                     # another N, other tiles
    wide = torch.zeros((N, H + 24), dtype=dtype, device="cuda")                             # a view with a row stride is read as it is
    wide[:, 8:8 + H] = x
    assert _same(run(wide[:, 8:8 + H], logits), got)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_fp8_block_replayed_from_a_graph_equals_the_eager_call(dtype):
    moe = _moe()
    E, K, H, I = 128, 8, 256, 128
    torch.manual_seed(11)
    block = moe.SparseMoeBlock(H, I, E, K, norm_topk=True, round_weights=True, expert_fp8=True).to(dtype).cuda().eval()
    assert isinstance(block.experts, moe.Fp8Experts) and block.kernel_max_tokens == moe.FP8_KERNEL_MAX_TOKENS
    src = _experts(E, H, I)
    with torch.no_grad():
        block.gate.weight.normal_(0.0, 0.3)
        for name, buf in block.experts.named_buffers():
            buf.copy_(getattr(src, name))
        assert block.experts.gate_up_proj_scale_inv.dtype == torch.int32               # .to(dtype) left the scale bits alone
        assert torch.equal(block.experts.gate_up_proj_scale_inv, src.gate_up_proj_scale_inv)
        g = torch.Generator().manual_seed(12)
        xs = [torch.randn((3, 1, H), generator=g).to(dtype).cuda() for _ in range(3)]
        static = xs[0].clone()
        assert block.uses_kernel(static.view(3, H))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            block(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = block(static)
        for x in xs[1:] + xs[:1]:
            static.copy_(x)
            graph.replay()
            assert _same(out, block(x))
        # the policy: more tokens than kernel_max_tokens take the loop outside a capture, the kernel inside one
        x2 = xs[1].view(3, H)
        logits = torch.nn.functional.linear(x2, block.gate.weight)
        kern = moe.experts_w8(x2, moe.route(logits, K, True, True), block.experts)
        loop = moe.experts_w8_torch(x2, moe.route_torch(logits, K, True, True), block.experts)
        assert _same(block(xs[1]).view(3, H), kern)
        block.kernel_max_tokens = 2
        assert not block.uses_kernel(x2) and _same(block(xs[1]).view(3, H), loop)
        static.copy_(xs[1])
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2):
            out2 = block(static)
        graph2.replay()
        assert _same(out2.view(3, H), kern)
        block.kernel = False
        assert _same(block(xs[1]).view(3, H), loop)
