"""GPU: 4-bit experts -- QuantExperts and SparseMoeBlock(expert_bits=4).  The experts are packed by
kivi_w4_pack and dequantised by kivi_w4_dequant (section 30's kernels); the block runs the dequantising loop.  The models are in
tests/test_moe_w4_model_gpu.py.

Packing  H in {128, 384, 640}, I in {128, 384}, E in {8, 16}, G in {64, 128}, fp16 and bf16; expert 1 all zero (every scale 0),
         expert 3 with constant groups.  Slab e of the stacked buffers equals wquant.pack of expert e's matrices bit for bit (itself
         held to the oracle by tests/test_w4_gpu.py), whether the gate and the up matrix arrive separately or as one; dequant_expert
         equals wquant.dequant of that pack.
Block    logits crafted to per-expert counts 0, 1, 16, 17, 33 and to "every token to one expert": the loop over the packed experts
         -- each hit expert dequantised into views of the shared scratch -- has the bits of experts_torch over the dequantised
         stacks, every element finite, and its worst |y - y64| / rms(y64) against the fp64 statement (tests/moe_ref.py) over the
         exact W~ = code * scale + mn is printed.  The module in front of it gives the same bits; fp32 activations are refused by
         name."""
import functools

import pytest
import torch

import moe_ref as R
import w4_ref as W

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
# H, I, E, K, G, dtype, kind, N
CASES = [
    (128, 128, 8, 2, 64, F16, "counts", 64), (128, 128, 8, 2, 128, BF16, "tied", 1),
    (384, 384, 16, 4, 128, F16, "counts", 64), (384, 128, 8, 2, 64, BF16, "counts", 130),
    (640, 128, 8, 2, 128, F16, "one", 64), (640, 384, 16, 4, 64, BF16, "one", 130), (640, 384, 16, 4, 64, F16, "tied", 5),
]
IDS = [f"H{h}-I{i}-E{e}K{k}-g{g}-{'fp16' if d == F16 else 'bf16'}-{kind}{n}" for h, i, e, k, g, d, kind, n in CASES]


def _moe():
    from kivi_amd import moe
    return moe


@functools.lru_cache(maxsize=None)
def _experts(H, I, E, G, dtype):
    """Dense stacks on the GPU, their QuantExperts, and the exact represented weights in fp64."""
    from kivi_amd import wquant
    moe = _moe()
    g = torch.Generator().manual_seed(H + 3 * I + E + G)
    gate_up = torch.randn((E, 2 * I, H), generator=g) * 0.08
    down = torch.randn((E, H, I), generator=g) * 0.08
    gate_up[1], down[1] = 0.0, 0.0                                      # an all-zero expert
    gate_up[3, :, :G], down[3, ::2, -G:] = 0.37, -0.21                  # constant groups: scale 0
    gate_up, down = gate_up.to(dtype).cuda(), down.to(dtype).cuda()
    q = moe.QuantExperts.from_dense(gate_up, down, G)
    wt_gu = torch.stack([W.represented(*wquant.to_ref(*(v.contiguous() for v in q.slab(e, "gate_up"))), G) for e in range(E)])
    wt_dn = torch.stack([W.represented(*wquant.to_ref(*(v.contiguous() for v in q.slab(e, "down"))), G) for e in range(E)])
    return gate_up, down, q, wt_gu, wt_dn


def _logits(kind, N, E, K, dtype):
    if kind == "tied":
        return R.tied_logits(N, E, 100 + N + E, dtype).cuda()
    return R.crafted_logits(R.crafted_assignment(N, E, K, kind, _moe().TOKEN_TILE), E, 200 + N + E, dtype).cuda()


@pytest.mark.parametrize("H,I,E,G,dtype", sorted({(h, i, e, g, d) for h, i, e, _, g, d, _, _ in CASES}, key=str))
def test_a_slab_is_wquant_pack_of_the_experts_matrices(H, I, E, G, dtype):
    from kivi_amd import wquant
    moe = _moe()
    gate_up, down, q, _, _ = _experts(H, I, E, G, dtype)
    want = wquant.shapes(2 * I, H, G), wquant.shapes(H, I, G)
    for stack, shp in ((q.gate_up_proj, want[0]), (q.down_proj, want[1])):
        assert tuple(stack.qweight.shape) == (E, *shp[0]) and tuple(stack.scales.shape) == (E, *shp[1]) == tuple(stack.mins.shape)
        assert stack.qweight.dtype == torch.int32 and stack.scales.dtype == torch.int16 and stack.mins.dtype == torch.int16
        assert all(t.is_contiguous() and t.is_cuda for t in stack.triple)
    other = moe.QuantExperts(E, H, I, G).cuda()                         # gate and up on their own, in reverse order
    for e in reversed(range(E)):
        other.pack_expert_(e, "down", down[e])
        other.pack_expert_(e, "up", gate_up[e, I:])
        other.pack_expert_(e, "gate", gate_up[e, :I])
    for e in range(E):
        for part, w in (("gate_up", gate_up[e]), ("down", down[e])):
            for a, b, c in zip(q.slab(e, part), wquant.pack(w, G), other.slab(e, part)):
                assert torch.equal(a, b) and torch.equal(c, b), (e, part)
    gu, dn = q.dequant_expert(3, dtype)
    assert torch.equal(gu, wquant.dequant(*wquant.pack(gate_up[3], G), dtype=dtype))
    assert torch.equal(dn, wquant.dequant(*wquant.pack(down[3], G), dtype=dtype))
    assert bool((q.down_proj.scales[1] == 0).all()) and bool((q.gate_up_proj.scales[1] == 0).all())      # the all-zero expert
    assert bool((q.gate_up_proj.scales[3, :, 0] == 0).all())                                             # its constant groups
    with pytest.raises(ValueError, match="out must be"):                # buffers of other shapes and dtypes are refused
        wquant.pack(down[0], G, out=tuple(reversed(q.slab(0, "down"))))


@pytest.mark.parametrize("H,I,E,K,G,dtype,kind,N", CASES, ids=IDS)
def test_block_has_the_bits_of_the_loop_over_dense_stacks(H, I, E, K, G, dtype, kind, N):
    moe = _moe()
    _, _, q, wt_gu, wt_dn = _experts(H, I, E, G, dtype)
    block = moe.SparseMoeBlock(H, I, E, K, norm_topk=True, round_weights=E == 16, expert_bits=4, expert_group=G).to(dtype).cuda().eval()
    assert type(block.experts) is moe.QuantExperts and [n for n, _ in block.named_parameters()] == ["gate.weight"]
    block.experts.load_state_dict(q.state_dict())
    x = torch.randn((N, H), generator=torch.Generator().manual_seed(N + E + I)).to(dtype).cuda()
    logits = _logits(kind, N, E, K, dtype)
    plan = moe.route_torch(logits, K, True, E == 16)
    ref = R.experts_ref(x, plan.idx.long(), plan.w, wt_gu, wt_dn)
    with torch.no_grad():
        got = moe.experts_w4_torch(x, plan, block.experts)
        dq_gu = torch.stack([q.dequant_expert(e, dtype)[0] for e in range(E)])
        dq_dn = torch.stack([q.dequant_expert(e, dtype)[1] for e in range(E)])
        loop = moe.experts_torch(x, plan, dq_gu, dq_dn)
    assert got.dtype == dtype and tuple(got.shape) == (N, H) and bool(torch.isfinite(got).all())
    rms = ref.pow(2).mean().sqrt().item()
    print(f"{IDS[CASES.index((H, I, E, K, G, dtype, kind, N))]}: worst |y - y64| / rms of the loop over 4-bit experts: "
          f"{(got.double() - ref).abs().max().item() / rms:.4g}")
    assert torch.equal(got.view(torch.int16), loop.view(torch.int16))       # the same arithmetic from other memory: the same bits
    # the module: its own router in front of the same loop
    with torch.no_grad():
        block.gate.weight.normal_(0.0, 0.3)
        x3 = x.view(1, N, H)
        own = moe.route_torch(torch.nn.functional.linear(x, block.gate.weight), K, True, E == 16)
        assert torch.equal(block(x3).view(N, H).view(torch.int16), moe.experts_w4_torch(x, own, block.experts).view(torch.int16))
        with pytest.raises(ValueError, match="float32"):
            block.float()(x3.float())
