"""GPU: the two launches of kivi_amd/csrc/kivi_lora.hip (kivi_lora_shrink, kivi_lora_expand), fp16 and bf16.

Shapes: K in {8, 24, 256, 1032} -- fewer 16-byte units than lanes, empty lanes, uneven tails --, O in {8, 264}, table rank R in {8, 64}
holding adapters of rank r in {1, 5, 8, 64}, S = 3, (B, Q) in {(1, 1), (3, 5), (17, 1)}, x a strided view, slots mixing -1, repeats and
all -1.  Every element is held to the bound of tests/lora_ref.py against the fp64 statement,

    |y' - y64| <= u |y64| + gamma_(K + R + 3) * scale * sum_j |B_oj| sum_k |A_jk| |x_k| + 2^-24 |y|,

u = 2^-11 (fp16) / 2^-8 (bf16); nothing is fitted to the kernel, and the worst ratio is printed.  Bit for bit: rows of slot -1 are
untouched; row n alone equals row n inside the batch; the result depends neither on the other rows' slots nor on R.  The kernels
equal apply_torch to within twice the bound.  The same launches captured in a graph and replayed three times equal the eager
result bit for bit, and a load() into the slot between replays shows up without a new capture."""
import pytest
import torch

import lora_ref as R

pytestmark = pytest.mark.gpu
RANKS = {8: (1, 5, 8), 64: (5, 8, 64)}
ROWS = [(1, 1, [[1], [-1]]),
        (3, 5, [[2, -1, 0], [-1, -1, -1]]),
        (17, 1, [[0, 1, 2, -1, 1, 1, 0, -1, 2, 0, 0, 1, -1, 2, 2, 1, 0]])]


def _inputs(dtype, K, O, Bt, Q, seed):
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn((Bt, Q, K + 8), generator=g).to(dtype).cuda()
    x = wide[:, :, :K]                                                  # a strided view: rows K + 8 apart
    y = torch.randn((Bt, Q, O), generator=g).to(dtype).cuda()
    return x, y


def _slots(slots):
    return torch.tensor(slots, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("O", [8, 264])
@pytest.mark.parametrize("K", [8, 24, 256, 1032])
def test_kernels_against_the_fp64_statement(K, O, dtype):
    from kivi_amd import lora
    worst = worst_torch = 0.0
    for Rk in (8, 64):
        A, B, scale, ranks = R.tables(3, Rk, K, O, RANKS[Rk], dtype, "cuda", K + O + Rk)
        for Bt, Q, mixes in ROWS:
            x, y0 = _inputs(dtype, K, O, Bt, Q, K + Bt)
            for slots in mixes:
                y = lora.apply_kernels(y0.clone(), x, A, B, scale, ranks, _slots(slots))
                y64, mag = R.statement64(y0, x, A, B, scale, slots)
                worst = max(worst, R.worst_ratio(y, y0, y64, mag, K, Rk, dtype))
                for b, s in enumerate(slots):
                    assert torch.equal(y[b], y0[b]) == (s < 0), (b, s)      # the base model's rows: untouched
                ref = lora.apply_torch(y0.clone(), x, A, B, scale.tolist(), ranks.tolist(), slots)
                # two results that each sit within the bound of y64 sit within twice the bound of each other
                worst_torch = max(worst_torch, R.worst_ratio(y, y0, ref.double().cpu(), mag, K, Rk, dtype, factor=2.0))
    print(f"{dtype} K={K} O={O}: worst |kernels - fp64| / bound = {worst:.3g}, |kernels - apply_torch| / (2 bound) = {worst_torch:.3g}")
    assert worst <= 1.0 and worst_torch <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("K,O", [(24, 8), (1032, 264)])
def test_a_row_depends_on_its_own_x_slot_and_tables_alone(K, O, dtype):
    from kivi_amd import lora
    A, B, scale, ranks = R.tables(3, 8, K, O, (1, 5, 8), dtype, "cuda", 11)
    Bt, Q = 5, 3
    x, y0 = _inputs(dtype, K, O, Bt, Q, 12)
    slots = [1, -1, 2, 1, 0]
    y = lora.apply_kernels(y0.clone(), x, A, B, scale, ranks, _slots(slots))
    for b in range(Bt):                                                 # row b alone, as a pass of one row
        alone = lora.apply_kernels(y0[b:b + 1].clone(), x[b:b + 1], A, B, scale, ranks, _slots(slots[b:b + 1]))
        assert torch.equal(alone[0], y[b]), b
    for q in range(Q):                                                  # token (0, q) alone, as a pass of one token
        one = lora.apply_kernels(y0[0:1, q:q + 1].clone(), x[0:1, q:q + 1], A, B, scale, ranks, _slots(slots[0:1]))
        assert torch.equal(one[0, 0], y[0, q]), q
    other = lora.apply_kernels(y0.clone(), x, A, B, scale, ranks, _slots([1, 0, -1, 2, 2]))      # the other rows' slots change
    assert torch.equal(other[0], y[0]) and not torch.equal(other[1], y[1])
    # the same adapters in tables of rank 64, among 5 slots: R and S do not matter
    A64, B64 = torch.zeros((5, 64, K), dtype=dtype, device="cuda"), torch.zeros((5, O, 64), dtype=dtype, device="cuda")
    A64[:3, :8], B64[:3, :, :8] = A, B
    scale5 = torch.cat([scale, scale[:2]])
    ranks5 = torch.cat([ranks, ranks[:2]])
    wide = lora.apply_kernels(y0.clone(), x, A64, B64, scale5, ranks5, _slots(slots))
    assert torch.equal(wide, y)
    # a slot value outside [-1, S) that reaches the device leaves its row untouched
    stray = lora.apply_kernels(y0.clone(), x, A, B, scale, ranks, _slots([3, -5, 2, 1 << 20, 0]))
    assert torch.equal(stray[0], y0[0]) and torch.equal(stray[1], y0[1]) and torch.equal(stray[3], y0[3])
    assert torch.equal(stray[2], y[2]) and torch.equal(stray[4], y[4])
    # a zero B (PEFT's initialisation) and an unloaded slot (rank 0) leave y bit-unchanged
    zero = lora.apply_kernels(y0.clone(), x, A, torch.zeros_like(B), scale, ranks, _slots(slots))
    assert torch.equal(zero, y0)
    empty = lora.apply_kernels(y0.clone(), x, A, B, scale, torch.zeros_like(ranks), _slots(slots))
    assert torch.equal(empty, y0)


class _Toy(torch.nn.Module):
    def __init__(self, K, O, dtype):
        super().__init__()
        self.q_proj = torch.nn.Linear(K, O, bias=True)
        self.lm_head = torch.nn.Linear(O, 16, bias=False)
        self.to(dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_captured_launches_replay_bit_for_bit_and_see_a_load(dtype):
    from kivi_amd import lora
    K, O, Bt, Q = 256, 264, 3, 5
    torch.manual_seed(5)
    toy = _Toy(K, O, dtype)
    lset = lora.LoraSet(toy, 3, 16, ("q_proj",)).attach()
    first, second = (R.make_adapter(toy, r, 2.0 * r, seed, ("q_proj",)) for r, seed in ((5, 1), (16, 2)))
    lset.load(first, 0)
    lset.load(second, 2)
    x, _ = _inputs(dtype, K, O, Bt, Q, 6)
    x = x.contiguous()
    binding = lora.RowBinding(Bt, "cuda", [0, None, 2])
    with torch.no_grad(), lset.bound(binding):
        eager = toy.q_proj(x).clone()
        base = torch.nn.functional.linear(x, toy.q_proj.weight, toy.q_proj.bias)
        assert torch.equal(eager[1], base[1]) and not torch.equal(eager[0], base[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            toy.q_proj(x)
        torch.cuda.current_stream().wait_stream(side)
        out = torch.empty_like(eager)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out.copy_(toy.q_proj(x))
        for _ in range(3):
            out.zero_()
            graph.replay()
            assert torch.equal(out, eager)
        lset.load(second, 0)                                            # in place: the captured launches read the same addresses
        binding.set_row(1, 2)
        graph.replay()
        again = toy.q_proj(x)
        assert torch.equal(out, again) and not torch.equal(out[0], eager[0]) and not torch.equal(out[1], eager[1])
        assert torch.equal(out[2], eager[2])
        lset.unload(0)
        graph.replay()
        assert torch.equal(out[0], base[0])
    lset.detach()
