"""GPU: kivi_moe_route / kivi_moe_experts and the sparse models through the public interface.  H = 256.

Route    E / K in {8 / 2, 60 / 4, 128 / 8}, fp16 and bf16, N in {1, 5, 64, 1000}: idx equals the fp64 restatement (tests/moe_ref.py)
         exactly, rows with deliberately equal logits included; w within 1e-5 relative of fp64 (an fp32 softmax of <= 256 terms plus
         two operations is far inside), with round_weights within one ulp of the dtype; counts / offsets exact, every expert's
         segment of `pairs` exactly its set of pairs, pos inverts pairs, the tile list covers each segment once.  Crafted logits
         give per-expert counts 0, 1, TILE, TILE + 1, 2 TILE + 1, and "every token to one expert".
Experts  I = 96 (a 32-granular tail: three 32-element steps) and I = 128, the same E / K, both dtypes, the crafted count patterns,
         against the fp64 restatement.  The bar is measured, not fixed: the worst |y - y64| / rms(y64) of the kernel path must not
         exceed 2 x the same figure of the torch loop in the model dtype on the same inputs -- both round the intermediate once and
         accumulate in fp32, only the order of summation differs, which the factor covers.  Both figures are printed.
Bits     a token run alone has the bits it has in the batch; permuting the tokens permutes the output bits; two calls agree; a
         torch.cuda.graph capture of SparseMoeBlock.forward replayed on new inputs equals the eager call bit for bit.
Models   tests/tiny_moe_models.py (Mixtral-like E = 8 / K = 2 / ratio 4; Qwen3-MoE-like E = 16 / K = 4 / ratio 8, one dense layer,
         head norms), fp16 and one bf16 case: generate equals generate_graphed token for token from a whole-step capture;
         generate_continuous, eager and graphed, equals the restated policy of tests/test_admit_gpu.py; per-step logits with the
         kernels against the same weights on the torch loop inside the band tests/test_qwen_gpu.py holds two forms of one model to
         (1e-2 of the rms on the prompt pass, 5e-2 on decode steps); weights saved under HF's per-expert names load through
         LlamaForCausalLM_KIVI.from_pretrained into the right class with bit-identical logits."""
import functools
import json

import pytest
import torch

import moe_ref as R
import tiny_moe_models as M
from helpers import same_bits

pytestmark = pytest.mark.gpu
H = 256
EK = [(8, 2), (60, 4), (128, 8)]
DTYPES = [torch.float16, torch.bfloat16]
T0, STEPS = 70, 40


def _moe():
    from kivi_amd import moe
    return moe


def _same(a, b) -> bool:
    """The same 16-bit patterns (helpers.same_bits compares bf16 by value)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _logits(kind, N, E, K, dtype):
    tile = _moe().TOKEN_TILE
    if kind == "tied":
        return R.tied_logits(N, E, 100 + N + E, dtype).cuda(), None
    assign = R.crafted_assignment(N, E, K, kind, tile)
    return R.crafted_logits(assign, E, 200 + N + E, dtype).cuda(), assign


# ------------------------------------------------------------------------------------------------------------------- route
ROUTE_CASES = [("tied", 1), ("tied", 5), ("tied", 64), ("tied", 1000), ("counts", 64), ("counts", 1000), ("one", 64), ("one", 1000)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,K", EK)
@pytest.mark.parametrize("kind,N", ROUTE_CASES)
def test_route_against_the_fp64_restatement(kind, N, E, K, dtype):
    moe = _moe()
    tile = moe.TOKEN_TILE
    logits, assign = _logits(kind, N, E, K, dtype)
    for norm, rnd in ((True, False), (False, True), (True, True)):
        plan = moe.route(logits, K, norm, rnd)
        idx64, w64 = R.route_ref(logits, K, norm, False)
        assert plan.idx.dtype == torch.int32 and plan.w.dtype == torch.float32 and tuple(plan.idx.shape) == (N, K)
        assert torch.equal(plan.idx.long(), idx64), (kind, norm, rnd)
        got = plan.w.double()
        if rnd:
            assert torch.equal(plan.w, plan.w.to(dtype).float())                    # the fp32 image of a value of the dtype
            assert bool(((got - w64).abs() <= R.ulp_of(w64, dtype)).all())
        else:
            worst = ((got - w64).abs() / w64).max().item()
            assert worst <= 1e-5, worst
        R.check_plan(plan, idx64, tile)
    if kind == "tied":
        assert plan.idx[0].tolist() == list(range(K)) and (N == 1 or plan.idx[1].tolist() == list(range(K)))
    else:
        assert torch.equal(plan.idx.long().cpu(), assign)
        counts = plan.counts.cpu().long()
        if kind == "counts":
            assert counts[:5].tolist() == [0, 1, tile, tile + 1, 2 * tile + 1]
        else:
            assert int(counts[3]) == N and int(plan.n_tiles[0]) >= (N + tile - 1) // tile


def test_route_reads_a_strided_view_and_random_logits():
    moe = _moe()
    g = torch.Generator().manual_seed(5)
    wide = torch.randn((37, 80), generator=g).half().cuda()
    view = wide[:, 3:63]
    plan = moe.route(view, 4, True, False)
    idx64, w64 = R.route_ref(view, 4, True, False)
    assert torch.equal(plan.idx.long(), idx64) and ((plan.w.double() - w64).abs() / w64).max().item() <= 1e-5
    R.check_plan(plan, idx64, moe.TOKEN_TILE)


# ----------------------------------------------------------------------------------------------------------------- experts
@functools.lru_cache(maxsize=None)
def _weights(E, I, dtype):
    g = torch.Generator().manual_seed(E * 1000 + I)
    gate_up = (torch.randn((E, 2 * I, H), generator=g) * 0.08).to(dtype).cuda()
    down = (torch.randn((E, H, I), generator=g) * 0.08).to(dtype).cuda()
    return gate_up, down


@functools.lru_cache(maxsize=None)
def _case(kind, N, E, K, I, dtype):
    """x, the plan of the kernels, the fp64 reference (computed once per case and shared)."""
    moe = _moe()
    logits, _ = _logits(kind, N, E, K, dtype)
    x = torch.randn((N, H), generator=torch.Generator().manual_seed(N + E + I)).to(dtype).cuda()
    gate_up, down = _weights(E, I, dtype)
    plan = moe.route(logits, K, True, dtype == torch.float16 and E == 60)       # (round_weights on in one of the families)
    ref = R.experts_ref(x, plan.idx.long(), plan.w, gate_up, down)
    return x, logits, plan, ref


EXPERT_CASES = [("tied", 5), ("counts", 64), ("one", 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("I", [96, 128])
@pytest.mark.parametrize("E,K", EK)
@pytest.mark.parametrize("kind,N", EXPERT_CASES)
def test_experts_within_twice_the_torch_loops_error(kind, N, E, K, I, dtype):
    moe = _moe()
    x, logits, plan, ref = _case(kind, N, E, K, I, dtype)
    gate_up, down = _weights(E, I, dtype)
    got = moe.experts(x, plan, gate_up, down)
    loop = moe.experts_torch(x, plan, gate_up, down)
    assert got.dtype == dtype and tuple(got.shape) == (N, H) and torch.isfinite(got).all()
    rms = ref.pow(2).mean().sqrt().item()
    d_kernel = (got.double() - ref).abs().max().item() / rms
    d_loop = (loop.double() - ref).abs().max().item() / rms
    print(f"{kind} N={N} E={E} K={K} I={I} {dtype}: worst |y - y64| / rms: kernels {d_kernel:.4g}, torch loop {d_loop:.4g}")
    assert d_kernel <= 2.0 * d_loop, (d_kernel, d_loop)
    out = torch.full((N, H), float("nan"), dtype=dtype, device="cuda")
    assert moe.experts(x, plan, gate_up, down, out=out) is out and _same(out, got)          # two calls: the same bits


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("E,K,I", [(8, 2, 96), (128, 8, 128)])
def test_a_tokens_bits_do_not_depend_on_the_batch(E, K, I, dtype):
    moe = _moe()
    N = 64
    x, logits, _, _ = _case("counts", N, E, K, I, dtype)
    gate_up, down = _weights(E, I, dtype)
    got = moe.experts(x, moe.route(logits, K, True, False), gate_up, down)
    assert _same(moe.experts(x, moe.route(logits, K, True, False), gate_up, down), got)         # two calls
    for n in (0, 1, 16, 17, 40, 63):                                        # alone: N = 1, one row per tile
        one = moe.experts(x[n:n + 1], moe.route(logits[n:n + 1], K, True, False), gate_up, down)
        assert _same(one[0], got[n]), n
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3)).cuda()
    shuffled = moe.experts(x[perm].contiguous(), moe.route(logits[perm].contiguous(), K, True, False), gate_up, down)
    assert _same(shuffled, got[perm])
    few = moe.experts(x[8:13], moe.route(logits[8:13], K, True, False), gate_up, down)          # another N, other tiles
    assert _same(few, got[8:13])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_block_replayed_from_a_graph_equals_the_eager_call(dtype):
    moe = _moe()
    torch.manual_seed(11)
    block = moe.SparseMoeBlock(H, 96, 60, 4, norm_topk=True, round_weights=True).to(dtype).cuda().eval()
    with torch.no_grad():
        block.gate.weight.normal_(0.0, 0.3)
        block.experts.gate_up_proj.normal_(0.0, 0.08)
        block.experts.down_proj.normal_(0.0, 0.08)
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
        # the policy: more tokens than kernel_max_tokens take the torch loop outside a capture, the kernels inside one
        x2 = xs[1].view(3, H)
        logits = torch.nn.functional.linear(x2, block.gate.weight)
        gate_up, down = block.experts.gate_up_proj, block.experts.down_proj
        kern = moe.experts(x2, moe.route(logits, 4, True, True), gate_up, down)
        loop = moe.experts_torch(x2, moe.route_torch(logits, 4, True, True), gate_up, down)
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


# ------------------------------------------------------------------------------------------------------------------ models
MODEL_CASES = [("mixtral", torch.float16), ("qwen3_moe", torch.float16), ("mixtral", torch.bfloat16)]
MODEL_IDS = ["mixtral-fp16", "qwen3_moe-fp16", "mixtral-bf16"]


@functools.lru_cache(maxsize=None)
def _model(family, dtype):
    return M.build(family, 31 + len(family), dtype)


def _forced_logits(model, ids, forced):
    logits, past = model(ids)
    out = [logits]
    for s in range(forced.shape[0]):
        logits, past = model(forced[s], past)
        out.append(logits)
    return out, past


@pytest.mark.parametrize("family,dtype", MODEL_CASES, ids=MODEL_IDS)
def test_sparse_models_generate_graphed_and_continuous(family, dtype):
    from kivi_amd.llama import MLP
    from kivi_amd.moe import SparseMoeBlock
    import test_admit_gpu as AD
    model = _model(family, dtype)
    kinds = [type(layer.mlp) for layer in model.model.layers]
    assert kinds == ([SparseMoeBlock, SparseMoeBlock] if family == "mixtral" else [MLP, SparseMoeBlock])
    sparse = model.model.layers[1].mlp
    assert sparse.kernel and sparse.round_weights == (family == "qwen3_moe") and sparse.experts.gate_up_proj.dtype == dtype
    ids = M.prompts(3, 2, T0)
    eager = model.generate(ids, STEPS)
    graphed = model.generate_graphed(ids, STEPS)
    assert torch.equal(eager, graphed)
    eager_steps, captures, replays = model.graphs.stats
    assert model.graphs.whole and captures >= 1 and replays >= STEPS - 2 * captures - 4, model.graphs.stats
    assert eager.shape == (2, T0 + STEPS) and int(eager.min()) >= 0 and int(eager.max()) < M.VOCAB
    model.release_graphs()
    g = torch.Generator().manual_seed(9)
    lens, limits = [21, 5, 33, 47, 12], [4, 30, 9, 12, 6]
    prompts = [torch.randint(1, M.VOCAB, (n,), generator=g).tolist() for n in lens]
    want, landed = AD._restate(model, prompts, limits, 3)
    out = model.generate_continuous(prompts, limits, 3)
    assert [o.tolist() for o in out] == want and len(landed) > 3
    out = model.generate_continuous(prompts, limits, 3, graphed=True)
    assert [o.tolist() for o in out] == want
    model.release_graphs()


@pytest.mark.parametrize("family,dtype", MODEL_CASES[:2], ids=MODEL_IDS[:2])
def test_logits_with_the_kernels_against_the_torch_loop(family, dtype):
    on = _model(family, dtype)
    off = M.twin(family, on, moe_kernel=False)
    assert on.model.layers[1].mlp.kernel and not off.model.layers[1].mlp.kernel
    ids = M.prompts(4, 2, T0)
    forced = torch.randint(1, M.VOCAB, (STEPS, 2, 1), generator=torch.Generator().manual_seed(5)).cuda()
    a, _ = _forced_logits(on, ids, forced)
    b, _ = _forced_logits(off, ids, forced)
    worst = 0.0
    for s, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all()
        rms = y.float().pow(2).mean().sqrt().item()
        d = (x.float() - y.float()).abs().max().item() / rms
        worst = max(worst, d)
        assert d <= (1e-2 if s == 0 else 5e-2), (s, d)             # tests/test_qwen_gpu.py
    print(f"{family}: worst |kernels - torch loop| / rms over {STEPS} steps = {worst:.3g}")


def _hf_names(state, family):
    """The state dict with the sparse blocks under HF's per-expert checkpoint names."""
    out = {}
    for name, t in state.items():
        if ".mlp.experts." in name:
            prefix = name[: name.index(".mlp.experts.")]
            mid = ".block_sparse_moe.experts." if family == "mixtral" else ".mlp.experts."
            gname, uname, dname = ("w1", "w3", "w2") if family == "mixtral" else ("gate_proj", "up_proj", "down_proj")
            for e in range(t.shape[0]):
                if name.endswith("gate_up_proj"):
                    inter = t.shape[1] // 2
                    out[f"{prefix}{mid}{e}.{gname}.weight"] = t[e, :inter].contiguous()
                    out[f"{prefix}{mid}{e}.{uname}.weight"] = t[e, inter:].contiguous()
                else:
                    out[f"{prefix}{mid}{e}.{dname}.weight"] = t[e].contiguous()
        elif name.endswith(".mlp.gate.weight") and family == "mixtral":
            out[name.replace(".mlp.", ".block_sparse_moe.")] = t
        else:
            out[name] = t
    return out


@pytest.mark.parametrize("family", ["mixtral", "qwen3_moe"])
def test_from_pretrained_takes_hfs_per_expert_names(family, tmp_path):
    st = pytest.importorskip("safetensors.torch")
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    model = M.build(family, 61)
    state = _hf_names({k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}, family)
    assert not any(k.endswith("gate_up_proj") for k in state)
    assert ("model.layers.1.block_sparse_moe.experts.7.w3.weight" if family == "mixtral"
            else "model.layers.1.mlp.experts.15.up_proj.weight") in state
    st.save_file(state, str(tmp_path / "model.safetensors"))
    (tmp_path / "config.json").write_text(json.dumps(M.config_dict(family)))
    loaded = LlamaForCausalLM_KIVI.from_pretrained(str(tmp_path), residual_length=32)
    assert type(loaded) is M.classes()[family] and loaded.model.layers[1].mlp.kernel
    for x, y in zip(model.model.layers, loaded.model.layers):     # the rotary frequencies are no part of a checkpoint
        x.self_attn.inv_freq = y.self_attn.inv_freq.clone()
    ids = M.prompts(6, 2, T0)
    forced = torch.randint(1, M.VOCAB, (8, 2, 1), generator=torch.Generator().manual_seed(7)).cuda()
    a, _ = _forced_logits(model, ids, forced)
    b, _ = _forced_logits(loaded, ids, forced)
    for s, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), s
