"""The contract of the sparse expert block (kivi_amd/moe.py) restated in fp64 on the exact fp16 / bf16 / fp32
inputs, shared by tests/test_moe_cpu.py and tests/test_moe_gpu.py: a stable descending sort of the logits (equal logits to the lower
expert), an fp64 softmax over all experts, SwiGLU per pair, the weighted sum over a token's slots.  Nothing here is rounded except,
with `round_weights`, the routing weights -- to the logits' dtype, as the contract says.  Also the crafted router logits of the GPU
tests (`crafted_logits`) and the check of a grouped plan (`check_plan`)."""
import torch


def route_ref(logits: torch.Tensor, top_k: int, norm_topk: bool, round_weights: bool):
    """-> idx (N, K) int64, w (N, K) fp64, on the logits' device."""
    l64 = logits.double()
    idx = torch.sort(l64 + 0.0, dim=-1, descending=True, stable=True).indices[:, :top_k]
    w = torch.softmax(l64, dim=-1).gather(1, idx)
    if norm_topk:
        w = w / w.sum(-1, keepdim=True)
    if round_weights:
        w = w.to(logits.dtype).double()
    return idx, w


def experts_ref(x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, gate_up: torch.Tensor, down: torch.Tensor) -> torch.Tensor:
    """out (N, H) fp64 = sum_k w[n, k] * down_e(silu(gate_e x[n]) * up_e x[n]), e = idx[n, k], every operation in fp64."""
    x64, w64 = x.double(), w.double()
    E, I = down.shape[0], down.shape[2]
    out = torch.zeros_like(x64)
    for e in range(E):
        tok, slot = torch.where(idx == e)
        if tok.numel() == 0:
            continue
        gu = x64[tok] @ gate_up[e].double().T
        g, u = gu[:, :I], gu[:, I:]
        y = (g * torch.sigmoid(g) * u) @ down[e].double().T
        out.index_add_(0, tok, y * w64[tok, slot, None])
    return out


def block_ref(x, gate_w, gate_up, down, top_k, norm_topk, round_weights):
    """The whole block in fp64 from x (N, H): the router GEMM in fp64 too (for the fp32 CPU comparison, where logits are not rounded)."""
    logits = x.double() @ gate_w.double().T
    idx, w = route_ref(logits, top_k, norm_topk, False)
    if round_weights:
        w = w.to(x.dtype).double()
    return experts_ref(x, idx, w, gate_up, down)


def ulp_of(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The spacing of `dtype` at |ref| (fp64), subnormal spacing at the bottom."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    _, ex = torch.frexp(ref.abs().clamp_min(1e-300))            # |ref| = m * 2^ex, m in [0.5, 1)
    return torch.pow(2.0, (ex - 1).clamp_min(emin).double() - mant)


def crafted_assignment(N: int, E: int, K: int, kind: str, tile: int) -> torch.Tensor:
    """(N, K) int64 experts per token, distinct inside a token.  `counts`: expert 0 receives no pair, experts 1..4 exactly 1, tile,
    tile + 1 and 2 * tile + 1, the others the rest (needs N >= 2 * tile + 1, N * K >= 4 * tile + 3, E >= K + 5).  `one`: expert 3 is
    every token's first choice, the other slots walk the remaining experts."""
    a = torch.empty((K, N), dtype=torch.int64)
    if kind == "one":
        for j in range(K):
            a[j] = 3 if j == 0 else (torch.arange(N) + 4 + j * 7) % E
        for j in range(1, K):                                   # keep the walk off expert 3 and off earlier slots
            for n in range(N):
                e = int(a[j, n])
                while e == 3 or e in a[:j, n].tolist():
                    e = (e + 1) % E
                a[j, n] = e
        return a.T.contiguous()
    assert kind == "counts" and N >= 2 * tile + 1 and N * K >= 4 * tile + 3 and E >= K + 5
    flat = a.view(-1)                                           # slot s = layer (s // N), token (s % N)
    layer = torch.arange(N * K) // N
    flat.copy_(5 + layer)                                       # the fillers: one expert per layer, so a token's are distinct
    s = 0
    for e, c in ((1, 1), (2, tile), (3, tile + 1), (4, 2 * tile + 1)):
        flat[s:s + c] = e                                       # c <= N consecutive slots: c distinct tokens
        s += c
    return a.T.contiguous()


def crafted_logits(assign: torch.Tensor, E: int, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """Router logits (N, E) whose K largest entries of row n are assign[n, :] in that order: the chosen experts at 8, 7.5, 7, ...,
    every other expert at a random multiple of 1 / 4 in [-4, 0) -- plenty of equal logits outside the top."""
    N, K = assign.shape
    g = torch.Generator().manual_seed(seed)
    lg = -torch.randint(1, 17, (N, E), generator=g).double() / 4
    lg.scatter_(1, assign, (8.0 - 0.5 * torch.arange(K, dtype=torch.float64)).expand(N, K).contiguous())
    return lg.to(dtype)


def tied_logits(N: int, E: int, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """Random logits on a grid of 1 / 2 (so most rows hold equal logits inside their top), row 0 all equal, row 1 (when there is one)
    zeros of both signs, which are equal."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randint(-6, 7, (N, E), generator=g).double() / 2
    lg[0] = 1.25
    if N > 1:
        lg[1] = 0.0
        lg[1, ::2] = -0.0
    return lg.to(dtype)


def check_plan(plan, idx_ref: torch.Tensor, tile: int) -> None:
    """counts / offsets exact; every expert's segment of `pairs` exactly its set of pairs; pos inverts pairs; the tile list covers each
    segment once, in tiles of at most `tile` rows, inside the bound."""
    N, K = idx_ref.shape
    E = plan.num_experts
    idx = idx_ref.cpu()
    counts = torch.bincount(idx.reshape(-1), minlength=E)
    assert torch.equal(plan.counts.cpu().long(), counts)
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    assert torch.equal(plan.offsets.cpu().long(), offsets)
    pairs, pos = plan.pairs.cpu().long(), plan.pos.cpu().long().reshape(-1)
    assert torch.equal(pairs.sort().values, torch.arange(N * K))
    assert torch.equal(pairs[pos], torch.arange(N * K))
    seg = torch.repeat_interleave(torch.arange(E), counts)                  # the expert owning each row of `pairs`
    assert torch.equal(idx.reshape(-1)[pairs], seg)
    if plan.tiles is None:
        return
    nt = int(plan.n_tiles.cpu()[0])
    assert nt == int(((counts + tile - 1) // tile).sum()) and nt <= plan.tiles.shape[0]
    assert plan.tiles.shape[0] == min(E, N * K) + N * K // tile
    tiles = plan.tiles.cpu().long()[:nt]
    covered = torch.zeros(N * K, dtype=torch.int64)
    for e, first, rows in tiles.tolist():
        assert 1 <= rows <= tile and offsets[e] <= first and first + rows <= offsets[e + 1], (e, first, rows)
        covered[first:first + rows] += 1
    assert bool((covered == 1).all())
