"""The sparse mixture-of-experts feed-forward block of Mixtral / Qwen3-MoE: a router over E experts, K of them
per token, each a SwiGLU MLP.  `route` / `experts` are the two HIP entries kivi_moe_route / kivi_moe_experts
(kivi_amd/csrc/kivi_moe.hip): launches only, nothing is read back, so a captured decode step may hold them.  `route_torch` /
`experts_torch` state the same contract in torch -- the per-expert loop of the Hugging Face modules, whose `nonzero` / `where`
synchronise with the host -- for tensors off the GPU, shapes the kernels refuse and passes of many tokens.  `SparseMoeBlock` is the
module the decoder layers carry as `mlp`; with `expert_bits=4` its experts are a `QuantExperts` -- the stacked matrices packed by
kivi_w4_pack -- and every call takes `experts_w4_torch`, the loop with each hit expert dequantised first.
With `expert_fp8=True` they are an `Fp8Experts` -- a checkpoint's own e4m3fn bytes and fp32 block scales -- served
by `experts_w8`, the HIP entry kivi_moe_experts_w8 (launches only, capturable), and by `experts_w8_torch`, the dequantising loop.

The contract: token n's experts are the K largest router LOGITS, descending, equal logits to the lower expert (a choice that is
decidable from the inputs; HF's top-k over the fp32 probabilities picks the same experts wherever two probabilities differ); its
weights are the fp32 softmax over all E logits at those experts, divided by their sum with `norm_topk`, rounded once to the logits'
dtype with `round_weights`; out[n] = sum_k w[n, k] * down_e(silu(gate_e(x[n])) * up_e(x[n])), e = idx[n, k]."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, wfp8, wquant

TOKEN_TILE = _lib.MOE_TOKEN_TILE        # pairs per tile of the grouped plan: include/kivi_hip.h, KIVI_MOE_TOKEN_TILE
MAX_EXPERTS, MAX_TOP_K = _lib.MOE_MAX_E, _lib.MOE_MAX_K
# Eager calls of more tokens than this take the torch loop (its GEMMs run on rocBLAS; a prompt pass of thousands of tokens belongs
# there).  The largest power of two at which tools/moe_time.py measured the kernels no slower than the loop at BOTH published
# geometries (profiles/moe_time.log, MI355X): at N = 64 they are 1.6-1.85x (Mixtral-8x7B) and 58-61x (Qwen3-30B-A3B) ahead, at the
# next measured size, 256, Mixtral's bf16 run is behind (0.84x; fp16 1.02x) while Qwen3's stay 38-44x ahead: a Qwen3-MoE user
# may raise it.
KERNEL_MAX_TOKENS = 64
# The same rule for a block of FP8 experts, whose loop dequantises every hit expert before its GEMMs.  From
# tools/moe_w8_time.py (profiles/moe_w8_time.log, MI355X): "crossover: w8 is no slower than the dequantising loop at both geometries
# (every dtype run) at N in [1, 8, 32, 64, 256]; the largest such N below the first N at which it loses somewhere (None): 256; worst
# loop / w8 per N: 1: 5.56, 8: 7.18, 32: 6.71, 64: 3.43, 256: 1.54" -- 256 is the largest size measured: at it the kernel is
# 1.54-1.58x (Mixtral-8x7B) and 72-74x (Qwen3-30B-A3B) ahead; nothing above it has been timed.
FP8_KERNEL_MAX_TOKENS = 256
_DTYPES = {torch.float16: 16, torch.bfloat16: _lib.LOGITS_BF16}


@dataclass
class MoePlan:
    """What route leaves on the device.  idx (N, K) int32, w (N, K) fp32; the grouped plan: counts (E), offsets (E + 1), pairs (N * K)
    -- pair id n * K + k, grouped by expert, in no specified order inside an expert --, pos (N, K) with pairs[pos[n, k]] == n * K + k,
    tiles (max_tiles, 3) rows (expert, first row of pairs, rows <= TOKEN_TILE) of which the first n_tiles[0] are written
    (route_torch leaves tiles / n_tiles None)."""
    idx: torch.Tensor
    w: torch.Tensor
    counts: torch.Tensor
    offsets: torch.Tensor
    pairs: torch.Tensor
    pos: torch.Tensor
    tiles: Optional[torch.Tensor]
    n_tiles: Optional[torch.Tensor]
    num_experts: int

    @property
    def top_k(self) -> int:
        return self.idx.shape[1]


def max_tiles(n_tokens: int, num_experts: int, top_k: int) -> int:
    """The bound the expert launches are sized by: min(E, N * K) + N * K // TOKEN_TILE (kivi_amd/csrc/kivi_moe_plan.h)."""
    return min(num_experts, n_tokens * top_k) + n_tokens * top_k // TOKEN_TILE


def _check_route(logits: torch.Tensor, top_k: int, what: str):
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise ValueError(f"{what}: logits must be (N >= 1, E), got {tuple(logits.shape)}")
    E = logits.shape[1]
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
        raise ValueError(f"{what}: top_k has to be an integer in [1, E = {E}], got {top_k!r}")


def usable(x: torch.Tensor, num_experts: int, top_k: int, hidden: int, intermediate: int) -> bool:
    """True where the kernels serve: fp16 or bf16 on the GPU, E <= 256, K <= min(E, 16), H and I multiples of 32, N * K < 2^31."""
    n = x.numel() // max(hidden, 1)
    return (x.is_cuda and x.dtype in _DTYPES and 1 <= num_experts <= MAX_EXPERTS and 1 <= top_k <= min(num_experts, MAX_TOP_K)
            and hidden >= 32 and hidden % 32 == 0 and intermediate >= 32 and intermediate % 32 == 0 and 1 <= n
            and n * top_k < 2 ** 31 and hidden <= 16 * 65535 and intermediate <= 16 * 65535)


def route_torch(logits: torch.Tensor, top_k: int, norm_topk: bool = True, round_weights: bool = False) -> MoePlan:
    """The contract of kivi_moe_route in torch, any dtype and device: a stable descending sort of the logits, the fp32 softmax (fp64
    for fp64 logits), the grouped plan by a stable sort of the pairs' experts (no tile list)."""
    _check_route(logits, top_k, "route_torch")
    N, E = logits.shape
    wide = logits if logits.dtype == torch.float64 else logits.float()
    idx = torch.sort(wide + 0.0, dim=-1, descending=True, stable=True).indices[:, :top_k]
    w = torch.softmax(wide, dim=-1).gather(1, idx)
    if norm_topk:
        w = w / w.sum(-1, keepdim=True)
    if round_weights:
        w = w.to(logits.dtype).to(wide.dtype)
    flat = idx.reshape(-1)
    counts = torch.zeros(E, dtype=torch.int64, device=logits.device).scatter_add_(0, flat, torch.ones_like(flat))
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    pairs = torch.sort(flat, stable=True).indices
    pos = torch.empty_like(pairs).scatter_(0, pairs, torch.arange(N * top_k, device=logits.device))
    return MoePlan(idx.int(), w, counts.int(), offsets.int(), pairs.int(), pos.view(N, top_k).int(), None, None, E)


def experts_torch(x: torch.Tensor, plan: MoePlan, gate_up: torch.Tensor, down: torch.Tensor) -> torch.Tensor:
    """The expert stage in torch, statement for statement the loop of HF's MixtralExperts / Qwen3MoeExperts: for every expert that
    received a pair, its tokens through gate_up and down in x's dtype, times the weight, index_add_ into the result.  x (N, H),
    gate_up (E, 2 I, H), down (E, H, I) -> (N, H).  Synchronises (nonzero / where)."""
    E = gate_up.shape[0]
    out = torch.zeros_like(x)
    idx, w = plan.idx.long(), plan.w
    mask = F.one_hot(idx, num_classes=E).permute(2, 1, 0)
    hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
    for e in hit:
        e = e[0]
        k_pos, tok = torch.where(mask[e])
        g, u = F.linear(x[tok], gate_up[e]).chunk(2, dim=-1)
        y = F.linear(F.silu(g) * u, down[e])
        y = y * w[tok, k_pos, None]
        out.index_add_(0, tok, y.to(out.dtype))
    return out


def route(logits: torch.Tensor, top_k: int, norm_topk: bool = True, round_weights: bool = False) -> MoePlan:
    """One kivi_moe_route call (a memset and two launches on the current stream).  logits (N, E) fp16 or bf16 on the GPU with unit
    expert stride (a view with a row stride is read as it is)."""
    _check_route(logits, top_k, "kivi_moe_route")
    _lib.require_gpu(logits, "logits")
    if logits.dtype not in _DTYPES or logits.stride(1) != 1:
        raise ValueError(f"kivi_moe_route: logits must be fp16 or bf16 with unit expert stride, got {logits.dtype}, strides "
                         f"{logits.stride()}")
    N, E = logits.shape
    if E > MAX_EXPERTS or top_k > MAX_TOP_K or N * top_k >= 2 ** 31:
        raise ValueError(f"kivi_moe_route: E = {E} (<= {MAX_EXPERTS}), top_k = {top_k} (<= {MAX_TOP_K}), N * top_k = {N * top_k} "
                         f"(< 2^31)")
    dev = logits.device
    i32 = dict(dtype=torch.int32, device=dev)
    plan = MoePlan(torch.empty((N, top_k), **i32), torch.empty((N, top_k), dtype=torch.float32, device=dev), torch.empty(E, **i32),
                   torch.empty(E + 1, **i32), torch.empty(N * top_k, **i32), torch.empty((N, top_k), **i32),
                   torch.empty((max_tiles(N, E, top_k), 3), **i32), torch.empty(1, **i32), E)
    flags = (_lib.MOE_NORM_TOPK if norm_topk else 0) | (_lib.MOE_ROUND_WEIGHTS if round_weights else 0)
    rc = _lib.load().kivi_moe_route(
        logits.data_ptr(), logits.stride(0), _DTYPES[logits.dtype], N, E, top_k, flags, plan.idx.data_ptr(), plan.w.data_ptr(),
        plan.counts.data_ptr(), plan.offsets.data_ptr(), plan.pairs.data_ptr(), plan.pos.data_ptr(), plan.tiles.data_ptr(),
        plan.n_tiles.data_ptr(), _lib.stream_ptr(logits))
    _lib.check(rc, "kivi_moe_route")
    return plan


def experts(x: torch.Tensor, plan: MoePlan, gate_up: torch.Tensor, down: torch.Tensor, out: Optional[torch.Tensor] = None
            ) -> torch.Tensor:
    """One kivi_moe_experts call (three launches).  x (N, H) with unit channel stride, gate_up (E, 2 I, H) and down (E, H, I)
    contiguous, all of one dtype (fp16 or bf16) on the GPU; `plan`: route's for the same N.  -> (N, H) in the dtype; `out`: a
    contiguous buffer of that shape to write into.  The workspace (N * K rows of I activations and of H fp32 outputs) is allocated
    per call: under capture it belongs to the graph's pool."""
    for t, name in ((x, "x"), (gate_up, "gate_up"), (down, "down")):
        _lib.require_gpu(t, name)
    if x.dim() != 2 or gate_up.dim() != 3 or down.dim() != 3:
        raise ValueError(f"kivi_moe_experts: x (N, H), gate_up (E, 2 I, H), down (E, H, I), got {tuple(x.shape)}, "
                         f"{tuple(gate_up.shape)}, {tuple(down.shape)}")
    N, H = x.shape
    E, I = down.shape[0], down.shape[2]
    if tuple(gate_up.shape) != (E, 2 * I, H) or tuple(down.shape) != (E, H, I) or E != plan.num_experts:
        raise ValueError(f"kivi_moe_experts: x {tuple(x.shape)}, gate_up {tuple(gate_up.shape)}, down {tuple(down.shape)} and a plan "
                         f"over {plan.num_experts} experts do not go together")
    if x.dtype not in _DTYPES or gate_up.dtype != x.dtype or down.dtype != x.dtype:
        raise ValueError(f"kivi_moe_experts: x, gate_up and down share one dtype, fp16 or bf16, got {x.dtype}, {gate_up.dtype}, "
                         f"{down.dtype}")
    if not gate_up.is_contiguous() or not down.is_contiguous() or x.stride(1) != 1:
        raise ValueError("kivi_moe_experts: gate_up and down must be contiguous, x of unit channel stride")
    if plan.tiles is None or tuple(plan.idx.shape) != (N, plan.top_k) or not plan.idx.is_cuda:
        raise ValueError(f"kivi_moe_experts: the plan must be route()'s for these {N} tokens")
    if x.stride(0) % 8 or x.data_ptr() % 16:
        x = x.contiguous()
    if out is None:
        out = torch.empty((N, H), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (N, H) or out.dtype != x.dtype or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"kivi_moe_experts: out must be contiguous {x.dtype} {(N, H)} on the GPU")
    lib = _lib.load()
    K = plan.top_k
    nbytes = lib.kivi_moe_workspace_bytes(N, H, I, E, K)
    if nbytes < 0:
        _lib.check(-1, "kivi_moe_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = lib.kivi_moe_experts(
        x.data_ptr(), x.stride(0), _DTYPES[x.dtype], N, H, I, E, K, plan.w.data_ptr(), plan.pairs.data_ptr(), plan.pos.data_ptr(),
        plan.tiles.data_ptr(), plan.n_tiles.data_ptr(), gate_up.data_ptr(), down.data_ptr(), out.data_ptr(), out.stride(0),
        ws.data_ptr(), nbytes, _lib.stream_ptr(x))
    _lib.check(rc, "kivi_moe_experts")
    return out


class _QuantStack(nn.Module):
    """The three buffers of E packed matrices (rows, cols) under QuantLinear's names: qweight (E, rows / 16, cols / 128, 256) int32,
    scales and mins (E, rows / 16, cols / G, 16) int16 -- fp16 bit patterns, which .half() / .bfloat16() cannot re-round."""

    def __init__(self, num_experts: int, rows: int, cols: int, group: int):
        super().__init__()
        qs, ss, ms = wquant.shapes(rows, cols, group)
        self.register_buffer("qweight", torch.zeros((num_experts, *qs), dtype=torch.int32))
        self.register_buffer("scales", torch.zeros((num_experts, *ss), dtype=torch.int16))
        self.register_buffer("mins", torch.zeros((num_experts, *ms), dtype=torch.int16))

    @property
    def triple(self):
        return self.qweight, self.scales, self.mins


class QuantExperts(nn.Module):
    """The stacked experts in 4 bits in `_Experts`' place: gate_up_proj and down_proj each hold qweight /
    scales / mins, slab e of which is exactly wquant.pack of expert e's (2 I, H) gate_up and (H, I) down matrix (section 30's
    quantiser and layout: I is a multiple of 16, so the gate stripes followed by the up stripes are the stripes of the (2 I, H)
    matrix).  No dense expert parameter exists."""

    def __init__(self, num_experts: int, hidden: int, intermediate: int, group: int = 128):
        super().__init__()
        if group not in wquant.GROUPS:
            raise ValueError(f"expert_group has to be one of {wquant.GROUPS}, got {group!r}")
        if hidden < wquant.K_TILE or hidden % wquant.K_TILE:
            raise ValueError(f"4-bit experts need hidden_size to be a positive multiple of {wquant.K_TILE}, got {hidden}")
        if intermediate < wquant.K_TILE or intermediate % wquant.K_TILE:
            raise ValueError(f"4-bit experts need the experts' intermediate_size to be a positive multiple of {wquant.K_TILE}, got "
                             f"{intermediate}")
        self.num_experts, self.hidden, self.intermediate, self.group = num_experts, hidden, intermediate, group
        self.gate_up_proj = _QuantStack(num_experts, 2 * intermediate, hidden, group)
        self.down_proj = _QuantStack(num_experts, hidden, intermediate, group)

    def extra_repr(self) -> str:
        return f"num_experts={self.num_experts}, hidden={self.hidden}, intermediate={self.intermediate}, group={self.group}"

    def slab(self, e: int, part: str):
        """The views (qweight, scales, mins) that hold `part` (gate, up, gate_up or down) of expert e: contiguous."""
        s = self.intermediate // wquant.ROW_TILE
        if part not in ("gate", "up", "gate_up", "down"):
            raise ValueError(f"part has to be gate, up, gate_up or down, got {part!r}")
        if not 0 <= e < self.num_experts:
            raise ValueError(f"expert {e} outside [0, {self.num_experts})")
        if part == "down":
            return tuple(t[e] for t in self.down_proj.triple)
        a, b = {"gate": (0, s), "up": (s, 2 * s), "gate_up": (0, 2 * s)}[part]
        return tuple(t[e, a:b] for t in self.gate_up_proj.triple)

    def shape_of(self, part: str):
        I, H = self.intermediate, self.hidden
        return {"gate": (I, H), "up": (I, H), "gate_up": (2 * I, H), "down": (H, I)}[part]

    def pack_expert_(self, e: int, part: str, weight: torch.Tensor, name: str = "weight") -> "QuantExperts":
        """Quantise `weight` -- the gate, up (I, H), gate_up (2 I, H) or down (H, I) matrix of expert e, fp16 or bf16 on the module's
        GPU -- straight into the expert's slab: one kivi_w4_pack launch."""
        views = self.slab(e, part)
        if weight.dtype not in _DTYPES:
            raise ValueError(f"{name}: 4-bit experts are packed from torch.float16 or torch.bfloat16 weights, got {weight.dtype}")
        if tuple(weight.shape) != self.shape_of(part):
            raise ValueError(f"{name}: shape {tuple(weight.shape)} does not fit the {part} matrix {self.shape_of(part)}")
        wquant.pack(weight, self.group, name, out=views)
        return self

    def load_ref_(self, e: int, part: str, code: torch.Tensor, scale: torch.Tensor, mn: torch.Tensor) -> "QuantExperts":
        """Put the reference's triple of a matrix (wquant.quantize_ref) into the expert's slab, on any device."""
        for view, t in zip(self.slab(e, part), wquant.from_ref(code, scale, mn, self.group)):
            view.copy_(t)
        return self

    def dequant_expert(self, e: int, dtype=torch.float16, out=None):
        """-> (gate_up (2 I, H), down (H, I)) of expert e in `dtype`: kivi_w4_dequant on the GPU, wquant.dequant_torch elsewhere.
        `out`: a pair of contiguous buffers of those shapes to write into."""
        res = []
        for i, part in enumerate(("gate_up", "down")):
            views = self.slab(e, part)
            buf = None if out is None else out[i]
            if views[0].is_cuda:
                if dtype not in _DTYPES:
                    raise ValueError(f"4-bit experts on the GPU serve torch.float16 and torch.bfloat16, got {dtype}")
                res.append(wquant.dequant(*views, dtype=dtype, out=buf))
            else:
                t = wquant.dequant_torch(*views, dtype=dtype)
                res.append(t if buf is None else buf.copy_(t))
        return tuple(res)

    @classmethod
    def from_dense(cls, gate_up: torch.Tensor, down: torch.Tensor, group: int = 128) -> "QuantExperts":
        """Quantise stacked dense experts gate_up (E, 2 I, H), down (E, H, I): on the GPU (fp16 or bf16) one kivi_w4_pack launch per
        matrix, elsewhere wquant.quantize_ref."""
        E, H, I = down.shape
        if tuple(gate_up.shape) != (E, 2 * I, H):
            raise ValueError(f"from_dense: gate_up {tuple(gate_up.shape)} and down {tuple(down.shape)} do not go together")
        with torch.device(down.device):
            m = cls(E, H, I, group)
        for e in range(E):
            for part, w in (("gate_up", gate_up[e]), ("down", down[e])):
                if w.is_cuda:
                    m.pack_expert_(e, part, w.detach(), f"experts.{part}[{e}]")
                else:
                    m.load_ref_(e, part, *wquant.quantize_ref(w.detach(), group))
        return m


def experts_w4_torch(x: torch.Tensor, plan: MoePlan, qexperts: QuantExperts) -> torch.Tensor:
    """experts_torch over 4-bit experts, on any device: every expert that received a pair is dequantised to x's dtype into
    wquant's shared scratch before its two F.linear's.  Synchronises."""
    E, H, I = qexperts.num_experts, qexperts.hidden, qexperts.intermediate
    out = torch.zeros_like(x)
    idx, w = plan.idx.long(), plan.w
    mask = F.one_hot(idx, num_classes=E).permute(2, 1, 0)
    hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
    buf = wquant._scratch(x.device, x.dtype, 3 * I, H)
    bufs = (buf[: 2 * I], buf[2 * I:].view(H, I))
    for e in hit:
        e = e[0]
        k_pos, tok = torch.where(mask[e])
        gate_up, down = qexperts.dequant_expert(int(e), x.dtype, bufs)
        g, u = F.linear(x[tok], gate_up).chunk(2, dim=-1)
        y = F.linear(F.silu(g) * u, down)
        y = y * w[tok, k_pos, None]
        out.index_add_(0, tok, y.to(out.dtype))
    return out


class Fp8Experts(nn.Module):
    """The stacked experts in FP8 in `_Experts`' place: the four buffers of transformers' FP8Experts under its
    names, holding a checkpoint's own bytes -- gate_up_proj (E, 2 I, H) and down_proj (E, H, I) uint8 (e4m3fn, gate rows first), and
    gate_up_proj_scale_inv (E, 2 I / 128, H / 128), down_proj_scale_inv (E, H / 128, I / 128) int32: the bit patterns of the fp32
    block scales, which .half() / .bfloat16() cannot re-round (Fp8Linear's reason).  H and I are positive multiples of 128, so the
    block grid of the stacked (2 I, H) matrix is the gate's followed by the up's.  No dense expert parameter exists."""

    def __init__(self, num_experts: int, hidden: int, intermediate: int):
        super().__init__()
        if hidden < wfp8.BLOCK or hidden % wfp8.BLOCK:
            raise ValueError(f"FP8 experts need hidden_size to be a positive multiple of {wfp8.BLOCK}, got {hidden}")
        if intermediate < wfp8.BLOCK or intermediate % wfp8.BLOCK:
            raise ValueError(f"FP8 experts need the experts' intermediate_size to be a positive multiple of {wfp8.BLOCK}, got "
                             f"{intermediate}")
        if not 1 <= num_experts <= MAX_EXPERTS:
            raise ValueError(f"FP8 experts need num_experts in [1, {MAX_EXPERTS}], got {num_experts}")
        self.num_experts, self.hidden, self.intermediate = num_experts, hidden, intermediate
        E, H, I, B = num_experts, hidden, intermediate, wfp8.BLOCK
        self.register_buffer("gate_up_proj", torch.zeros((E, 2 * I, H), dtype=torch.uint8))
        self.register_buffer("gate_up_proj_scale_inv", torch.zeros((E, 2 * I // B, H // B), dtype=torch.int32))
        self.register_buffer("down_proj", torch.zeros((E, H, I), dtype=torch.uint8))
        self.register_buffer("down_proj_scale_inv", torch.zeros((E, H // B, I // B), dtype=torch.int32))

    def extra_repr(self) -> str:
        return f"num_experts={self.num_experts}, hidden={self.hidden}, intermediate={self.intermediate}, fp8=e4m3fn [128, 128]"

    def shape_of(self, part: str):
        I, H = self.intermediate, self.hidden
        return {"gate": (I, H), "up": (I, H), "gate_up": (2 * I, H), "down": (H, I)}[part]

    def slab(self, e: int, part: str):
        """The views (bytes uint8, scale bits int32) that hold `part` (gate, up, gate_up or down) of expert e: contiguous."""
        if part not in ("gate", "up", "gate_up", "down"):
            raise ValueError(f"part has to be gate, up, gate_up or down, got {part!r}")
        if not 0 <= e < self.num_experts:
            raise ValueError(f"expert {e} outside [0, {self.num_experts})")
        if part == "down":
            return self.down_proj[e], self.down_proj_scale_inv[e]
        I = self.intermediate
        a, b = {"gate": (0, I), "up": (I, 2 * I), "gate_up": (0, 2 * I)}[part]
        return self.gate_up_proj[e, a:b], self.gate_up_proj_scale_inv[e, a // wfp8.BLOCK:b // wfp8.BLOCK]

    def load_expert_(self, e: int, part: str, weight_fp8: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                     name: str = "weight") -> "Fp8Experts":
        """Take a checkpoint's tensors of `part` of expert e as they are, either or both: `weight_fp8` float8_e4m3fn is checked for
        NaN bytes and copied as bytes; `scale`, fp32, is checked to be finite and copied as bits, a per-tensor scalar expanded to
        the grid.  Refusals are ValueErrors by `name`."""
        try:
            wv, sv = self.slab(e, part)
        except ValueError as err:
            raise ValueError(f"{name}: {err}") from None
        O, K = self.shape_of(part)
        if weight_fp8 is not None:
            if tuple(weight_fp8.shape) != (O, K):
                raise ValueError(f"{name}: shape {tuple(weight_fp8.shape)} does not fit the {part} matrix {(O, K)}")
            wv.copy_(wfp8.as_bytes(weight_fp8, name))
        if scale is not None:
            sv.copy_(wfp8.as_scale(scale, O, K, name).view(torch.int32))
        return self

    def quantize_expert_(self, e: int, part: str, weight16: torch.Tensor, name: str = "weight") -> "Fp8Experts":
        """Quantise `weight16` -- the gate, up (I, H), gate_up (2 I, H) or down (H, I) matrix of expert e -- on its device into the
        expert's slab (wfp8.quantize).  I is a multiple of 128: the stacked matrix quantises as gate and up apart."""
        try:
            wv, sv = self.slab(e, part)
        except ValueError as err:
            raise ValueError(f"{name}: {err}") from None
        if tuple(weight16.shape) != self.shape_of(part):
            raise ValueError(f"{name}: shape {tuple(weight16.shape)} does not fit the {part} matrix {self.shape_of(part)}")
        codes, inv = wfp8.quantize(weight16, name)
        if codes.device != wv.device:
            raise ValueError(f"{name}: the weight is on {codes.device}, the module on {wv.device}")
        wv.copy_(codes)
        sv.copy_(inv.view(torch.int32))
        return self

    def dequant_expert(self, e: int, dtype=torch.float16, out=None):
        """-> (gate_up (2 I, H), down (H, I)) of expert e in `dtype`: kivi_w8_dequant on the GPU, wfp8.dequant_torch (the same bits)
        elsewhere.  `out`: a pair of contiguous buffers of those shapes to write into."""
        res = []
        for i, part in enumerate(("gate_up", "down")):
            wv, sv = self.slab(e, part)
            buf = None if out is None else out[i]
            if wv.is_cuda:
                if dtype not in _DTYPES:
                    raise ValueError(f"FP8 experts on the GPU serve torch.float16 and torch.bfloat16, got {dtype}")
                res.append(wfp8.dequant(wv, sv, dtype=dtype, out=buf))
            else:
                t = wfp8.dequant_torch(wv, sv.view(torch.float32), dtype)
                res.append(t if buf is None else buf.copy_(t))
        return tuple(res)

    def dequant(self, dtype=torch.float16):
        """-> the dense stacks gate_up (E, 2 I, H), down (E, H, I) in `dtype` (what a dense twin of the block holds)."""
        pairs = [self.dequant_expert(e, dtype) for e in range(self.num_experts)]
        return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    @classmethod
    def from_dense(cls, gate_up: torch.Tensor, down: torch.Tensor) -> "Fp8Experts":
        """Quantise stacked dense experts gate_up (E, 2 I, H), down (E, H, I) on their device (wfp8.quantize per matrix)."""
        E, H, I = down.shape
        if tuple(gate_up.shape) != (E, 2 * I, H):
            raise ValueError(f"from_dense: gate_up {tuple(gate_up.shape)} and down {tuple(down.shape)} do not go together")
        with torch.device(down.device):
            m = cls(E, H, I)
        for e in range(E):
            m.quantize_expert_(e, "gate_up", gate_up[e].detach(), f"experts.gate_up[{e}]")
            m.quantize_expert_(e, "down", down[e].detach(), f"experts.down[{e}]")
        return m


def usable_w8(x: torch.Tensor, num_experts: int, top_k: int, hidden: int, intermediate: int) -> bool:
    """True where kivi_moe_experts_w8 serves: `usable`, with H and I multiples of 128."""
    return usable(x, num_experts, top_k, hidden, intermediate) and hidden % wfp8.BLOCK == 0 and intermediate % wfp8.BLOCK == 0


def experts_w8(x: torch.Tensor, plan: MoePlan, fp8experts: Fp8Experts, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One kivi_moe_experts_w8 call (three launches) over the four buffers of `fp8experts`.  x (N, H) fp16 or bf16 with unit channel
    stride on the GPU; `plan`: route's for the same N.  -> (N, H) in the dtype; `out`: a contiguous buffer of that shape to write
    into.  The workspace is kivi_moe_experts': allocated per call, under capture it belongs to the graph's pool."""
    _lib.require_gpu(x, "x")
    _lib.require_gpu(fp8experts.gate_up_proj, "gate_up_proj")
    E, H, I = fp8experts.num_experts, fp8experts.hidden, fp8experts.intermediate
    if x.dim() != 2 or x.shape[1] != H or E != plan.num_experts:
        raise ValueError(f"kivi_moe_experts_w8: x {tuple(x.shape)}, experts (E = {E}, H = {H}, I = {I}) and a plan over "
                         f"{plan.num_experts} experts do not go together")
    if x.dtype not in _DTYPES or x.stride(1) != 1:
        raise ValueError(f"kivi_moe_experts_w8: x must be fp16 or bf16 of unit channel stride, got {x.dtype}, strides {x.stride()}")
    bufs = (fp8experts.gate_up_proj, fp8experts.gate_up_proj_scale_inv, fp8experts.down_proj, fp8experts.down_proj_scale_inv)
    if [b.dtype for b in bufs] != [torch.uint8, torch.int32, torch.uint8, torch.int32] or not all(b.is_contiguous() for b in bufs):
        raise ValueError("kivi_moe_experts_w8: the experts' buffers must be contiguous uint8 bytes and int32 scale bits")
    N = x.shape[0]
    if plan.tiles is None or tuple(plan.idx.shape) != (N, plan.top_k) or not plan.idx.is_cuda:
        raise ValueError(f"kivi_moe_experts_w8: the plan must be route()'s for these {N} tokens")
    if x.stride(0) % 8 or x.data_ptr() % 16:
        x = x.contiguous()
    if out is None:
        out = torch.empty((N, H), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (N, H) or out.dtype != x.dtype or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"kivi_moe_experts_w8: out must be contiguous {x.dtype} {(N, H)} on the GPU")
    lib = _lib.load()
    K = plan.top_k
    nbytes = lib.kivi_moe_workspace_bytes(N, H, I, E, K)
    if nbytes < 0:
        _lib.check(-1, "kivi_moe_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = lib.kivi_moe_experts_w8(
        x.data_ptr(), x.stride(0), _DTYPES[x.dtype], N, H, I, E, K, plan.w.data_ptr(), plan.pairs.data_ptr(), plan.pos.data_ptr(),
        plan.tiles.data_ptr(), plan.n_tiles.data_ptr(), *(b.data_ptr() for b in bufs), out.data_ptr(), out.stride(0), ws.data_ptr(),
        nbytes, _lib.stream_ptr(x))
    _lib.check(rc, "kivi_moe_experts_w8")
    return out


def experts_w8_torch(x: torch.Tensor, plan: MoePlan, fp8experts: Fp8Experts) -> torch.Tensor:
    """experts_torch over FP8 experts, on any device: every expert that received a pair is dequantised to x's dtype into wquant's
    shared scratch before its two F.linear's.  Synchronises."""
    E, H, I = fp8experts.num_experts, fp8experts.hidden, fp8experts.intermediate
    out = torch.zeros_like(x)
    idx, w = plan.idx.long(), plan.w
    mask = F.one_hot(idx, num_classes=E).permute(2, 1, 0)
    hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
    buf = wquant._scratch(x.device, x.dtype, 3 * I, H)
    bufs = (buf[: 2 * I], buf[2 * I:].view(H, I))
    for e in hit:
        e = e[0]
        k_pos, tok = torch.where(mask[e])
        gate_up, down = fp8experts.dequant_expert(int(e), x.dtype, bufs)
        g, u = F.linear(x[tok], gate_up).chunk(2, dim=-1)
        y = F.linear(F.silu(g) * u, down)
        y = y * w[tok, k_pos, None]
        out.index_add_(0, tok, y.to(out.dtype))
    return out


class _Router(nn.Module):
    def __init__(self, num_experts: int, hidden: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_experts, hidden))


class _Experts(nn.Module):
    """The stacked expert weights under the names of transformers 5: gate_up_proj (E, 2 I, H), down_proj (E, H, I)."""

    def __init__(self, num_experts: int, hidden: int, intermediate: int):
        super().__init__()
        self.gate_up_proj = nn.Parameter(torch.empty(num_experts, 2 * intermediate, hidden))
        self.down_proj = nn.Parameter(torch.empty(num_experts, hidden, intermediate))


class SparseMoeBlock(nn.Module):
    """HF's MixtralSparseMoeBlock / Qwen3MoeSparseMoeBlock: gate.weight (E, H), experts.gate_up_proj, experts.down_proj.  The
    router GEMM is F.linear.  `kernel`: route and experts run the HIP entries -- always under stream capture, where the torch loop
    cannot run, and for at most `kernel_max_tokens` tokens otherwise; what the kernels do not serve (usable) takes the torch loop.
    `expert_bits=4`: the experts are a QuantExperts in groups of `expert_group` and every call takes the
    loop, with each hit expert dequantised into wquant's shared scratch first.  That loop synchronises, and there is no expert
    kernel over the packed buffers yet: under stream capture such a block raises.
    `expert_fp8`: the experts are an Fp8Experts, exclusive with `expert_bits`.  kivi_moe_experts_w8 runs under
    stream capture and for at most `kernel_max_tokens` tokens otherwise (None: FP8_KERNEL_MAX_TOKENS); above that, off the GPU and
    with `kernel=False` the dequantising loop runs, which under capture raises as the 4-bit block does."""

    def __init__(self, hidden: int, intermediate: int, num_experts: int, top_k: int, norm_topk: bool = True,
                 round_weights: bool = False, kernel: bool = True, kernel_max_tokens: Optional[int] = None,
                 expert_bits: Optional[int] = None, expert_group: int = 128, expert_fp8: bool = False):
        super().__init__()
        if not 1 <= top_k <= num_experts:
            raise ValueError(f"num_experts_per_tok = {top_k} outside [1, num_experts = {num_experts}]")
        if expert_bits not in (None, 4):
            raise ValueError(f"expert_bits has to be None or 4, got {expert_bits!r}")
        if expert_fp8 and expert_bits is not None:
            raise ValueError("expert_fp8 and expert_bits=4 are two formats of the same experts: choose one")
        self.hidden, self.intermediate, self.num_experts, self.top_k = hidden, intermediate, num_experts, top_k
        self.norm_topk, self.round_weights = bool(norm_topk), bool(round_weights)
        self.kernel = bool(kernel)
        self.expert_bits = expert_bits
        self.expert_fp8 = bool(expert_fp8)
        default = FP8_KERNEL_MAX_TOKENS if self.expert_fp8 else KERNEL_MAX_TOKENS
        self.kernel_max_tokens = default if kernel_max_tokens is None else int(kernel_max_tokens)
        self.gate = _Router(num_experts, hidden)
        if self.expert_fp8:
            self.experts = Fp8Experts(num_experts, hidden, intermediate)
        elif expert_bits is None:
            self.experts = _Experts(num_experts, hidden, intermediate)
        else:
            self.experts = QuantExperts(num_experts, hidden, intermediate, expert_group)
        for p in self.parameters():
            nn.init.normal_(p, 0.0, 0.02)

    def uses_kernel(self, x2: torch.Tensor) -> bool:
        if self.expert_bits is not None or not self.kernel or not usable(x2, self.num_experts, self.top_k, self.hidden, self.intermediate):
            return False
        return torch.cuda.is_current_stream_capturing() or x2.shape[0] <= self.kernel_max_tokens

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, Q, H = x.shape
        x2 = x.reshape(B * Q, H)
        logits = F.linear(x2, self.gate.weight)
        if self.uses_kernel(x2):
            plan = route(logits, self.top_k, self.norm_topk, self.round_weights)
            if self.expert_fp8:
                return experts_w8(x2, plan, self.experts).view(B, Q, H)
            return experts(x2, plan, self.experts.gate_up_proj, self.experts.down_proj).view(B, Q, H)
        if (self.expert_bits is not None or self.expert_fp8) and x2.is_cuda and torch.cuda.is_current_stream_capturing():
            what = "expert_fp8 and kernel=False" if self.expert_fp8 else "expert_bits=4"
            why = "the kernel over them is switched off" if self.expert_fp8 else "no kernel over the packed experts exists"
            raise _lib.KiviHipError(f"a sparse block with {what} cannot run under stream capture: its experts go through the "
                                    f"dequantising loop, which synchronises, and {why}")
        plan = route_torch(logits, self.top_k, self.norm_topk, self.round_weights)
        if self.expert_fp8:
            return experts_w8_torch(x2, plan, self.experts).view(B, Q, H)
        if self.expert_bits is not None:
            return experts_w4_torch(x2, plan, self.experts).view(B, Q, H)
        return experts_torch(x2, plan, self.experts.gate_up_proj, self.experts.down_proj).view(B, Q, H)
