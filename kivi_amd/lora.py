"""Per-request LoRA adapters: every row of a batch names an adapter slot, and every targeted linear adds
scale * B_s (A_s x) for that row after the base linear has run -- two tenants share a batch, and a base model with 4-bit weights
takes adapters it could never absorb.

The contract, which the kernels (kivi_amd/csrc/kivi_lora.hip), `apply_torch` and the tests restate: a LoraSet has S slots of table
rank R in {8, 16, 32, 64}; for every target linear (out = O, in = K) A (S, R, K) and B (S, O, R) in the model dtype, scale (S,) fp32,
ranks (S,) int32.  Row b of a pass is bound to slot[b] in {-1, 0 .. S - 1}; token n of a (B, Q, .) pass belongs to row n // Q.  After
the base linear has produced y (bias included), for s = slot[n // Q] >= 0

    t[n, j]  = sum_k float(A[s, j, k]) * float(x[n, k])        fp32, order a function of K alone
    d[n, o]  = sum_j float(B[s, o, j]) * t[n, j]               fp32, j ascending
    y'[n, o] = round_dtype(float(y[n, o]) + scale[s] * d[n, o])

Rows with slot -1 are not touched: their bytes are the base model's.  An adapter of rank r < R occupies rows / columns [0, r) of its
slot, the rest are zeros, and both paths stop at ranks[s] rounded up to 8, so a token's bits depend on its own x, its slot and that
slot's tables alone -- not on its batch, the other rows' slots, R or S.  scale = lora_alpha / r, or lora_alpha / sqrt(r) with
use_rslora.

`apply_` picks the path by token count alone: the two launches kivi_lora_shrink / kivi_lora_expand under stream capture and for at
most LORA_KERNEL_MAX_TOKENS tokens, `apply_torch` -- rows selected per distinct slot from the binding's HOST copy, two fp32 matmuls
per slot, no synchronisation -- above that and off the GPU.  Out of scope, refused by name where it can arrive: adapters on experts,
routers, embed_tokens or lm_head; DoRA; LoRA bias; per-module ranks or alphas; merging; training."""
from __future__ import annotations

import json
import math
import os
from contextlib import contextmanager, nullcontext
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
RANKS = (8, 16, 32, 64)
# Eager passes of more tokens than this take apply_torch.  The largest power of two tools/lora_time.py measured
# (profiles/lora_time.log, MI355X; r = 16, rows of one token): the two launches take 23-28 us up to N = 256 and 39-57 us at N = 1024
# -- launch latency, then the tables' bytes -- against apply_torch's 123-206 us with one adapter and 455-593 us with four (an
# index_select, two matmuls and an index_copy_ per distinct slot): 3.6-6.0x and 10-20x ahead at every N in {1, 8, 32, 64, 128, 256,
# 1024}, at 4096 -> 4096 and 11008 -> 4096, fp16 and bf16.  No crossover was reached; larger passes are not measured (DESIGN.md
# section 34).
LORA_KERNEL_MAX_TOKENS = 1024
_DTYPES = {torch.float16: 16, torch.bfloat16: _lib.LOGITS_BF16}
_REFUSED_IN_KEYS = ("embed_tokens", "lm_head", "experts", "router", "block_sparse_moe", ".mlp.gate.")


def _up8(r: int) -> int:
    return (r + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ adapters on disk
class LoraAdapter:
    """One adapter as PEFT writes it: `tensors` maps a module path of the model ("model.layers.0.self_attn.q_proj") to its pair
    (A (r, in), B (out, r)), as stored; `r`, `alpha`, `rslora`; `scale` by the rule of the module docstring."""

    def __init__(self, tensors: Dict[str, tuple], r: int, alpha: float, rslora: bool = False, target_modules: Sequence[str] = ()):
        if isinstance(r, bool) or not isinstance(r, int) or r < 1:
            raise ValueError(f"r has to be a positive integer, got {r!r}")
        self.tensors, self.r, self.alpha, self.rslora = dict(tensors), r, float(alpha), bool(rslora)
        self.target_modules = tuple(target_modules)
        for name, (a, b) in self.tensors.items():
            if a.dim() != 2 or b.dim() != 2 or a.shape[0] != r or b.shape[1] != r:
                raise ValueError(f"{name}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not have the shapes (r, in) / (out, r) "
                                 f"with r = {r}")

    @property
    def scale(self) -> float:
        return self.alpha / math.sqrt(self.r) if self.rslora else self.alpha / self.r

    @classmethod
    def from_peft(cls, path: str) -> "LoraAdapter":
        """Read the directory `path`: adapter_config.json and adapter_model.safetensors.  Keys are
        base_model.model.<module path>.lora_A.weight (r, in) and .lora_B.weight (out, r).  ValueError naming the field or key for
        what is out of scope: use_dora, a bias other than "none", non-empty modules_to_save / rank_pattern / alpha_pattern,
        fan_in_fan_out, an A without its B or the reverse, a key on embed_tokens, lm_head, a router or experts."""
        from safetensors.torch import load_file
        with open(os.path.join(path, "adapter_config.json")) as f:
            cfg = json.load(f)
        if cfg.get("use_dora"):
            raise ValueError("adapter_config.json: use_dora is set; DoRA adapters are not served")
        if cfg.get("bias", "none") not in ("none", None):
            raise ValueError(f"adapter_config.json: bias = {cfg['bias']!r}; LoRA bias is not served (bias has to be \"none\")")
        for field in ("modules_to_save", "rank_pattern", "alpha_pattern"):
            if cfg.get(field):
                raise ValueError(f"adapter_config.json: {field} = {cfg[field]!r} is not empty; per-module ranks, alphas and saved modules "
                                 f"are not served")
        if cfg.get("fan_in_fan_out"):
            raise ValueError("adapter_config.json: fan_in_fan_out is set; transposed base weights are not served")
        if "r" not in cfg or "lora_alpha" not in cfg:
            raise ValueError("adapter_config.json: r and lora_alpha are required")
        state = load_file(os.path.join(path, "adapter_model.safetensors"))
        halves: Dict[str, dict] = {}
        for key, t in state.items():
            for bad in _REFUSED_IN_KEYS:
                if bad in key:
                    raise ValueError(f"{key}: adapters on embed_tokens, lm_head, routers or experts are not served")
            for which in ("lora_A", "lora_B"):
                tail = f".{which}.weight"
                if key.endswith(tail):
                    name = key[: -len(tail)]
                    name = name[len("base_model.model."):] if name.startswith("base_model.model.") else name
                    halves.setdefault(name, {})[which] = t
                    break
            else:
                raise ValueError(f"{key}: not a lora_A.weight / lora_B.weight tensor (DoRA magnitudes, LoRA bias and saved modules are "
                                 f"not served)")
        for name, h in halves.items():
            for which, other in (("lora_A", "lora_B"), ("lora_B", "lora_A")):
                if which not in h:
                    raise ValueError(f"{name}.{which}.weight is missing: the file holds {name}.{other}.weight without it")
        return cls({n: (h["lora_A"], h["lora_B"]) for n, h in halves.items()}, int(cfg["r"]), cfg["lora_alpha"],
                   bool(cfg.get("use_rslora", False)), cfg.get("target_modules") or ())


# ------------------------------------------------------------------------------------------------ which slot a row runs
class RowBinding:
    """The slots of the rows of a pass: a device int32 buffer `slots` (rows,) the kernels read, and its host copy, which
    apply_torch selects rows by without a synchronisation.  `key()` names the buffer: a captured step holds its pointer, so
    set_row() / bind() between replays change what the step computes without a new capture.  `prompt`: with beams or n samples
    per prompt the prompt pass runs on the requests and the steps on rows = requests * fan; the binding then also holds the
    requests' slots, and a pass finds its buffer by its row count."""

    def __init__(self, rows: int, device, slots: Optional[Sequence[int]] = None, prompt: Optional[Sequence[int]] = None):
        self.rows, self.device = int(rows), torch.device(device)
        self.host: List[int] = [-1] * self.rows
        self.slots = torch.full((self.rows,), -1, dtype=torch.int32, device=self.device)
        self.prompt: Optional[RowBinding] = None
        if slots is not None:
            self.bind(slots)
        if prompt is not None and len(prompt) != self.rows:
            self.prompt = RowBinding(len(prompt), device, prompt)

    def key(self):
        return ("lora", self.rows, self.slots.data_ptr())

    def _upload(self) -> None:
        host = torch.tensor(self.host, dtype=torch.int32)
        self.slots.copy_(host.pin_memory() if self.slots.is_cuda else host, non_blocking=True)

    def bind(self, slots: Sequence[int]) -> "RowBinding":
        """All rows at once, in place (an asynchronous copy on the current stream, ordered before the next pass on it)."""
        slots = [-1 if s is None else int(s) for s in slots]
        if len(slots) != self.rows:
            raise ValueError(f"{len(slots)} slots for a binding of {self.rows} rows")
        self.host = slots
        self._upload()
        return self

    def set_row(self, b: int, slot: Optional[int]) -> None:
        if not 0 <= b < self.rows:
            raise ValueError(f"row {b} outside [0, {self.rows})")
        self.host[b] = -1 if slot is None else int(slot)
        self._upload()

    def for_rows(self, rows: int) -> "RowBinding":
        if rows == self.rows:
            return self
        if self.prompt is not None and rows == self.prompt.rows:
            return self.prompt
        raise ValueError(f"a pass of {rows} rows under a LoRA binding of {self.rows} rows"
                         + ("" if self.prompt is None else f" (prompt pass: {self.prompt.rows})"))


def resolve_adapters(adapters, n: int, num_slots: Optional[int], what: str = "adapters"):
    """`adapters=` of an entry point -> None (the base model, no binding), a list of n slots with -1 for the base model, or the
    RowBinding itself.  None; one int for all rows; one int | None per request; a ready RowBinding of the pass's rows.  ValueError for
    anything else, before any pass runs."""
    if adapters is None:
        return None
    if num_slots is None:
        raise ValueError(f"{what}= needs a model with adapters: call enable_lora() first")
    if isinstance(adapters, RowBinding):
        return adapters
    if isinstance(adapters, int) and not isinstance(adapters, bool):
        adapters = [adapters] * n
    if not isinstance(adapters, (list, tuple)):
        raise ValueError(f"{what} has to be None, one slot, one slot or None per request, or a RowBinding, got {adapters!r}")
    if len(adapters) != n:
        raise ValueError(f"{len(adapters)} {what} for {n} requests")
    out = []
    for a in adapters:
        if a is None:
            a = -1
        if isinstance(a, bool) or not isinstance(a, int) or not -1 <= a < num_slots:
            raise ValueError(f"{what}: a slot has to be None, -1 (the base model) or an integer in [0, {num_slots}), got {a!r}")
        out.append(a)
    return None if all(a < 0 for a in out) else out


# ------------------------------------------------------------------------------------------------ the two paths of a linear
def _check(y, x, A, B, scale, ranks, what: str):
    if x.dim() != 3 or y.dim() != 3 or y.shape[:2] != x.shape[:2]:
        raise ValueError(f"{what}: x (B, Q, K) and y (B, Q, O), got {tuple(x.shape)} and {tuple(y.shape)}")
    S, R, K = A.shape
    O = B.shape[1]
    if tuple(B.shape) != (S, O, R) or x.shape[2] != K or y.shape[2] != O or tuple(scale.shape) != (S,) or tuple(ranks.shape) != (S,):
        raise ValueError(f"{what}: A {tuple(A.shape)}, B {tuple(B.shape)}, x {tuple(x.shape)}, y {tuple(y.shape)}, scale "
                         f"{tuple(scale.shape)}, ranks {tuple(ranks.shape)} do not go together")
    if not (x.dtype == y.dtype == A.dtype == B.dtype):
        raise ValueError(f"{what}: x, y, A and B share one dtype, got {x.dtype}, {y.dtype}, {A.dtype}, {B.dtype}")
    return S, R, K, O


def apply_torch(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale_host: Sequence[float],
                ranks_host: Sequence[int], slots_host: Sequence[int]) -> torch.Tensor:
    """The contract in torch, in place on y (B, Q, O), on any device: for every distinct slot s >= 0 of `slots_host` its rows' tokens
    through two fp32 matmuls over the slot's first ranks_host[s] (rounded up to 8) ranks, y <- round(float(y) + scale * d).  Rows of
    slot -1 (or outside [0, S)) are not read or written.  Everything that selects is on the host: no synchronisation."""
    S, R, K = A.shape
    Bt, Q = x.shape[:2]
    if len(slots_host) != Bt:
        raise ValueError(f"apply_torch: {len(slots_host)} slots for {Bt} rows")
    for s in sorted({s for s in slots_host if 0 <= s < S}):
        rr = min(R, _up8(int(ranks_host[s])))
        if rr < 1:
            continue
        rows = torch.tensor([b for b in range(Bt) if slots_host[b] == s], dtype=torch.long, device=x.device)
        t = x.index_select(0, rows).reshape(-1, K).float() @ A[s, :rr].float().t()
        d = t @ B[s, :, :rr].float().t()
        upd = y.index_select(0, rows).float() + float(scale_host[s]) * d.view(rows.numel(), Q, -1)
        y.index_copy_(0, rows, upd.to(y.dtype))
    return y


def _row_stride(v: torch.Tensor) -> Optional[int]:
    """The stride between tokens n = b * Q + q and n + 1 of a (B, Q, C) tensor read in place, None where no single one exists."""
    Bt, Q, C = v.shape
    if v.stride(2) != 1:
        return None
    if Bt * Q == 1:
        return C
    if Q == 1:
        return v.stride(0) if v.stride(0) >= C else None
    if Bt > 1 and v.stride(0) != Q * v.stride(1):
        return None
    return v.stride(1) if v.stride(1) >= C else None


def apply_kernels(y: torch.Tensor, x: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: torch.Tensor, ranks: torch.Tensor,
                  slots: torch.Tensor) -> torch.Tensor:
    """kivi_lora_shrink, then kivi_lora_expand in place on y: two launches on the current stream, nothing read back.  x (B, Q, K)
    with unit channel stride (a view is read as it is where its rows are 16-byte aligned), y (B, Q, O) a view of (B * Q, O) rows;
    A, B contiguous; fp16 or bf16 on the GPU.  `t` (B * Q, R) fp32 is allocated per call: under capture it belongs to the graph's
    pool."""
    for t_, name in ((y, "y"), (x, "x"), (A, "A"), (B, "B"), (scale, "scale"), (ranks, "ranks"), (slots, "slots")):
        _lib.require_gpu(t_, name)
    S, R, K, O = _check(y, x, A, B, scale, ranks, "kivi_lora")
    if x.dtype not in _DTYPES:
        raise ValueError(f"kivi_lora: fp16 or bf16, got {x.dtype}")
    Bt, Q = x.shape[:2]
    N = Bt * Q
    if tuple(slots.shape) != (Bt,) or slots.dtype != torch.int32 or ranks.dtype != torch.int32 or scale.dtype != torch.float32:
        raise ValueError(f"kivi_lora: slots ({Bt},) int32, ranks int32, scale fp32")
    if not (A.is_contiguous() and B.is_contiguous() and scale.is_contiguous() and ranks.is_contiguous() and slots.is_contiguous()):
        raise ValueError("kivi_lora: A, B, scale, ranks and slots must be contiguous")
    xs = _row_stride(x)
    if xs is None or xs % 8 or x.data_ptr() % 16:
        x, xs = x.contiguous(), K
    ys = _row_stride(y)
    if ys is None:
        raise ValueError(f"kivi_lora: y has to be a view of (B * Q, O) rows, got strides {y.stride()}")
    t = torch.empty((N, R), dtype=torch.float32, device=x.device)
    lib, dt, stream = _lib.load(), _DTYPES[x.dtype], _lib.stream_ptr(x)
    rc = lib.kivi_lora_shrink(x.data_ptr(), xs, dt, N, Q, K, slots.data_ptr(), S, R, ranks.data_ptr(), A.data_ptr(), t.data_ptr(), stream)
    _lib.check(rc, "kivi_lora_shrink")
    rc = lib.kivi_lora_expand(t.data_ptr(), slots.data_ptr(), S, R, ranks.data_ptr(), scale.data_ptr(), B.data_ptr(), y.data_ptr(), ys,
                              dt, N, Q, O, stream)
    _lib.check(rc, "kivi_lora_expand")
    return y


def usable(x: torch.Tensor, K: int, O: int) -> bool:
    """True where the kernels serve: fp16 or bf16 on the GPU, K and O multiples of 8."""
    return x.is_cuda and x.dtype in _DTYPES and K % 8 == 0 and O % 8 == 0


# ------------------------------------------------------------------------------------------------ the tables of a model
class LoraSet:
    """The adapter tables of a model: for every target linear A (S, R, K) and B (S, O, R), zeroed, on the model's device in the
    model's dtype; `scale` (S,) fp32 and `ranks` (S,) int32 with host copies.  load() / unload() write in place: addresses never
    change, so a captured step sees a new adapter at its next replay.  `active`: the RowBinding the target linears' forward hooks
    apply (None: the hooks return at once and the pass is the base model's, byte for byte); the entry points' `adapters=` sets it
    for the length of a call (`bound`)."""

    def __init__(self, model: nn.Module, max_adapters: int, max_rank: int, target_modules: Sequence[str] = ("q_proj", "v_proj")):
        from .wfp8 import Fp8Linear
        from .wquant import QuantLinear
        if isinstance(max_adapters, bool) or not isinstance(max_adapters, int) or max_adapters < 1:
            raise ValueError(f"max_adapters has to be a positive integer, got {max_adapters!r}")
        if max_rank not in RANKS:
            raise ValueError(f"max_rank has to be one of {RANKS}, got {max_rank!r}")
        if isinstance(target_modules, str):
            target_modules = (target_modules,)
        target_modules = tuple(target_modules)
        if not target_modules or any(t not in TARGETS for t in target_modules):
            raise ValueError(f"target_modules has to be a non-empty subset of {TARGETS} (experts, routers, embed_tokens and lm_head "
                             f"are never targets), got {target_modules!r}")
        head = model.lm_head.weight
        self.device, self.dtype = head.device, head.dtype
        if self.device.type == "cuda" and self.dtype not in _DTYPES:
            raise ValueError(f"LoRA tables on the GPU are fp16 or bf16, the model is {self.dtype}")
        self.S, self.R, self.target_modules = max_adapters, max_rank, target_modules
        self.modules: Dict[str, nn.Module] = {}
        self.A: Dict[str, torch.Tensor] = {}
        self.B: Dict[str, torch.Tensor] = {}
        for name, m in model.named_modules():
            leaf = name.rsplit(".", 1)[-1]
            if leaf not in target_modules or not isinstance(m, (nn.Linear, QuantLinear, Fp8Linear)) or ".experts." in name:
                continue
            K, O = m.in_features, m.out_features
            if K % 8 or O % 8:
                raise ValueError(f"{name}: in_features = {K} and out_features = {O} have to be multiples of 8")
            self.modules[name] = m
            self.A[name] = torch.zeros((self.S, self.R, K), dtype=self.dtype, device=self.device)
            self.B[name] = torch.zeros((self.S, O, self.R), dtype=self.dtype, device=self.device)
        if not self.modules:
            raise ValueError(f"the model has no linear named {target_modules}")
        self.scale = torch.zeros(self.S, dtype=torch.float32, device=self.device)
        self.ranks = torch.zeros(self.S, dtype=torch.int32, device=self.device)
        self.scale_host: List[float] = [0.0] * self.S
        self.ranks_host: List[int] = [0] * self.S
        self.active: Optional[RowBinding] = None
        self.kernel = True                       # tests only: False sends every pass through apply_torch
        self._handles = []

    # -------------------------------------------------------------- memory
    @property
    def nbytes(self) -> int:
        """S * R * (K + O) * 2 bytes per target linear, and 8 S for scale and ranks."""
        return sum(t.numel() * t.element_size() for d in (self.A, self.B) for t in d.values()) + 8 * self.S

    # -------------------------------------------------------------- slots
    def _check_slot(self, slot) -> int:
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.S:
            raise ValueError(f"slot has to be an integer in [0, {self.S}), got {slot!r}")
        return slot

    def _set_meta(self, slot: int, scale: float, rank: int) -> None:
        self.scale_host[slot] = torch.tensor(scale, dtype=torch.float32).item()      # the fp32 value the device holds
        self.ranks_host[slot] = rank
        for dst, host in ((self.scale, torch.tensor(self.scale_host, dtype=torch.float32)),
                          (self.ranks, torch.tensor(self.ranks_host, dtype=torch.int32))):
            dst.copy_(host.pin_memory() if dst.is_cuda else host, non_blocking=True)

    def load(self, adapter: LoraAdapter, slot: Optional[int] = None) -> int:
        """Copy `adapter` into `slot` (None: the first free one) in place -> the slot.  fp32 files are rounded once to the model
        dtype.  Every check runs before anything is written: r <= max_rank (ValueError), shapes against the target module
        (ValueError naming it), a module the set does not target (KeyError naming it).  Modules of the set that the adapter does not
        name are zeroed in the slot."""
        if slot is None:
            free = [s for s in range(self.S) if self.ranks_host[s] == 0]
            if not free:
                raise ValueError(f"all {self.S} slots hold an adapter; unload() one or name the slot to overwrite")
            slot = free[0]
        slot = self._check_slot(slot)
        if adapter.r > self.R:
            raise ValueError(f"the adapter has r = {adapter.r}, the set was built with max_rank = {self.R}")
        for name, (a, b) in adapter.tensors.items():
            if name not in self.modules:
                raise KeyError(f"{name}: the adapter names a module the set does not target (target_modules = {self.target_modules})")
            m = self.modules[name]
            if tuple(a.shape) != (adapter.r, m.in_features) or tuple(b.shape) != (m.out_features, adapter.r):
                raise ValueError(f"{name}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit the module's "
                                 f"({adapter.r}, {m.in_features}) / ({m.out_features}, {adapter.r})")
        r = adapter.r
        for name in self.modules:
            self.A[name][slot].zero_()
            self.B[name][slot].zero_()
            if name in adapter.tensors:
                a, b = adapter.tensors[name]
                self.A[name][slot, :r].copy_(a.to(self.dtype))
                self.B[name][slot, :, :r].copy_(b.to(self.dtype))
        self._set_meta(slot, adapter.scale, r)
        return slot

    def unload(self, slot: int) -> None:
        """Zero the slot's tables, scale and rank: rows bound to it compute the base model (their launches walk no rank)."""
        slot = self._check_slot(slot)
        for name in self.modules:
            self.A[name][slot].zero_()
            self.B[name][slot].zero_()
        self._set_meta(slot, 0.0, 0)

    # -------------------------------------------------------------- the pass
    @contextmanager
    def bound(self, binding: Optional[RowBinding]):
        """The passes inside run under `binding` (None: the base model)."""
        prev, self.active = self.active, binding
        try:
            yield binding
        finally:
            self.active = prev

    def apply_(self, y: torch.Tensor, x: torch.Tensor, module_name: str, binding: RowBinding, kernel: bool = True) -> torch.Tensor:
        """y (B, Q, O), the base linear's output for x (B, Q, K), gains the low-rank update of `module_name` for the rows `binding`
        sends to a slot, in place.  Under stream capture, or for at most LORA_KERNEL_MAX_TOKENS tokens, the two launches; otherwise
        apply_torch.  `kernel=False` (tests): apply_torch."""
        A, B = self.A[module_name], self.B[module_name]
        _check(y, x, A, B, self.scale, self.ranks, module_name)
        bind = binding.for_rows(x.shape[0])
        capturing = x.is_cuda and torch.cuda.is_current_stream_capturing()
        n_tokens = x.shape[0] * x.shape[1]
        if kernel and self.kernel and usable(x, A.shape[2], B.shape[1]) and (capturing or n_tokens <= LORA_KERNEL_MAX_TOKENS):
            return apply_kernels(y, x, A, B, self.scale, self.ranks, bind.slots)
        if capturing:
            raise _lib.KiviHipError(f"{module_name}: no LoRA kernel serves {x.dtype} {tuple(x.shape)} under stream capture")
        return apply_torch(y, x, A, B, self.scale_host, self.ranks_host, bind.host)

    def _hook(self, name: str):
        def hook(module, inputs, output):
            binding = self.active
            if binding is None:
                return None
            x = inputs[0]
            if output.dim() != 3:
                raise ValueError(f"{name}: a LoRA target is called with (B, Q, K) inputs, got {tuple(x.shape)}")
            y = output if output.is_contiguous() else output.contiguous()
            return self.apply_(y, x, name, binding)
        return hook

    def attach(self) -> "LoraSet":
        for name, m in self.modules.items():
            self._handles.append(m.register_forward_hook(self._hook(name)))
            m._kivi_lora = self             # (a plain attribute: no parameter, buffer or child module)
        return self

    def detach(self) -> None:
        for h in self._handles:
            h.remove()
        self._handles = []
        for m in self.modules.values():
            if getattr(m, "_kivi_lora", None) is self:
                del m._kivi_lora
        self.active = None


def active_binding(*modules) -> Optional[RowBinding]:
    """The binding under which one of `modules` (linears) applies an adapter in this pass, or None."""
    for m in modules:
        s = getattr(m, "_kivi_lora", None)
        if s is not None and s.active is not None:
            return s.active
    return None


# ------------------------------------------------------------------------------------------------ the model's entry points
def call_binding(model, adapters, n: int, fan: int = 1, kept: bool = False):
    """The context of an entry point's `adapters=`: None -> nothing changes (a binding an outer call has set stays); otherwise the
    passes inside run under a binding of n * fan rows (request b's slot on rows b * fan .. b * fan + fan - 1; the prompt pass of the n
    requests finds the requests' slots), or under no binding when every request names the base model.  `kept`: the model's own
    binding for (rows, device), rebound in place -- graphed calls, whose captured steps hold its buffer.  ValueError before any pass."""
    lset = getattr(model, "lora", None)
    slots = resolve_adapters(adapters, n, None if lset is None else lset.S)
    if adapters is None:
        return nullcontext()
    if slots is None:
        return lset.bound(None)
    if isinstance(slots, RowBinding):
        slots.for_rows(n * fan)
        return lset.bound(slots)
    rows = [s for s in slots for _ in range(fan)]
    if kept:
        key = (len(rows), str(lset.device))
        binding = model._lora_bindings.get(key)
        if binding is None:
            binding = model._lora_bindings[key] = RowBinding(len(rows), lset.device)
        binding.bind(rows)
        if fan > 1:
            binding.prompt = RowBinding(n, lset.device, slots)
        return lset.bound(binding)
    return lset.bound(RowBinding(len(rows), lset.device, rows, prompt=slots if fan > 1 else None))


def graph_key(model):
    """What a captured decode step of `model` depends on, LoRA-wise: None, or the active binding's key()."""
    lset = getattr(model, "lora", None)
    return None if lset is None or lset.active is None else lset.active.key()
