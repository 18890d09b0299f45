"""Temperature / top-k / top-p / min-p sampling (transformers' do_sample path) with the fused HIP sampler kivi_sample.

`Sampler` holds the device RNG state {seed, n} (two int64) and draws one token per row per call; the call advances n on the device,
so it can be captured into a hipGraph and replayed.  The contract: s = float(logit) / temperature; top-k keeps
s >= the k-th largest s; top-p keeps a token when the mass strictly above it (over the top-k survivors) is < top_p; min-p keeps
p >= min_p * p_max; the draw takes the first token in vocabulary order whose inclusive running sum of kept probabilities exceeds
u * (kept mass), u = (x0 >> 8) * 2^-24 from Philox4x32-10 at key (seed low, seed high), counter (row, 0, n low, n high).

`SamplingParams` / `RowSampler`: the same draw with the parameters, seed and RNG stream of every row in
device memory (kivi_sample_rows), so requests with different parameters -- greedy ones among them -- share one launch, a row's
tokens do not depend on its place in the batch, and a captured decode step depends on two buffers, not on parameter values.

`philox4x32` and `reference_sample` (fp64, explicit u) restate the contract on the CPU for tests and tools; the product path
never calls them.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def check_params(temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None) -> None:
    """Raise ValueError for parameters outside transformers' ranges (no device work)."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) \
            or temperature <= 0:
        raise ValueError(f"temperature has to be a strictly positive finite float, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k has to be a non-negative integer (0 = off), got {top_k!r}")
    if not isinstance(top_p, (int, float)) or not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p has to be a float in (0, 1] (1 = off), got {top_p!r}")
    if min_p is not None and (not isinstance(min_p, (int, float)) or not (0.0 <= min_p < 1.0)):
        raise ValueError(f"min_p has to be None or a float in [0, 1), got {min_p!r}")


def check_seed(seed) -> None:
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"seed has to be None or an integer in [0, 2^64), got {seed!r}")


def draw_seed() -> int:
    """A 63-bit seed from torch's default CPU generator (so torch.manual_seed makes a seed=None run reproducible)."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def _call_args(logits: torch.Tensor, out: Optional[torch.Tensor], rows: Optional["RowSampler"] = None):
    """The checks of a sampler call -> (logits (B, V), last dimension contiguous; out).  `rows`: the RowSampler they have to fit."""
    _lib.require_gpu(logits, "logits")
    if logits.dim() == 3:
        if logits.shape[1] != 1:
            raise ValueError(f"logits (B, 1, V) expected, got {tuple(logits.shape)}")
        logits = logits[:, 0]
    if logits.dim() != 2 or logits.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"logits must be (B, V) or (B, 1, V) fp16 / fp32, got {tuple(logits.shape)} {logits.dtype}")
    B, V = logits.shape
    if rows is not None and (B != rows.B or logits.device != rows.records.device):
        raise ValueError(f"this RowSampler holds {rows.B} rows on {rows.records.device}, got logits of {B} rows on {logits.device}")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    if out is None:
        out = torch.empty((B, 1), dtype=torch.int64, device=logits.device)
    if out.dtype != torch.int64 or out.numel() != B or out.device != logits.device:
        raise ValueError(f"out must hold B={B} int64 tokens on {logits.device}")
    return logits, out


class Sampler:
    """The fused sampler with its device RNG state.  `__call__(logits, out=None)`: logits (B, V) or (B, 1, V) fp16 / fp32 on the
    GPU (the last dimension contiguous in memory or not -- rows are read with their stride) -> (B, 1) int64 tokens, written into
    `out` when given (e.g. the token buffer of a captured decode step).  Each call uses draw index n and then advances it."""

    def __init__(self, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0, min_p: Optional[float] = None,
                 seed: Optional[int] = None, device="cuda"):
        check_params(temperature, top_k, top_p, min_p)
        check_seed(seed)
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.min_p = float(min_p or 0.0)
        self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self.reset(seed)

    def reset(self, seed: Optional[int] = None) -> None:
        """Start a new stream: {seed, n = 0} (seed None: draw_seed())."""
        self.seed = draw_seed() if seed is None else int(seed)
        s = self.seed - 2 ** 64 if self.seed >= 2 ** 63 else self.seed
        self.state.copy_(torch.tensor([s, 0], dtype=torch.int64))

    def key(self):
        """What a captured call depends on: the parameters and the state buffer."""
        return (self.temperature, self.top_k, self.top_p, self.min_p, self.state.data_ptr())

    def __call__(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        logits, out = _call_args(logits, out)
        B, V = logits.shape
        lib = _lib.load()
        _lib.check(lib.kivi_sample(_lib.ptr(logits), 16 if logits.dtype == torch.float16 else 32, logits.stride(0), B, V,
                                   self.temperature, self.top_k, self.top_p, self.min_p, _lib.ptr(self.state), _lib.ptr(out),
                                   out.stride(0) if out.dim() else 1, _lib.stream_ptr(logits)),
                   "kivi_sample")
        return out


# ------------------------------------------------------------------ per-row parameters (kivi_sample_rows)
GREEDY = 1          # include/kivi_hip.h: KIVI_SAMPLE_ROW_GREEDY


class SampleRow(ctypes.Structure):
    """include/kivi_hip.h: kivi_sample_row (32 bytes)."""
    _fields_ = [("temperature", ctypes.c_float), ("top_k", ctypes.c_int32), ("top_p", ctypes.c_float), ("min_p", ctypes.c_float),
                ("seed", ctypes.c_int64), ("stream", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


@dataclasses.dataclass(frozen=True)
class SamplingParams:
    """The sampling parameters of one request, with HF's names, ranges and defaults.  `do_sample=False`: a greedy row (the lowest
    index of the largest logit; the other fields are still validated, and ignored).  `seed=None`: one is drawn with draw_seed()
    when the parameters are bound to a row of a RowSampler."""
    do_sample: bool = True
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    min_p: Optional[float] = None
    seed: Optional[int] = None

    def __post_init__(self):
        if not isinstance(self.do_sample, bool):
            raise ValueError(f"do_sample has to be a bool, got {self.do_sample!r}")
        check_params(self.temperature, self.top_k, self.top_p, self.min_p)
        check_seed(self.seed)


def _check_stream(stream) -> int:
    if isinstance(stream, bool) or not isinstance(stream, int) or not 0 <= stream < 2 ** 32:
        raise ValueError(f"stream has to be an integer in [0, 2^32), got {stream!r}")
    return stream


def _record(p: SamplingParams, stream: int) -> torch.Tensor:
    """The 32 bytes of one bound row (p.seed is set) as 4 int64 on the CPU."""
    seed = p.seed - 2 ** 64 if p.seed >= 2 ** 63 else p.seed
    rec = SampleRow(float(p.temperature), int(p.top_k), float(p.top_p), float(p.min_p or 0.0), seed, stream,
                    0 if p.do_sample else GREEDY)
    return torch.tensor(np.frombuffer(bytes(rec), dtype=np.int64))


class RowSampler:
    """The fused sampler with one record {temperature, top_k, top_p, min_p, seed, stream, greedy} and one draw index per row, both
    in device memory and owned by the sampler (`records` (B, 4) int64, `draw_index` (B,) int64).  `params`: one SamplingParams for
    every row, or a sequence of B of them; `streams`: the Philox stream of every row (default 0, so a request with seed s draws in
    ANY row what Sampler(seed=s) draws for a batch of one); rows that share a seed need different streams to draw differently.
    `B`: the number of rows when `params` is a single SamplingParams (default 1).
    Every argument is checked before a device is touched."""

    def __init__(self, params: Union[SamplingParams, Sequence[SamplingParams]], device="cuda",
                 streams: Optional[Sequence[int]] = None, B: Optional[int] = None):
        if isinstance(params, SamplingParams):
            if B is None:
                B = 1 if streams is None else len(streams)
            if isinstance(B, bool) or not isinstance(B, int) or B < 1:
                raise ValueError(f"B has to be a positive integer, got {B!r}")
            params = [params] * B
        else:
            params = list(params)
            if not params or not all(isinstance(p, SamplingParams) for p in params):
                raise ValueError("params has to be a SamplingParams or a non-empty sequence of them")
            if B is not None and B != len(params):
                raise ValueError(f"{len(params)} SamplingParams for B={B} rows")
        streams = [0] * len(params) if streams is None else [_check_stream(s) for s in streams]
        if len(streams) != len(params):
            raise ValueError(f"{len(streams)} streams for {len(params)} rows")
        self.params = [self._bind(p) for p in params]
        self.streams = streams
        self.records = torch.stack([_record(p, s) for p, s in zip(self.params, streams)]).to(device)
        self.draw_index = torch.zeros(len(params), dtype=torch.int64, device=device)

    @staticmethod
    def _bind(p: SamplingParams) -> SamplingParams:
        return p if p.seed is not None else dataclasses.replace(p, seed=draw_seed())

    @property
    def B(self) -> int:
        return len(self.params)

    def key(self):
        """What a captured call depends on: the number of rows and the two buffers -- not the parameter values, which a replay reads
        from the records.  (The leading string keeps it apart from every Sampler.key().)"""
        return ("rows", self.B, self.records.data_ptr(), self.draw_index.data_ptr())

    def set_row(self, b: int, params: SamplingParams, stream: int = 0, draw_index: int = 0) -> None:
        """A new request takes over row b: its record is rewritten and its draw index set to `draw_index` (default 0; a scheduler
        that has drawn the request's first tokens elsewhere passes how many), by asynchronous copies on the current stream (ordered
        after the calls already enqueued there); no other row is touched and nothing has to be captured again."""
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.B:
            raise ValueError(f"row {b!r} outside [0, {self.B})")
        if not isinstance(params, SamplingParams):
            raise ValueError("params has to be a SamplingParams")
        stream = _check_stream(stream)
        if isinstance(draw_index, bool) or not isinstance(draw_index, int) or not 0 <= draw_index < 2 ** 63:
            raise ValueError(f"draw_index has to be an integer in [0, 2^63), got {draw_index!r}")
        p = self._bind(params)
        rec = _record(p, stream)
        if self.records.is_cuda:
            rec = rec.pin_memory()
        self.records[b].copy_(rec, non_blocking=True)
        self.draw_index[b: b + 1].fill_(draw_index)
        self.params[b], self.streams[b] = p, stream

    def reset(self) -> None:
        """All draw indices back to 0 (the records stay)."""
        self.draw_index.zero_()

    def select(self, idx, streams: Optional[Sequence[int]] = None) -> "RowSampler":
        """A new RowSampler (its own buffers) whose row i is this one's row idx[i], seeds and draw indices included: the sampler side
        of a cache fork by index_select.  `streams`: new streams for the rows (default: those of the source rows)."""
        idx = [int(i) for i in (idx.tolist() if torch.is_tensor(idx) else idx)]
        if not idx or not all(0 <= i < self.B for i in idx):
            raise ValueError(f"idx has to be a non-empty sequence of rows in [0, {self.B})")
        new = RowSampler([self.params[i] for i in idx], self.records.device,
                         [self.streams[i] for i in idx] if streams is None else streams)
        new.draw_index.copy_(self.draw_index.index_select(0, torch.tensor(idx, device=self.draw_index.device)))
        return new

    def __call__(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """As Sampler.__call__: one token per row into (B, 1) int64 (`out` when given), in ONE kivi_sample_rows launch."""
        logits, out = _call_args(logits, out, self)
        B, V = logits.shape
        lib = _lib.load()
        _lib.check(lib.kivi_sample_rows(_lib.ptr(logits), 16 if logits.dtype == torch.float16 else 32, logits.stride(0), B, V,
                                        _lib.ptr(self.records), _lib.ptr(self.draw_index), _lib.ptr(out),
                                        out.stride(0) if out.dim() else 1, _lib.stream_ptr(logits)),
                   "kivi_sample_rows")
        return out


# ------------------------------------------------------------------ CPU restatement (tests, tools)
def philox4x32(ctr, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32-R over arrays: ctr (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Random123's philox4x32_R)."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., i].copy() for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i].copy() for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(PHILOX_W[0])) & mask, (k[1] + np.uint64(PHILOX_W[1])) & mask]
        p0 = np.uint64(PHILOX_M[0]) * c[0]
        p1 = np.uint64(PHILOX_M[1]) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
    return np.stack(c, -1).astype(np.uint32)


def philox_x0(seed: int, rows, n: int) -> np.ndarray:
    """x0 of the draw of rows `rows` at draw index n (the kivi_sample counter mapping)."""
    rows = np.asarray(rows, dtype=np.uint64)
    seed, n = int(seed) % 2 ** 64, int(n) % 2 ** 64
    ctr = np.stack([rows, np.zeros_like(rows), np.full_like(rows, n & 0xFFFFFFFF), np.full_like(rows, n >> 32)], -1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), ctr.shape[:-1] + (2,))
    return philox4x32(ctr, key)[..., 0]


def draw_u(seed: int, rows, n: int) -> np.ndarray:
    """u = (x0 >> 8) * 2^-24 in [0, 1), float64."""
    return (philox_x0(seed, rows, n) >> 8).astype(np.float64) * 2.0 ** -24


def draw_u_rows(seeds, streams, ns) -> np.ndarray:
    """u of kivi_sample_rows per row: key seeds[i], counter (streams[i], 0, ns[i] low, ns[i] high); float64 in [0, 1).
    draw_u_rows([seed] * B, range(B), [n] * B) is draw_u(seed, range(B), n)."""
    seeds = np.array([int(s) % 2 ** 64 for s in seeds], dtype=np.uint64)
    ns = np.array([int(n) % 2 ** 64 for n in ns], dtype=np.uint64)
    streams = np.asarray(streams, dtype=np.uint64)
    lo, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    ctr = np.stack([streams, np.zeros_like(streams), ns & lo, ns >> sh], -1)
    key = np.stack([seeds & lo, seeds >> sh], -1)
    return (philox4x32(ctr, key)[..., 0] >> 8).astype(np.float64) * 2.0 ** -24


def reference_kept(logits: torch.Tensor, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                   min_p: Optional[float] = None):
    """(kept (B, V) bool, p (B, V) float64 unnormalised exp(s - max)) of the contract, in float64 on the CPU."""
    s = logits.detach().cpu().float() / torch.tensor(float(temperature), dtype=torch.float32)    # IEEE fp32, as the kernel
    s = s.double()
    B, V = s.shape
    keep = torch.ones((B, V), dtype=torch.bool)
    k = min(top_k, V)
    if 0 < k < V:
        kth = torch.topk(s, k, dim=-1).values[:, -1:]
        keep &= s >= kth
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m).nan_to_num(0.0)
    if top_p < 1.0:
        ek = torch.where(keep, e, torch.zeros_like(e))
        Z = ek.sum(-1, keepdim=True)
        order = torch.argsort(s, dim=-1, descending=True, stable=True)
        ss, es = s.gather(-1, order), ek.gather(-1, order)
        cum = es.cumsum(-1)
        # mass strictly above a token: the cumulative mass before its tie class
        first = torch.ones_like(ss, dtype=torch.bool)
        first[:, 1:] = ss[:, 1:] != ss[:, :-1]
        before = torch.where(first, cum - es, torch.zeros_like(cum))
        idx = torch.where(first, torch.arange(V).expand(B, V), torch.zeros((B, V), dtype=torch.long))
        idx = torch.cummax(idx, -1).values
        above = before.gather(-1, idx)
        keep_sorted = above / Z < top_p
        keep &= torch.zeros_like(keep).scatter(-1, order, keep_sorted)
    if min_p:
        keep &= e >= min_p
    return keep, e


def reference_sample(logits: torch.Tensor, u, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                     min_p: Optional[float] = None) -> torch.Tensor:
    """fp64 CPU restatement of kivi_sample with explicit u (B,) in [0, 1): (B,) int64 tokens."""
    keep, e = reference_kept(logits, temperature, top_k, top_p, min_p)
    w = torch.where(keep, e, torch.zeros_like(e))
    cum = w.cumsum(-1)
    u = torch.as_tensor(np.asarray(u, dtype=np.float64)).reshape(-1, 1)
    tok = (cum <= u * cum[:, -1:]).sum(-1)
    return tok.clamp(max=logits.shape[-1] - 1)
