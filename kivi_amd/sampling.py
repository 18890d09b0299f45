"""Temperature / top-k / top-p / min-p sampling (transformers' do_sample path) with the fused HIP sampler kivi_sample.

`Sampler` holds the device RNG state {seed, n} (two int64) and draws one token per row per call; the call advances n on the device,
so it can be captured into a hipGraph and replayed.  The contract: s = float(logit) / temperature; top-k keeps
s >= the k-th largest s; top-p keeps a token when the mass strictly above it (over the top-k survivors) is < top_p; min-p keeps
p >= min_p * p_max; the draw takes the first token in vocabulary order whose inclusive running sum of kept probabilities exceeds
u * (kept mass), u = (x0 >> 8) * 2^-24 from Philox4x32-10 at key (seed low, seed high), counter (row, 0, n low, n high).

`SamplingParams` / `RowSampler`: the same draw with the parameters, seed and RNG stream of every row in
device memory (kivi_sample_rows), so requests with different parameters -- greedy ones among them -- share one launch, a row's
tokens do not depend on its place in the batch, and a captured decode step depends on two buffers, not on parameter values.

Penalties: `SamplingParams(repetition_penalty=, presence_penalty=, frequency_penalty=)`; a RowSampler made with
`vocab_size=` owns one penalty record per row and a history table (row, token) in device memory, draws through
kivi_sample_rows_pen -- the penalties applied where the kernel reads a logit, the drawn token counted where it is written -- and
marks prompts and earlier outputs with kivi_seen_mark (`observe_prompt`, `set_row(prompt=, generated=)`).

Constraints: `SamplingParams(logit_bias=, allowed_token_ids=, min_new_tokens=)`; a RowSampler made with
`constraints=True` (the default when a row is constrained) also owns one constraint record, one allow mask and one list of biased /
suppressed tokens per row, and draws through kivi_sample_rows_con, which applies them where the kernel reads a logit; `set_allowed`
rebinds a row's mask between steps (a grammar engine's bitmask, or ids), `set_row(..., suppress=)` binds a request.

`philox4x32`, `reference_sample` (fp64, explicit u), `reference_penalise` and `reference_constrain` (fp32, the kernel's bits) restate
the contract on the CPU for tests and tools; the product path never calls them.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import types
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


NEUTRAL = (1.0, 0.0, 0.0)     # (repetition_penalty, presence_penalty, frequency_penalty) that change nothing
UNCONSTRAINED = (None, None, 0)    # (logit_bias, allowed_token_ids, min_new_tokens) that change nothing


def check_penalties(repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0) -> None:
    """Raise ValueError, naming the field, for a penalty outside its range (no device work)."""
    def real(v):
        return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)
    if not real(repetition_penalty) or repetition_penalty <= 0:
        raise ValueError(f"repetition_penalty has to be a strictly positive finite float (1 = off), got {repetition_penalty!r}")
    if not real(presence_penalty):
        raise ValueError(f"presence_penalty has to be a finite float (0 = off), got {presence_penalty!r}")
    if not real(frequency_penalty):
        raise ValueError(f"frequency_penalty has to be a finite float (0 = off), got {frequency_penalty!r}")


MAX_LIST = _lib.SAMPLE_MAX_LIST      # include/kivi_hip.h: KIVI_SAMPLE_MAX_LIST
MAX_TOKEN_ID = (1 << 20) - 1         # bits 0-19 of a list entry's word (KIVI_LIST_TOKEN)


def _token_id(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 0 <= v <= MAX_TOKEN_ID


def check_constraints(logit_bias=None, allowed_token_ids=None, min_new_tokens=0):
    """-> (logit_bias as a tuple of (id, float) pairs in ascending id order or None, allowed_token_ids as an ascending tuple or
    None, min_new_tokens); ValueError, naming the field, for anything else (no device work)."""
    bias = None
    if logit_bias is not None:
        if not hasattr(logit_bias, "items"):
            raise ValueError(f"logit_bias has to be None or a dict from token id to float, got {logit_bias!r}")
        for t, v in logit_bias.items():
            if not _token_id(t):
                raise ValueError(f"logit_bias: token id {t!r} is not an integer in [0, {MAX_TOKEN_ID}]")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
                raise ValueError(f"logit_bias[{t}] has to be a float (+-inf allowed, NaN not), got {v!r}")
        if len(logit_bias) > MAX_LIST:
            raise ValueError(f"logit_bias lists {len(logit_bias)} tokens; a row's list holds at most {MAX_LIST}")
        bias = tuple(sorted((int(t), float(v)) for t, v in logit_bias.items())) or None
    allowed = None
    if allowed_token_ids is not None:
        try:
            ids = list(allowed_token_ids.tolist() if hasattr(allowed_token_ids, "tolist") else allowed_token_ids)
        except TypeError:
            raise ValueError(f"allowed_token_ids has to be None or a non-empty sequence of token ids, got {allowed_token_ids!r}")
        if not ids or not all(_token_id(t) for t in ids):
            raise ValueError(f"allowed_token_ids has to be None or a non-empty sequence of token ids in [0, {MAX_TOKEN_ID}], "
                             f"got {allowed_token_ids!r}")
        if len(set(ids)) != len(ids):
            raise ValueError("allowed_token_ids holds a token id twice")
        allowed = tuple(sorted(int(t) for t in ids))
    if isinstance(min_new_tokens, bool) or not isinstance(min_new_tokens, int) or min_new_tokens < 0:
        raise ValueError(f"min_new_tokens has to be a non-negative integer (0 = off), got {min_new_tokens!r}")
    return bias, allowed, min_new_tokens


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
    if logits.dim() != 2 or logits.dtype not in _lib.LOGITS_BITS:
        raise ValueError(f"logits must be (B, V) or (B, 1, V) fp16 / bf16 / fp32, got {tuple(logits.shape)} {logits.dtype}")
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
        _lib.check(lib.kivi_sample(_lib.ptr(logits), _lib.LOGITS_BITS[logits.dtype], logits.stride(0), B, V,
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
    when the parameters are bound to a row of a RowSampler.
    `repetition_penalty` (HF, vLLM: over prompt and output tokens; finite, > 0, 1 = off), `presence_penalty` and `frequency_penalty`
    (OpenAI, vLLM: over output tokens; finite, 0 = off): DESIGN.md section 22; greedy rows are penalised too.  The three are
    init-only variables that __post_init__ stores: they are attributes, keywords of the constructor and of dataclasses.replace,
    and part of ==, hash and repr, while the dataclass's own field tuple -- astuple(), positional construction -- stays the six
    fields above.
    `logit_bias` (OpenAI, vLLM; HF's sequence_bias over single tokens: a dict from token id to an additive fp32 bias, +-inf allowed,
    -inf bans the token; None when empty), `allowed_token_ids` (vLLM: a non-empty sequence of distinct ids, the only tokens the
    request may emit; None = all) and `min_new_tokens` (HF: the row's eos / stop ids are masked for its first so many tokens; 0 =
    off): DESIGN.md section 25, init-only in the same way.  They are stored in a canonical form -- `logit_bias` as a read-only
    mapping in ascending id order, `allowed_token_ids` as an ascending tuple -- so equal constraints compare and hash equal."""
    do_sample: bool = True
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    min_p: Optional[float] = None
    seed: Optional[int] = None
    repetition_penalty: dataclasses.InitVar[float] = 1.0
    presence_penalty: dataclasses.InitVar[float] = 0.0
    frequency_penalty: dataclasses.InitVar[float] = 0.0
    logit_bias: dataclasses.InitVar[Optional[dict]] = None
    allowed_token_ids: dataclasses.InitVar[Optional[Sequence[int]]] = None
    min_new_tokens: dataclasses.InitVar[int] = 0

    def __post_init__(self, repetition_penalty, presence_penalty, frequency_penalty, logit_bias=None, allowed_token_ids=None,
                      min_new_tokens=0):
        if not isinstance(self.do_sample, bool):
            raise ValueError(f"do_sample has to be a bool, got {self.do_sample!r}")
        check_params(self.temperature, self.top_k, self.top_p, self.min_p)
        check_seed(self.seed)
        check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        for name, v in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                        ("frequency_penalty", frequency_penalty)):
            object.__setattr__(self, name, float(v))
        bias, allowed, min_new = check_constraints(logit_bias, allowed_token_ids, min_new_tokens)
        object.__setattr__(self, "logit_bias", None if bias is None else types.MappingProxyType(dict(bias)))
        object.__setattr__(self, "allowed_token_ids", allowed)
        object.__setattr__(self, "min_new_tokens", min_new)

    @property
    def constraints(self):
        """(logit_bias as a tuple of (id, value) pairs or None, allowed_token_ids, min_new_tokens): hashable."""
        return (None if self.logit_bias is None else tuple(self.logit_bias.items()), self.allowed_token_ids, self.min_new_tokens)

    @property
    def constrained(self) -> bool:
        return self.constraints != UNCONSTRAINED

    def check_vocab(self, vocab_size: Optional[int]) -> None:
        """ValueError when a constraint names a token id outside [0, vocab_size) (None: not known, nothing is checked)."""
        if vocab_size is None:
            return
        for name, ids in (("logit_bias", self.logit_bias or ()), ("allowed_token_ids", self.allowed_token_ids or ())):
            bad = [t for t in ids if t >= vocab_size]
            if bad:
                raise ValueError(f"{name} names token id {bad[0]}, outside the vocabulary [0, {vocab_size})")

    @property
    def penalties(self):
        """(repetition_penalty, presence_penalty, frequency_penalty)."""
        return (self.repetition_penalty, self.presence_penalty, self.frequency_penalty)

    @property
    def penalised(self) -> bool:
        return self.penalties != NEUTRAL

    def __eq__(self, other):
        if other.__class__ is not self.__class__:
            return NotImplemented
        return dataclasses.astuple(self) + self.penalties + self.constraints == \
            dataclasses.astuple(other) + other.penalties + other.constraints

    def __hash__(self):
        return hash(dataclasses.astuple(self) + self.penalties + self.constraints)

    def __repr__(self):
        body = [f"{f.name}={getattr(self, f.name)!r}" for f in dataclasses.fields(self)]
        body += [f"{n}={getattr(self, n)!r}" for n in ("repetition_penalty", "presence_penalty", "frequency_penalty")]
        if self.constrained:                          # (an unconstrained request prints as it did)
            body += [f"logit_bias={None if self.logit_bias is None else dict(self.logit_bias)!r}",
                     f"allowed_token_ids={self.allowed_token_ids!r}", f"min_new_tokens={self.min_new_tokens!r}"]
        return f"SamplingParams({', '.join(body)})"


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


SEEN_CLEAR, SEEN_PROMPT, SEEN_OUTPUT = 1, 2, 4     # include/kivi_hip.h: KIVI_SEEN_*
SEEN_PROMPT_BIT, SEEN_COUNT_MAX = 0x8000, 0x7FFF   # a word of the history table: bit 15 = in the prompt, bits 0-14 = times emitted


class SamplePenalty(ctypes.Structure):
    """include/kivi_hip.h: kivi_sample_penalty (16 bytes)."""
    _fields_ = [("repetition", ctypes.c_float), ("presence", ctypes.c_float), ("frequency", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


def _penalty_record(p: SamplingParams) -> torch.Tensor:
    """The 16 bytes of one row's kivi_sample_penalty as 4 fp32 on the CPU (the reserved word 0 is the bits of 0.0)."""
    rec = SamplePenalty(p.repetition_penalty, p.presence_penalty, p.frequency_penalty, 0)
    return torch.tensor(np.frombuffer(bytes(rec), dtype=np.float32))


def _upload(dst: torch.Tensor, host: torch.Tensor) -> None:
    """A CPU tensor into `dst` by an asynchronous copy on the current stream (from pinned memory when `dst` is on a device)."""
    dst.copy_(host.pin_memory() if dst.is_cuda else host, non_blocking=True)


def _token_rows(tokens, device) -> Optional[torch.Tensor]:
    """Token ids (a sequence, a 1-D or a 2-D tensor) as (n, T) int64 on `device` with unit inner stride; None when there are none."""
    if tokens is None:
        return None
    t = torch.as_tensor(tokens, dtype=torch.long)
    t = t.reshape(1, -1) if t.dim() < 2 else t
    if t.dim() != 2:
        raise ValueError(f"token ids have to be (T,) or (n, T), got {tuple(t.shape)}")
    if not t.numel():
        return None
    t = t.to(device)
    return t if t.stride(1) == 1 else t.contiguous()


CONSTRAINT_MASK = 1                               # include/kivi_hip.h: KIVI_CONSTRAINT_MASK
LIST_TOKEN, LIST_SUPPRESS = 0x000FFFFF, 0x80000000    # KIVI_LIST_TOKEN, KIVI_LIST_SUPPRESS
ALLOW_NONE, ALLOW_ALL, ALLOW_SET, ALLOW_UNSET = 1, 2, 4, 8     # KIVI_ALLOW_*


class SampleConstraint(ctypes.Structure):
    """include/kivi_hip.h: kivi_sample_constraint (32 bytes)."""
    _fields_ = [("flags", ctypes.c_uint32), ("n_list", ctypes.c_int32), ("suppress_until", ctypes.c_int64),
                ("reserved", ctypes.c_uint32 * 4)]


class SampleListEntry(ctypes.Structure):
    """include/kivi_hip.h: kivi_sample_list_entry (8 bytes)."""
    _fields_ = [("word", ctypes.c_uint32), ("value", ctypes.c_float)]


def allow_words(vocab_size: int) -> int:
    """The words of one row of the allow masks: ceil(vocab_size / 32) rounded up to the stride quantum of 4."""
    return ((vocab_size + 31) // 32 + 3) // 4 * 4


def allow_bitmask(ids, vocab_size: int) -> torch.Tensor:
    """Token ids -> one row of the allow masks on the CPU, (allow_words(vocab_size),) int32: bit (e & 31) of word (e >> 5) is 1
    exactly for the ids in [0, vocab_size) (the layout grammar engines emit)."""
    bits = np.zeros(allow_words(vocab_size) * 32, dtype=bool)
    ids = np.asarray(list(ids), dtype=np.int64).reshape(-1)
    bits[ids[(ids >= 0) & (ids < vocab_size)]] = True
    return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy())


def constraint_list(p: "SamplingParams", suppress=()) -> list:
    """The list of a row bound to `p`, sorted and merged as kivi_sample_rows_con wants it: [(token, value, suppressed)] in ascending
    token order, one entry per token -- the tokens of logit_bias, and, when min_new_tokens > 0, the `suppress` ids (a token in both
    keeps its bias for the draws after the suppression).  ValueError for more than MAX_LIST entries or an id that does not fit."""
    merged = {t: (v, False) for t, v in (p.logit_bias or {}).items()}
    if p.min_new_tokens > 0:
        for t in suppress:
            if not _token_id(t):
                raise ValueError(f"suppress: token id {t!r} is not an integer in [0, {MAX_TOKEN_ID}]")
            merged[int(t)] = (merged.get(int(t), (0.0, False))[0], True)
    if len(merged) > MAX_LIST:
        raise ValueError(f"{len(merged)} biased and suppressed tokens for one row; its list holds at most {MAX_LIST}")
    return [(t, v, sup) for t, (v, sup) in sorted(merged.items())]


def _list_words(entries) -> torch.Tensor:
    """[(token, value, suppressed)] -> (len, 2) int32 on the CPU: kivi_sample_list_entry after kivi_sample_list_entry."""
    raw = b"".join(bytes(SampleListEntry(t | (LIST_SUPPRESS if sup else 0), v)) for t, v, sup in entries)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int32).reshape(-1, 2).copy())


def _constraint_record(flags: int, n_list: int, suppress_until: int) -> torch.Tensor:
    """The 32 bytes of one row's kivi_sample_constraint as 4 int64 on the CPU."""
    return torch.tensor(np.frombuffer(bytes(SampleConstraint(flags, n_list, suppress_until)), dtype=np.int64))


class RowSampler:
    """The fused sampler with one record {temperature, top_k, top_p, min_p, seed, stream, greedy} and one draw index per row, both
    in device memory and owned by the sampler (`records` (B, 4) int64, `draw_index` (B,) int64).  `params`: one SamplingParams for
    every row, or a sequence of B of them; `streams`: the Philox stream of every row (default 0, so a request with seed s draws in
    ANY row what Sampler(seed=s) draws for a batch of one); rows that share a seed need different streams to draw differently.
    `B`: the number of rows when `params` is a single SamplingParams (default 1).
    `vocab_size`: the sampler also owns the state of the penalties: `penalties` (B, 4) fp32, one
    kivi_sample_penalty per row, and `seen` (B, vocab_size rounded up to 8) int16, the history table -- bit 15 of a word: the token
    is in the row's prompt, bits 0-14: how often the row has emitted it.  Both are allocated here, once, so before anything can be
    captured; calls then go through kivi_sample_rows_pen, which counts every token it draws.  Without it (None) the sampler is
    what it was, and penalised `params` are refused: the table's width has to be known here.
    `constraints` (None: on exactly when a row of `params` is constrained; needs `vocab_size`): the sampler also
    owns `constraint` (B, 4) int64, one kivi_sample_constraint per row; `allowed` (B, allow_words(vocab_size)) int32, the allow
    masks, all ones at first -- public: a grammar engine on the device may write a row between two steps, after set_allowed(b, ...)
    has put the row's mask in force --; and `bias_list` (B, 1024, 2) int32, {token | suppress bit, fp32 bits} pairs.  All allocated
    here, once; calls then go through kivi_sample_rows_con.  `suppress`: the ids that `min_new_tokens` masks (the eos / stop ids),
    one sequence for every row or B of them.  Off, nothing changes: the same buffers, key() and entry as before.
    Every argument is checked before a device is touched."""

    def __init__(self, params: Union[SamplingParams, Sequence[SamplingParams]], device="cuda",
                 streams: Optional[Sequence[int]] = None, B: Optional[int] = None, vocab_size: Optional[int] = None,
                 constraints: Optional[bool] = None, suppress=None):
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
        if vocab_size is not None and (isinstance(vocab_size, bool) or not isinstance(vocab_size, int)
                                       or not 1 <= vocab_size <= _lib.SAMPLE_MAX_V):
            raise ValueError(f"vocab_size has to be None or an integer in [1, {_lib.SAMPLE_MAX_V}], got {vocab_size!r}")
        if vocab_size is None and any(p.penalised for p in params):
            raise ValueError("a row has a repetition / presence / frequency penalty: pass vocab_size= so that the sampler can "
                             "allocate its history table")
        if constraints is not None and not isinstance(constraints, bool):
            raise ValueError(f"constraints has to be None or a bool, got {constraints!r}")
        constrained = any(p.constrained for p in params)
        if constraints is None:
            constraints = constrained
        if constrained and not constraints:
            raise ValueError("a row has a logit_bias, allowed_token_ids or min_new_tokens, but constraints=False")
        if constraints and vocab_size is None:
            raise ValueError("constrained rows (logit_bias / allowed_token_ids / min_new_tokens): pass vocab_size= so that the "
                             "sampler can allocate its allow masks")
        if suppress is None or (len(suppress) and not isinstance(suppress[0], (list, tuple, torch.Tensor))):
            suppress = [suppress] * len(params)
        if len(suppress) != len(params):
            raise ValueError(f"{len(suppress)} lists of suppressed ids for {len(params)} rows")
        suppress = [() if ids is None else [int(t) for t in (ids.tolist() if torch.is_tensor(ids) else ids)] for ids in suppress]
        lists = None
        if constraints:
            for p in params:
                p.check_vocab(vocab_size)
            lists = [constraint_list(p, ids) for p, ids in zip(params, suppress)]
        self.params = [self._bind(p) for p in params]
        self.streams = streams
        self.records = torch.stack([_record(p, s) for p, s in zip(self.params, streams)]).to(device)
        self.draw_index = torch.zeros(len(params), dtype=torch.int64, device=device)
        self.vocab_size, self.penalties, self.seen = vocab_size, None, None
        if vocab_size is not None:
            self.penalties = torch.stack([_penalty_record(p) for p in self.params]).to(device)
            self.seen = torch.zeros((len(params), (vocab_size + 7) // 8 * 8), dtype=torch.int16, device=device)
        self.constraint, self.allowed, self.bias_list, self._con = None, None, None, None
        if constraints:
            n = len(params)
            self._con = [dict(mask=p.allowed_token_ids is not None, list=ls, min_new=p.min_new_tokens, until=p.min_new_tokens)
                         for p, ls in zip(self.params, lists)]
            self.constraint = torch.stack([self._con_record(c) for c in self._con]).to(device)
            allowed = torch.full((n, allow_words(vocab_size)), -1, dtype=torch.int32)
            bias_list = torch.zeros((n, MAX_LIST, 2), dtype=torch.int32)
            for b, (p, ls) in enumerate(zip(self.params, lists)):
                if p.allowed_token_ids is not None:
                    allowed[b] = allow_bitmask(p.allowed_token_ids, vocab_size)
                if ls:
                    bias_list[b, : len(ls)] = _list_words(ls)
            self.allowed, self.bias_list = allowed.to(device), bias_list.to(device)

    @staticmethod
    def _con_record(c: dict) -> torch.Tensor:
        return _constraint_record(CONSTRAINT_MASK if c["mask"] else 0, len(c["list"]), c["until"])

    def _write_constraint(self, b: int) -> None:
        _upload(self.constraint[b], self._con_record(self._con[b]))

    def _bind_constraint(self, b: int, allowed_ids=False) -> None:
        """Row b's constraint state from self._con[b], on the current stream: its list words, its mask row -- the ids it allows (None:
        every token; False: the row stays as it is) -- and its record."""
        entries = self._con[b]["list"]
        if entries:
            _upload(self.bias_list[b, : len(entries)], _list_words(entries))
        if allowed_ids is not False:
            _upload(self.allowed[b], torch.full((self.allowed.shape[1],), -1, dtype=torch.int32) if allowed_ids is None else
                    allow_bitmask(allowed_ids, self.vocab_size))
        self._write_constraint(b)

    def _require_constraints(self, what: str) -> None:
        if self._con is None:
            raise ValueError(f"{what}, but this RowSampler has no constraint state: pass vocab_size= and constraints=True when it "
                             "is made")

    def bind_suppress(self, suppress) -> None:
        """The ids that `min_new_tokens` masks, one sequence per row (the rows' eos / stop ids): the list and the record of every row
        whose params carry a min_new_tokens are rewritten -- a generate call does this once its finish conditions are resolved.
        Rows without one, the masks and suppress_until stay as they are."""
        self._require_constraints("bind_suppress")
        if len(suppress) != self.B:
            raise ValueError(f"{len(suppress)} lists of suppressed ids for {self.B} rows")
        for b, (p, ids) in enumerate(zip(self.params, suppress)):
            if p.min_new_tokens > 0:
                self._con[b]["list"] = constraint_list(p, [int(t) for t in ids])
                self._bind_constraint(b)

    def set_allowed(self, b: int, allowed=None) -> None:
        """Row b's allow mask, on the current stream (ordered after the calls already enqueued there); nothing is captured again.
        `allowed`: None -- no mask: the row's record drops KIVI_CONSTRAINT_MASK and its mask row is all ones again; a torch.int32
        tensor -- a bitmask of at least ceil(vocab_size / 32) words in the layout of `allowed` (what grammar engines emit), copied
        into the row; anything else -- token ids (a sequence or an integer tensor; ids outside the vocabulary are ignored): the row
        allows exactly those.  Ids in host memory are packed here and copied; ids in device memory go through kivi_allow_mark
        without being read on the host.  An empty set masks every token (the draw is then some token, include/kivi_hip.h)."""
        self._require_constraints("set_allowed")
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.B:
            raise ValueError(f"row {b!r} outside [0, {self.B})")
        row, W = self.allowed[b], (self.vocab_size + 31) // 32
        if allowed is None:
            row.fill_(-1)
        elif torch.is_tensor(allowed) and allowed.dtype == torch.int32:
            if allowed.dim() != 1 or allowed.numel() < W:
                raise ValueError(f"a bitmask of at least {W} int32 words expected, got {tuple(allowed.shape)}")
            row[:W].copy_(allowed[:W], non_blocking=True)
        elif torch.is_tensor(allowed) and allowed.is_cuda:
            ids = allowed.reshape(1, -1).to(torch.long).contiguous()
            lib = _lib.load()
            _lib.check(lib.kivi_allow_mark(_lib.ptr(self.allowed), self.allowed.stride(0), self.vocab_size, _lib.ptr(
                torch.tensor([b], dtype=torch.int32).to(allowed.device)), 1, _lib.ptr(ids) if ids.numel() else None, ids.shape[1],
                ids.shape[1], None, ALLOW_NONE | ALLOW_SET, _lib.stream_ptr(self.allowed)), "kivi_allow_mark")
        else:
            _upload(row, allow_bitmask(allowed.tolist() if torch.is_tensor(allowed) else allowed, self.vocab_size))
        if self._con[b]["mask"] != (allowed is not None):
            self._con[b]["mask"] = allowed is not None
            self._write_constraint(b)

    @staticmethod
    def _bind(p: SamplingParams) -> SamplingParams:
        return p if p.seed is not None else dataclasses.replace(p, seed=draw_seed())

    @property
    def B(self) -> int:
        return len(self.params)

    def key(self):
        """What a captured call depends on: the number of rows and the two buffers -- not the parameter values, which a replay reads
        from the records -- and, when they exist, the penalty records and the history table, and the constraint records, allow
        masks and lists.  (The leading string keeps it apart from every Sampler.key().)"""
        key = ("rows", self.B, self.records.data_ptr(), self.draw_index.data_ptr())
        key = key if self.seen is None else key + (self.penalties.data_ptr(), self.seen.data_ptr())
        return key if self._con is None else key + (self.constraint.data_ptr(), self.allowed.data_ptr(), self.bias_list.data_ptr())

    def _mark(self, flags: int, tokens=None, rows: Optional[Sequence[int]] = None, lead: Optional[torch.Tensor] = None) -> None:
        """kivi_seen_mark on the current stream: `tokens` (n, T) for the table rows `rows` (None: all B, in order)."""
        _lib.require_gpu(self.seen, "the history table")
        dev = self.seen.device
        n = self.B if rows is None else len(rows)
        tokens = _token_rows(tokens, dev)
        if tokens is not None and tokens.shape[0] != n:
            raise ValueError(f"{tokens.shape[0]} rows of token ids for {n} rows of the sampler")
        if tokens is None and not flags & SEEN_CLEAR:
            return
        rows_t = None if rows is None else torch.tensor(list(rows), dtype=torch.int32).to(dev)
        T = 0 if tokens is None else tokens.shape[1]
        _lib.check(_lib.load().kivi_seen_mark(_lib.ptr(self.seen), self.seen.stride(0), self.vocab_size,
                                              None if rows_t is None else _lib.ptr(rows_t), n,
                                              None if tokens is None else _lib.ptr(tokens), 0 if tokens is None else tokens.stride(0),
                                              T, None if lead is None or tokens is None else _lib.ptr(lead), flags,
                                              _lib.stream_ptr(self.seen)),
                   "kivi_seen_mark")

    def observe_prompt(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                       lead: Optional[torch.Tensor] = None) -> None:
        """Marks `input_ids` (B, T) as the rows' prompts (bit 15 of the tokens' words; what the table holds stays).  The pads of a
        left-padded batch are not marked: `attention_mask`, HF's 2D (B, T) mask, or `lead`, (B,) int32 on the device, the leading
        pads of every row -- never read on the host.  A sampler without a table has nothing to mark."""
        if self.seen is None:
            return
        if input_ids.dim() != 2 or input_ids.shape[0] != self.B:
            raise ValueError(f"input_ids (B = {self.B}, T) expected, got {tuple(input_ids.shape)}")
        if attention_mask is not None:
            if lead is not None:
                raise ValueError("pass either attention_mask= or lead=, not both")
            if tuple(attention_mask.shape) != tuple(input_ids.shape):
                raise ValueError(f"the 2D attention mask should be of size {tuple(input_ids.shape)}, but is "
                                 f"{tuple(attention_mask.shape)}")
            from .generation import leading_pads
            lead = leading_pads(attention_mask.to(self.seen.device))
        if lead is not None:
            if lead.dtype != torch.int32 or tuple(lead.shape) != (self.B,) or lead.device != self.seen.device:
                raise ValueError(f"lead has to be ({self.B},) int32 on {self.seen.device}")
            lead = lead.contiguous()
        self._mark(SEEN_PROMPT, input_ids, lead=lead)

    def set_row(self, b: int, params: SamplingParams, stream: int = 0, draw_index: int = 0, prompt=None, generated=None,
                suppress=None) -> None:
        """A new request takes over row b: its record is rewritten and its draw index set to `draw_index` (default 0; a scheduler
        that has drawn the request's first tokens elsewhere passes how many), by asynchronous copies on the current stream (ordered
        after the calls already enqueued there); no other row is touched and nothing has to be captured again.
        With a history table the row's penalty record is rewritten too, and its row of the table is cleared and marked again:
        `prompt`, the request's prompt tokens (1-D, no pads), `generated`, the tokens it has emitted so far (1-D; duplicates
        count).  Without a table they are ignored, and penalised `params` are a ValueError.
        With constraint state the row's constraint record, list and mask row are rewritten too, and nothing else: `suppress`, the
        ids `params.min_new_tokens` masks (the request's eos / stop ids); suppress_until = draw_index - len(generated) +
        min_new_tokens, the request's first draw plus its minimum.  Without that state constrained `params` are a ValueError."""
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.B:
            raise ValueError(f"row {b!r} outside [0, {self.B})")
        if not isinstance(params, SamplingParams):
            raise ValueError("params has to be a SamplingParams")
        stream = _check_stream(stream)
        if isinstance(draw_index, bool) or not isinstance(draw_index, int) or not 0 <= draw_index < 2 ** 63:
            raise ValueError(f"draw_index has to be an integer in [0, 2^63), got {draw_index!r}")
        if self.seen is None and params.penalised:
            raise ValueError("params carry a repetition / presence / frequency penalty, but this RowSampler has no history table: "
                             "pass vocab_size= when it is made")
        if self._con is None and params.constrained:
            raise ValueError("params carry a logit_bias, allowed_token_ids or min_new_tokens, but this RowSampler has no constraint "
                             "state: pass vocab_size= and constraints=True when it is made")
        if self._con is not None:
            params.check_vocab(self.vocab_size)
            entries = constraint_list(params, () if suppress is None else
                                      [int(t) for t in (suppress.tolist() if torch.is_tensor(suppress) else suppress)])
        p = self._bind(params)
        _upload(self.records[b], _record(p, stream))
        self.draw_index[b: b + 1].fill_(draw_index)
        if self.seen is not None:
            _upload(self.penalties[b], _penalty_record(p))
            self._mark(SEEN_CLEAR | SEEN_PROMPT, prompt, rows=[b])
            self._mark(SEEN_OUTPUT, generated, rows=[b])
        if self._con is not None:
            done = 0 if generated is None else int(torch.as_tensor(generated).numel())
            self._con[b] = dict(mask=p.allowed_token_ids is not None, list=entries, min_new=p.min_new_tokens,
                                until=max(draw_index - done, 0) + p.min_new_tokens)
            self._bind_constraint(b, p.allowed_token_ids)
        self.params[b], self.streams[b] = p, stream

    def reset(self) -> None:
        """All draw indices back to 0 (the records stay); the history table, if there is one, back to all zeros; the constraint
        records, if there are any, count their min_new_tokens from draw 0 again (masks and lists stay)."""
        self.draw_index.zero_()
        if self.seen is not None:
            self.seen.zero_()
        if self._con is not None:
            for c in self._con:
                c["until"] = c["min_new"]
            self.constraint.copy_(torch.stack([self._con_record(c) for c in self._con]))

    def select(self, idx, streams: Optional[Sequence[int]] = None) -> "RowSampler":
        """A new RowSampler (its own buffers) whose row i is this one's row idx[i], seeds, draw indices, penalty records and rows of
        the history table, constraint records, allow masks and lists included: the sampler side of a cache fork by index_select.  `streams`: new streams for the rows
        (default: those of the source rows)."""
        idx = [int(i) for i in (idx.tolist() if torch.is_tensor(idx) else idx)]
        if not idx or not all(0 <= i < self.B for i in idx):
            raise ValueError(f"idx has to be a non-empty sequence of rows in [0, {self.B})")
        new = RowSampler([self.params[i] for i in idx], self.records.device,
                         [self.streams[i] for i in idx] if streams is None else streams, vocab_size=self.vocab_size,
                         constraints=self._con is not None)
        at = torch.tensor(idx, device=self.draw_index.device)
        new.draw_index.copy_(self.draw_index.index_select(0, at))
        if self.seen is not None:
            new.seen.copy_(self.seen.index_select(0, at))
        if self._con is not None:
            new._con = [dict(self._con[i]) for i in idx]
            for dst, src in ((new.constraint, self.constraint), (new.allowed, self.allowed), (new.bias_list, self.bias_list)):
                dst.copy_(src.index_select(0, at))
        return new

    def __call__(self, logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """As Sampler.__call__: one token per row into (B, 1) int64 (`out` when given), in ONE launch: kivi_sample_rows, or -- exactly
        when the sampler has a history table -- kivi_sample_rows_pen, which also counts the tokens in the table, or -- exactly when
        it has constraint state -- kivi_sample_rows_con, which does that too."""
        logits, out = _call_args(logits, out, self)
        if self.seen is not None and logits.shape[1] > self.vocab_size:
            raise ValueError(f"logits of {logits.shape[1]} tokens do not fit the history table of this RowSampler "
                             f"(vocab_size={self.vocab_size})")
        name, args = self.entry(logits, out)
        _lib.check(getattr(_lib.load(), name)(*args), name)
        return out

    def entry(self, logits: torch.Tensor, out: torch.Tensor):
        """(the name of the entry a call goes through, its arguments) for checked `logits` (B, V) and `out`, on the current stream:
        the common arguments, then the penalty records and the history table when there is one, then the constraint records, allow
        masks and lists when there are any."""
        B, V = logits.shape
        name, args = "kivi_sample_rows", (_lib.ptr(logits), _lib.LOGITS_BITS[logits.dtype], logits.stride(0), B, V,
                                          _lib.ptr(self.records), _lib.ptr(self.draw_index))
        if self.seen is not None:
            name, args = "kivi_sample_rows_pen", args + (_lib.ptr(self.penalties), _lib.ptr(self.seen), self.seen.stride(0))
        if self._con is not None:
            name, args = "kivi_sample_rows_con", args + (_lib.ptr(self.constraint), _lib.ptr(self.allowed), self.allowed.stride(0),
                                                         _lib.ptr(self.bias_list), self.bias_list.stride(0) // 2)
        return name, args + (_lib.ptr(out), out.stride(0) if out.dim() else 1, _lib.stream_ptr(logits))


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


def reference_penalise(logits: torch.Tensor, prompt_mask: torch.Tensor, counts: torch.Tensor, theta, presence, frequency) -> torch.Tensor:
    """The penalised logit of kivi_sample_rows_pen (include/kivi_hip.h) restated in torch fp32 on the CPU, one
    separately rounded operation per step as in the kernel, so the result is the kernel's bit for bit: (B, V) fp32.
    `logits` (B, V) fp16 / fp32; `prompt_mask` (B, V) bool, the token is in the row's prompt (bit 15 of the history word); `counts`
    (B, V) integers, how often the row has emitted it (bits 0-14); `theta`, `presence`, `frequency`: a number or one per row.
    seen_words() takes a history table apart into the two."""
    x = logits.detach().cpu().float()
    B = x.shape[0]

    def col(v):
        return torch.as_tensor(v, dtype=torch.float32).reshape(-1, 1).expand(B, 1)
    theta, presence, frequency = col(theta), col(presence), col(frequency)
    c = counts.detach().cpu().to(torch.int64)
    seen = prompt_mask.detach().cpu().bool() | (c > 0)
    x = torch.where(seen, torch.where(x > 0, x / theta, x * theta), x)
    x = x - frequency * c.float()
    return torch.where(c > 0, x - presence, x)


def reference_constrain(logits: torch.Tensor, lists=None, suppressing=None, allow=None, penalties=None) -> torch.Tensor:
    """The rule of kivi_sample_rows_con (include/kivi_hip.h) restated in torch fp32 on the CPU, one separately
    rounded operation per step as in the kernel: the fp32 logits (B, V) that kivi_sample_rows draws the kernel's tokens from.
    `lists`: None, or per row None / a sequence of (token, value, suppressed) -- constraint_list()'s result; ids >= V are skipped
    and a NaN value reads as 0, as in the kernel.  `suppressing`: None (no row), one bool or one per row: draw_index <
    suppress_until.  `allow`: None, or per row None (no mask in force) / a (V,) bool tensor / an int32 bitmask in allow_bitmask()'s
    layout.  `penalties`: None, or reference_penalise's arguments after `logits` -- (prompt_mask, counts, theta, presence,
    frequency) -- applied between the bias and the masks."""
    x = logits.detach().cpu().float().clone()
    B, V = x.shape
    masked = torch.zeros((B, V), dtype=torch.bool)
    if suppressing is None or isinstance(suppressing, bool):
        suppressing = [bool(suppressing)] * B
    for b in range(B):
        for t, v, sup in (lists[b] if lists is not None and lists[b] is not None else ()):
            if not 0 <= t < V:
                continue
            if sup and suppressing[b]:
                masked[b, t] = True
            else:
                x[b, t] = x[b, t] + torch.tensor(0.0 if math.isnan(v) else v, dtype=torch.float32)
    if penalties is not None:
        x = reference_penalise(x, *penalties)
    for b in range(B):
        a = None if allow is None else allow[b]
        if a is None:
            continue
        a = torch.as_tensor(a)
        if a.dtype != torch.bool:
            words = a.detach().cpu().to(torch.int64) & 0xFFFFFFFF
            a = ((words[torch.arange(V) >> 5] >> (torch.arange(V) & 31)) & 1).bool()
        masked[b] |= ~a[:V].cpu()
    return x.masked_fill(masked, float("-inf"))


def seen_words(seen: torch.Tensor, V: Optional[int] = None):
    """A history table (B, stride) int16 -> (prompt_mask (B, V) bool, counts (B, V) int64) on the CPU."""
    w = seen.detach().cpu().to(torch.int64) & 0xFFFF
    w = w if V is None else w[:, :V]
    return (w & SEEN_PROMPT_BIT) != 0, w & SEEN_COUNT_MAX
