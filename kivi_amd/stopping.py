"""What decides that a request is finished: stop token ids, stop sequences and a length limit per request.

ONE rule, stated three times: `StopState` / `reference_stop` in pure Python (the reference, and what generate_continuous runs on the
tokens its scheduler reads anyway), `kivi_stop_rows` on the device (include/kivi_hip.h, kivi_amd/csrc/kivi_stop.hip), and `StopRows`,
the host class that owns the kernel's buffers -- the analogue of sampling.RowSampler: per-row records in device memory, advanced by
one launch inside a captured step, rebound in place with set_row().

The rule, for one request that has produced tokens t_0 .. t_{p-1} since it was bound and now produces t:
  * the request has finished: nothing changes (a batch row then gets `pad`);
  * otherwise p += 1 and the request finishes if (a) t is one of its stop ids -- reason TOKEN, index = the lowest position in the id
    list --, else (b) one of its sequences of length m <= p equals the last m produced tokens -- reason SEQUENCE, index = the lowest
    such sequence --, else (c) p == limit -- reason LENGTH, index -1.  t itself is part of the output.
Only tokens produced since the binding count: a sequence never matches across two requests that used the same row, nor into a prompt.
"""
from __future__ import annotations

import ctypes
import dataclasses
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

LIVE, TOKEN, SEQUENCE, LENGTH = 0, 1, 2, 3          # include/kivi_hip.h: KIVI_STOP_*
MAX_IDS, MAX_SEQS, MAX_LEN = _lib.STOP_MAX_IDS, _lib.STOP_MAX_SEQS, _lib.STOP_MAX_LEN
NO_LIMIT = 2 ** 31 - 1                              # the limit of a record without max_new_tokens
SYNC_EVERY = 1                                      # a graphed decode reads n_live before every SYNC_EVERY-th step (measured: DESIGN.md section 24)


def check_sync_every(sync_every) -> None:
    if sync_every is not None and (isinstance(sync_every, bool) or not isinstance(sync_every, int) or sync_every < 1):
        raise ValueError(f"sync_every has to be None (never look) or a positive integer, got {sync_every!r}")


class StopParamsRecord(ctypes.Structure):
    """include/kivi_hip.h: kivi_stop_params (624 bytes)."""
    _fields_ = [("n_ids", ctypes.c_int32), ("n_seqs", ctypes.c_int32), ("limit", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ids", ctypes.c_int32 * MAX_IDS), ("seq_len", ctypes.c_int32 * MAX_SEQS),
                ("seq", (ctypes.c_int32 * MAX_LEN) * MAX_SEQS)]


class StopStateRecord(ctypes.Structure):
    """include/kivi_hip.h: kivi_stop_state (80 bytes)."""
    _fields_ = [("produced", ctypes.c_int32), ("reason", ctypes.c_int32), ("index", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ring", ctypes.c_int32 * MAX_LEN)]


PARAM_WORDS, STATE_WORDS = ctypes.sizeof(StopParamsRecord) // 4, ctypes.sizeof(StopStateRecord) // 4
assert (PARAM_WORDS, STATE_WORDS) == (156, 20)


def _token_id(x, what: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < 2 ** 31:
        raise ValueError(f"{what} has to be a token id, an integer in [0, 2^31), got {x!r}")
    return int(x)


@dataclasses.dataclass(frozen=True)
class StopParams:
    """The finish conditions of one request: `stop_token_ids` (at most 16 ids), `stop_sequences` (at most 8 sequences of 1 to 16
    token ids each) and `max_new_tokens` (None, or the number of tokens it may produce, >= 1).  Validated here; stored as tuples."""
    stop_token_ids: Tuple[int, ...] = ()
    stop_sequences: Tuple[Tuple[int, ...], ...] = ()
    max_new_tokens: Optional[int] = None

    def __post_init__(self):
        ids, seqs, limit = self.stop_token_ids, self.stop_sequences, self.max_new_tokens
        if torch.is_tensor(ids):
            ids = ids.tolist()
        if isinstance(ids, (int, np.integer)) and not isinstance(ids, bool):
            ids = (ids,)
        if not isinstance(ids, (list, tuple)):
            raise ValueError(f"stop_token_ids has to be a sequence of token ids, got {ids!r}")
        ids = tuple(_token_id(t, "a stop token id") for t in ids)
        if len(ids) > MAX_IDS:
            raise ValueError(f"{len(ids)} stop token ids: at most {MAX_IDS} (KIVI_STOP_MAX_IDS)")
        if not isinstance(seqs, (list, tuple)):
            raise ValueError(f"stop_sequences has to be a sequence of token id sequences, got {seqs!r}")
        out = []
        for s in seqs:
            if torch.is_tensor(s):
                s = s.tolist()
            if not isinstance(s, (list, tuple)):
                raise ValueError(f"a stop sequence has to be a sequence of token ids, got {s!r}")
            if not s:
                raise ValueError("an empty stop sequence would match everything: leave it out")
            if len(s) > MAX_LEN:
                raise ValueError(f"a stop sequence of {len(s)} tokens: at most {MAX_LEN} (KIVI_STOP_MAX_LEN)")
            out.append(tuple(_token_id(t, "a token of a stop sequence") for t in s))
        if len(out) > MAX_SEQS:
            raise ValueError(f"{len(out)} stop sequences: at most {MAX_SEQS} (KIVI_STOP_MAX_SEQS)")
        if limit is not None and (isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 1 <= limit <= NO_LIMIT):
            raise ValueError(f"max_new_tokens has to be None or an integer in [1, 2^31), got {limit!r}")
        object.__setattr__(self, "stop_token_ids", ids)
        object.__setattr__(self, "stop_sequences", tuple(out))
        object.__setattr__(self, "max_new_tokens", None if limit is None else int(limit))

    @property
    def limit(self) -> int:
        return NO_LIMIT if self.max_new_tokens is None else self.max_new_tokens

    def capped(self, max_new_tokens: Optional[int]) -> "StopParams":
        """The same conditions with the limit min(own, max_new_tokens)."""
        if max_new_tokens is None or self.limit <= max_new_tokens:
            return self
        return dataclasses.replace(self, max_new_tokens=max_new_tokens)

    def check_vocab(self, vocab_size: Optional[int]) -> None:
        if vocab_size is None:
            return
        worst = max(self.stop_token_ids + tuple(t for s in self.stop_sequences for t in s), default=-1)
        if worst >= vocab_size:
            raise ValueError(f"stop token id {worst} outside the vocabulary [0, {vocab_size})")

    def record(self) -> np.ndarray:
        """The 624 bytes of kivi_stop_params as 156 int32."""
        rec = StopParamsRecord(len(self.stop_token_ids), len(self.stop_sequences), self.limit, 0)
        for j, t in enumerate(self.stop_token_ids):
            rec.ids[j] = t
        for j, s in enumerate(self.stop_sequences):
            rec.seq_len[j] = len(s)
            for i, t in enumerate(s):
                rec.seq[j][i] = t
        return np.frombuffer(bytes(rec), dtype=np.int32)


# ------------------------------------------------------------------ the rule in Python
class StopState:
    """The rule of the module docstring for ONE request, token by token: `push(t)` -> the reason after t (LIVE: go on).  Holds what
    the kernel's state record holds: `produced`, the last 16 produced tokens, `reason`, `index`."""

    def __init__(self, params: StopParams):
        self.params, self.produced, self.last, self.reason, self.index = params, 0, [], LIVE, -1

    def push(self, t: int) -> int:
        if self.reason != LIVE:
            return self.reason
        p = self.params
        self.produced += 1
        self.last = (self.last + [int(t)])[-MAX_LEN:]
        if t in p.stop_token_ids:
            self.reason, self.index = TOKEN, p.stop_token_ids.index(t)
            return self.reason
        for j, s in enumerate(p.stop_sequences):
            if len(s) <= self.produced and tuple(self.last[-len(s):]) == s:
                self.reason, self.index = SEQUENCE, j
                return self.reason
        if self.produced == p.limit:
            self.reason = LENGTH
        return self.reason


def reference_stop(tokens: Sequence[int], params: StopParams) -> Tuple[int, int, int]:
    """(length, reason, index) of one request's token stream under the rule: `length` tokens belong to the output -- the stop token,
    or the last token of the matched sequence, is token length - 1 --, and nothing after them changes the result.  A stream that
    ends before the request has finished: (len(tokens), LIVE, -1)."""
    st = StopState(params)
    for t in tokens:
        if st.push(int(t)) != LIVE:
            break
    return st.produced, st.reason, st.index


# ------------------------------------------------------------------ the device tracker
def _params_list(params, B: Optional[int]) -> List[StopParams]:
    if isinstance(params, StopParams):
        if B is None:
            B = 1
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"B has to be a positive integer, got {B!r}")
        return [params] * B
    if not isinstance(params, (list, tuple)) or not params or not all(isinstance(p, StopParams) for p in params):
        raise ValueError("params has to be a StopParams or a non-empty sequence of them")
    if B is not None and B != len(params):
        raise ValueError(f"{len(params)} StopParams for B={B} rows")
    return list(params)


def _fresh_state(n: int) -> torch.Tensor:
    st = torch.zeros((n, STATE_WORDS), dtype=torch.int32)
    st[:, 2] = -1
    return st


class StopRows:
    """The finish tracker of a batch of B rows (kivi_stop_rows): owns `params` (B, 156) int32, one kivi_stop_params per row, `state`
    (B, 20) int32, one kivi_stop_state per row, and `n_live` (1,) int32, the number of live rows of the table, all in device memory.
    `params`: one StopParams for every row, or a sequence of B of them (`B`: the row count for a single one, default 1);
    `vocab_size`: ids at or above it are refused.  Every argument is checked before a device is touched.
    A call advances the state by one token per row in one launch and writes `pad` over the tokens of finished rows; a captured
    graph holds what key() names, so set_row() / rebind() / reset() replay it."""

    def __init__(self, params: Union[StopParams, Sequence[StopParams]], device="cuda", vocab_size: Optional[int] = None,
                 pad_token_id: int = 0, B: Optional[int] = None):
        params = _params_list(params, B)
        if len(params) > _lib.SAMPLE_MAX_B:
            raise ValueError(f"{len(params)} rows: at most {_lib.SAMPLE_MAX_B}")
        if vocab_size is not None and (isinstance(vocab_size, bool) or not isinstance(vocab_size, int) or vocab_size < 1):
            raise ValueError(f"vocab_size has to be None or a positive integer, got {vocab_size!r}")
        for p in params:
            p.check_vocab(vocab_size)
        self.rows, self.vocab_size, self.pad_token_id = params, vocab_size, self._check_pad(pad_token_id)
        self.params = torch.from_numpy(np.stack([p.record() for p in params])).to(device)
        self.state = _fresh_state(len(params)).to(device)
        self.n_live = torch.full((1,), len(params), dtype=torch.int32, device=device)

    @staticmethod
    def _check_pad(pad) -> int:
        if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or not -2 ** 63 <= pad < 2 ** 63:
            raise ValueError(f"pad_token_id has to be an integer, got {pad!r}")
        return int(pad)

    @property
    def B(self) -> int:
        return len(self.rows)

    def key(self):
        """What a captured call depends on: the number of rows, the three buffers and the pad (a kernel argument) -- not the values
        in the records, which a replay reads."""
        return ("stop", self.B, self.params.data_ptr(), self.state.data_ptr(), self.n_live.data_ptr(), self.pad_token_id)

    def _upload(self, dst: torch.Tensor, src: torch.Tensor) -> None:
        dst.copy_(src.pin_memory() if dst.is_cuda else src, non_blocking=True)

    def _count(self) -> None:
        """n_live from the table as it stands: a call without entries (ordered after the copies on the current stream)."""
        self(None)

    def set_row(self, b: int, params: StopParams) -> None:
        """A new request takes over row b: its parameter record is rewritten and its state reset (nothing produced, live), by
        asynchronous copies on the current stream, and n_live is counted again; no other row is touched, nothing is captured again."""
        if isinstance(b, bool) or not isinstance(b, int) or not 0 <= b < self.B:
            raise ValueError(f"row {b!r} outside [0, {self.B})")
        if not isinstance(params, StopParams):
            raise ValueError("params has to be a StopParams")
        params.check_vocab(self.vocab_size)
        self._upload(self.params[b], torch.from_numpy(params.record().copy()))
        self._upload(self.state[b], _fresh_state(1)[0])
        self.rows[b] = params
        self._count()

    def rebind(self, params: Union[StopParams, Sequence[StopParams]]) -> None:
        """set_row for every row at once (one copy per table): B new requests."""
        params = _params_list(params, self.B if isinstance(params, StopParams) else None)
        if len(params) != self.B:
            raise ValueError(f"{len(params)} StopParams for the {self.B} rows of this StopRows")
        for p in params:
            p.check_vocab(self.vocab_size)
        self._upload(self.params, torch.from_numpy(np.stack([p.record() for p in params])))
        self.rows = params
        self.reset()

    def reset(self) -> None:
        """Every row live again with nothing produced (the parameter records stay)."""
        self._upload(self.state, _fresh_state(self.B))
        self.n_live.fill_(self.B)

    def __call__(self, tok: Optional[torch.Tensor], rows: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """One kivi_stop_rows launch on the current stream.  `tok`: (n, 1) or (n,) int64 on the device, the token just picked for
        every entry, rewritten in place (pad where the row had finished).  `rows`: None -- entry i is row i, n <= B -- or n int32 /
        int64 indices on the device: entry i serves row rows[i] (an index outside [0, B) leaves the entry unused).  None for `tok`:
        no entry, n_live is counted.  Returns `tok`."""
        _lib.require_gpu(self.state, "the finish tracker")
        n, stride, rows_bytes = 0, 1, 4
        if tok is not None:
            if tok.dtype != torch.int64 or tok.device != self.state.device or tok.dim() not in (1, 2) or \
                    (tok.dim() == 2 and tok.shape[1] != 1):
                raise ValueError(f"tok has to be (n, 1) or (n,) int64 on {self.state.device}, got {tuple(tok.shape)} {tok.dtype} "
                                 f"on {tok.device}")
            n, stride = tok.shape[0], max(tok.stride(0), 1)
            if rows is not None:
                if rows.dtype not in (torch.int32, torch.int64) or rows.device != self.state.device or rows.dim() != 1 or \
                        rows.shape[0] != n or not rows.is_contiguous():
                    raise ValueError(f"rows has to be ({n},) int32 or int64, contiguous, on {self.state.device}")
                rows_bytes = rows.element_size()
            elif n > self.B:
                raise ValueError(f"{n} tokens for the {self.B} rows of this StopRows")
        _lib.check(_lib.load().kivi_stop_rows(None if n == 0 else _lib.ptr(tok), stride, _lib.ptr(self.params), _lib.ptr(self.state),
                                              None if rows is None or n == 0 else _lib.ptr(rows), rows_bytes, n, self.B,
                                              self.pad_token_id, _lib.ptr(self.n_live), _lib.stream_ptr(self.state)),
                   "kivi_stop_rows")
        return tok

    # read-outs: views of the state table, on the device
    @property
    def length(self) -> torch.Tensor:
        """(B,) int32: the tokens every row has produced -- at the finish, or so far."""
        return self.state[:, 0]

    @property
    def reason(self) -> torch.Tensor:
        """(B,) int32: LIVE (0), TOKEN (1), SEQUENCE (2) or LENGTH (3)."""
        return self.state[:, 1]

    @property
    def index(self) -> torch.Tensor:
        """(B,) int32: the position of the id or the sequence that matched; -1 for LENGTH and for a live row."""
        return self.state[:, 2]


# ------------------------------------------------------------------ the arguments of a generate call
def stop_ids(eos_token_id, stop_token_ids) -> Tuple[int, ...]:
    """eos_token_id (None, an int or a list) followed by stop_token_ids (None or a list): the stop ids of a call."""
    def as_list(x, name):
        if x is None:
            return []
        if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            return [x]
        if torch.is_tensor(x):
            return x.flatten().tolist()
        if not isinstance(x, (list, tuple)):
            raise ValueError(f"{name} has to be None, a token id or a list of token ids, got {x!r}")
        return list(x)
    return tuple(_token_id(t, "a stop token id") for t in as_list(eos_token_id, "eos_token_id") + as_list(stop_token_ids, "stop_token_ids"))


def resolve_stopping(B: int, max_new_tokens: int, eos_token_id=None, pad_token_id=None, stop_token_ids=None, stop_sequences=None,
                     stopping=None, num_beams: int = 1, vocab_size: Optional[int] = None, fan: int = 1, torch_eos: bool = True):
    """The finish conditions of a generate / generate_graphed call over B requests with `fan` rows each -> None (the call as it was:
    no condition, or -- `torch_eos` -- one int `eos_token_id` alone, which keeps the loop's torch path), a list of B * fan StopParams
    (limits capped at the call's max_new_tokens), or the caller's StopRows of B * fan rows, used as it is (its state is not reset).
    ValueError, before any device work, for `stopping=` combined with the keyword forms, anything but one eos_token_id with beams, a
    missing pad_token_id, counts that do not fit."""
    keywords = stop_token_ids is not None or (stop_sequences is not None and len(stop_sequences) > 0)
    single_eos = isinstance(eos_token_id, (int, np.integer)) and not isinstance(eos_token_id, bool)
    if stopping is None and not keywords and (eos_token_id is None or (single_eos and (torch_eos or num_beams != 1))):
        return None
    if stopping is not None and (keywords or eos_token_id is not None):
        raise ValueError("stopping= carries the finish conditions of every row: it cannot be combined with eos_token_id, "
                         "stop_token_ids or stop_sequences")
    if num_beams != 1:
        if stopping is not None or (stop_sequences is not None and len(stop_sequences) > 0):
            raise ValueError(f"stop_sequences / stopping= with beam search (num_beams={num_beams}) are not supported: beam search "
                             "keeps its own eos_token_id handling")
        raise ValueError(f"beam search (num_beams={num_beams}) takes one eos_token_id; lists of ids and stop_token_ids are for greedy "
                         "decoding and sampling")
    if pad_token_id is None:
        raise ValueError("finish conditions need a pad_token_id for the rows that have finished")
    StopRows._check_pad(pad_token_id)
    if isinstance(stopping, StopRows):
        if stopping.B != B * fan:
            raise ValueError(f"the StopRows holds {stopping.B} rows; the call has {B * fan}")
        if stopping.pad_token_id != pad_token_id:
            raise ValueError(f"the StopRows pads with {stopping.pad_token_id}, the call with pad_token_id={pad_token_id}")
        return stopping
    if stopping is None:
        stopping = [StopParams(stop_ids(eos_token_id, stop_token_ids), stop_sequences or (), max_new_tokens or None)] * B
    elif isinstance(stopping, StopParams):
        stopping = [stopping] * B
    elif not isinstance(stopping, (list, tuple)) or not all(isinstance(p, StopParams) for p in stopping):
        raise ValueError("stopping has to be a StopParams, a list of B of them, or a StopRows")
    if len(stopping) != B:
        raise ValueError(f"{len(stopping)} StopParams for a batch of {B} requests")
    out = []
    for p in stopping:
        p.check_vocab(vocab_size)
        out += [p.capped(max_new_tokens or None)] * fan
    return out
