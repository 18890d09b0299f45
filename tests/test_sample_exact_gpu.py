"""GPU: the fused samplers (kivi_sample, kivi_sample_rows, kivi_sample_rows_pen) against EXACT expectations at every vocabulary
boundary of tests/sample_plan.py -- no tolerance anywhere in this file.

The header fixes the arithmetic: weights are floor(exp(s - max) * 2^40), the token is the first one in vocabulary order whose
inclusive running sum exceeds floor(S * u24 / 2^24).  A planted row has three levels: a top class of one value on an index set P
(n_a tokens), a floor class at least 80 logit units lower (weight exactly 0 at every temperature used here -- exp(-80 / 1.7) * 2^40
is 4e-9 -- but counted by top-k), and -inf elsewhere.  Every kept weight is then exactly 2^40, S = n_a * 2^40, and the token is
sorted(P)[(n_a * u24) >> 24] with u24 = philox_x0(...) >> 8 from the numpy Philox: integers on both sides.

1. Plants from the launch geometry (token 0, token V - 1, the last bucket alone, both sides of the first / a middle / the last
   bucket boundary, the ends of every wave segment, one token per segment, the uniform row, a random third), three top values
   (1.5, -3.25, a mix of +0 and -0), fp16 and fp32, a strided (B, 1, V + 40) view, twelve parameter sets that leave exactly the top
   class drawable, draw indices that reach the smallest and the largest u24 of 4096 and n = 2^32 + 3 -- through Sampler and through
   RowSampler with streams.
2. The same plants through the penalised entry, the levels made by the history table from a flat row: unseen tokens stay, counted
   tokens fall by presence_penalty = 80, prompt tokens at 3.0 (-0.75) join the top class at exactly 1.5 (-1.5) under
   repetition_penalty = 2.  The draw index advances by one, the drawn token's history word by one, no other word changes.
3. Greedy rows at every V: the maximum at V - 1, a tie across a bucket boundary (the lowest index wins), one finite entry among
   -inf, a -0 / +0 tie; plain, with a neutral table, and penalised (against reference_penalise, fp32 for fp32).
4. The chunk bitmap of the penalised kernel at awkward V, with the table's pad words [V, stride) set to 0xFFFF and canaries around
   the table; kivi_seen_mark at an odd V = 2^20 - 1.
Every V of sample_plan.VS; B = 3 (4 for greedy rows)."""
import functools

import numpy as np
import pytest
import torch

from sample_plan import VS, boundaries, last_bucket, plan
from test_sample_penalty_gpu import _canaries_intact, _canary_table, _from_table, _mark, _to_table

pytestmark = pytest.mark.gpu

NEG = -float("inf")
PROMPT, COUNT = 0x8000, 0x7FFF
SEARCH, NBIG = 4096, 2 ** 32 + 3
SEED, SEED_ROWS = 0x5EED_0123_4567_89AB, 2 ** 64 - 7
STREAMS = (5, 2 ** 32 - 1, 17)
TOPS = [(1.5, -78.5, False), (-3.25, -83.25, False), (0.0, -80.0, True)]      # (top value, floor value, every other top token -0)


# ------------------------------------------------------------------ the draws, on the CPU
@functools.lru_cache(maxsize=None)
def _u24_table(seed, counters):
    """(SEARCH, len(counters)) u24 of the draws n = 0 .. SEARCH - 1 at Philox counter word 0 = counters[i]."""
    from kivi_amd.sampling import philox_x0
    c = np.array(counters, dtype=np.uint64)
    return np.stack([philox_x0(seed, c, n) >> 8 for n in range(SEARCH)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _u24(seed, counter, n):
    """u24 of draw n at Philox counter word 0 = counter (the row of kivi_sample, the stream of kivi_sample_rows)."""
    from kivi_amd.sampling import philox_x0
    return int(philox_x0(seed, [counter], n)[0] >> 8)


def _extremes(seed, counters):
    """Per counter, the n in [0, SEARCH) with the smallest and with the largest u24."""
    t = _u24_table(seed, counters)
    return [int(n) for n in t.argmin(0)], [int(n) for n in t.argmax(0)]


def _token(P, u24):
    return int(P[(len(P) * u24) >> 24])


# ------------------------------------------------------------------ the plants
def _plants(V):
    """name -> sorted index set P (int64 array) of the top class."""
    p = plan(V)
    rng = np.random.default_rng(V)
    out = {"token 0": [0], "token V-1": [V - 1], "last bucket": range(last_bucket(V)[0], V)}
    for b in boundaries(V):
        out[f"boundary {b}"] = [b - 1, b]
    segs = [(a, b) for a, b in p.segments if b > a]
    out["segment ends"] = sorted({x for a, b in segs for x in (a, b - 1)})
    out["one per segment"] = [a + (37 * w + 11) % (b - a) for w, (a, b) in enumerate(segs)]
    out["uniform"] = range(V)
    third = np.flatnonzero(rng.random(V) < 1 / 3)
    out["random third"] = third if len(third) else [V // 2]
    return {k: np.asarray(sorted(v), dtype=np.int64) for k, v in out.items()}


def _planted_rows(V, P, rng, near=False):
    """(3, V) fp32 on the CPU: the three top values on P, their floor on P's neighbours, on both ends of the row and on a random
    fifth of the rest, -inf elsewhere.  Every value is an fp16 number.  `near`: the lower class lies one unit below the top class
    instead -- a positive weight, so a filter that lets it in changes the draw."""
    top = np.zeros(V, dtype=bool)
    top[P] = True
    fl = rng.random(V) < 0.2
    fl[1:] |= top[:-1]
    fl[:-1] |= top[1:]
    fl[0] = fl[-1] = True
    fl &= ~top
    rows = np.full((len(TOPS), V), NEG, dtype=np.float32)
    for r, (c, floor, zeros) in enumerate(TOPS):
        rows[r, fl] = c - 1.0 if near else floor
        rows[r, top] = c
        if zeros:
            rows[r, P[::2]] = -0.0
    return torch.from_numpy(rows)


def _strided(x, dtype):
    """(B, V) on the CPU -> a (B, 1, V) view on the GPU with row stride V + 40 and an odd element offset."""
    B, V = x.shape
    buf = torch.zeros((B, 1, V + 40), dtype=dtype, device="cuda")
    view = buf[..., 7: 7 + V]
    view.copy_(x.to(dtype)[:, None])
    assert torch.equal(view[:, 0].float().cpu().nan_to_num(neginf=-1e30), x.nan_to_num(neginf=-1e30))       # exact in fp16
    return view


def _param_sets(n_a):
    """(temperature, top_k, top_p, min_p): each leaves exactly the top class drawable.  top_k = n_a - 1 cuts inside the tie class
    (0, for one token, is off), n_a + 3 takes zero-weight floor tokens (or is clamped to V)."""
    return [(1.0, 0, 1.0, None), (0.7, 0, 1.0, None), (1.7, 0, 1.0, None), (1.0, 1, 1.0, None), (0.7, n_a - 1, 1.0, None),
            (1.7, n_a, 1.0, None), (1.0, n_a + 3, 1.0, None), (0.7, 0, 1e-6, None), (1.7, 0, 0.5, None), (1.0, 0, 0.999, None),
            (0.7, 0, 1.0, 0.5), (1.7, n_a + 3, 0.5, 0.5)]


class _Ledger:
    """Tokens land in one device buffer, call after call, and are compared with the expected ones at the end: one copy per test."""

    def __init__(self, calls, B):
        self.out = torch.full((calls, B, 1), -1, dtype=torch.int64, device="cuda")
        self.want, self.what = [], []

    def slot(self, want, what):
        self.want.append(want)
        self.what.append(what)
        return self.out[len(self.want) - 1]

    def check(self):
        got = self.out[: len(self.want), :, 0].cpu().numpy()
        want = np.array(self.want, dtype=np.int64).reshape(got.shape)
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), (f"{len(bad)} of {len(want)} calls differ",
                              [(self.what[i], got[i].tolist(), want[i].tolist()) for i in bad[:6]])
        return len(self.want)


# ------------------------------------------------------------------ 1. Sampler and RowSampler
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_planted_rows_sampler(V, dtype):
    from kivi_amd.sampling import Sampler
    B = len(TOPS)
    lo, hi = _extremes(SEED, (0, 1, 2))
    ns = sorted(set(lo + hi)) + [NBIG]
    plants = _plants(V)
    led = _Ledger(len(plants) * 12 * len(ns), B)
    rng = np.random.default_rng(V + 1)
    for name, P in plants.items():
        view = _strided(_planted_rows(V, P, rng), dtype)
        for t, k, p, mp in _param_sets(len(P)):
            smp = Sampler(t, int(k), p, mp, seed=SEED)
            for n in ns:
                smp.state[1] = n
                smp(view, out=led.slot([_token(P, _u24(SEED, b, n)) for b in range(B)], (name, t, k, p, mp, n)))
            assert smp.state.tolist() == [SEED, NBIG + 1]
    led.check()
    # the search did its work: the smallest / largest u24 draw the first / last token of every top class of up to 256 tokens
    t = _u24_table(SEED, (0, 1, 2))
    assert (t.min(0) < 2 ** 24 // 256).all() and (t.max(0) >= 2 ** 24 - 2 ** 24 // 256).all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_planted_rows_row_sampler(V, dtype):
    from kivi_amd.sampling import RowSampler, SamplingParams
    B = len(TOPS)
    lo, hi = _extremes(SEED_ROWS, STREAMS)
    draws = [lo, hi, [NBIG] * B]
    plants = _plants(V)
    led = _Ledger(len(plants) * 12 * len(draws), B)
    rng = np.random.default_rng(V + 1)
    for name, P in plants.items():
        view = _strided(_planted_rows(V, P, rng), dtype)
        for t, k, p, mp in _param_sets(len(P)):
            rs = RowSampler(SamplingParams(True, t, int(k), p, mp, SEED_ROWS), "cuda", streams=list(STREAMS))
            for ns in draws:
                rs.draw_index.copy_(torch.tensor(ns, dtype=torch.int64))
                rs(view, out=led.slot([_token(P, _u24(SEED_ROWS, s, n)) for s, n in zip(STREAMS, ns)], (name, t, k, p, mp, ns)))
            assert rs.draw_index.tolist() == [NBIG + 1] * B
    led.check()


def _near_param_sets(n_a):
    """Parameter sets that must cut between the top class and a class ONE unit below it (weight 0.24 to 0.56 of the top's): top_k up
    to n_a (the k-th largest is the top value), the smallest top_p, min_p = 0.5 at the temperatures where exp(-1 / t) < 0.5."""
    return [(1.0, 1, 1.0, None), (0.7, max(n_a - 1, 1), 1.0, None), (1.7, n_a, 1.0, None), (1.0, n_a, 0.999, None),
            (0.7, 0, 1e-6, None), (1.0, 0, 1.0, 0.5), (0.7, n_a, 1e-6, 0.5)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_filters_cut_below_the_top_class(V, dtype):
    """The floor class of the plants above has weight 0, so a filter that keeps too much goes unseen there.  Here the lower class
    has a positive weight and every parameter set has to drop it: the expectation stays the integer formula."""
    from kivi_amd.sampling import RowSampler, SamplingParams
    B = len(TOPS)
    lo, hi = _extremes(SEED_ROWS, STREAMS)
    draws = [lo, hi, [NBIG] * B]
    plants = {k: P for k, P in _plants(V).items() if len(P) < V}
    led = _Ledger(len(plants) * 7 * len(draws) + 1, B)
    rng = np.random.default_rng(V + 3)
    for name, P in plants.items():
        view = _strided(_planted_rows(V, P, rng, near=True), dtype)
        for t, k, p, mp in _near_param_sets(len(P)):
            rs = RowSampler(SamplingParams(True, t, int(k), p, mp, SEED_ROWS), "cuda", streams=list(STREAMS))
            for ns in draws:
                rs.draw_index.copy_(torch.tensor(ns, dtype=torch.int64))
                rs(view, out=led.slot([_token(P, _u24(SEED_ROWS, s, n)) for s, n in zip(STREAMS, ns)], (name, t, k, p, mp, ns)))
    if led.want:
        led.check()


# ------------------------------------------------------------------ 2. the penalised entry: the history makes the levels
PEN = dict(repetition_penalty=2.0, presence_penalty=80.0)
FLAT = [(1.5, 3.0, 0, 2), (-1.5, -0.75, 1, 2), (1.5, 3.0, 0, 3)]             # (flat value, a joiner's logit, joiners = P[first::step])


def _history_rows(V, P, rng):
    """-> (logits (3, V) fp32, history words (3, V) int64).  In P the row is flat, but for the joiners: prompt tokens (bit 15, count
    0) whose logit repetition_penalty = 2 brings to the flat value exactly.  Outside P, half of the tokens keep the flat logit and
    carry a count >= 1 -- presence_penalty = 80 drops them to the floor --, the others are -inf under whatever history."""
    top = np.zeros(V, dtype=bool)
    top[P] = True
    counted = (rng.random(V) < 0.5) & ~top
    dead = ~top & ~counted
    logits = np.empty((len(FLAT), V), dtype=np.float32)
    words = np.zeros((len(FLAT), V), dtype=np.int64)
    some = np.array([1, 5, PROMPT | 3, 32767])[rng.integers(0, 4, V)]
    other = np.array([0, PROMPT, 7, PROMPT | 32767])[rng.integers(0, 4, V)]
    for r, (c, joiner, first, step) in enumerate(FLAT):
        logits[r] = c
        logits[r, dead] = NEG
        logits[r, P[first::step]] = joiner
        words[r, P[first::step]] = PROMPT
        words[r, counted] = some[counted]
        words[r, dead] = other[dead]
    return torch.from_numpy(logits), torch.from_numpy(words)


def _pen_param_sets(n_a):
    return [(1.0, 0, 1.0, None), (0.7, n_a - 1, 1.0, None), (1.7, 0, 0.5, None), (1.0, 0, 1.0, 0.5), (0.7, n_a + 3, 0.5, 0.5)]


class _TableWatch:
    """After a penalised call: the table is the one before the call plus one count at (row, drawn token).  The verdicts stay on the
    device until the end."""

    def __init__(self, calls):
        self.ok = torch.zeros(calls, dtype=torch.bool, device="cuda")
        self.i = 0

    def after(self, seen, before, tok):
        diff = seen.to(torch.int32) - before.to(torch.int32)
        want = torch.zeros_like(diff).scatter_(1, tok.view(-1, 1), 1)
        self.ok[self.i] = (diff == want).all()
        self.i += 1

    def check(self):
        assert bool(self.ok[: self.i].all()), ("history table after call", (~self.ok[: self.i]).nonzero().view(-1).tolist()[:8])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_planted_rows_penalised(V, dtype):
    from kivi_amd.sampling import RowSampler, SamplingParams
    B = len(FLAT)
    lo, hi = _extremes(SEED_ROWS, STREAMS)
    draws = [lo, hi, [NBIG] * B]
    plants = _plants(V)
    led, watch = _Ledger(len(plants) * 5 * len(draws), B), _TableWatch(len(plants) * 5 * len(draws))
    rng = np.random.default_rng(V + 2)
    for name, P in plants.items():
        logits, words = _history_rows(V, P, rng)
        view, before = _strided(logits, dtype), _to_table(words)
        for t, k, p, mp in _pen_param_sets(len(P)):
            rs = RowSampler(SamplingParams(True, t, int(k), p, mp, SEED_ROWS, **PEN), "cuda", streams=list(STREAMS), vocab_size=V)
            for ns in draws:
                rs.draw_index.copy_(torch.tensor(ns, dtype=torch.int64))
                rs.seen.copy_(before)
                tok = rs(view, out=led.slot([_token(P, _u24(SEED_ROWS, s, n)) for s, n in zip(STREAMS, ns)], (name, t, k, p, mp, ns)))
                watch.after(rs.seen, before, tok)
            assert rs.draw_index.tolist() == [NBIG + 1] * B
    led.check()
    watch.check()


# ------------------------------------------------------------------ 3. greedy rows
def _greedy_rows(V):
    """-> ((4, V) fp32 of fp16 values, the expected tokens)."""
    g = torch.Generator().manual_seed(V)
    x = (torch.randn((4, V), generator=g) * 3).half().float()
    x[3] = (-x[3].abs() - 1).half().float()
    top = float((x.max() + 1).half())
    bs = boundaries(V)
    x[0, V - 1] = top                                                        # the maximum in the last place
    tie = [bs[len(bs) // 2] - 1, bs[len(bs) // 2], bs[-1] - 1, bs[-1], V - 1] if bs else [V // 2, V - 1]
    x[1, tie] = top                                                          # a tie across bucket boundaries: the lowest index
    x[2] = NEG
    x[2, (2 * V) // 3] = -7.5                                                # one finite entry
    a = bs[-1] - 1 if bs else 0
    x[3, a], x[3, V - 1] = -0.0, 0.0                                         # -0 and +0 tie (V = 1: one token)
    return x, [V - 1, min(tie), (2 * V) // 3, a]


def _lowest_argmax(x):
    x = x.float()
    return [int((r == r.max()).nonzero()[0]) for r in x]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("V", VS)
def test_greedy_rows(V, dtype):
    from kivi_amd.sampling import RowSampler, SamplingParams, reference_penalise, seen_words
    x, want = _greedy_rows(V)
    assert _lowest_argmax(x) == want
    view = _strided(x, dtype)
    greedy = SamplingParams(do_sample=False)
    for rs in (RowSampler(greedy, "cuda", B=4), RowSampler(greedy, "cuda", B=4, vocab_size=V),
               RowSampler(SamplingParams(do_sample=False, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.25), "cuda",
                          B=4, vocab_size=V)):                               # (the last: the penalised reader over an empty table)
        assert rs(view)[:, 0].tolist() == want and rs.draw_index.tolist() == [1] * 4
        if rs.seen is not None:
            table = _from_table(rs.seen, rs.seen.shape[1])
            assert int(table.sum()) == 4 and table[range(4), want].tolist() == [1] * 4
    # a history that moves the maximum: the winners so far have been emitted once (presence 80), the runners-up are prompt tokens
    rs = RowSampler(SamplingParams(do_sample=False, **PEN), "cuda", B=4, vocab_size=V)
    words = torch.zeros((4, V), dtype=torch.int64)
    words[range(4), want] = 1
    for r, i in enumerate(_lowest_argmax(x.index_put((torch.arange(4), torch.tensor(want)), torch.tensor(NEG)))):
        words[r, i] |= PROMPT
    rs.seen.copy_(_to_table(words))
    for call in range(2):                                                    # the second call reads what the first one counted
        mask, counts = seen_words(rs.seen, V)
        moved = _lowest_argmax(reference_penalise(view[:, 0], mask, counts, 2.0, 80.0, 0.0))
        assert rs(view)[:, 0].tolist() == moved, (call, want, moved)
        words[range(4), moved] += 1
        assert torch.equal(_from_table(rs.seen, V), words) and rs.draw_index.tolist() == [call + 1] * 4


# ------------------------------------------------------------------ 4. the chunk bitmap and the history table
def _bitmap_cases(V):
    """name -> the marked tokens (count >= 1 under presence 80: they fall to the floor; the top class is the rest)."""
    every = np.arange(V)
    cases = {"only V-1": [V - 1], "none": [], "all but V-1": every[:-1], "all but one": np.delete(every, V // 3)}
    for a in (63, 511):
        if a + 1 < V:
            cases[f"only {a}, {a + 1}"] = [a, a + 1]
    return {k: np.asarray(v, dtype=np.int64) for k, v in cases.items()}


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("V", [9, 63, 65, 511, 512, 513, 1025, 65537])
def test_chunk_bitmap_edges(V, extra, dtype):
    from kivi_amd.sampling import RowSampler, SamplingParams
    stride = (V + 7) // 8 * 8 + extra
    cases = _bitmap_cases(V)
    names = list(cases)
    lo, hi = _extremes(SEED_ROWS, STREAMS)
    rng = np.random.default_rng(V)
    led, watch = _Ledger(2 * 3, 3), _TableWatch(2 * 3)
    for at in range(0, len(names), 3):                                       # three rows a launch
        group = (names[at: at + 3] * 3)[:3]
        Ps, words = [], torch.zeros((3, stride), dtype=torch.int64)
        for r, name in enumerate(group):
            marked = cases[name]
            words[r, marked] = torch.from_numpy(np.array([1, 5, PROMPT | 1, 32767])[rng.integers(0, 4, len(marked))])
            Ps.append(np.setdiff1d(np.arange(V), marked))
        words[:, V:] = 0xFFFF                                                # the row's pad words: never read as history, never written
        buf, table = _canary_table(3, stride)
        before = _to_table(words, stride)
        view = _strided(torch.full((3, V), 1.5), dtype)
        rs = RowSampler(SamplingParams(True, 1.0, 0, 1.0, None, SEED_ROWS, presence_penalty=80.0), "cuda", streams=list(STREAMS),
                        vocab_size=V)
        rs.seen = table
        for ns in (lo, hi, [NBIG] * 3):
            rs.draw_index.copy_(torch.tensor(ns, dtype=torch.int64))
            rs.seen.copy_(before)
            tok = rs(view, out=led.slot([_token(P, _u24(SEED_ROWS, s, n)) for P, s, n in zip(Ps, STREAMS, ns)], (group, ns)))
            watch.after(rs.seen, before, tok)                                # (the pad words among them)
        assert _canaries_intact(buf) and bool((rs.seen[:, V:] == -1).all())
    led.check()
    watch.check()


def test_seen_mark_at_an_odd_vocabulary():
    from kivi_amd import _lib
    from kivi_amd.sampling import SEEN_CLEAR, SEEN_OUTPUT, SEEN_PROMPT
    lib = _lib.load()
    V, stride = 1048575, 1048576
    buf, seen = _canary_table(2, stride)
    seen.fill_(0x1234)
    ids = [0, 1, V - 2, V - 1, V, -1]
    toks = torch.tensor([ids + [V - 1, 0, 0], ids[::-1] + [V - 2, V - 2, 1]], device="cuda")
    _mark(lib, seen, V, None, toks, None, SEEN_CLEAR | SEEN_PROMPT)
    want = [{}, {}]
    for r in range(2):
        for t in toks[r].tolist():
            if 0 <= t < V:
                want[r][t] = PROMPT
    _mark(lib, seen, V, None, toks, None, SEEN_OUTPUT)
    for r in range(2):
        for t in toks[r].tolist():
            if 0 <= t < V:
                want[r][t] += 1
    got = seen.cpu().long() & 0xFFFF
    for r in range(2):
        assert {int(i): int(got[r, i]) for i in got[r].nonzero().view(-1)} == want[r], r
    assert int(got[0, V]) == 0 and _canaries_intact(buf)                      # the pad word: cleared, never marked (id V is skipped)
    seen.fill_(-1)
    _mark(lib, seen, V, torch.tensor([1], dtype=torch.int32, device="cuda"), None, None, SEEN_CLEAR)
    assert not seen[1].any() and bool((seen[0] == -1).all()) and _canaries_intact(buf)   # the whole stride of row 1, row 0 untouched
