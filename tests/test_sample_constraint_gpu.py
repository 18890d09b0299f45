"""GPU: constrained decoding in the fused row sampler (kivi_sample_rows_con, kivi_allow_mark).

1. IDENTITY A: neutral constraint records draw kivi_sample_rows_pen's tokens, draw indices and history table bit for bit, whatever
   the masks and lists hold; with null pen / seen, kivi_sample_rows' tokens.
2. IDENTITY B: any records draw kivi_sample_rows' tokens on reference_constrain(...) uploaded as fp32, at every vocabulary size that
   crosses a mask word, a wave's run, the stride quantum, a bitmap byte or the workgroup.  No tolerance: every step of the rule is
   one fp32 operation in the kernel and in the restatement.
3. Edges: an allowed set of one token; an all-masked row; records outside the contract.
4. suppress_until advances on the device: 40 calls, eager and replayed from a graph.
5. kivi_allow_mark.
6. set_row / set_allowed / select / reset on a live sampler.
7. A tiny model, both cache layouts: generate with each keyword against a loop of the model's passes, reference_constrain and a
   RowSampler without constraints; generate_graphed; n samples per prompt; min_new_tokens against a dominant eos.
8. generate_continuous with per-request constraints and an allowed_fn: graphed == eager, every token obeys its request's rule.
"""
import dataclasses

import pytest
import torch

from test_extend_gpu import _model
from test_sample_gpu import _layouts
from test_sample_penalty_gpu import COUNT, PROMPT, _from_table, _logits, _to_table, _words

pytestmark = pytest.mark.gpu

INF = float("inf")
EDGES = [0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129, 510, 511, 512, 513, 1022, 1023, 1024, 1025, 2047, 2048, 2049]


def _base_rows():
    """Four mixed rows: sampling with filters, greedy, sampling at temperature 1, sampling with min_p."""
    from kivi_amd.sampling import SamplingParams
    return [SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=11), SamplingParams(do_sample=False),
            SamplingParams(temperature=1.0, top_k=0, seed=12), SamplingParams(temperature=1.4, top_k=0, min_p=0.02, seed=13)]


def _lg(B, V, seed, dtype):
    """_logits, or for a vocabulary too small for its ties a plain strided random view."""
    if V >= 8:
        return _logits(B, V, seed, dtype)
    g = torch.Generator("cuda").manual_seed(seed)
    buf = torch.zeros((B, 1, V + 24), dtype=dtype, device="cuda")
    buf[:, 0, :V] = (torch.randn((B, V), device="cuda", generator=g) * 3).half().to(dtype)
    return buf[:, :, :V]


class Raw:
    """The buffers of one kivi_sample_rows_con call, built by hand so that a test can put anything into them.  `lists`: per row
    [(token, value, suppressed)]; `masks`: per row None or a (V,) bool tensor; `until`: per row suppress_until; `words`: (B, V) int64
    history words (None: null pen / seen); `pens`: per row (theta, presence, frequency).  Mask rows that are not in force and list
    entries beyond n_list hold garbage."""

    def __init__(self, params, V, lists=None, masks=None, until=None, words=None, pens=None, n_list=None, flags=None):
        from kivi_amd.sampling import RowSampler, _constraint_record, _list_words, allow_bitmask, allow_words
        B = len(params)
        self.B, self.V = B, V
        self.plain = RowSampler(params, "cuda")                            # records and draw indices
        self.lists = lists or [[] for _ in range(B)]
        self.masks = masks or [None] * B
        self.until = until or [0] * B
        self.pens = pens or [(1.0, 0.0, 0.0)] * B
        self.words = None if words is None else words.clone()
        self.seen = None if words is None else _to_table(words)
        self.pen = None if words is None else torch.tensor([list(p) + [0.0] for p in self.pens], dtype=torch.float32, device="cuda")
        g = torch.Generator().manual_seed(99)
        W = allow_words(V)
        self.guard = torch.full((B * W + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        allow = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, W), generator=g, dtype=torch.int64).to(torch.int32)       # garbage
        for b, m in enumerate(self.masks):
            if m is not None:
                allow[b] = allow_bitmask(m.nonzero().view(-1).tolist(), V)
                allow[b, (V + 31) // 32:] = 0x55555555                     # words beyond ceil(V / 32) are never read
                if V % 32:                                                 # nor the bits at or beyond V in the last word
                    allow[b, (V - 1) // 32] |= torch.tensor(-1 << (V % 32), dtype=torch.int64).to(torch.int32)
        self.allow = self.guard[32: 32 + B * W].view(B, W)
        self.allow.copy_(allow)
        assert self.allow.data_ptr() % 16 == 0
        lst = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, 1024, 2), generator=g, dtype=torch.int64).to(torch.int32)    # garbage
        for b, ls in enumerate(self.lists):
            if ls:
                lst[b, : len(ls)] = _list_words(ls)
        self.list = lst.cuda()
        n_list = n_list or [len(ls) for ls in self.lists]
        flags = flags or [0 if m is None else 1 for m in self.masks]
        self.con = torch.stack([_constraint_record(f, n, u) for f, n, u in zip(flags, n_list, self.until)]).cuda()

    def __call__(self, logits, out=None):
        from kivi_amd import _lib
        lib = _lib.load()
        lg = logits[:, 0] if logits.dim() == 3 else logits
        out = torch.empty((self.B, 1), dtype=torch.int64, device="cuda") if out is None else out
        rc = lib.kivi_sample_rows_con(_lib.ptr(lg), 16 if lg.dtype == torch.float16 else 32, lg.stride(0), self.B, self.V,
                                      _lib.ptr(self.plain.records), _lib.ptr(self.plain.draw_index),
                                      None if self.pen is None else _lib.ptr(self.pen), None if self.seen is None else _lib.ptr(self.seen),
                                      0 if self.seen is None else self.seen.stride(0), _lib.ptr(self.con), _lib.ptr(self.allow),
                                      self.allow.stride(0), _lib.ptr(self.list), self.list.stride(0) // 2, _lib.ptr(out), 1,
                                      _lib.stream_ptr(lg))
        assert rc == 0, lib.kivi_last_error()
        return out

    def expect(self, logits, lists=None):
        """kivi_sample_rows on the restated logits, uploaded as fp32, at the current draw indices."""
        from kivi_amd.sampling import RowSampler, reference_constrain
        lg = logits[:, 0] if logits.dim() == 3 else logits
        draw = self.plain.draw_index.tolist()
        pen = None
        if self.words is not None:
            pen = ((self.words & PROMPT) != 0, self.words & COUNT, [p[0] for p in self.pens], [p[1] for p in self.pens],
                   [p[2] for p in self.pens])
        x = reference_constrain(lg, lists or self.lists, [d < u for d, u in zip(draw, self.until)], self.masks, pen)
        ref = RowSampler(self.plain.params, "cuda", self.plain.streams)
        ref.draw_index.copy_(self.plain.draw_index)
        return ref(x.cuda()), x

    def count(self, toks):
        if self.words is not None:
            for r, t in enumerate(toks.view(-1).tolist()):
                if self.words[r, t] & COUNT != COUNT:
                    self.words[r, t] += 1

    def intact(self):
        return bool((self.guard[:32] == 0x5A5A5A5A).all() and (self.guard[-32:] == 0x5A5A5A5A).all())


# ------------------------------------------------------------------ 1. identity A
@pytest.mark.parametrize("V,dtype", [(1, torch.float16), (33, torch.float32), (320, torch.float16), (513, torch.float32),
                                     (32000, torch.float16), (128256, torch.float32)])
def test_identity_a_neutral_records(V, dtype):
    from kivi_amd.sampling import RowSampler
    logits = _lg(4, V, 1, dtype)
    g = torch.Generator().manual_seed(2)
    words = torch.randint(0, 1 << 16, (4, V), generator=g)
    pens = [(1.3, 0.6, 0.25), (1.0, 0.0, 0.0), (0.5, -0.7, 0.0), (1.0, 0.0, 0.0)]
    params = _base_rows()
    con = Raw(params, V, words=words, pens=pens)                            # neutral records over garbage masks and lists
    pen = RowSampler([dataclasses.replace(p, repetition_penalty=t, presence_penalty=a, frequency_penalty=f)
                      for p, (t, a, f) in zip(params, pens)], "cuda", vocab_size=V)
    pen.seen.copy_(_to_table(words))
    bare, plain = Raw(params, V), RowSampler(params, "cuda")                # null pen / seen against kivi_sample_rows
    for call in range(3):
        a, b = con(logits), pen(logits)
        assert torch.equal(a, b), (call, a.view(-1).tolist(), b.view(-1).tolist())
        assert torch.equal(con.seen, pen.seen) and torch.equal(con.plain.draw_index, pen.draw_index)
        c, d = bare(logits), plain(logits)
        assert torch.equal(c, d) and torch.equal(bare.plain.draw_index, plain.draw_index)
    assert pen.draw_index.tolist() == [3] * 4 and con.intact() and bare.intact()


# ------------------------------------------------------------------ 2. identity B
def _list(V, n, seed, suppress_every=0):
    """n entries in ascending token order: the tokens at both sides of every boundary that lie below V, then random ones, and -- when
    V has fewer than n tokens -- ids at or above V, which the kernel skips.  Values: +-inf, +-0 and ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    toks = sorted({e for e in EDGES + [V - 2, V - 1] if 0 <= e < V})
    if len(toks) > n:
        toks = toks[:n - 1] + [V - 1] if n > 1 else [V - 1]
    rest = [t for t in torch.randperm(min(V, 1 << 20), generator=g).tolist() if t not in set(toks)][: n - len(toks)]
    toks = sorted(toks + rest)
    toks += list(range(V, V + n - len(toks)))
    pool = [-INF, 0.0, -0.0, 1.5, -2.25, 6.0, 0.1, -INF, 3.0]
    vals = [pool[int(i)] for i in torch.randint(0, len(pool), (n,), generator=g)]
    return [(t, v, bool(suppress_every) and i % suppress_every == 0) for i, (t, v) in enumerate(zip(toks, vals))]


def _mask(V, seed, logits_row=None):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(V, generator=g) < 0.5
    for e in EDGES:
        if e < V:
            m[e] = (e % 3) != 0
    if logits_row is not None:                                              # a candidate of every filter stays allowed
        m[logits_row.float().topk(min(3, V)).indices.cpu()] = True
    m[V - 1] = True
    return m


def _identity_b(V, dtype, sizes, inf_row=None):
    logits = _lg(4, V, 3 + V % 7, dtype)
    words = _words(4, V, 4, logits) if V >= 8 else torch.randint(0, 3, (4, V))
    lists = [[], _list(V, sizes[0], 5, 3), _list(V, sizes[1], 6, 2), _list(V, sizes[2], 7, 4)]
    if inf_row is not None:                                                 # +inf on a greedy row: that token wins
        t, _, s = lists[inf_row][0]
        lists[inf_row][0] = (t, INF, s)
    masks = [_mask(V, 8, logits[0, 0]), None, _mask(V, 9, logits[2, 0]), _mask(V, 10, logits[3, 0])]
    pens = [(1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.3, 0.6, 0.25)]
    con = Raw(_base_rows(), V, lists, masks, until=[0, 4, 4, 4], words=words, pens=pens)
    con.plain.draw_index.fill_(3)                                           # draws 3, 4, 5: one below, at, one above suppress_until
    seen = set()
    for call in range(3):
        want, x = con.expect(logits)
        got = con(logits)
        assert torch.equal(got, want), (V, call, got.view(-1).tolist(), want.view(-1).tolist())
        con.count(got)
        assert torch.equal(_from_table(con.seen, V), con.words)
        assert bool(x.gather(1, got.cpu()).isfinite().all()) or inf_row is not None or V == 1    # no masked token is drawn
        seen.update(got.view(-1).tolist())
    assert con.plain.draw_index.tolist() == [6] * 4 and con.intact()
    return seen


@pytest.mark.parametrize("V", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025])
def test_identity_b_boundaries(V):
    dtype = torch.float16 if V % 2 else torch.float32
    _identity_b(V, dtype, (1, 2, 1024))
    _identity_b(V, torch.float32 if V % 2 else torch.float16, (2, 1023, 1), inf_row=1)


@pytest.mark.parametrize("V,dtype", [(32000, torch.float16), (128256, torch.float32)])
def test_identity_b_vocabularies(V, dtype):
    assert len(_identity_b(V, dtype, (1023, 1024, 300))) > 2


# ------------------------------------------------------------------ 3. edges
def test_one_allowed_token_and_all_masked_rows():
    V = 513
    logits = _logits(4, V, 12, torch.float16)
    only = [5, 512, 64, 31]
    masks = [torch.zeros(V, dtype=torch.bool) for _ in range(4)]
    for m, t in zip(masks, only):
        m[t] = True
    con = Raw(_base_rows(), V, masks=masks)
    assert con(logits).view(-1).tolist() == only                            # greedy and sampling rows alike
    # all masked: by the mask, by -inf biases over every token (V = 513 <= 1024), by suppression
    V = 320
    logits = _logits(4, V, 13, torch.float32)
    every = [(t, -INF, False) for t in range(V)]
    sup = [(t, 0.0, True) for t in range(V)]
    con = Raw(_base_rows(), V, [[], every, sup, sup], [torch.zeros(V, dtype=torch.bool), None, None, None], until=[0, 0, 1, 1])
    want, x = con.expect(logits)
    assert bool((x == -INF).all())
    got = con(logits)
    assert torch.equal(got, want) and bool(((got >= 0) & (got < V)).all())
    want, x = con.expect(logits)                                            # draw 1: rows 2 and 3 are free again
    assert bool(x[2:].isfinite().all())
    assert torch.equal(con(logits), want) and con.intact()


def test_records_outside_the_contract_degrade():
    V = 320
    logits = _logits(4, V, 14, torch.float16)
    full = _list(V, 320, 15) + [(V + i, 5.0, False) for i in range(704)]    # 1024 entries, the last 704 at or above V
    nan = [(7, float("nan"), False), (9, 2.0, False), (V, 50.0, False), (V + 100, INF, False)]
    top = int(logits[2, 0].float().argmax())
    unsorted = [(top, -INF, False), (3, 1.0, False), (3, 2.0, False), (1, 0.5, False)] if top > 3 else []
    con = Raw(_base_rows(), V, [full, full, nan, unsorted], n_list=[-1, 5000, 4, len(unsorted)])
    clamped = [[], full, [(7, 0.0, False), (9, 2.0, False)], None]
    want, _ = con.expect(logits, clamped)
    got = con(logits)
    assert torch.equal(got[:3], want[:3])                                   # n_list -1 -> 0, 5000 -> 1024, NaN -> 0, ids >= V skipped
    assert 0 <= int(got[3]) < V and con.intact()                            # unsorted: some token, nothing read outside


# ------------------------------------------------------------------ 4. suppress_until advances on the device
def _forty_calls(graph):
    V, B = 320, 4
    logits = _logits(B, V, 16, torch.float16).contiguous()
    eos = 77
    logits[:, 0, eos] = logits.float().max() + 4.0                          # the suppressed id holds every row's largest logit
    params = _base_rows()
    params[0] = dataclasses.replace(params[0], do_sample=False)
    params[2] = dataclasses.replace(params[2], temperature=0.05)            # sampling, but all but certain to take the maximum
    con = Raw(params, V, [[(eos, 0.0, True)]] * B, until=[5, 5, 5, 0], words=torch.zeros((B, V), dtype=torch.long))
    out = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    toks = []
    if graph:
        Raw(params, V, [[(eos, 0.0, True)]] * B)(logits)                    # (the kernel has run once before it is captured)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            con(logits, out)
        assert con.plain.draw_index.tolist() == [0] * B                     # a capture runs nothing
        for _ in range(40):
            g.replay()
            toks.append(out.clone())
    else:
        for _ in range(40):
            toks.append(con(logits, out).clone())
    return torch.cat(toks, 1).cpu(), _from_table(con.seen, V), con.plain.draw_index.tolist(), eos


def test_suppress_until_advances_eager_and_replayed():
    toks, table, draws, eos = _forty_calls(False)
    assert draws == [40] * 4
    for r in (0, 1, 2):
        assert eos not in toks[r, :5].tolist()
    assert toks[0, 5:].tolist() == [eos] * 35 and toks[1, 5:].tolist() == [eos] * 35 and int(toks[2, 5]) == eos
    assert int(toks[3, 0]) in range(320) and eos in toks[3].tolist()        # until 0: never suppressed
    assert torch.equal(table, torch.stack([torch.bincount(toks[r], minlength=320) for r in range(4)]))
    replayed = _forty_calls(True)
    assert torch.equal(replayed[0], toks) and torch.equal(replayed[1], table) and replayed[2] == draws


# ------------------------------------------------------------------ 5. kivi_allow_mark
def _allow_mark(allow, V, rows, tokens, lens, flags, T=None):
    from kivi_amd import _lib
    lib = _lib.load()
    n = tokens.shape[0] if tokens is not None else len(rows)
    rc = lib.kivi_allow_mark(_lib.ptr(allow), allow.stride(0), V, None if rows is None else _lib.ptr(rows), n,
                             None if tokens is None else _lib.ptr(tokens), 0 if tokens is None else tokens.stride(0),
                             (tokens.shape[1] if tokens is not None else 0) if T is None else T,
                             None if lens is None else _lib.ptr(lens), flags, _lib.stream_ptr(allow))
    assert rc == 0, lib.kivi_last_error()


def _bits(allow, V):
    """(B, stride * 32) bool of a mask table."""
    w = allow.cpu().long() & 0xFFFFFFFF
    return ((w[:, :, None] >> torch.arange(32)) & 1).bool().flatten(1)


def test_allow_mark():
    from kivi_amd.sampling import ALLOW_ALL, ALLOW_NONE, ALLOW_SET, ALLOW_UNSET
    B, V, stride, T = 5, 70, 8, 9                                           # ceil(V / 32) = 3 words of 8
    guard = torch.full((B * stride + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    allow = guard[32: 32 + B * stride].view(B, stride)
    g = torch.Generator().manual_seed(17)
    before = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, stride), generator=g).to(torch.int32)
    allow.copy_(before)
    toks = torch.tensor([[3, 3, -1, 70, 69, 0, 3, 32, 31],                   # duplicates; -1 and V are skipped
                         [1, 2, 3, 4, 5, 6, 7, 8, 9],
                         [60, 61, 62, 63, 64, 65, 66, 67, 68]], device="cuda")
    lens = torch.tensor([9, 4, 0], dtype=torch.int32, device="cuda")        # full, short, 0
    rows = torch.tensor([4, 0, 2], dtype=torch.int32, device="cuda")        # a permuted subset
    _allow_mark(allow, V, rows, toks, lens, ALLOW_NONE | ALLOW_SET)
    want = _bits(before, V)
    want[[4, 0, 2], :96] = False
    want[4, [3, 69, 0, 32, 31]] = True
    want[0, [1, 2, 3, 4]] = True
    assert torch.equal(_bits(allow, V), want)                               # rows 1, 3 and words 3..7 of every row as they were
    _allow_mark(allow, V, rows, toks, None, ALLOW_ALL | ALLOW_UNSET)         # len null: T ids
    want[[4, 0, 2], :96] = True
    want[4, [3, 69, 0, 32, 31]] = False
    want[0, 1:10] = False
    want[2, 60:69] = False
    assert torch.equal(_bits(allow, V), want)
    _allow_mark(allow, V, None, toks[:2], lens[:2], ALLOW_SET)               # rows null: rows 0, 1; no fill
    want[0, [3, 69, 0, 32, 31]] = True
    want[1, [1, 2, 3, 4]] = True
    assert torch.equal(_bits(allow, V), want)
    _allow_mark(allow, V, torch.tensor([3, -1], dtype=torch.int32, device="cuda"), None, None, ALLOW_ALL)      # a fill alone; -1 skipped
    want[3, :96] = True
    assert torch.equal(_bits(allow, V), want)
    _allow_mark(allow, V, rows, toks, None, ALLOW_NONE | ALLOW_SET, T=0)     # T = 0: the fill alone
    want[[4, 0, 2], :96] = False
    assert torch.equal(_bits(allow, V), want)
    many = torch.arange(64, device="cuda").repeat(80).view(1, -1)           # contention on two words
    _allow_mark(allow, V, torch.tensor([1], dtype=torch.int32, device="cuda"), many, None, ALLOW_NONE | ALLOW_SET)
    want[1, :96] = False
    want[1, :64] = True
    assert torch.equal(_bits(allow, V), want)
    assert bool((guard[:32] == 0x5A5A5A5A).all() and (guard[-32:] == 0x5A5A5A5A).all())


# ------------------------------------------------------------------ 6. a live sampler
def _host_lists(rs):
    return [c["list"] for c in rs._con]


def _sampler_expect(rs, logits, words=None):
    """What a RowSampler with constraint state has to draw next, from its host-side mirror and its device buffers."""
    from kivi_amd.sampling import RowSampler, SampleConstraint, reference_constrain
    V = rs.vocab_size
    recs = [SampleConstraint.from_buffer_copy(r.numpy().tobytes()) for r in rs.constraint.cpu()]
    table = _from_table(rs.seen, V) if words is None else words
    pen = ((table & PROMPT) != 0, table & COUNT, [p.repetition_penalty for p in rs.params], [p.presence_penalty for p in rs.params],
           [p.frequency_penalty for p in rs.params])
    draw = rs.draw_index.tolist()
    x = reference_constrain(logits[:, 0], _host_lists(rs), [d < r.suppress_until for d, r in zip(draw, recs)],
                            [rs.allowed[b].cpu() if r.flags & 1 else None for b, r in enumerate(recs)], pen)
    plain = RowSampler([dataclasses.replace(p, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                                            allowed_token_ids=None, min_new_tokens=0) for p in rs.params], "cuda", rs.streams)
    plain.draw_index.copy_(rs.draw_index)
    return plain(x.cuda())


def test_set_row_set_allowed_select_reset_on_a_live_sampler():
    from kivi_amd.sampling import RowSampler, SampleConstraint, SampleListEntry, SamplingParams, allow_bitmask
    V = 320
    base = _base_rows()
    params = [dataclasses.replace(base[0], logit_bias={5: 2.0, 300: -INF}), dataclasses.replace(base[1], min_new_tokens=2),
              dataclasses.replace(base[2], allowed_token_ids=[1, 64, 319], frequency_penalty=0.5), base[3]]
    rs = RowSampler(params, "cuda", vocab_size=V, suppress=[7, 300])
    plain = RowSampler(base, "cuda", vocab_size=V)
    assert len(plain.key()) == 6 and plain.constraint is None               # no constrained row: nothing changes
    assert len(rs.key()) == 9 and rs.allowed.shape == (4, 12) and rs.bias_list.shape == (4, 1024, 2)

    def rec(b):
        return SampleConstraint.from_buffer_copy(rs.constraint[b].cpu().numpy().tobytes())

    def entries(b, n):
        raw = rs.bias_list[b, :n].cpu().numpy().tobytes()
        return [(e.word, e.value) for e in (SampleListEntry.from_buffer_copy(raw[8 * i: 8 * i + 8]) for i in range(n))]

    assert [(rec(b).flags, rec(b).n_list, rec(b).suppress_until) for b in range(4)] == [(0, 2, 0), (0, 2, 2), (1, 0, 0), (0, 0, 0)]
    assert entries(0, 2) == [(5, 2.0), (300, -INF)] and entries(1, 2) == [(7 | 1 << 31, 0.0), (300 | 1 << 31, 0.0)]
    assert torch.equal(rs.allowed[2].cpu(), allow_bitmask([1, 64, 319], V)) and bool((rs.allowed[[0, 1, 3]] == -1).all())
    key = rs.key()
    logits = _logits(4, V, 18, torch.float16)
    logits[1, 0, 7] = 50.0                                                   # the greedy row's maximum is suppressed for two draws
    toks = []
    for _ in range(3):
        want = _sampler_expect(rs, logits)
        toks.append(rs(logits))
        assert torch.equal(toks[-1], want)
    assert [int(t[1]) for t in toks][2] == 7 and 7 not in [int(t[1]) for t in toks][:2]
    assert all(int(t[2]) in (1, 64, 319) for t in toks)
    # set_allowed: ids from the host, ids on the device (kivi_allow_mark), a bitmask, None
    rs.set_allowed(3, [2, 3, 400, -1])
    assert torch.equal(rs.allowed[3].cpu(), allow_bitmask([2, 3], V)) and rec(3).flags == 1
    assert int(rs(logits)[3]) in (2, 3)
    rs.set_allowed(3, torch.tensor([9, 10, 10], device="cuda"))
    assert torch.equal(rs.allowed[3, :10].cpu(), allow_bitmask([9, 10], V)[:10]) and int(rs(logits)[3]) in (9, 10)
    rs.set_allowed(3, allow_bitmask([100], V)[:10].cuda())
    assert int(rs(logits)[3]) == 100 and torch.equal(rs.allowed[3, :10].cpu(), allow_bitmask([100], V)[:10])
    rs.set_allowed(3, None)
    assert rec(3).flags == 0 and bool((rs.allowed[3] == -1).all())
    want = _sampler_expect(rs, logits)
    assert torch.equal(rs(logits), want)
    # set_row: record, list and mask row of that row alone
    before = (rs.constraint.clone(), rs.allowed.clone(), rs.bias_list.clone())
    new = SamplingParams(do_sample=False, logit_bias={7: 1.0, 2: 3.0}, allowed_token_ids=[2, 7, 8], min_new_tokens=3)
    rs.set_row(0, new, draw_index=1, generated=[8], suppress=[7])
    assert (rec(0).flags, rec(0).n_list, rec(0).suppress_until) == (1, 2, 3) and rs.key() == key
    assert entries(0, 2) == [(2, 3.0), (7 | 1 << 31, 1.0)] and torch.equal(rs.allowed[0].cpu(), allow_bitmask([2, 7, 8], V))
    for now, was in zip((rs.constraint, rs.allowed, rs.bias_list), before):
        assert torch.equal(now[1:], was[1:])
    logits[0, 0, 7] = 60.0
    got = []
    for _ in range(4):                                                      # draws 1, 2 suppress token 7; draws 3, 4 take it
        want = _sampler_expect(rs, logits)
        got.append(rs(logits))
        assert torch.equal(got[-1], want)
    assert [int(t[0]) for t in got][2:] == [7, 7] and all(int(t[0]) in (2, 8) for t in got[:2])
    rs.set_row(0, base[0])                                                  # an unconstrained request: the row is free again
    assert (rec(0).flags, rec(0).n_list) == (0, 0) and bool((rs.allowed[0] == -1).all())
    with pytest.raises(ValueError, match="constraint"):
        plain.set_row(0, new)
    # select carries the state; reset counts min_new_tokens from 0 again
    sel = rs.select([1, 1, 2], streams=[0, 1, 0])
    assert torch.equal(sel.constraint, rs.constraint[[1, 1, 2]]) and torch.equal(sel.allowed, rs.allowed[[1, 1, 2]])
    assert torch.equal(sel.bias_list, rs.bias_list[[1, 1, 2]]) and sel.allowed.data_ptr() != rs.allowed.data_ptr()
    fork = logits[[1, 1, 2]]
    want = _sampler_expect(sel, fork)
    assert torch.equal(sel(fork), want)
    rs.reset()
    assert rs.draw_index.tolist() == [0] * 4 and rec(1).suppress_until == 2
    assert 7 != int(rs(logits)[1])                                          # suppressed again


# ------------------------------------------------------------------ 7. the model
def _unconstrained(p):
    return dataclasses.replace(p, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                               allowed_token_ids=None, min_new_tokens=0)


def _compose(model, ids, n, params, streams, mask=None, fan=1, suppress=()):
    """The call by hand: the model's passes, reference_constrain on the CPU, a RowSampler WITHOUT constraint state on the uploaded
    fp32 logits.  `fan`: every request's row is forked that often after the prompt pass; `suppress`: the ids min_new_tokens masks."""
    from kivi_amd.sampling import RowSampler, allow_bitmask, constraint_list, reference_constrain
    V = model.config.vocab_size
    plain = RowSampler([_unconstrained(p) for p in params], "cuda", streams)
    lg, past = model(ids, None) if mask is None else model(ids, None, padding_mask=mask)
    if fan > 1:
        rows = torch.arange(ids.shape[0], device="cuda").repeat_interleave(fan)
        past = [p.layer.index_select(rows).as_tuple() for p in past]
        lg, ids, mask = lg.index_select(0, rows), ids[rows], None if mask is None else mask[rows]
    lists = [constraint_list(p, suppress) for p in params]
    allow = [None if p.allowed_token_ids is None else allow_bitmask(p.allowed_token_ids, V) for p in params]
    out = [ids]
    for s in range(n):
        x = reference_constrain(lg[:, 0], lists, [s < p.min_new_tokens for p in params], allow)
        tok = plain(x.cuda())
        out.append(tok)
        if s == n - 1:
            break
        if mask is None:
            lg, past = model(tok, past)
        else:
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            lg, past = model(tok, past, padding_mask=mask)
    return torch.cat(out, 1)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_with_constraints_equals_composition(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 45)
    n = 10
    pids, mask = left_pad([list(range(3, 40)), list(range(50, 71)), list(range(100, 110))], pad_token_id=0, device="cuda")
    free = model.generate(pids, n, attention_mask=mask)
    assert getattr(model(pids, padding_mask=mask)[1][0].layer, "layout", "hook") == layout
    hot = sorted(set(free[:, pids.shape[1]:].flatten().tolist()))           # what the unconstrained call emits
    sampled = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.9, seed=5)
    for kw in (dict(logit_bias={t: -INF for t in hot[:6]} | {1: 3.0, 319: 0.5}), dict(allowed_token_ids=list(range(2, 320, 3))),
               dict(min_new_tokens=4, logit_bias={hot[0]: 1.0})):
        # greedy
        a = model.generate(pids, n, attention_mask=mask, **kw)
        want = _compose(model, pids, n, [SamplingParams(do_sample=False, seed=0, **kw)] * 3, [0, 1, 2], mask)
        assert torch.equal(a, want), kw
        assert torch.equal(model.generate_graphed(pids, n, attention_mask=mask, **kw), a), kw
        # sampled: the call's seed in every row, streams 0..B-1
        b = model.generate(pids, n, attention_mask=mask, **sampled, **kw)
        p = SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=5, **kw)
        assert torch.equal(b, _compose(model, pids, n, [p] * 3, [0, 1, 2], mask)), kw
        assert torch.equal(model.generate_graphed(pids, n, attention_mask=mask, **sampled, **kw), b), kw
    a = model.generate(pids, n, attention_mask=mask, logit_bias={t: -INF for t in hot[:6]})
    assert not set(a[:, pids.shape[1]:].flatten().tolist()) & set(hot[:6]) and not torch.equal(a, free)
    a = model.generate(pids, n, attention_mask=mask, allowed_token_ids=list(range(2, 320, 3)))
    assert bool((a[:, pids.shape[1]:] % 3 == 2).all())
    # per-request constraints inside sampling=, and n samples per prompt
    req = [SamplingParams(temperature=0.8, top_k=40, seed=7, allowed_token_ids=[4, 5, 6, 7], logit_bias={5: -INF}),
           SamplingParams(do_sample=False), SamplingParams(temperature=1.2, top_k=0, seed=9, logit_bias={t: 4.0 for t in range(0, 320, 5)})]
    c = model.generate(pids, n, attention_mask=mask, sampling=req)
    assert torch.equal(c, _compose(model, pids, n, req, [0, 0, 0], mask))
    assert torch.equal(c[1], free[1]) and set(c[0, pids.shape[1]:].tolist()) <= {4, 6, 7}      # the free request, as in a free batch
    assert torch.equal(model.generate_graphed(pids, n, attention_mask=mask, sampling=req), c)
    d = model.generate(pids, 6, attention_mask=mask, sampling=req[0], num_return_sequences=3)
    assert d.shape == (9, pids.shape[1] + 6) and torch.equal(d, _compose(model, pids, 6, [req[0]] * 9, [0, 1, 2] * 3, mask, fan=3))


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_min_new_tokens_holds_back_a_dominant_eos(layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 46)
    ids = torch.randint(1, 320, (3, 21), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    eos, T = 9, 21
    kw = dict(logit_bias={eos: 80.0}, min_new_tokens=6, pad_token_id=0)     # the eos logit dominates every step
    for stop in (dict(eos_token_id=eos), dict(eos_token_id=[eos, 11]), dict(stop_token_ids=[eos])):
        for extra in (dict(), dict(do_sample=True, temperature=0.9, seed=3)):
            out = model.generate(ids, 12, **stop, **kw, **extra)
            new = out[:, T:]
            assert new.shape[1] == 7 and bool((new[:, :6] != eos).all()) and bool((new[:, 6] == eos).all()), (stop, extra)
            assert torch.equal(model.generate_graphed(ids, 12, **stop, **kw, **extra), out), (stop, extra)
    assert bool((model.generate(ids, 12, eos_token_id=eos, pad_token_id=0, logit_bias={eos: 80.0})[:, T] == eos).all())
    # per request, through sampling=: the call binds the suppressed ids of the samplers it makes
    req = [SamplingParams(do_sample=False, logit_bias={eos: 80.0}, min_new_tokens=m) for m in (0, 2, 5)]
    out = model.generate(ids, 12, eos_token_id=eos, pad_token_id=0, sampling=req)[:, T:]
    assert [row.index(eos) for row in out.tolist()] == [0, 2, 5] and out.shape[1] == 6


# ------------------------------------------------------------------ 8. continuous batching
LENS, LIMITS, EOS = [17, 9, 30, 12], [3, 5, 6, 4], 5     # two rows: requests 2 and 3 are admitted into rows that have finished


def _next_mod7(generated):
    last = generated[-1] if generated else 0
    return [t for t in range(320) if t % 7 == (last + 1) % 7 and t != EOS]


def _requests():
    from kivi_amd.sampling import SamplingParams
    return [SamplingParams(temperature=0.9, top_k=0, seed=21), SamplingParams(do_sample=False),
            SamplingParams(do_sample=False, logit_bias={t: 2.0 for t in range(0, 320, 2)}, allowed_token_ids=list(range(1, 320))),
            SamplingParams(temperature=0.8, top_k=40, seed=22, logit_bias={EOS: 80.0}, min_new_tokens=3)]


def _continuous(model, requests, fns, **kw):
    g = torch.Generator().manual_seed(31)
    prompts = [torch.randint(6, 320, (n,), generator=g).tolist() for n in LENS]
    out = model.generate_continuous(prompts, LIMITS, 2, eos_token_id=EOS, pad_token_id=0, sampling=requests, allowed_fn=fns, **kw)
    return [o.tolist() for o in out]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_with_constraints(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 47)
    fns = [_next_mod7, None, _next_mod7, None]
    out = _continuous(model, _requests(), fns)
    for r in (0, 2):                                                        # the allowed_fn's rule, token by token
        assert len(out[r]) == LIMITS[r]
        for i, t in enumerate(out[r]):
            assert t % 7 == ((out[r][i - 1] if i else 0) + 1) % 7 and t != EOS, (r, out[r])
    assert out[3][-1] == EOS and len(out[3]) == 4 and EOS not in out[3][:3]  # min_new_tokens = 3 against a dominant eos
    assert len(out[1]) == LIMITS[1] or out[1][-1] == EOS
    model.release_graphs()
    assert _continuous(model, _requests(), fns, graphed=True) == out
    model.release_graphs()
    # the unconstrained request draws what it draws when nobody is constrained
    plain = _continuous(model, [_unconstrained(p) for p in _requests()], None)
    assert plain[1] == out[1] and plain[0] != out[0]
    # one allowed_fn for every request, greedy requests (sampling=None)
    g = torch.Generator().manual_seed(31)
    prompts = [torch.randint(6, 320, (n,), generator=g).tolist() for n in LENS]
    every = [o.tolist() for o in model.generate_continuous(prompts, LIMITS, 2, allowed_fn=_next_mod7)]
    for o in every:
        assert all(t % 7 == ((o[i - 1] if i else 0) + 1) % 7 for i, t in enumerate(o)), o
