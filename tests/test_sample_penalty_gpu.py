"""GPU: repetition / presence / frequency penalties in the fused row sampler (kivi_sample_rows_pen, kivi_seen_mark; DESIGN.md
section 22).

1. IDENTITY A: neutral records draw kivi_sample_rows' tokens bit for bit, whatever the history table holds.
2. IDENTITY B: any records and table draw kivi_sample_rows' tokens on reference_penalise(...) uploaded as fp32.  No tolerance: every
   step of the rule is one fp32 operation in the kernel and in the restatement, so a mismatch is a defect.
3. The table after 40 calls = prompt bits | counts of the emitted tokens, saturating; canaries around it; two runs bit-identical; a
   replayed graph of the call gives the eager tokens and the eager table.
4. kivi_seen_mark: CLEAR / PROMPT / OUTPUT, duplicates, leads, ids outside the vocabulary, a permutation subset of rows, T = 0.
5. set_row / select / reset on a live sampler.
6. A tiny model, both cache layouts: generate(repetition_penalty=, frequency_penalty=) against a loop composed of the model's
   passes, reference_penalise and a RowSampler without a table; generate_graphed; n samples per prompt.
7. generate_continuous with per-request penalties: graphed == eager, no repeated token under a huge frequency penalty, and the
   table of every row = its last request's prompt bits | counts of what that request emitted (no stale history).
"""
import dataclasses

import pytest
import torch

from test_extend_gpu import _model
from test_sample_gpu import _layouts

pytestmark = pytest.mark.gpu

PROMPT, COUNT = 0x8000, 0x7FFF


def _logits(B, V, seed, dtype):
    """(B, 1, V) view with a row stride above V: exact zeros, both signs, ties."""
    g = torch.Generator("cuda").manual_seed(seed)
    buf = torch.zeros((B, 1, V + 24), dtype=dtype, device="cuda")
    x = (torch.randn((B, V), device="cuda", generator=g) * 3).half()        # fp16 values: ties at any V
    x[:, 3::11] = 0.0
    x[:, 5::17] = -0.0
    x[:, 1] = x[:, 0]                                                        # a tie at the front, whatever was drawn
    top = x.float().topk(6, -1).indices
    x.scatter_(1, top[:, 1:2], x.gather(1, top[:, :1]))                      # the two largest tie
    buf[:, 0, :V] = x.to(dtype)
    view = buf[:, :, :V]
    assert view.stride(0) == V + 24 and not view.is_contiguous()
    return view


def _words(B, V, seed, logits=None):
    """(B, V) int64 history words: prompt bits, counts 0 / 1 / 5 / 32767, words with both; the largest logits are marked."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([0, 0, 0, 1, 5, 32767])[torch.randint(0, 6, (B, V), generator=g)]
    w = counts | (torch.rand((B, V), generator=g) < 0.3).long() * PROMPT
    w[:, 2] = PROMPT | 5                                                     # one word with both, in every row
    if logits is not None:                                                   # the candidates of every filter carry history
        top = logits[:, 0].float().topk(8, -1).indices.cpu()
        w.scatter_(1, top[:, 0:1], torch.full((B, 1), 1))
        w.scatter_(1, top[:, 1:2], torch.full((B, 1), PROMPT))
        w.scatter_(1, top[:, 2:3], torch.full((B, 1), PROMPT | 5))
        w.scatter_(1, top[:, 3:4], torch.full((B, 1), 32767))
    return w


def _to_table(w, stride=None):
    """history words (B, V) int64 -> int16 table on the GPU (bit 15 is the sign bit)."""
    B, V = w.shape
    t = torch.zeros((B, stride or (V + 7) // 8 * 8), dtype=torch.int64)
    t[:, :V] = w
    return torch.where(t >= 0x8000, t - 0x10000, t).to(torch.int16).cuda()


def _from_table(seen, V):
    return (seen.cpu().long() & 0xFFFF)[:, :V]


def _rows(pens):
    """Four mixed rows: sampling with filters, greedy, sampling at temperature 1, sampling with min_p."""
    from kivi_amd.sampling import SamplingParams
    base = [dict(temperature=0.8, top_k=40, top_p=0.9, seed=11), dict(do_sample=False),
            dict(temperature=1.0, top_k=0, seed=12), dict(temperature=1.4, top_k=0, min_p=0.02, seed=13)]
    return [SamplingParams(**b, repetition_penalty=t, presence_penalty=p, frequency_penalty=f) for b, (t, p, f) in zip(base, pens)]


def _neutral(params):
    return [dataclasses.replace(p, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0) for p in params]


SHAPES = [(320, torch.float16), (320, torch.float32), (32000, torch.float16), (32000, torch.float32), (128256, torch.float16),
          (128256, torch.float32)]


@pytest.mark.parametrize("V,dtype", SHAPES)
def test_identity_a_neutral_records(V, dtype):
    from kivi_amd.sampling import RowSampler
    params = _rows([(1.0, 0.0, 0.0)] * 4)
    logits = _logits(4, V, 1, dtype)
    pen, plain = RowSampler(params, "cuda", vocab_size=V), RowSampler(params, "cuda")
    g = torch.Generator().manual_seed(2)
    words = torch.randint(0, 1 << 16, (4, V), generator=g)                   # random words, saturated counts among them
    pen.seen.copy_(_to_table(words))
    want_words = words.clone()
    for call in range(3):
        a, b = pen(logits), plain(logits)
        assert torch.equal(a, b), (call, a.view(-1).tolist(), b.view(-1).tolist())
        for r, t in enumerate(a.view(-1).tolist()):
            if want_words[r, t] & COUNT != COUNT:
                want_words[r, t] += 1
    assert torch.equal(pen.draw_index, plain.draw_index) and pen.draw_index.tolist() == [3] * 4
    assert torch.equal(_from_table(pen.seen, V), want_words)                 # counted, nothing else touched
    assert len({int(t) for t in a.view(-1)}) > 1


PENS = [(0.5, -0.7, 0.0), (1.3, 0.6, 0.25), (1.3, -0.7, 0.25), (0.5, 0.6, 0.0)]


def _expect(logits, words, params, draw_index):
    """kivi_sample_rows on the restated penalised logits, uploaded as fp32, at the given draw indices."""
    from kivi_amd.sampling import RowSampler, reference_penalise
    x = reference_penalise(logits[:, 0], (words & PROMPT) != 0, words & COUNT, [p.repetition_penalty for p in params],
                           [p.presence_penalty for p in params], [p.frequency_penalty for p in params])
    plain = RowSampler(_neutral(params), "cuda")
    plain.draw_index.copy_(draw_index)
    return plain(x.cuda())


@pytest.mark.parametrize("V,dtype", SHAPES)
def test_identity_b_penalised_records(V, dtype):
    from kivi_amd.sampling import RowSampler
    logits = _logits(4, V, 3, dtype)
    for order in (PENS, PENS[::-1], [(1.3, 0.6, 0.25), (1.0, 0.0, 0.0), (0.5, -0.7, 0.0), (1.0, 0.0, 0.0)]):   # (neutral rows among them)
        params = _rows(order)
        words = _words(4, V, 4, logits)
        pen = RowSampler(params, "cuda", vocab_size=V)
        pen.seen.copy_(_to_table(words))
        for call in range(2):                                                # the second call reads what the first one counted
            want = _expect(logits, words, params, pen.draw_index)
            got = pen(logits)
            assert torch.equal(got, want), (order, call, got.view(-1).tolist(), want.view(-1).tolist())
            for r, t in enumerate(got.view(-1).tolist()):
                if words[r, t] & COUNT != COUNT:
                    words[r, t] += 1
            assert torch.equal(_from_table(pen.seen, V), words)


def _canary_table(B, stride):
    """A (B, stride) int16 view in the middle of a buffer of 0x5A5A words, 16-byte aligned."""
    buf = torch.full((B * stride + 128,), 0x5A5A, dtype=torch.int16, device="cuda")
    view = buf[64: 64 + B * stride].view(B, stride)
    assert view.data_ptr() % 16 == 0
    view.zero_()
    return buf, view


def _canaries_intact(buf):
    return bool((buf[:64] == 0x5A5A).all() and (buf[-64:] == 0x5A5A).all())


def _forty_calls(graph):
    from kivi_amd.sampling import RowSampler
    V, B = 320, 4
    params = _rows([(1.0, 0.0, 0.0), (1.3, 0.6, 0.25), (1.3, 0.0, 2.0), (0.5, -0.7, 0.0)])
    params[0] = dataclasses.replace(params[0], do_sample=False)              # row 0: greedy and neutral, it emits ONE token
    logits = _logits(B, V, 5, torch.float16).contiguous()
    rs = RowSampler(params, "cuda", vocab_size=V)
    buf, rs.seen = _canary_table(B, 320)
    ids = torch.randint(0, V, (B, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    mask = torch.ones_like(ids)
    mask[1, :4] = 0
    rs.observe_prompt(ids, attention_mask=mask)
    top0 = int((logits[0, 0] == logits[0, 0].max()).nonzero()[0])            # the lowest index of the tie: the greedy rule
    rs.seen[0, top0] += 32760                                                # 7 calls below saturation
    start = _from_table(rs.seen, V)
    out = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    toks = []
    if graph:
        RowSampler(params, "cuda", vocab_size=V)(logits)                     # (the kernel has run once before it is captured)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rs(logits, out=out)
        assert torch.equal(_from_table(rs.seen, V), start) and rs.draw_index.tolist() == [0] * B    # a capture runs nothing
        for _ in range(40):
            g.replay()
            toks.append(out.clone())
    else:
        for _ in range(40):
            toks.append(rs(logits, out=out).clone())
    toks = torch.cat(toks, 1).cpu()
    return toks, _from_table(rs.seen, V), start, ids.cpu(), mask.cpu(), _canaries_intact(buf), top0


def test_table_after_40_calls_eager_and_replayed():
    toks, table, start, ids, mask, intact, top0 = _forty_calls(False)
    V = 320
    assert intact
    want_bits = torch.zeros((4, V), dtype=torch.long)
    for r in range(4):
        want_bits[r, ids[r][mask[r] != 0]] = PROMPT
    assert torch.equal(start & PROMPT, want_bits) and int(start[1, ids[1, 0]] & PROMPT) == int(want_bits[1, ids[1, 0]])
    counts = torch.stack([torch.bincount(toks[r], minlength=V) for r in range(4)])
    assert torch.equal(table & PROMPT, want_bits)
    assert torch.equal(table & COUNT, ((start & COUNT) + counts).clamp(max=32767))
    assert toks[0].tolist() == [top0] * 40 and int(table[0, top0] & COUNT) == 32767            # saturated: 32760 + 40 > 32767
    assert len(set(toks[1].tolist())) > 2                                    # the penalised greedy row moves on
    again = _forty_calls(False)
    assert torch.equal(again[0], toks) and torch.equal(again[1], table)      # two runs: bit-identical
    replayed = _forty_calls(True)
    assert torch.equal(replayed[0], toks) and torch.equal(replayed[1], table) and replayed[5]


def _mark(lib, seen, V, rows, tokens, lead, flags, T=None):
    from kivi_amd import _lib
    n = tokens.shape[0] if tokens is not None else len(rows)
    rc = lib.kivi_seen_mark(_lib.ptr(seen), seen.stride(0), V, None if rows is None else _lib.ptr(rows), n,
                            None if tokens is None else _lib.ptr(tokens), 0 if tokens is None else tokens.stride(0),
                            (tokens.shape[1] if tokens is not None else 0) if T is None else T,
                            None if lead is None else _lib.ptr(lead), flags, _lib.stream_ptr(seen))
    assert rc == 0, lib.kivi_last_error()


def test_seen_mark():
    from kivi_amd import _lib
    from kivi_amd.sampling import SEEN_CLEAR, SEEN_OUTPUT, SEEN_PROMPT
    lib = _lib.load()
    B, V, stride, T = 5, 37, 40, 9
    buf, seen = _canary_table(B, stride)
    g = torch.Generator().manual_seed(7)
    before = torch.randint(0, 1 << 16, (B, stride), generator=g)
    seen.copy_(_to_table(before, stride))
    toks = torch.tensor([[3, 3, -1, 37, 36, 0, 3, 20, 21],                   # duplicates; -1 and V are skipped; 36 = V - 1, an odd id
                         [1, 2, 3, 4, 5, 6, 7, 8, 9],
                         [30, 31, 32, 33, 34, 35, 36, 36, 36]], device="cuda")
    lead = torch.tensor([0, 3, 9], dtype=torch.int32, device="cuda")         # leads 0, 3 and T
    rows = torch.tensor([4, 0, 2], dtype=torch.int32, device="cuda")         # a permutation subset
    _mark(lib, seen, V, rows, toks, lead, SEEN_CLEAR | SEEN_PROMPT)
    want = before.clone()
    want[[4, 0, 2]] = 0
    want[4, [3, 36, 0, 20, 21]] = PROMPT
    want[0, [4, 5, 6, 7, 8, 9]] = PROMPT
    got = seen.cpu().long() & 0xFFFF
    assert torch.equal(got, want) and _canaries_intact(buf)                  # rows 1 and 3 byte-identical, the pad columns cleared
    # OUTPUT: exact counts with duplicates, on top of the prompt bits; saturation keeps bit 15
    seen[2, 36] = 32766
    seen[2, 35] = -2                                                         # 0xFFFE: prompt bit, count 32766
    want[2, 36], want[2, 35] = 32766, 0xFFFE
    out_lead = torch.tensor([0, 0, 4], dtype=torch.int32, device="cuda")
    _mark(lib, seen, V, rows, toks, out_lead, SEEN_OUTPUT)
    want[4, 3] += 3
    want[4, [36, 0, 20, 21]] += 1
    want[0, [1, 2, 3, 4, 5, 6, 7, 8, 9]] += 1
    want[2, 34] += 1
    want[2, 35] = 0xFFFF                                                     # 32766 + 1, then stays
    want[2, 36] = 32767                                                      # 32766 + 3 saturates, no carry into bit 15
    assert torch.equal(seen.cpu().long() & 0xFFFF, want) and _canaries_intact(buf)
    # a long row of one token: exact under contention
    many = torch.full((1, 5000), 11, device="cuda")
    many[0, ::2] = 10                                                        # both halves of one 32-bit word
    _mark(lib, seen, V, torch.tensor([1], dtype=torch.int32, device="cuda"), many, None, SEEN_CLEAR | SEEN_OUTPUT)
    want[1] = 0
    want[1, 10] = want[1, 11] = 2500
    assert torch.equal(seen.cpu().long() & 0xFFFF, want)
    # rows = null: rows 0..n-1; T = 0 with CLEAR resets them, tokens may be null
    _mark(lib, seen, V, None, toks[:2], None, SEEN_PROMPT)
    want[0, [3, 36, 0, 20, 21]] |= PROMPT
    want[1, [1, 2, 3, 4, 5, 6, 7, 8, 9]] |= PROMPT
    assert torch.equal(seen.cpu().long() & 0xFFFF, want)
    _mark(lib, seen, V, torch.tensor([3, 1], dtype=torch.int32, device="cuda"), None, None, SEEN_CLEAR)
    want[[3, 1]] = 0
    assert torch.equal(seen.cpu().long() & 0xFFFF, want)
    _mark(lib, seen, V, rows, toks, None, SEEN_CLEAR | SEEN_PROMPT, T=0)
    want[[4, 0, 2]] = 0
    assert torch.equal(seen.cpu().long() & 0xFFFF, want) and _canaries_intact(buf) and not seen.any()


def test_set_row_select_reset_on_a_live_sampler():
    from kivi_amd.sampling import RowSampler, SamplePenalty, SamplingParams
    V = 320
    params = _rows(PENS[:3])[:3]
    rs = RowSampler(params, "cuda", vocab_size=V)
    key = rs.key()
    ids = torch.tensor([[0, 0, 7, 8, 9], [1, 2, 3, 4, 5], [0, 0, 0, 0, 6]], device="cuda")
    mask = (ids != 0).long()
    rs.observe_prompt(ids, attention_mask=mask)
    logits = _logits(3, V, 8, torch.float16)
    t0, t1 = rs(logits), rs(logits)
    before = _from_table(rs.seen, V)
    assert int((before & PROMPT).ne(0).sum()) == 3 + 5 + 1 and int((before & COUNT).sum()) == 6
    assert int(before[0, 0]) & PROMPT == 0                                   # the pads (id 0) are not marked
    new = SamplingParams(do_sample=False, repetition_penalty=2.0, presence_penalty=0.25)
    rs.set_row(1, new, draw_index=3, prompt=[40, 41, 41, 319], generated=torch.tensor([5, 5, 9]))
    after = _from_table(rs.seen, V)
    want = before.clone()
    want[1] = 0
    want[1, [40, 41, 319]] = PROMPT
    want[1, 5], want[1, 9] = 2, 1
    assert torch.equal(after, want) and rs.key() == key and rs.draw_index.tolist() == [2, 3, 2]
    rec = SamplePenalty.from_buffer_copy(rs.penalties[1].cpu().numpy().tobytes())
    assert (rec.repetition, rec.presence, rec.frequency, rec.reserved) == (2.0, 0.25, 0.0, 0)
    assert torch.equal(rs.penalties[[0, 2]].cpu(), torch.tensor([[0.5, -0.7, 0.0, 0.0], [1.3, -0.7, 0.25, 0.0]]))
    # the row now draws by its new record and history, the others as if nothing had happened
    words = after.clone()
    want_tok = _expect(logits, words, rs.params, rs.draw_index)
    assert torch.equal(rs(logits), want_tok)
    rs.set_row(2, params[2])                                                 # no prompt, no history: a cleared row
    assert not _from_table(rs.seen, V)[2].any()
    sel = rs.select([1, 1, 0], streams=[0, 1, 0])
    assert torch.equal(sel.seen, rs.seen[[1, 1, 0]]) and torch.equal(sel.penalties, rs.penalties[[1, 1, 0]])
    assert sel.seen.data_ptr() != rs.seen.data_ptr() and sel.draw_index.tolist() == [4, 4, 3]
    same = logits.clone()
    same[1] = same[0]
    a = sel(same)
    assert int(a[0]) == int(a[1])                                            # two greedy copies of one row, on the same logits
    assert torch.equal(_from_table(rs.seen, V)[0], _from_table(sel.seen, V)[2] - torch.nn.functional.one_hot(a[2], V)[0].cpu())
    rs.reset()
    assert not rs.seen.any() and rs.draw_index.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="do not fit"):
        rs(_logits(3, V + 8, 9, torch.float16))


# ------------------------------------------------------------------ 6. the model
def _compose(model, ids, n, params, streams, mask=None, fan=1):
    """The call by hand: the model's passes, reference_penalise on the CPU, a RowSampler WITHOUT a table on the uploaded fp32
    logits, the history kept in two Python-side tensors.  `fan`: every request's row is forked that often after the prompt pass."""
    from kivi_amd.sampling import RowSampler, reference_penalise
    V = model.config.vocab_size
    plain = RowSampler(_neutral(params), "cuda", streams)
    lg, past = model(ids, None) if mask is None else model(ids, None, padding_mask=mask)
    if fan > 1:
        rows = torch.arange(ids.shape[0], device="cuda").repeat_interleave(fan)
        past = [p.layer.index_select(rows).as_tuple() for p in past]
        lg, ids, mask = lg.index_select(0, rows), ids[rows], None if mask is None else mask[rows]
    B = ids.shape[0]
    prompt = torch.zeros((B, V), dtype=torch.bool)
    for r in range(B):
        real = ids[r].cpu() if mask is None else ids[r][mask[r] != 0].cpu()
        prompt[r, real] = True
    counts = torch.zeros((B, V), dtype=torch.long)
    out = [ids]
    for s in range(n):
        x = reference_penalise(lg[:, 0], prompt, counts, [p.repetition_penalty for p in params],
                               [p.presence_penalty for p in params], [p.frequency_penalty for p in params])
        tok = plain(x.cuda())
        counts.scatter_add_(1, tok.cpu(), torch.ones((B, 1), dtype=torch.long))
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
def test_generate_with_penalties_equals_composition(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler, SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 43)
    n = 12
    pids, mask = left_pad([list(range(3, 40)), list(range(50, 71)), list(range(100, 110))], pad_token_id=0, device="cuda")
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2)
    # greedy
    a = model.generate(pids, n, attention_mask=mask, **pen)
    assert getattr(model(pids, padding_mask=mask)[1][0].layer, "layout", "hook") == layout
    want = _compose(model, pids, n, [SamplingParams(do_sample=False, seed=0, **pen)] * 3, [0, 1, 2], mask)
    assert torch.equal(a, want)
    assert not torch.equal(a, model.generate(pids, n, attention_mask=mask))  # the penalties change this output
    assert torch.equal(model.generate_graphed(pids, n, attention_mask=mask, **pen), a)
    # sampled: the call's seed in every row, streams 0..B-1
    kw = dict(do_sample=True, temperature=0.8, top_k=40, top_p=0.9, seed=5)
    b = model.generate(pids, n, attention_mask=mask, **kw, **pen)
    p = SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=5, **pen)
    assert torch.equal(b, _compose(model, pids, n, [p] * 3, [0, 1, 2], mask))
    assert torch.equal(model.generate_graphed(pids, n, attention_mask=mask, **kw, **pen), b)
    # without pads, and with the penalties inside sampling=
    ids = torch.randint(0, 320, (3, 29), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    req = [p, SamplingParams(do_sample=False), SamplingParams(temperature=1.2, top_k=0, seed=9, presence_penalty=0.6)]
    c = model.generate(ids, n, sampling=req)
    assert torch.equal(c, _compose(model, ids, n, req, [0, 0, 0]))
    assert torch.equal(c[1], model.generate(ids, n)[1])                      # the neutral greedy request, as in a greedy batch
    # n samples per prompt: the marks are repeated per forked row
    d = model.generate(pids, 8, attention_mask=mask, sampling=p, num_return_sequences=3)
    assert d.shape == (9, pids.shape[1] + 8) and torch.equal(d, _compose(model, pids, 8, [p] * 9, [0, 1, 2] * 3, mask, fan=3))
    # a caller's RowSampler keeps its table over calls: the second call sees the first one's prompt and output
    mine = RowSampler(req, "cuda", vocab_size=320)
    model.generate(ids, 4, sampling=mine)
    table = (mine.seen.cpu().long() & 0xFFFF)
    assert int(((table & PROMPT) != 0).sum()) == sum(len(set(r.tolist())) for r in ids) and int((table & COUNT).sum()) == 3 * 5


# ------------------------------------------------------------------ 7. continuous batching
LENS, LIMITS = [17, 9, 30, 12], [3, 5, 6, 4]          # two rows: requests 2 and 3 take over at picks 2 and 4, both end at pick 7


def _requests():
    from kivi_amd.sampling import SamplingParams
    return [SamplingParams(temperature=0.9, top_k=0, seed=21, frequency_penalty=1e4), SamplingParams(do_sample=False),
            SamplingParams(do_sample=False, frequency_penalty=1e4),
            SamplingParams(temperature=0.8, top_k=40, seed=22, repetition_penalty=1.3, presence_penalty=0.6)]


def _continuous(model, monkeypatch, **kw):
    """-> (outputs, the table of the batch's sampler at the end)"""
    import kivi_amd.serving as S
    from kivi_amd.sampling import RowSampler
    made = []

    class Recording(RowSampler):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(S, "RowSampler", Recording)
    g = torch.Generator().manual_seed(31)
    prompts = [torch.randint(1, 320, (n,), generator=g).tolist() for n in LENS]
    out = model.generate_continuous(prompts, LIMITS, 2, sampling=_requests(), **kw)
    assert made[0].B == 2 and made[0].seen is not None and all(m.seen is not None for m in made)
    return prompts, [o.tolist() for o in out], made[0].seen.cpu().long() & 0xFFFF


def _check_final_table(prompts, out, table):
    for row, r in ((0, 2), (1, 3)):                                          # the last request of every row, live until the last pick
        want = torch.bincount(torch.tensor(out[r]), minlength=320)
        want[torch.tensor(sorted(set(prompts[r])))] |= PROMPT
        assert torch.equal(table[row], want), (row, r)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_with_penalties(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 44)
    prompts, out, table = _continuous(model, monkeypatch)
    assert [len(o) for o in out] == LIMITS
    for r in (0, 2):
        assert len(set(out[r])) == len(out[r])                               # frequency_penalty=1e4: no token twice in one output
    _check_final_table(prompts, out, table)
    model.release_graphs()
    _, graphed, gtable = _continuous(model, monkeypatch, graphed=True)
    assert graphed == out and torch.equal(gtable, table)
    # the neutral greedy request draws what it draws when no request is penalised and no table exists (the same schedule)
    plain = model.generate_continuous(prompts, LIMITS, 2, sampling=_neutral(_requests()))
    assert plain[1].tolist() == out[1]
    # compact= and short_admissions=: the table is not tied to cache positions
    for kw in (dict(compact=32), dict(short_admissions=True), dict(short_admissions=True, compact=32, graphed=True)):
        model.release_graphs()
        p2, o2, t2 = _continuous(model, monkeypatch, **kw)
        assert [len(o) for o in o2] == LIMITS and all(len(set(o2[r])) == len(o2[r]) for r in (0, 2))
        _check_final_table(p2, o2, t2)
