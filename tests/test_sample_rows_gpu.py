"""GPU: per-request sampling -- kivi_sample_rows, RowSampler and generate / generate_graphed / decode_graphed(sampling=)
(DESIGN.md section 15).

1. THE IDENTITY: uniform records with seed = s, stream = b, draw_index = n give exactly kivi_sample's tokens at {s, n} (a grid of
   parameters, fp16 / fp32, a strided view, n = 0, 1, 2^32 + 3; V = 320, 32000, 128256); both draw-index forms end at n + 1.
2. Rows are independent: a batch of 7 different records equals 7 one-row calls, the fp64 reference at u = draw_u_rows(...) under the
   boundary rule of tests/test_sample_gpu.py, and permutes with its rows.
3. Greedy rows: torch.argmax on tie-free rows, the lowest index of a planted tie, a maximum in the last partial chunk, -inf rows;
   the index advances, seed and n do not matter.  Records outside the contract degrade as the header says.
4. set_row / select.
5. generate(sampling=[...]) on both layouts against an explicit composition; EOS / pad; left padding; a second turn.
6. Batch position does not matter at the sampler (given logits, 20 calls, rows 0 / 2 / 4 of differently filled batches).
7. n samples per prompt: one prompt pass, forked caches, streams 0..n-1; the caller's caches untouched; return_logprobs.
8. generate_graphed(sampling=) equals generate(sampling=) across a K flush; new parameters in the same RowSampler replay the
   captured step.
9. Chi-square of 2^14 draws (streams 0..3 interleaved) at top_k = 8.
Logits as in tests/test_sample_gpu.py: random fp16 with tie classes and -inf entries; the tiny model of tests/test_extend_gpu.py."""
import numpy as np
import pytest
import torch

from test_extend_gpu import _model
from test_sample_gpu import _accepted, _compose, _layouts

pytestmark = pytest.mark.gpu
NS = (0, 1, 2 ** 32 + 3)


def _logits(B, V, seed, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((B, V), generator=g) * 3
    if dtype == torch.float16:
        lg = lg.half()
        lg[: max(1, B // 3)] = (lg[: max(1, B // 3)].float() * 2).round().half() / 2      # coarse rows: large tie classes
    lg[-1, : V // 3] = -float("inf")
    lg[0, V // 2:: 7] = -float("inf")
    return lg.cuda()


def _params(t, k, p, mp, seed, do_sample=True):
    from kivi_amd.sampling import SamplingParams
    return SamplingParams(do_sample, t, k, p, mp, seed)


def _set_n(rs, ns):
    rs.draw_index.copy_(torch.tensor([n if np.isscalar(n) else int(n) for n in ns], dtype=torch.int64))


# ------------------------------------------------------------------ 1. uniform parameters equal the old kernel
def _check_identity(logits, grid, seed):
    from kivi_amd.sampling import RowSampler, Sampler
    B = logits.shape[0]
    for t, k, p, mp in grid:
        smp = Sampler(t, k, p, mp, seed=seed)
        rs = RowSampler(_params(t, k, p, mp, seed), "cuda", streams=list(range(B)))
        for n in NS:
            smp.state[1] = n
            _set_n(rs, [n] * B)
            old, new = smp(logits), rs(logits)
            assert torch.equal(old, new), (t, k, p, mp, n, old[:, 0].tolist(), new[:, 0].tolist())
            assert int(smp.state[1]) == n + 1 and rs.draw_index.tolist() == [n + 1] * B


def test_uniform_rows_equal_kivi_sample():
    V, B = 320, 5
    grid = [(t, k, p, mp) for t in (0.6, 1.7) for k in (0, 1, 50, V + 5) for p in (1.0, 0.9, 0.5) for mp in (None, 0.05)]
    lg16 = _logits(B, V, 1)
    _check_identity(lg16, grid, 0x5EED_0123_4567_89AB)
    _check_identity(_logits(B, V, 2, torch.float32), grid, 2 ** 64 - 5)
    buf = torch.zeros((B, 1, V + 40), dtype=torch.float16, device="cuda")
    view = buf[..., 7: 7 + V]                          # (B, 1, V), row stride V + 40, odd element offset
    view.copy_(lg16[:, None])
    _check_identity(view, grid[::5], 77)


@pytest.mark.parametrize("V", [32000, 128256])
def test_uniform_rows_equal_kivi_sample_large_vocab(V):
    grid = [(1.0, 50, 1.0, None), (0.7, 50, 0.9, None), (1.3, 0, 0.5, 0.05), (1.0, 1, 1.0, None), (0.8, V + 5, 0.9, 0.05)]
    _check_identity(_logits(5, V, V), grid, 21)
    _check_identity(_logits(5, V, V + 1, torch.float32), grid[1:3], 22)


# ------------------------------------------------------------------ 2. rows are independent
def _mixed_rows():
    return [_params(1.0, 50, 1.0, None, 101), _params(1.0, 0, 1.0, None, 102, do_sample=False), _params(0.7, 1, 1.0, None, 103),
            _params(1.0, 0, 1.0, None, 104), _params(1.6, 40, 0.9, None, 2 ** 64 - 1), _params(0.8, 0, 0.5, 0.05, 106),
            _params(1.2, 400, 0.95, 0.02, 101)]          # (greedy, top_k = 1, all off, a seed shared with row 0)


def _lowest_argmax(row):
    x = row.float()
    return int((x == x.max()).nonzero()[0])


def test_rows_are_independent():
    from kivi_amd.sampling import RowSampler, draw_u_rows
    V, B = 320, 7
    ps, streams = _mixed_rows(), [0, 3, 0, 9, 2 ** 32 - 1, 1, 0]
    perm = [4, 0, 6, 2, 5, 1, 3]
    stats = [0, 0]
    for lg in (_logits(B, V, 3), _logits(B, V, 4, torch.float32)):
        rs = RowSampler(ps, "cuda", streams=streams)
        for call in range(6):
            ns = [call + (2 ** 33 if b == 5 else 0) for b in range(B)]
            _set_n(rs, ns)
            tok = rs(lg)[:, 0].cpu()
            assert rs.draw_index.tolist() == [n + 1 for n in ns]
            u = draw_u_rows([p.seed for p in ps], streams, ns)
            for b, p in enumerate(ps):
                one = RowSampler(p, "cuda", streams=[streams[b]])
                _set_n(one, [ns[b]])
                assert int(one(lg[b: b + 1])) == int(tok[b]), (call, b)
                if not p.do_sample:
                    assert int(tok[b]) == _lowest_argmax(lg[b])
                    continue
                acc = _accepted(lg[b: b + 1], u[b: b + 1], p.temperature, p.top_k, p.top_p, p.min_p)[0]
                stats[1] += 1
                stats[0] += int(tok[b] != acc[0])
                assert bool((acc == tok[b]).any()), (call, b, int(tok[b]), acc.tolist())
            # the permuted batch gives the permuted tokens
            prs = rs.select(perm)
            _set_n(prs, [ns[i] for i in perm])
            assert torch.equal(prs(lg[perm])[:, 0].cpu(), tok[perm]), call
    assert stats[0] <= max(2, stats[1] // 1000), stats


# ------------------------------------------------------------------ 3. greedy rows, records outside the contract
def test_greedy_rows():
    from kivi_amd.sampling import RowSampler
    g = torch.Generator().manual_seed(5)
    for V in (320, 323, 1, 64, 1500):
        B = 8
        lg = torch.randn((B, V), generator=g) * 3
        assert all(len(set(r.tolist())) == V for r in lg)                     # tie-free
        want = lg.argmax(-1)
        if V >= 320:
            top = lg.max() + 1
            lg[1, [V - 2, 17, 200]] = top                                      # a planted tie at the maximum: the lowest index
            lg[2, V - 2] = top                                                 # the maximum in the last partial chunk (V = 320 + 3)
            lg[3, :] = -float("inf")
            lg[3, V - 1] = -5.0                                                # one finite entry among -inf: never a -inf token
            lg[4, :] = -float("inf")                                           # all -inf: some token
            lg[5, [5, 9]] = torch.tensor([0.0, -0.0]) + 100                    # (+-0 offsets: equal values)
            want = torch.tensor([int(want[0]), 17, V - 2, V - 1, -1, 5, int(want[6]), int(want[7])])
        for dtype in (torch.float32, torch.float16):
            x = lg.to(dtype).cuda()
            if dtype == torch.float16:
                ref = torch.tensor([_lowest_argmax(r) for r in x.cpu()])       # fp16 rounding makes ties: the rule decides
            else:
                ref = want.clone()
            a = RowSampler([_params(1.0, 50, 1.0, None, 7 + b, do_sample=False) for b in range(B)], "cuda")
            b_ = RowSampler([_params(0.3, 2, 0.4, 0.5, 900 + b, do_sample=False) for b in range(B)], "cuda", streams=list(range(B)))
            _set_n(b_, [2 ** 32 + 5] * B)
            ta, tb = a(x)[:, 0].cpu(), b_(x)[:, 0].cpu()
            assert torch.equal(ta, tb)                                         # neither seed, stream, n nor the filters matter
            assert a.draw_index.tolist() == [1] * B and b_.draw_index.tolist() == [2 ** 32 + 6] * B
            assert bool(((ta >= 0) & (ta < V)).all())
            live = torch.ones(B, dtype=torch.bool)
            if V >= 320:
                live[4] = False
            assert torch.equal(ta[live], ref[live]), (V, dtype, ta.tolist(), ref.tolist())
            if dtype == torch.float32 and V < 320:
                assert torch.equal(ta, x.argmax(-1).cpu())


def test_records_outside_the_contract_degrade():
    """The rules of include/kivi_hip.h for records the host entry cannot check: read as the nearest legal value."""
    from kivi_amd.sampling import RowSampler, SampleRow
    V = 320
    lg = _logits(1, V, 6).expand(8, V).contiguous()
    nan, inf = float("nan"), float("inf")
    #         written                              read as
    cases = [((1.0, -5, 1.0, 0.0, 0), (1.0, 0, 1.0, None, True)), ((0.9, 40, 1.5, 0.0, 0), (0.9, 40, 1.0, None, True)),
             ((0.9, 40, nan, 0.0, 0), (0.9, 40, 1.0, None, True)), ((1.1, 0, 0.9, -1.0, 0), (1.1, 0, 0.9, None, True)),
             ((1.1, 0, 0.9, nan, 0), (1.1, 0, 0.9, None, True)), ((nan, 50, 1.0, 0.0, 0), (1.0, 50, 1.0, None, False)),
             ((0.0, 50, 1.0, 0.0, 0), (1.0, 50, 1.0, None, False)), ((inf, 50, 1.0, 0.0, 0), (1.0, 50, 1.0, None, False)),
             ((-2.0, 50, 1.0, 0.0, 0), (1.0, 50, 1.0, None, False)), ((1.0, 0, 0.0, 0.0, 0), (1.0, 1, 1.0, None, True)),
             ((1.0, 0, -3.0, 0.0, 0), (1.0, 1, 1.0, None, True)), ((1.0, 0, 1.0, 1.0, 0), (1.0, 1, 1.0, None, True)),
             ((1.0, 0, 1.0, 7.0, 0), (1.0, 1, 1.0, None, True))]
    for n in (0, 5):
        for raw, (t, k, p, mp, sample) in cases:
            want = RowSampler(_params(t, k, p, mp, 42, do_sample=sample), "cuda", B=8)
            got = RowSampler(_params(1.0, 50, 1.0, None, 42), "cuda", B=8)
            rec = SampleRow(raw[0], raw[1], raw[2], raw[3], 42, 0, raw[4])
            got.records.copy_(torch.tensor(np.frombuffer(bytes(rec), dtype=np.int64)).expand(8, 4))
            _set_n(want, range(n, n + 8))
            _set_n(got, range(n, n + 8))
            a, b = got(lg), want(lg)
            assert torch.equal(a, b), (raw, a[:, 0].tolist(), b[:, 0].tolist())
            assert got.draw_index.tolist() == list(range(n + 1, n + 9))


# ------------------------------------------------------------------ 4. set_row and select
def test_set_row_and_select():
    from kivi_amd.sampling import RowSampler, SamplingParams
    V, B = 320, 4
    lg = _logits(B, V, 8)
    ps = [_params(1.0, 50, 1.0, None, 11), _params(0.8, 0, 0.9, None, 12), _params(1.0, 50, 1.0, None, 13, do_sample=False),
          _params(1.3, 20, 1.0, 0.02, 14)]
    rs, ref = RowSampler(ps, "cuda", streams=[0, 1, 2, 3]), RowSampler(ps, "cuda", streams=[0, 1, 2, 3])
    key = rs.key()
    for _ in range(3):
        assert torch.equal(rs(lg), ref(lg))
    new = SamplingParams(temperature=0.5, top_k=7, seed=99)
    rs.set_row(1, new, stream=5)
    assert rs.key() == key and rs.draw_index.tolist() == [3, 0, 3, 3]
    fresh = RowSampler(new, "cuda", streams=[5])
    for _ in range(4):
        tok, want = rs(lg), ref(lg)
        assert int(tok[1]) == int(fresh(lg[1:2]))                              # the new request, as if alone
        assert torch.equal(tok[[0, 2, 3]], want[[0, 2, 3]])                    # the others continue their streams
    # a sampled row becomes greedy, a greedy one sampled
    rs.set_row(0, SamplingParams(do_sample=False))
    rs.set_row(2, ps[3], stream=3)
    twin = RowSampler(ps[3], "cuda", streams=[3])
    tok = rs(lg)
    assert int(tok[0]) == _lowest_argmax(lg[0]) and int(tok[2]) == int(twin(lg[2:3]))
    # select: rows, seeds and draw indices travel; the source is not advanced by the copy
    before = rs.draw_index.clone()
    sel = rs.select([3, 1, 1])
    assert sel.draw_index.tolist() == before[[3, 1, 1]].tolist() and sel.key() != rs.key()
    want = rs(lg)
    assert torch.equal(sel(lg[[3, 1, 1]]), want[[3, 1, 1]])
    sel.reset()
    assert sel.draw_index.tolist() == [0, 0, 0] and rs.draw_index.tolist() == (before + 1).tolist()


# ------------------------------------------------------------------ 5. generate(sampling=[...])
def _requests():
    from kivi_amd.sampling import SamplingParams
    return [SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=71), SamplingParams(do_sample=False),
            SamplingParams(temperature=1.4, top_k=0, min_p=0.02, seed=72)]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_rows_equals_composition(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler
    _layouts(monkeypatch, layout)
    model = _model(4, 41)
    T, n = 29, 12
    ids = torch.randint(0, 320, (3, T), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    req = _requests()
    a = model.generate(ids, n, sampling=req)
    assert getattr(model(ids)[1][0].layer, "layout", "hook") == layout and a.shape == (3, T + n)
    assert torch.equal(a, _compose(model, ids, n, RowSampler(req, "cuda")))
    assert torch.equal(a, model.generate(ids, n, sampling=RowSampler(req, "cuda")))           # a ready RowSampler
    plain = model.generate(ids, n)
    assert torch.equal(a[1], plain[1])                                          # the greedy request, as in a greedy batch
    assert not torch.equal(a[0], plain[0]) and not torch.equal(a[2], plain[2])
    # one SamplingParams for every request: every row draws what a batch of one with that seed draws from its logits
    one = model.generate(ids, n, sampling=req[0])
    assert torch.equal(one, _compose(model, ids, n, RowSampler(req[0], "cuda", B=3))) and torch.equal(one[0], a[0])
    # EOS / pad: a row stops after its first EOS, the rows and tokens before it are unchanged
    eos = int(a[0, T + 3])
    c = model.generate(ids, n, sampling=req, eos_token_id=eos, pad_token_id=0)
    for r in range(3):
        gen = a[r, T:].tolist()
        stop = gen.index(eos) + 1 if eos in gen else len(gen)
        assert c[r, T: T + stop].tolist() == gen[:stop]
        assert (c[r, T + stop:] == 0).all()
    # a left-padded batch, then a second turn over its caches
    pids, mask = left_pad([list(range(3, 40)), list(range(50, 71)), list(range(100, 110))], pad_token_id=0, device="cuda")
    b = model.generate(pids, 10, attention_mask=mask, sampling=req)
    assert torch.equal(b, _compose(model, pids, 10, RowSampler(req, "cuda"), mask=mask))
    assert torch.equal(b[1], model.generate(pids, 10, attention_mask=mask)[1])
    ids2 = torch.randint(0, 320, (3, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    mask2 = torch.cat([mask, torch.ones_like(ids2)], 1)
    _, past = model(pids, padding_mask=mask)
    d = model.generate(ids2, 8, past_key_values=past, attention_mask=mask2, sampling=req)
    _, past = model(pids, padding_mask=mask)
    assert torch.equal(d, _compose(model, ids2, 8, RowSampler(req, "cuda"), mask=mask2, past=past))


# ------------------------------------------------------------------ 6. batch position does not matter at the sampler
def test_batch_position_does_not_matter():
    from kivi_amd.sampling import RowSampler, SamplingParams
    V, calls = 320, 20
    p = SamplingParams(temperature=0.9, top_k=30, top_p=0.95, seed=0xABCDEF)
    mine = _logits(calls, V, 9)                                                # the request's logits, one row per call
    seqs = []
    for row, B, fill in ((0, 1, 0), (2, 5, 1), (4, 6, 2)):
        others = [SamplingParams(do_sample=bool((i + fill) % 3), temperature=0.5 + 0.3 * i, top_k=(0, 5, 60)[(i + fill) % 3],
                                 seed=1000 * fill + i) for i in range(B)]
        others[row] = p
        rs = RowSampler(others, "cuda")
        batch = _logits(B, V, 10 + fill)
        out = []
        for c in range(calls):
            batch[row] = mine[c]
            out.append(int(rs(batch)[row]))
        seqs.append(out)
    assert seqs[0] == seqs[1] == seqs[2]
    assert len(set(seqs[0])) > 3


# ------------------------------------------------------------------ 7. n samples per prompt
def _caches_bytes(past):
    return [[t.clone() for t in p.layer.__dict__.values() if torch.is_tensor(t)] for p in past]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_n_samples_per_prompt(layout, monkeypatch):
    from kivi_amd.sampling import RowSampler, SamplingParams
    from kivi_amd.scoring import token_logprobs
    _layouts(monkeypatch, layout)
    model = _model(4, 42)
    B, T, n, G = 2, 29, 3, 12
    ids = torch.randint(0, 320, (B, T), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    req = [SamplingParams(temperature=0.9, top_k=40, seed=81), SamplingParams(temperature=1.3, top_k=0, top_p=0.9, seed=82)]
    rows = torch.arange(B, device="cuda").repeat_interleave(n)

    def compose(ids, G, past=None):
        """One prompt pass on the B requests, caches forked by index_select, a RowSampler of streams 0..n-1 per request."""
        lg, past = model(ids, past)
        assert getattr(past[0].layer, "layout", "hook") == layout
        past = [p.layer.index_select(rows).as_tuple() for p in past]
        fork = [p.layer.clone().as_tuple() for p in past]
        lg = lg.index_select(0, rows)
        rs = RowSampler([req[b] for b in range(B) for _ in range(n)], "cuda", streams=[j for _ in range(B) for j in range(n)])
        out, lps = [ids.repeat_interleave(n, 0)], []
        for s in range(G):
            tok = rs(lg)
            out.append(tok)
            lps.append(token_logprobs(lg, tok))
            if s < G - 1:
                lg, past = model(tok, past)
        return torch.cat(out, 1), torch.cat(lps, 1), fork

    seqs, lps = model.generate(ids, G, sampling=req, num_return_sequences=n, return_logprobs=True)
    want, want_lps, fork = compose(ids, G)
    assert seqs.shape == (B * n, T + G) and lps.shape == (B * n, G) and lps.dtype == torch.float32
    assert torch.equal(seqs, want) and torch.equal(lps, want_lps)
    assert torch.equal(seqs, model.generate(ids, G, sampling=req, num_return_sequences=n))
    assert torch.equal(seqs[:, :T], ids.repeat_interleave(n, 0))
    for b in range(B):                                                         # n different samples of each prompt
        assert len({tuple(seqs[b * n + j, T:].tolist()) for j in range(n)}) == n
    # stream 0 of a request is the request sampled alone (n = 1) in the same batch
    assert torch.equal(model.generate(ids, 1, sampling=req), seqs[::n, : T + 1])
    # log-probabilities as DESIGN.md section 14 has them for generate: from the second new token on they are score() with
    # chunk_size = 1 over the forked caches, bit for bit (the same head call on the same states); the first comes from the
    # prompt pass's row of logits, the same one for the n rows of a request
    ref = model.score(seqs[:, T:], past_key_values=fork, first_chunk=1, chunk_size=1)[0]
    assert torch.equal(lps[:, 1:], ref)
    first = token_logprobs(model(ids)[0].index_select(0, rows), seqs[:, T: T + 1])
    assert torch.equal(lps[:, :1], first)
    assert bool((lps <= 0).all()) and bool(lps.isfinite().all())
    # second turn: the caller's caches are byte for byte what they were
    ids2 = torch.randint(0, 320, (B, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    _, past = model(ids)
    before = _caches_bytes(past)
    length = past[0][-1]
    got = model.generate(ids2, 8, past_key_values=past, sampling=req, num_return_sequences=n)
    after = _caches_bytes(past)
    assert past[0][-1] == length and len(before[0]) > 2
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for a, b in zip(before, after) for x, y in zip(a, b))
    want2, _, _ = compose(ids2, 8, [p.layer.clone().as_tuple() for p in past])
    assert torch.equal(got, want2)


# ------------------------------------------------------------------ 8. the graphed path
@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_graphed_rows_equals_eager(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler, SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 43)
    ids = torch.randint(0, 320, (3, 21), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    n = 40                                           # past a K flush (residual_length 32); the whole graph captures, replays
    req = _requests()
    g = model.generate_graphed(ids, n, sampling=req)
    assert torch.equal(g, model.generate(ids, n, sampling=req)), layout
    if layout == "mfma":
        assert model.graphs.stats[1] >= 1 and model.graphs.stats[2] >= n // 2      # captured, then replayed
    pids, mask = left_pad([list(range(3, 30)), list(range(60, 70)), list(range(80, 99))], pad_token_id=0, device="cuda")
    g = model.generate_graphed(pids, 36, attention_mask=mask, sampling=req)
    assert torch.equal(g, model.generate(pids, 36, attention_mask=mask, sampling=req)), layout
    # greedy, and the scalar sampler, after a RowSampler: nothing stale is replayed
    assert torch.equal(model.generate_graphed(ids, 8), model.generate(ids, 8))
    kw = dict(do_sample=True, seed=5, top_k=30)
    assert torch.equal(model.generate_graphed(ids, 8, **kw), model.generate(ids, 8, **kw))

    # one RowSampler over one set of caches: other parameters (set_row between calls) replay what was captured
    short = ids[:, :8]
    second = [SamplingParams(temperature=0.6, top_k=5, seed=91), SamplingParams(temperature=1.2, top_k=0, top_p=0.8, seed=92),
              SamplingParams(do_sample=False)]
    steps = 6                                        # 8 + 2 * 6 tokens: inside one residual, one geometry class

    def run(graphed):
        rs = RowSampler(req, "cuda")
        lg, past = model(short)
        tok, out, stats = rs(lg), [], []
        for call in range(2):
            if graphed:
                new = model.decode_graphed(tok, past, short.shape[1] + call * steps, steps, sampling=rs)
                tok = model.graphs.tok.clone()
                stats.append(model.graphs.stats)
            else:
                new = []
                for _ in range(steps):
                    new.append(tok)
                    lg, past = model(tok, past)
                    tok = rs(lg)
                new = torch.cat(new, 1)
            out.append(new)
            for b, p in enumerate(second):           # new requests take over the rows
                rs.set_row(b, p, stream=b)
            tok = tok.clone()
        return torch.cat(out, 1), stats, rs

    model.release_graphs()
    got, stats, rs = run(True)
    graphs = model.graphs
    want, _, _ = run(False)
    assert torch.equal(got, want), layout
    assert model.graphs is graphs and graphs.sampler_key == rs.key()            # keyed by buffers: built once for both calls
    if layout == "mfma":
        (e1, c1, r1), (e2, c2, r2) = stats
        assert (e1, c1, r1) == (1, 1, steps - 1)     # first call: one eager step, one capture, the rest replayed
        assert (e2, c2, r2) == (1, 1, 2 * steps - 1)     # second call, other parameters: no new capture, every step a replay


# ------------------------------------------------------------------ 9. distribution
def test_rows_distribution_chi_square():
    from scipy.stats import chi2
    from kivi_amd.sampling import RowSampler, SamplingParams, reference_kept
    V, streams, calls = 24, 4, 4096                  # 2^14 draws of one row: streams 0..3 of one seed, interleaved call by call
    row = torch.linspace(2.0, -3.0, V)[torch.randperm(V, generator=torch.Generator().manual_seed(3))]
    t, k = 1.2, 8
    keep, e = reference_kept(row[None], t, k, 1.0, None)
    prob = torch.where(keep, e, torch.zeros_like(e))[0]
    prob = (prob / prob.sum()).numpy()
    assert int((prob > 0).sum()) == k
    rs = RowSampler(SamplingParams(temperature=t, top_k=k, seed=1234), "cuda", streams=list(range(streams)))
    logits = row[None].expand(streams, V).contiguous().cuda()
    out = torch.empty((calls, streams), dtype=torch.int64, device="cuda")
    for c in range(calls):
        rs(logits, out=out[c])
    assert rs.draw_index.tolist() == [calls] * streams
    toks = out.cpu().numpy()
    assert len({tuple(toks[:64, j]) for j in range(streams)}) == streams     # the streams differ
    counts = np.bincount(toks.reshape(-1), minlength=V)
    N = calls * streams
    assert counts[prob == 0].sum() == 0              # filtered tokens are never drawn
    kept = prob > 0
    stat = float((((counts[kept] - N * prob[kept]) ** 2) / (N * prob[kept])).sum())
    assert stat < chi2.isf(1e-6, int(kept.sum()) - 1), (stat, counts, prob)
