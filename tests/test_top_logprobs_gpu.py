"""GPU: the fused top-k log-probability kernel kivi_token_top_logprobs and the paths that return its lists.

(a) The kernel against the fp64 restatement (kivi_amd.scoring.reference_top_logprobs): V from 1 to 128256, k = 1 / 2 / 5 / 20 / 32,
    N = 1 / 5 / 37, fp16 and fp32; the input kinds of tests/test_score_gpu.py and four more (one repeated value, three distinct
    values, a tie class planted across the k-th place at indices V - 1, 0 and V // 2, -0 / +0 mixed at the maximum).  Ids EXACTLY
    (the order is on input values, there is no arithmetic in it); values and lse within section 14's derived bar
    2^-19 * max(1, |x|, |lse|); entries on -inf exactly -inf.  The worst ratio to the bar is printed.
(b) Identity with kivi_token_logprob: target_logprob, lse and rank in the same bits; a scored target of rank < k sits at position
    `rank` of the list with the bits of target_logprob; targets=None gives the same lists.  (Checked on every input of (a).)
(c) Determinism and layout: two calls, row_stride > V, (B, T, V)[:, a:b], odd element offsets, top_stride > k with canaries, strided
    targets, 70000 rows, ignored / out-of-range targets inside a batch, a launch replayed from a graph.
(d) score / generate / generate_graphed / generate_continuous with top_logprobs on the tiny model of tests/test_extend_gpu.py."""
import pytest
import torch

from test_extend_gpu import _model
from test_score_gpu import _inputs

pytestmark = pytest.mark.gpu
BAR = 2.0 ** -19
INF = float("inf")
WORST = {"ratio": 0.0}
KS = (1, 2, 5, 20, 32)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32
                                                                     else a, b.contiguous().view(torch.int32)
                                                                     if b.dtype == torch.float32 else b)


def _same(a, b):
    """Two TopLogprobs (or tuples of tensors / None) hold the same bits."""
    return all((x is None and y is None) or (x is not None and y is not None and _bits_equal(x, y)) for x, y in zip(a, b))


def _check(x, k, t, what, ref=None):
    """x (N, V) on the CPU in its dtype, t (N,) targets: (a) and (b) for one input and one k.  `ref`: the restatement at k = 32 (or
    V), shared among the k of one input."""
    from kivi_amd.scoring import reference_top_logprobs, token_logprobs, top_logprobs
    N, V = x.shape
    xc, tc = x.cuda(), t.cuda()
    got = top_logprobs(xc, k, tc, return_lse=True, return_rank=True)
    ids, lps, lse = got.ids.cpu(), got.logprobs.cpu(), got.lse.cpu()
    assert ids.shape == lps.shape == (N, k) and ids.dtype == torch.int64 and lps.dtype == lse.dtype == torch.float32
    rids, rlps = ref if ref is not None else reference_top_logprobs(x, k)
    rids, rlps = rids[:, :k], rlps[:, :k]
    assert torch.equal(ids, rids), (what, (ids != rids).nonzero()[:4], ids[(ids != rids).any(-1)][:2], rids[(ids != rids).any(-1)][:2])
    rlse = torch.logsumexp(x.double(), -1)
    xs = x.double().gather(1, rids)
    ninf = xs == -INF
    assert torch.equal(lps[ninf].double(), rlps[ninf]) and not lps.isnan().any() and not lse.isnan().any(), what
    scale = torch.maximum(torch.ones_like(rlse), rlse.abs())
    r_lse = ((lse.double() - rlse).abs() / (BAR * scale)).max().item()
    bar = BAR * torch.maximum(scale.unsqueeze(1), xs.abs())
    r_lp = ((lps.double() - rlps).abs()[~ninf] / bar[~ninf]).max().item() if (~ninf).any() else 0.0
    WORST["ratio"] = max(WORST["ratio"], r_lse, r_lp)
    print(f"kivi_token_top_logprobs {what} k={k}: worst |got - ref| / bar = lse {r_lse:.3f}, values {r_lp:.3f} "
          f"(so far {WORST['ratio']:.3f})")
    assert r_lse <= 1.0 and r_lp <= 1.0, (what, r_lse, r_lp)
    # (b) the same bits as kivi_token_logprob; the target inside its list
    base = token_logprobs(xc, tc, return_lse=True, return_rank=True)
    assert _same((got.target_logprob, got.lse, got.rank), base), what
    rank = got.rank.cpu().long()
    inside = (rank >= 0) & (rank < k)
    rows = inside.nonzero().squeeze(1)
    assert torch.equal(ids[rows, rank[rows]], t[rows]), what
    assert torch.equal(lps[rows, rank[rows]].view(torch.int32), got.target_logprob.cpu()[rows].view(torch.int32)), what
    return got


def _straddle(x, k):
    """Plant a tie class across the k-th place at indices V - 1, 0 and V // 2: with the other tokens' (k - 1)-th largest value the
    class holds at least four tokens from rank <= k - 2 on, so it reaches past the cut and only its lowest indices may be taken."""
    N, V = x.shape
    x = x.clone()
    planted = torch.tensor([V - 1, 0, V // 2])
    others = x.clone()
    others[:, planted] = -INF
    v = others.double().sort(-1, descending=True).values[:, max(k - 2, 0)]
    x[:, planted] = v.to(x.dtype).unsqueeze(1)
    return x


@pytest.mark.parametrize("N", [1, 5, 37])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("V", [1, 2, 31, 32, 33, 63, 64, 65, 320, 1025, 4099, 32000, 128256])
def test_kernel_against_fp64_restatement(V, dtype, N):
    from kivi_amd.scoring import reference_top_logprobs, top_logprobs
    g = torch.Generator().manual_seed(1000 * N + V)
    ks = [k for k in KS if k <= V]
    tag = f"V={V} N={N} {str(dtype)[6:]}"
    for kind in ("randn", "x30", "big", "ninf", "const", "three", "pm0"):
        if kind == "const":
            x = torch.full((N, V), 1.5)
        elif kind == "three":
            x = torch.tensor([-1.0, 0.5, 2.0])[torch.randint(0, 3, (N, V), generator=g)]
        elif kind == "pm0":                            # negative everywhere but a few zeros of both signs
            x = -torch.randn((N, V), generator=g).abs() - 1.0
            z = torch.rand((N, V), generator=g) < max(0.01, 6.0 / V)
            z[:, V // 2] = True
            x = torch.where(z, torch.where(torch.rand((N, V), generator=g) < 0.5, -0.0, 0.0), x)
        else:
            x = _inputs(kind, N, V, g)
        x = x.to(dtype)
        t = torch.randint(0, V, (N,), generator=g)
        ref = reference_top_logprobs(x, ks[-1])
        for k in ks:
            got = _check(x, k, t, f"{tag} {kind}", ref)
            if kind == "const":
                assert torch.equal(got.ids.cpu(), torch.arange(k).expand(N, k))
        none = top_logprobs(x.cuda(), ks[-1])          # without targets: the same lists, nothing else
        assert none.target_logprob is None and none.lse is None and none.rank is None
        assert _same((none.ids, none.logprobs), (got.ids, got.logprobs))
    if V >= 8:
        for k in [k for k in ks if k < V - 3]:
            x = _straddle(torch.randn((N, V), generator=g).to(dtype), k)
            got = _check(x, k, torch.randint(0, V, (N,), generator=g), f"{tag} straddle")
            ids = got.ids.cpu()
            assert bool((ids == 0).any(-1).all()) and not bool((ids == V - 1).any()), (tag, k)


def test_many_rows():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((70000, 8), generator=g) * 4).half()
    _check(x, 8, torch.randint(0, 8, (70000,), generator=g), "N=70000 V=8")


def test_ignore_index_and_out_of_range_inside_a_batch():
    from kivi_amd.scoring import top_logprobs
    g = torch.Generator().manual_seed(8)
    x = torch.randn((9, 1025), generator=g).half()
    t = torch.randint(0, 1025, (9,), generator=g)
    kw = dict(return_lse=True, return_rank=True)
    clean = top_logprobs(x.cuda(), 5, t.cuda(), **kw)
    t2 = t.clone()
    t2[2], t2[4], t2[5], t2[7] = -100, 1025, -1, 2 ** 40
    got = _check(x, 5, t2, "ignore / out of range")
    keep = torch.tensor([0, 1, 3, 6, 8])
    assert _same([c[keep] for c in clean], [c[keep] for c in got])
    assert _same((clean.ids, clean.logprobs, clean.lse), (got.ids, got.logprobs, got.lse))     # every row keeps its list and its lse
    assert got.target_logprob[2].item() == 0.0 and got.target_logprob[[4, 5, 7]].isnan().all()
    assert got.rank[[2, 4, 5, 7]].tolist() == [-1] * 4
    _check(x, 5, t, "ignore_index inside the vocabulary")
    inside = top_logprobs(x.cuda(), 5, t.cuda(), ignore_index=int(t[3]), **kw)
    assert inside.target_logprob[3].item() == 0.0 and inside.rank[3].item() == -1
    assert _same((clean.ids, clean.logprobs, clean.lse), (inside.ids, inside.logprobs, inside.lse))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_determinism_and_strides(dtype):
    from kivi_amd import _lib
    from kivi_amd.scoring import top_logprobs
    g = torch.Generator().manual_seed(9)
    kw = dict(return_lse=True, return_rank=True)
    bits = 16 if dtype == torch.float16 else 32
    for V, k in ((65, 5), (1025, 20), (4099, 32)):
        N = 6
        x = (torch.randn((N, V), generator=g) * 5).to(dtype)
        x[1, ::3] = x[1, 0]                            # a row whose class at the cut is large: the index digits run
        x = x.cuda()
        t = torch.randint(0, V, (N,), generator=g).cuda()
        base = top_logprobs(x, k, t, **kw)
        assert _same(base, top_logprobs(x, k, t, **kw))
        wide = torch.zeros((N, V + 13), dtype=dtype, device="cuda")
        wide[:, :V] = x
        assert wide[:, :V].stride(0) == V + 13 and _same(base, top_logprobs(wide[:, :V], k, t, **kw))
        flat = torch.zeros(N * V + 8, dtype=dtype, device="cuda")
        for off in (1, 3):
            view = flat[off: off + N * V].view(N, V)
            view.copy_(x)
            assert view.data_ptr() % 16 != 0 and _same(base, top_logprobs(view, k, t, **kw))
        for B in (1, 2):                               # (B, T, V)[:, a:b]: B = 1 is taken by stride, B = 2 is copied
            full = (torch.randn((B, 7, V), generator=g) * 5).to(dtype).cuda()
            tt = torch.randint(0, V, (B, 7), generator=g).cuda()
            ref = top_logprobs(full.clone(), k, tt, **kw)
            got = top_logprobs(full[:, 2:6], k, tt[:, 2:6], **kw)
            assert got.ids.shape == (B, 4, k) and _same([r[:, 2:6].contiguous() for r in ref], got)
            got = top_logprobs(full[:, 6:], k, tt[:, 6:], **kw)
            assert _same([r[:, 6:].contiguous() for r in ref], got)
        # the ABI: strided targets, top_stride > k with canaries around and between the rows, no targets with an lse
        t3 = torch.full((N, 3), -7, dtype=torch.long, device="cuda")
        t3[:, 0] = t
        pitch = k + 3
        ids = torch.full((N + 2, pitch), -77, dtype=torch.int64, device="cuda")
        top = torch.full((N + 2, pitch), 7.5, dtype=torch.float32, device="cuda")
        out, lse = (torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(2))
        rank = torch.empty(N, dtype=torch.int32, device="cuda")
        f = _lib.load().kivi_token_top_logprobs
        _lib.check(f(_lib.ptr(x), bits, V, N, V, k, _lib.ptr(t3), 3, -100, _lib.ptr(ids[1]), _lib.ptr(top[1]), pitch, _lib.ptr(out),
                     _lib.ptr(lse), _lib.ptr(rank), _lib.stream_ptr(x)), "kivi_token_top_logprobs")
        assert _same(base, (ids[1:-1, :k], top[1:-1, :k], out, lse, rank))
        assert bool((ids[0] == -77).all() and (ids[-1] == -77).all() and (ids[:, k:] == -77).all())
        assert bool((top[0] == 7.5).all() and (top[-1] == 7.5).all() and (top[:, k:] == 7.5).all())
        ids2, top2, lse2 = torch.empty_like(base.ids), torch.empty_like(base.logprobs), torch.empty_like(lse)
        _lib.check(f(_lib.ptr(x), bits, V, N, V, k, None, 0, -100, _lib.ptr(ids2), _lib.ptr(top2), k, None, _lib.ptr(lse2), None,
                     _lib.stream_ptr(x)), "kivi_token_top_logprobs")
        assert _same((base.ids, base.logprobs, base.lse), (ids2, top2, lse2))


def test_replayed_from_a_graph_equals_eager():
    from kivi_amd.scoring import top_logprobs
    g = torch.Generator().manual_seed(10)
    x = (torch.randn((5, 4099), generator=g) * 5).half().cuda()
    x[2, 100:200] = x[2].max()                         # ties at the top: the index digits inside the graph
    t = torch.randint(0, 4099, (5,), generator=g).cuda()
    kw = dict(return_lse=True, return_rank=True)
    eager = top_logprobs(x, 20, t, **kw)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        top_logprobs(x, 20, t, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = top_logprobs(x, 20, t, **kw)
    for _ in range(2):
        for o in held:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, held)


# ------------------------------------------------------------------ (d) the model API
def _compose_top(model, ids, plan, k, mask=None):
    """The lists of score(top_logprobs=k) by hand: public forward() calls over the same pieces, top_logprobs on each piece's logits."""
    from kivi_amd.scoring import top_logprobs
    past, ti, tl = None, [], []
    for a, b in plan:
        lg, past = model(ids[:, a:b], past, last_token_only=False, padding_mask=None if mask is None else mask[:, :b])
        res = top_logprobs(lg, k)
        ti.append(res.ids)
        tl.append(res.logprobs)
    return torch.cat(ti, 1)[:, :-1], torch.cat(tl, 1)[:, :-1]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_score_top_logprobs(nkv, layout, monkeypatch):
    from kivi_amd.scoring import score_plan
    from kivi_amd.llama import left_pad
    from test_score_gpu import _layouts, _same_caches
    _layouts(monkeypatch, layout)
    model = _model(nkv, 61)
    T = 90
    ids = torch.randint(0, 320, (2, T), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    for kw in (dict(), dict(first_chunk=40, chunk_size=1), dict(first_chunk=40, chunk_size=7)):
        lp0, valid0, past0 = model.score(ids, **kw)
        lp, valid, past, ti, tl = model.score(ids, top_logprobs=5, **kw)
        assert getattr(past[0].layer, "layout", "hook") == layout
        assert _bits_equal(lp, lp0) and torch.equal(valid, valid0), (layout, kw)
        _same_caches(past, past0)
        assert ti.shape == tl.shape == (2, T - 1, 5) and ti.dtype == torch.int64 and tl.dtype == torch.float32
        ri, rl = _compose_top(model, ids, score_plan(ids, kw.get("first_chunk"), kw.get("chunk_size")), 5)
        assert torch.equal(ti, ri) and _bits_equal(tl, rl), (layout, kw)
        # with the rank: the scored token sits at its rank with the bits of its log-probability
        res = model.score(ids, return_rank=True, top_logprobs=5, **kw)
        assert len(res) == 6 and _bits_equal(res[0], lp0) and torch.equal(res[4], ti) and _bits_equal(res[5], tl)
        rank = res[3].long()
        inside = rank < 5
        assert bool(inside.any()) and torch.equal(ti.gather(-1, rank.clamp(max=4).unsqueeze(-1)).squeeze(-1)[inside], ids[:, 1:][inside])
        assert _bits_equal(tl.gather(-1, rank.clamp(max=4).unsqueeze(-1)).squeeze(-1)[inside], lp0[inside])
    # a left-padded batch: entries that are not valid hold id -1 and value 0
    g = torch.Generator().manual_seed(4)
    seqs = [torch.randint(1, 320, (n,), generator=g).tolist() for n in (50, 23, 41)]
    pids, mask = left_pad(seqs, pad_token_id=0, device="cuda")
    lp0, valid0, _ = model.score(pids, attention_mask=mask, first_chunk=40, chunk_size=7)
    lp, valid, _, ti, tl = model.score(pids, attention_mask=mask, first_chunk=40, chunk_size=7, top_logprobs=5)
    assert _bits_equal(lp, lp0) and torch.equal(valid, valid0) and not bool(valid.all())
    assert bool((ti[~valid] == -1).all()) and bool((tl[~valid] == 0).all()) and bool((ti[valid] >= 0).all())
    ri, rl = _compose_top(model, pids, score_plan(pids, 40, 7), 5, mask=mask)
    assert torch.equal(ti[valid], ri[valid]) and _bits_equal(tl[valid], rl[valid])


SAMPLED = dict(do_sample=True, seed=77, temperature=0.8, top_k=40, top_p=0.9)


def _check_lists(new, lps, ti, tl, greedy):
    """Token (..., n), its log-probabilities and lists: finite, <= 0, ordered; a greedy token is entry 0, any token that appears in
    its list has the bits of its log-probability there."""
    assert bool(tl.isfinite().all()) and bool((tl <= 0).all()) and bool((tl[..., :-1] >= tl[..., 1:]).all())
    hit = ti == new.unsqueeze(-1)
    assert torch.equal(tl[hit].view(torch.int32), lps.unsqueeze(-1).expand_as(tl)[hit].view(torch.int32))
    if greedy:
        assert torch.equal(ti[..., 0], new) and _bits_equal(tl[..., 0].contiguous(), lps.contiguous())


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_generate_top_logprobs(nkv, layout, monkeypatch):
    from test_score_gpu import _layouts
    _layouts(monkeypatch, layout)
    model = _model(nkv, 62)
    assert _layout_of(model) == layout
    T, n = 29, 12
    ids = torch.randint(0, 320, (3, T), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    for kw in (dict(), SAMPLED):
        seqs0, lps0 = model.generate(ids, n, return_logprobs=True, **kw)
        seqs, lps, ti, tl = model.generate(ids, n, return_logprobs=True, top_logprobs=5, **kw)
        assert torch.equal(seqs, seqs0) and _bits_equal(lps, lps0), (layout, kw)
        assert ti.shape == tl.shape == (3, n, 5) and ti.dtype == torch.int64 and tl.dtype == torch.float32
        _check_lists(seqs[:, T:], lps, ti, tl, greedy=not kw)
        eos = int(seqs0[0, T + 3])
        e0 = model.generate(ids, n, eos_token_id=eos, pad_token_id=0, return_logprobs=True, **kw)
        e = model.generate(ids, n, eos_token_id=eos, pad_token_id=0, return_logprobs=True, top_logprobs=5, **kw)
        assert torch.equal(e[0], e0[0]) and _bits_equal(e[1], e0[1]) and e[2].shape == e[3].shape == (3, e[0].shape[1] - T, 5)
        stopped = 0
        for r in range(3):
            new = e[0][r, T:].tolist()
            stop = new.index(eos) + 1 if eos in new else len(new)
            stopped += stop < len(new)
            assert torch.equal(e[2][r, :stop], ti[r, :stop]) and _bits_equal(e[3][r, :stop], tl[r, :stop])
            assert bool((e[2][r, stop:] == -1).all()) and bool((e[3][r, stop:] == 0).all())
        assert stopped >= 1
    seqs, lps, ti, tl = model.generate(ids, 0, return_logprobs=True, top_logprobs=5)
    assert torch.equal(seqs, ids) and lps.shape == (3, 0) and ti.shape == tl.shape == (3, 0, 5)


def _first_difference(a, b):
    d = (a.double() - b.double()).abs()
    where = (a.view(torch.int32) != b.view(torch.int32)).nonzero()
    return f"largest difference {d.max().item():.3e}, first at {where[0].tolist() if len(where) else None}"


def _layout_of(model):
    return getattr(model(torch.zeros((1, 8), dtype=torch.long, device="cuda"))[1][0].layer, "layout", "hook")


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_generate_graphed_top_logprobs_equal_generate(nkv, layout, monkeypatch):
    """Whole-step graph (mfma) and per-layer graphs (hook), across a K flush (residual_length 32)."""
    from test_score_gpu import _layouts
    _layouts(monkeypatch, layout)
    model = _model(nkv, 63)
    assert _layout_of(model) == layout
    ids = torch.randint(0, 320, (3, 21), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    n = 40
    plain = model.generate_graphed(ids, n)
    assert torch.is_tensor(plain)
    for kw in (dict(), SAMPLED):
        want = model.generate(ids, n, return_logprobs=True, top_logprobs=5, **kw)
        got = model.generate_graphed(ids, n, return_logprobs=True, top_logprobs=5, **kw)
        assert len(got) == 4 and torch.equal(got[0], want[0]), (layout, kw)
        assert torch.equal(got[0], model.generate_graphed(ids, n, **kw))
        assert _bits_equal(got[1], want[1]), (layout, kw, _first_difference(got[1], want[1]))
        assert torch.equal(got[2], want[2]) and _bits_equal(got[3], want[3]), (layout, kw, _first_difference(got[3], want[3]))
        _check_lists(got[0][:, 21:], got[1], got[2], got[3], greedy=not kw)
        two = model.generate_graphed(ids, n, return_logprobs=True, **kw)          # the log-probabilities alone
        assert len(two) == 2 and torch.equal(two[0], want[0]) and _bits_equal(two[1], want[1])
    if layout == "mfma":
        assert model.graphs.stats[1] >= 1 and model.graphs.stats[2] >= n // 2     # captured, then replayed
    # the graphs are keyed by k: the same k keeps them, another k (and none) builds new ones
    model.generate_graphed(ids, 4, return_logprobs=True, top_logprobs=5)
    held = model.graphs
    assert held.logprobs == 5 and held.top_ids.shape == (3, 1, 5) and held.lp.shape == (3, 1)
    model.generate_graphed(ids, 4, return_logprobs=True, top_logprobs=5)
    assert model.graphs is held
    model.generate_graphed(ids, 4, return_logprobs=True, top_logprobs=3)
    assert model.graphs is not held and model.graphs.logprobs == 3
    model.generate_graphed(ids, 4)
    assert model.graphs.logprobs is None and model.graphs.lp is None
    # decode_graphed: entry s is the score of the token step s produced
    lg, past = model(ids)
    toks, lp, ti, tl = model.decode_graphed(lg.argmax(-1), past, 21, 6, logprobs=2)
    assert toks.shape == lp.shape == (3, 6) and ti.shape == tl.shape == (3, 6, 2)
    produced = torch.cat([toks[:, 1:], model.graphs.tok], dim=1)
    assert torch.equal(ti[..., 0], produced) and _bits_equal(tl[..., 0].contiguous(), lp)
    model.graphs.end()


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_generate_continuous_full_batch_equals_generate(nkv, layout, monkeypatch):
    from test_score_gpu import _layouts
    _layouts(monkeypatch, layout)
    model = _model(nkv, 64)
    assert _layout_of(model) == layout
    ids = torch.randint(1, 320, (3, 26), device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    n = 9
    seqs, lps, ti, tl = model.generate(ids, n, return_logprobs=True, top_logprobs=3)
    for graphed in (False, True):
        toks, clp, cti, ctl = model.generate_continuous([r.tolist() for r in ids], n, 3, return_logprobs=True, top_logprobs=3,
                                                        graphed=graphed)
        for r in range(3):
            assert torch.equal(toks[r], seqs[r, 26:]) and _bits_equal(clp[r], lps[r].contiguous()), (layout, graphed, r)
            assert torch.equal(cti[r], ti[r]) and _bits_equal(ctl[r], tl[r].contiguous()), (layout, graphed, r)
    two = model.generate_continuous([r.tolist() for r in ids], n, 3, return_logprobs=True)
    assert len(two) == 2 and all(_bits_equal(a, b.contiguous()) for a, b in zip(two[1], lps))


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("kw", [dict(), dict(compact=32, short_admissions=True)], ids=["plain", "compact_short"])
def test_generate_continuous_mixed_requests(kw, layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    from test_admit_gpu import LENS, LIMITS, _prompts
    from test_score_gpu import _layouts
    _layouts(monkeypatch, layout)
    model = _model(4, 65)
    assert _layout_of(model) == layout
    prompts = _prompts(5, LENS)
    params = [SamplingParams(temperature=0.8, top_k=40, top_p=0.9, seed=71), SamplingParams(do_sample=False),
              SamplingParams(temperature=1.4, top_k=0, min_p=0.02, seed=72), SamplingParams(temperature=0.9, top_k=30, seed=73),
              SamplingParams(seed=74), SamplingParams(do_sample=False), SamplingParams(temperature=1.1, top_k=0, top_p=0.8, seed=75)]
    plain = model.generate_continuous(prompts, LIMITS, 3, sampling=params, **kw)
    runs = []
    for graphed in (False, True):
        toks, lps, ti, tl = model.generate_continuous(prompts, LIMITS, 3, sampling=params, graphed=graphed, return_logprobs=True,
                                                      top_logprobs=3, **kw)
        runs.append((toks, lps, ti, tl))
        assert [t.tolist() for t in toks] == [t.tolist() for t in plain], graphed
        for r in range(7):
            n = toks[r].numel()
            assert n == LIMITS[r] and lps[r].shape == (n,) and ti[r].shape == tl[r].shape == (n, 3)
            assert lps[r].dtype == tl[r].dtype == torch.float32 and ti[r].dtype == torch.int64
            assert bool(lps[r].isfinite().all()) and bool((lps[r] <= 0).all())
            _check_lists(toks[r], lps[r], ti[r], tl[r], greedy=not params[r].do_sample)
    for a, b in zip(runs[0], runs[1]):                               # graphed equals eager bit for bit
        assert all(_bits_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_picked_scores_is_the_direct_launch_and_what_score_into_leaves(dtype):
    """The one choice of the decode loops: nothing, kivi_token_logprob, or kivi_token_top_logprobs -- the bits of the direct calls
    and of the captured step's buffers, a row with the ignore index among them."""
    from kivi_amd.scoring import picked_scores, score_into, token_logprobs, top_logprobs
    g = torch.Generator().manual_seed(23)
    logits = (torch.randn((3, 1, 320), generator=g) * 4).to(dtype).cuda()
    tokens = torch.tensor([[7], [-100], [319]], device="cuda")
    assert picked_scores(logits, tokens, None) == ()
    one = picked_scores(logits, tokens, 0)
    assert len(one) == 1 and _bits_equal(one[0], token_logprobs(logits, tokens)) and one[0].shape == (3, 1)
    assert one[0][:, 0].tolist()[1] == 0 and bool((one[0][[0, 2]] < 0).all())
    lp, ids, top = picked_scores(logits, tokens, 3)
    ref = top_logprobs(logits, 3, tokens)
    assert _bits_equal(lp, ref.target_logprob) and torch.equal(ids, ref.ids) and _bits_equal(top, ref.logprobs)
    assert _bits_equal(lp, one[0]) and ids.shape == top.shape == (3, 1, 3) and ids.dtype == torch.int64
    buf = torch.full((3, 1), float("nan"), device="cuda")
    score_into(logits, tokens, buf)
    assert _bits_equal(buf, one[0])
    buf, bi, bt = torch.full((3, 1), float("nan"), device="cuda"), torch.full((3, 1, 3), -7, device="cuda"), torch.full((3, 1, 3), 1.0, device="cuda")
    score_into(logits, tokens, buf, bi, bt)
    assert _bits_equal(buf, lp) and torch.equal(bi, ids) and _bits_equal(bt, top)
