"""GPU: the fused log-prob kernel kivi_token_logprob, score() / perplexity() and generate(return_logprobs=True).

1. The kernel against its fp64 restatement (kivi_amd.scoring.reference_token_logprobs): V from 1 to 128256, N = 1 / 5 / 37, fp16 and
   fp32; randn, randn * 30, values near +-60000, rows with random -inf entries (one row all but one).  logprob and lse within
   BAR = 2^-19 * max(1, |x_t|, |lse|) -- derived, not tuned: integer truncation <= V * 2^-40 <= 2^-20, expf <= 2 ulp on S ~ 2^-22,
   logf, and two fp32 roundings <= 2^-23 * max(|x_t|, |lse|) -- ranks exactly (planted ties before, at and after the target),
   targets on -inf exactly -inf, no NaN.  The worst ratio to the bar is printed (DESIGN.md section 14 quotes it).
2. Determinism: two calls, and a strided view against its contiguous copy (row_stride > V, a (B, T, V)[:, a:b] slice, an odd element
   offset that breaks the 16-byte alignment, strided targets), give identical bits.  N = 70000 rows.  ignore_index and
   out-of-range targets inside a batch.
3. The model API on the tiny model of tests/test_extend_gpu.py, both cache layouts: one-pass score() against the restatement on
   forward()'s logits; chunked score() BIT FOR BIT against the same chunking composed from public forward() calls, caches included;
   a left-padded batch; a second turn; perplexity; generate(return_logprobs=True) against score(first_chunk=T, chunk_size=1)."""
import pytest
import torch

from helpers import same_bits
from test_extend_gpu import _model

pytestmark = pytest.mark.gpu
BAR = 2.0 ** -19
INF = float("inf")
WORST = {"ratio": 0.0}


def _layouts(monkeypatch, layout):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM
    if layout == "hook":
        monkeypatch.setattr(CM, "supported", lambda *a, **k: False)
        monkeypatch.setattr(A, "_mf_supported", lambda *a, **k: False)


def _check(x, t, ignore_index=-100, what=""):
    """x (N, V) on the CPU, t (N,): the kernel on the GPU copy against the fp64 restatement."""
    from kivi_amd.scoring import reference_token_logprobs, token_logprobs
    lp, lse, rank = (o.cpu() for o in token_logprobs(x.cuda(), t.cuda(), ignore_index, return_lse=True, return_rank=True))
    rlp, rlse, rrank = reference_token_logprobs(x, t, ignore_index)
    assert lp.dtype == lse.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(rank.long(), rrank), (what, rank, rrank)
    assert not lse.isnan().any() and torch.equal(lp.isnan(), rlp.isnan()), what
    scored = rrank >= 0
    xt = x.double().gather(1, t.clamp(0, x.shape[1] - 1).unsqueeze(1)).squeeze(1)
    fin = scored & rlp.isfinite()
    assert torch.equal(lp[scored & ~fin].double(), rlp[scored & ~fin]), what                # a target on -inf: exactly -inf
    assert torch.equal(lp[~scored & ~rlp.isnan()].double(), rlp[~scored & ~rlp.isnan()]), what     # ignored: exactly 0
    scale = torch.maximum(torch.ones_like(rlse), rlse.abs())
    r_lse = ((lse.double() - rlse).abs() / (BAR * scale)).max().item()
    r_lp = 0.0
    if fin.any():
        r_lp = ((lp.double() - rlp).abs()[fin] / (BAR * torch.maximum(scale, xt.abs())[fin])).max().item()
    WORST["ratio"] = max(WORST["ratio"], r_lse, r_lp)
    print(f"kivi_token_logprob {what}: worst |got - ref| / bar = lse {r_lse:.3f}, logprob {r_lp:.3f} (so far {WORST['ratio']:.3f})")
    assert r_lse <= 1.0 and r_lp <= 1.0, (what, r_lse, r_lp)


def _inputs(kind, N, V, g):
    x = torch.randn((N, V), generator=g)
    if kind == "x30":
        x = x * 30
    elif kind == "big":                                # fp16 values near +-60000 (spacing 32)
        x = (torch.where(torch.rand((N, V), generator=g) < 0.5, -1.0, 1.0) * (60000 + 32 * torch.randint(-40, 40, (N, V), generator=g))
             ).half().float()
    elif kind == "ninf":
        x = x.masked_fill(torch.rand((N, V), generator=g) < 0.3, -INF)
        x[0] = -INF                                    # all but one
        x[0, V // 2] = 0.25
        for r in range(1, N):                          # no row of the contract is all -inf
            if x[r].max() == -INF:
                x[r, 0] = 1.0
    return x


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 320, 1025, 4099, 32000, 128256])
def test_kernel_against_fp64_restatement(V, dtype):
    g = torch.Generator().manual_seed(V)
    for N in (1, 5, 37):
        for kind in ("randn", "x30", "big", "ninf"):
            x = _inputs(kind, N, V, g).to(dtype)
            t = torch.randint(0, V, (N,), generator=g)
            if V >= 3:                                 # planted ties: before the target, after it, both
                t = t.clamp(1, V - 2)
                for r in range(N):
                    if r % 4 == 0:
                        x[r, t[r] - 1] = x[r, t[r]]
                    elif r % 4 == 1:
                        x[r, t[r] + 1] = x[r, t[r]]
                    elif r % 4 == 2:
                        x[r, 0] = x[r, V - 1] = x[r, t[r]]
            if kind == "ninf" and N > 1:               # targets on -inf entries
                t[0] = 0 if V // 2 != 0 else t[0]
                if V > 1:
                    x[1, t[1]] = -INF
                    x[1, (t[1] + 1) % V] = 0.5
            for r in range(N):                         # planting may have emptied a row: none of the contract is all -inf
                if x[r].max() == -INF:
                    x[r, (t[r] + 1) % V] = 0.5
            _check(x, t, what=f"V={V} N={N} {kind} {str(dtype)[6:]}")


def test_many_rows():
    g = torch.Generator().manual_seed(7)
    x = (torch.randn((70000, 8), generator=g) * 4).half()
    _check(x, torch.randint(0, 8, (70000,), generator=g), what="N=70000 V=8")


def test_ignore_index_and_out_of_range_inside_a_batch():
    from kivi_amd.scoring import token_logprobs
    g = torch.Generator().manual_seed(8)
    x = torch.randn((9, 1025), generator=g).half()
    t = torch.randint(0, 1025, (9,), generator=g)
    clean = token_logprobs(x.cuda(), t.cuda(), return_lse=True, return_rank=True)
    t2 = t.clone()
    t2[2], t2[4], t2[5], t2[7] = -100, 1025, -1, 2 ** 40
    _check(x, t2, what="ignore / out of range")
    got = token_logprobs(x.cuda(), t2.cuda(), return_lse=True, return_rank=True)
    keep = torch.tensor([0, 1, 3, 6, 8])
    for a, b in zip(clean, got):                       # the neighbours are unaffected, lse is written for every row
        assert torch.equal(a[keep], b[keep])
    assert torch.equal(clean[1], got[1])
    assert got[0][2].item() == 0.0 and got[0][[4, 5, 7]].isnan().all() and got[2][[2, 4, 5, 7]].tolist() == [-1] * 4
    _check(x, t, ignore_index=int(t[3]), what="ignore_index inside the vocabulary")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_determinism_and_strides(dtype):
    from kivi_amd import _lib
    from kivi_amd.scoring import token_logprobs
    g = torch.Generator().manual_seed(9)
    kw = dict(return_lse=True, return_rank=True)

    def same(a, b):
        return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))

    for V in (65, 1025, 4099):
        N = 6
        x = (torch.randn((N, V), generator=g) * 5).to(dtype).cuda()
        t = torch.randint(0, V, (N,), generator=g).cuda()
        base = token_logprobs(x, t, **kw)
        assert same(base, token_logprobs(x, t, **kw))
        # row_stride > V: a padded-vocabulary buffer
        wide = torch.zeros((N, V + 13), dtype=dtype, device="cuda")
        wide[:, :V] = x
        assert wide[:, :V].stride(0) == V + 13 and same(base, token_logprobs(wide[:, :V], t, **kw))
        # an odd element offset: no row starts on a 16-byte boundary it would start on in the contiguous copy
        flat = torch.zeros(N * V + 8, dtype=dtype, device="cuda")
        for off in (1, 3):
            view = flat[off: off + N * V].view(N, V)
            view.copy_(x)
            assert view.data_ptr() % 16 != 0 and same(base, token_logprobs(view, t, **kw))
        # (B, T, V)[:, a:b]: B = 1 is taken by stride, B = 2 is copied; (B, 1, V) views of a (B, T, V) buffer by stride
        for B in (1, 2):
            full = (torch.randn((B, 7, V), generator=g) * 5).to(dtype).cuda()
            tt = torch.randint(0, V, (B, 7), generator=g).cuda()
            ref = token_logprobs(full.clone(), tt, **kw)
            got = token_logprobs(full[:, 2:6], tt[:, 2:6], **kw)
            assert got[0].shape == (B, 4) and same([r[:, 2:6].contiguous() for r in ref], got)
            got = token_logprobs(full[:, 6:], tt[:, 6:], **kw)
            assert same([r[:, 6:].contiguous() for r in ref], got)
        # strided targets (the ABI; the Python layer passes stride 1)
        t3 = torch.full((N, 3), -7, dtype=torch.long, device="cuda")
        t3[:, 0] = t
        out = torch.empty(N, dtype=torch.float32, device="cuda")
        _lib.check(_lib.load().kivi_token_logprob(_lib.ptr(x), 16 if dtype == torch.float16 else 32, V, N, V, _lib.ptr(t3), 3, -100,
                                                  _lib.ptr(out), None, None, _lib.stream_ptr(x)), "kivi_token_logprob")
        assert same([base[0]], [out])


# ------------------------------------------------------------------ 3. the model API
def _compose(model, ids, plan, mask=None, past=None, return_rank=False):
    """score() by hand: public forward() calls over the same pieces, token_logprobs on each piece's logits."""
    from kivi_amd.scoring import token_logprobs
    B, T = ids.shape
    past_len = model._past_len(past)
    tgt = torch.full((B, T), -100, dtype=torch.long, device=ids.device)
    tgt[:, :-1] = ids[:, 1:]
    if mask is not None:
        real = mask[:, past_len:] != 0
        tgt[:, :-1][~(real[:, 1:] & real[:, :-1])] = -100
    out = []
    for a, b in plan:
        lg, past = model(ids[:, a:b], past, last_token_only=False, padding_mask=None if mask is None else mask[:, : past_len + b])
        out.append(token_logprobs(lg, tgt[:, a:b]))
    return torch.cat(out, 1)[:, :-1], past


def _same_caches(pa, pb):
    for a, b in zip(pa, pb):
        ta, tb = a.layer.as_tuple(), b.layer.as_tuple()
        assert ta[8] == tb[8]
        for x, y in zip(ta[:8], tb[:8]):
            assert (x is None and y is None) or (x is not None and y is not None and same_bits(x, y))


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_score_one_pass_and_chunked(nkv, layout, monkeypatch):
    from kivi_amd.scoring import score_plan
    from kivi_amd.scoring import reference_token_logprobs
    _layouts(monkeypatch, layout)
    model = _model(nkv, 31)
    T = 90
    ids = torch.randint(0, 320, (2, T), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    lp, valid, past, rank = model.score(ids, return_rank=True)
    assert getattr(past[0].layer, "layout", "hook") == layout and past[0][-1] == T
    assert lp.shape == valid.shape == rank.shape == (2, T - 1) and lp.dtype == torch.float32 and bool(valid.all())
    lg, _ = model(ids, last_token_only=False)
    rlp, rlse, rrank = reference_token_logprobs(lg[:, :-1], ids[:, 1:])
    xt = lg[:, :-1].double().cpu().gather(-1, ids[:, 1:].cpu().unsqueeze(-1)).squeeze(-1)
    bar = BAR * torch.maximum(torch.maximum(torch.ones_like(rlse), rlse.abs()), xt.abs())
    assert ((lp.cpu().double() - rlp).abs() <= bar).all() and torch.equal(rank.cpu().long(), rrank)
    for c in (1, 7, 33):
        plan = score_plan(ids, 40, c)
        assert len(plan) == 1 + -(-50 // c)
        got, v, pa = model.score(ids, first_chunk=40, chunk_size=c)
        ref, pb = _compose(model, ids, plan)
        assert torch.equal(got, ref) and bool(v.all()), (nkv, layout, c)
        _same_caches(pa, pb)
        assert not torch.equal(got, lp)                # the chunked score sees the quantiser, the one-pass score does not


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_score_left_padded_batch(nkv, layout, monkeypatch):
    from kivi_amd.scoring import score_plan
    from kivi_amd.llama import left_pad
    _layouts(monkeypatch, layout)
    model = _model(nkv, 32)
    g = torch.Generator().manual_seed(4)
    seqs = [torch.randint(1, 320, (n,), generator=g).tolist() for n in (50, 23, 41)]
    ids, mask = left_pad(seqs, pad_token_id=0, device="cuda")
    got, valid, pa = model.score(ids, attention_mask=mask, first_chunk=40, chunk_size=7)
    ref, pb = _compose(model, ids, score_plan(ids, 40, 7), mask=mask)
    want = torch.zeros((3, 49), dtype=torch.bool)
    for r, n in enumerate((50, 23, 41)):
        want[r, 50 - n:] = True                        # context and target real: from the row's first real token on
    assert torch.equal(valid.cpu(), want)
    assert getattr(pa[0].layer, "layout", "hook") == layout and pa[0][-1] == 50
    assert torch.equal(got, ref) and bool((got[~valid] == 0).all()) and bool((got[valid] < 0).all())
    _same_caches(pa, pb)
    # perplexity divides by the number of valid entries (49, 22, 40), not by T - 1
    row, overall = model.perplexity(ids, attention_mask=mask, first_chunk=40, chunk_size=7)
    d, n = got.double().cpu(), torch.tensor([49.0, 22.0, 40.0], dtype=torch.float64)
    assert torch.equal(valid.sum(-1).cpu().double(), n)
    assert torch.allclose(row.cpu(), torch.exp(-d.sum(-1) / n), rtol=1e-12, atol=0)
    assert torch.allclose(overall.cpu(), torch.exp(-d.sum() / n.sum()), rtol=1e-12, atol=0)
    # a mask without a pad is the unmasked path
    a = model.score(ids[:1], attention_mask=mask[:1], first_chunk=40, chunk_size=7)[0]
    assert torch.equal(a, model.score(ids[:1], first_chunk=40, chunk_size=7)[0])


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_score_second_turn_and_perplexity(nkv, layout, monkeypatch):
    from kivi_amd.scoring import score_plan
    _layouts(monkeypatch, layout)
    model = _model(nkv, 33)
    gen = torch.Generator("cuda").manual_seed(5)
    ids1 = torch.randint(0, 320, (2, 45), device="cuda", generator=gen)
    ids2 = torch.randint(0, 320, (2, 23), device="cuda", generator=gen)
    _, _, past = model.score(ids1)
    got, valid, pa = model.score(ids2, past_key_values=past, first_chunk=9, chunk_size=5)
    assert getattr(pa[0].layer, "layout", "hook") == layout and pa[0][-1] == 68 and got.shape == (2, 22)
    _, past = model(ids1)
    ref, pb = _compose(model, ids2, score_plan(ids2, 9, 5), past=past)
    assert torch.equal(got, ref)
    _same_caches(pa, pb)
    # perplexity: exp(-mean) of those entries in fp64, per row and over all rows
    _, past = model(ids1)
    row, overall = model.perplexity(ids2, past_key_values=past, first_chunk=9, chunk_size=5)
    assert row.dtype == overall.dtype == torch.float64 and row.shape == (2,) and overall.shape == ()
    d = got.double().cpu()
    assert torch.allclose(row.cpu(), torch.exp(-d.mean(-1)), rtol=1e-12, atol=0)
    assert torch.allclose(overall.cpu(), torch.exp(-d.mean()), rtol=1e-12, atol=0)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
@pytest.mark.parametrize("nkv", [1, 4])
def test_generate_logprobs_equal_score(nkv, layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(nkv, 34)
    assert getattr(model(torch.zeros((1, 8), dtype=torch.long, device="cuda"))[1][0].layer, "layout", "hook") == layout
    T, n = 29, 12
    ids = torch.randint(0, 320, (3, T), device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    for kw in (dict(), dict(do_sample=True, seed=77, temperature=0.8, top_k=40, top_p=0.9)):
        plain = model.generate(ids, n, **kw)
        seqs, lps = model.generate(ids, n, return_logprobs=True, **kw)
        assert torch.equal(seqs, plain) and lps.shape == (3, n) and lps.dtype == torch.float32
        ref = model.score(seqs, first_chunk=T, chunk_size=1)[0][:, T - 1:]
        # from the second new token on: the same head call on the same (B, 1, H) states, equal by construction
        assert torch.equal(lps[:, 1:], ref[:, 1:]), (layout, kw)
        # the first new token comes from the prompt pass, whose head generate() runs on the last position alone and score() on all
        # T positions: equal bits where the GEMM library gives a row the same bits at both row counts, as it does at this shape
        assert torch.equal(lps[:, :1], ref[:, :1]), (layout, kw)
        assert bool((lps <= 0).all()) and bool(lps.isfinite().all())
        # EOS: a row stops after its first EOS; live positions as before, 0 afterwards
        eos = int(plain[0, T + 3])
        plain_e = model.generate(ids, n, eos_token_id=eos, pad_token_id=0, **kw)
        seqs_e, lps_e = model.generate(ids, n, eos_token_id=eos, pad_token_id=0, return_logprobs=True, **kw)
        assert torch.equal(seqs_e, plain_e) and lps_e.shape[1] == seqs_e.shape[1] - T
        ref_e = model.score(seqs_e, first_chunk=T, chunk_size=1)[0][:, T - 1:]
        stopped = 0
        for r in range(3):
            new = seqs_e[r, T:].tolist()
            stop = new.index(eos) + 1 if eos in new else len(new)
            stopped += stop < len(new)
            assert torch.equal(lps_e[r, :stop], ref_e[r, :stop]) and torch.equal(lps_e[r, :stop], lps[r, :stop])
            assert bool((lps_e[r, stop:] == 0).all())
        assert stopped >= 1
    # no new token: the sequences as they came, and no log-probability
    seqs, lps = model.generate(ids, 0, return_logprobs=True)
    assert torch.equal(seqs, ids) and lps.shape == (3, 0) and lps.dtype == torch.float32


def test_score_head_runs_in_slabs(monkeypatch):
    """More rows than a slab: the head runs on pieces of at most _HEAD_SLAB rows and their log-probabilities land where they belong."""
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    from kivi_amd.scoring import reference_token_logprobs
    model = _model(4, 35)
    T = 90
    ids = torch.randint(0, 320, (2, T), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    whole = model.score(ids)[0]
    monkeypatch.setattr(LlamaForCausalLM_KIVI, "_HEAD_SLAB", 16)
    seen = []
    hook = model.lm_head.register_forward_hook(lambda mod, inp, out: seen.append(out))
    try:
        lp, valid, _, rank = model.score(ids, return_rank=True)
        plain = model.score(ids)[0]
    finally:
        hook.remove()
    assert [tuple(o.shape) for o in seen] == ([(16, 320)] * 11 + [(4, 320)]) * 2 and bool(valid.all())
    assert torch.equal(plain, lp)
    logits = torch.cat(seen[:12]).view(2, T, 320)                      # rows are taken batch-major
    rlp, rlse, rrank = reference_token_logprobs(logits[:, :-1], ids[:, 1:])
    xt = logits[:, :-1].double().cpu().gather(-1, ids[:, 1:].cpu().unsqueeze(-1)).squeeze(-1)
    bar = BAR * torch.maximum(torch.maximum(torch.ones_like(rlse), rlse.abs()), xt.abs())
    assert ((lp.cpu().double() - rlp).abs() <= bar).all() and torch.equal(rank.cpu().long(), rrank)
    # against one slab: the GEMM library may round a logit differently at another row count, by at most one fp16 ulp (two fp32
    # accumulations of the same products, each rounded to fp16 once), so a log-probability moves by at most the ulp of its own
    # logit plus the ulp of the largest
    ulp = 2.0 ** -10 * logits.abs().max().item()
    assert (lp - whole).abs().max().item() <= 2 * ulp + 2 * BAR * max(1.0, rlse.abs().max().item())
