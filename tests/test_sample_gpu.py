"""GPU: the fused sampler kivi_sample and generate / generate_graphed(do_sample=True).

1. The RNG on the device: uniform logits over V = 65536 make every prefix sum exact, so the token is x0 >> 16 of the numpy
   Philox at counter (row, 0, n); 256 rows, several n; n advances by one per call.
2. Against the fp64 reference with the same u (fp16 logits with ties, fp32 logits; V = 320, 32000, 128256; a grid of temperature /
   top_k / top_p / min_p).  A token that differs must be explained by a decision within EPS of its boundary (top-p mass, min-p
   ratio, or u * S against the CDF) -- counted, and rare.  fp16 and fp32 copies of a row, and a strided (B, 1, V) view and a
   contiguous copy, give the same tokens.
3. Distribution: 2^16 draws from a small vocabulary; filtered tokens never appear, chi-square under the p = 1e-6 bound.
4. generate(do_sample=True) on both cache layouts equals an explicit composition of forward steps and Sampler calls; seeds;
   seed=None under torch.manual_seed; EOS / pad; a left-padded batch; a second turn over past_key_values; top_k = 1.
5. generate_graphed(do_sample=True) equals generate(do_sample=True) token for token (whole-step graph and per-layer graphs, with
   and without padding, across a K flush and a capture-then-replay); new parameters never replay a stale capture.
Tiny random-weight models as in tests/test_extend_gpu.py; V = 32000 / 128256 appear only at the single-kernel level."""
import numpy as np
import pytest
import torch

from test_extend_gpu import _model

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _layouts(monkeypatch, layout):
    import kivi_amd.attention as A
    import kivi_amd.cache_mf as CM
    if layout == "hook":
        monkeypatch.setattr(CM, "supported", lambda *a, **k: False)
        monkeypatch.setattr(A, "_mf_supported", lambda *a, **k: False)


# ------------------------------------------------------------------ 1. the RNG
def test_rng_on_device_uniform_rows():
    from kivi_amd.sampling import Sampler, philox_x0
    B, V, seed = 256, 65536, 0x5EED_0123_4567_89AB
    logits = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    smp = Sampler(top_k=0, seed=seed)
    for n in range(4):
        assert int(smp.state[1]) == n
        tok = smp(logits)[:, 0].cpu().numpy()
        assert np.array_equal(tok, (philox_x0(seed, np.arange(B), n) >> 16).astype(np.int64)), n
    assert int(smp.state[1]) == 4 and int(smp.state[0]) == seed


# ------------------------------------------------------------------ 2. against the fp64 reference
def _accepted(logits, u, t, k, p, mp):
    """Tokens of the reference at the nominal parameters and with one boundary moved by EPS (B, up to 7)."""
    from kivi_amd.sampling import reference_sample
    runs = [(u, p, mp), (u, p * (1 - EPS), mp), (u, min(1.0, p * (1 + EPS)), mp), (np.clip(u - EPS, 0, None), p, mp),
            (np.minimum(u + EPS, 1 - 2 ** -24), p, mp)]
    if mp:
        runs += [(u, p, mp * (1 - EPS)), (u, p, mp * (1 + EPS))]
    return torch.stack([reference_sample(logits, uu, t, k, pp, mm) for uu, pp, mm in runs], 1)


def _check_against_reference(logits, grid, seed, stats):
    from kivi_amd.sampling import Sampler, draw_u
    B = logits.shape[0]
    u = draw_u(seed, np.arange(B), 0)
    for t, k, p, mp in grid:
        smp = Sampler(t, k, p, mp, seed=seed)
        tok = smp(logits)[:, 0].cpu()
        acc = _accepted(logits, u, t, k, p, mp)
        stats[1] += B
        off = tok != acc[:, 0]
        stats[0] += int(off.sum())
        assert ((acc == tok[:, None]).any(1)).all(), (t, k, p, mp, tok[off], acc[off])
        smp.reset(seed)
        if logits.dtype == torch.float16:          # the same values in fp32: the same tokens
            assert torch.equal(smp(logits.float())[:, 0].cpu(), tok)


def test_against_reference_small_vocab():
    V, B = 320, 64
    g = torch.Generator().manual_seed(0)
    lg16 = (torch.randn((B, V), generator=g) * 3).half()
    lg16[:8] = (lg16[:8].float() * 2).round().half() / 2               # coarse rows: large tie classes
    lg16[8, :100] = -float("inf")
    lg32 = torch.randn((B, V), generator=g) * 2
    grid = [(t, k, p, mp) for t in (0.6, 1.0, 1.7) for k in (0, 1, 50, V + 5) for p in (1.0, 0.9, 0.5) for mp in (None, 0.05)]
    stats = [0, 0]
    for lg, seed in ((lg16, 11), (lg32, 12)):
        _check_against_reference(lg.cuda(), grid, seed, stats)
    assert stats[0] <= max(2, stats[1] // 1000), stats


@pytest.mark.parametrize("V", [32000, 128256])
def test_against_reference_large_vocab(V):
    B = 4
    g = torch.Generator().manual_seed(V)
    lg16 = (torch.randn((B, V), generator=g) * 3).half()
    lg32 = torch.randn((B, V), generator=g) * 4
    grid = [(1.0, 50, 1.0, None), (0.7, 50, 0.9, None), (1.0, 0, 0.9, None), (1.3, 0, 0.5, 0.05), (1.0, 1, 1.0, None),
            (0.8, V + 5, 0.9, 0.05)]
    stats = [0, 0]
    for lg, seed in ((lg16, 21), (lg32, 22)):
        _check_against_reference(lg.cuda(), grid, seed, stats)
    assert stats[0] <= 2, stats


def test_strided_view_equals_contiguous():
    from kivi_amd.sampling import Sampler
    B, V = 8, 32000
    buf = (torch.randn((B, 1, V + 40), device="cuda") * 3).half()
    view = buf[..., 7: 7 + V]                         # (B, 1, V), row stride V + 40, odd element offset
    a = Sampler(0.9, 50, 0.9, seed=5)(view)
    b = Sampler(0.9, 50, 0.9, seed=5)(view.contiguous())
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. distribution
def test_distribution_chi_square():
    from scipy.stats import chi2
    from kivi_amd.sampling import Sampler, reference_kept
    V, B, calls = 24, 4096, 16
    row = torch.linspace(2.0, -3.0, V)[torch.randperm(V, generator=torch.Generator().manual_seed(3))]
    t, k, p, mp = 1.2, 12, 0.95, 0.02
    keep, e = reference_kept(row[None], t, k, p, mp)
    prob = torch.where(keep, e, torch.zeros_like(e))[0]
    prob = (prob / prob.sum()).numpy()
    smp = Sampler(t, k, p, mp, seed=1234)
    logits = row[None].expand(B, V).contiguous().cuda()
    counts = np.zeros(V, dtype=np.int64)
    for _ in range(calls):
        counts += np.bincount(smp(logits)[:, 0].cpu().numpy(), minlength=V)
    N = B * calls
    assert counts[prob == 0].sum() == 0
    kept = prob > 0
    stat = float((((counts[kept] - N * prob[kept]) ** 2) / (N * prob[kept])).sum())
    assert stat < chi2.isf(1e-6, int(kept.sum()) - 1), (stat, counts, prob)


# ------------------------------------------------------------------ 4. generate(do_sample=True)
def _compose(model, ids, n, sampler, mask=None, past=None):
    """forward over the prompt (or the new turn), then n - 1 steps, each next token drawn by `sampler`."""
    if mask is None:
        lg, past = model(ids, past)
    else:
        lg, past = model(ids, past, padding_mask=mask)
    out = [ids]
    for s in range(n):
        tok = sampler(lg)
        out.append(tok)
        if s == n - 1:
            break
        if mask is None:
            lg, past = model(tok, past)
        else:
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            lg, past = model(tok, past, padding_mask=mask)
    return torch.cat(out, 1)


KW = dict(temperature=0.8, top_k=40, top_p=0.9)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_sampling_equals_composition(layout, monkeypatch):
    from kivi_amd.sampling import Sampler
    _layouts(monkeypatch, layout)
    model = _model(4, 21)
    ids = torch.randint(0, 320, (3, 29), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    n = 12
    a = model.generate(ids, n, do_sample=True, seed=77, **KW)
    assert getattr(model(ids)[1][0].layer, "layout", "hook") == layout
    assert torch.equal(a, _compose(model, ids, n, Sampler(seed=77, **KW)))
    assert torch.equal(a, model.generate(ids, n, do_sample=True, seed=77, **KW))
    assert not torch.equal(a, model.generate(ids, n, do_sample=True, seed=78, **KW))
    torch.manual_seed(5)
    b = model.generate(ids, n, do_sample=True, **KW)
    torch.manual_seed(5)
    assert torch.equal(b, model.generate(ids, n, do_sample=True, **KW))
    # top_k = 1: every token is in the argmax tie class of its logits
    smp = Sampler(top_k=1, seed=3)
    lg, past = model(ids)
    for _ in range(6):
        tok = smp(lg)
        assert bool((lg[:, 0].gather(1, tok) == lg[:, 0].max(-1, keepdim=True).values).all())
        lg, past = model(tok, past)
    # EOS / pad: a row stops after its first EOS, the rows and tokens before it are unchanged
    eos = int(a[0, 29 + 3])
    c = model.generate(ids, n, do_sample=True, seed=77, eos_token_id=eos, pad_token_id=0, **KW)
    for r in range(3):
        gen = a[r, 29:].tolist()
        stop = gen.index(eos) + 1 if eos in gen else len(gen)
        assert c[r, 29: 29 + stop].tolist() == gen[:stop]
        assert (c[r, 29 + stop:] == 0).all()


def test_generate_sampling_padded_and_second_turn():
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import Sampler
    model = _model(4, 22)
    ids, mask = left_pad([list(range(3, 40)), list(range(50, 71)), list(range(100, 110))], pad_token_id=0, device="cuda")
    a = model.generate(ids, 10, attention_mask=mask, do_sample=True, seed=9, **KW)
    assert torch.equal(a, _compose(model, ids, 10, Sampler(seed=9, **KW), mask=mask))
    # second turn over the caches of the first
    ids2 = torch.randint(0, 320, (3, 9), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    mask2 = torch.cat([mask, torch.ones_like(ids2)], 1)
    _, past = model(ids, padding_mask=mask)
    b = model.generate(ids2, 8, past_key_values=past, attention_mask=mask2, do_sample=True, seed=10, min_p=0.05)
    _, past = model(ids, padding_mask=mask)
    assert torch.equal(b, _compose(model, ids2, 8, Sampler(min_p=0.05, seed=10), mask=mask2, past=past))


# ------------------------------------------------------------------ 5. generate_graphed(do_sample=True)
@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_graphed_sampling_equals_eager(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    _layouts(monkeypatch, layout)
    model = _model(4, 23)
    ids = torch.randint(0, 320, (2, 21), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    n = 40                                           # past a K flush (residual_length 32); the whole graph captures, replays
    for kw in (dict(seed=31, **KW), dict(seed=32, temperature=1.5, top_k=0, top_p=0.7, min_p=0.02)):
        g = model.generate_graphed(ids, n, do_sample=True, **kw)
        assert torch.equal(g, model.generate(ids, n, do_sample=True, **kw)), (layout, kw)
    if layout == "mfma":
        assert model.graphs.stats[1] >= 1 and model.graphs.stats[2] >= n // 2      # captured, then replayed
    pids, mask = left_pad([list(range(3, 30)), list(range(60, 70))], pad_token_id=0, device="cuda")
    g = model.generate_graphed(pids, 36, attention_mask=mask, do_sample=True, seed=33, **KW)
    assert torch.equal(g, model.generate(pids, 36, attention_mask=mask, do_sample=True, seed=33, **KW)), layout
    # greedy after sampling: no sampled capture is replayed
    assert torch.equal(model.generate_graphed(ids, 8), model.generate(ids, 8))
