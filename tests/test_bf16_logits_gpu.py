"""GPU: bf16 logits in the fused kernels (KIVI_LOGITS_BF16).

A bf16 logit is its exact fp32 image, so every entry gives on a bf16 tensor, bit for bit, what it gives with logits_bits 32 on
`logits.float()` -- the entry the suite already holds to fp64.  No tolerance, at every vocabulary of tests/sample_plan.VS.
Rows: tests/sample_edges.rows(V)["fp32"] rounded to bf16 (general values, -inf stretches), a coarse row of large tie classes with a
-inf tail, a row whose values tie in threes from the top (the k-th and (k + 1)-th largest tie for k = 1, 5 and 32) and a row of
all-equal values.  The bf16 rows are read at an ODD element stride from a base that is only 2-byte aligned, so every row meets the
16-byte loads of the scorers at another alignment; the fp32 copy is contiguous.

* Sampler over sample_edges.grid(V): identical tokens.
* RowSampler: plain; with a history table and penalties -- identical tokens, identical updated table; with an allow mask, a bias
  list and min_new_tokens in force -- identical tokens.
* token_logprobs (lse, rank) and top_logprobs (k in {1, 5, 32}, with and without targets, lse, rank): every output bit-identical."""
import pytest
import torch

import sample_edges as E
from sample_plan import VS

pytestmark = pytest.mark.gpu
INF = float("inf")


def _rows(V):
    """-> (bf16 (n, V) on the GPU at an odd row stride from a 2-byte aligned base, its contiguous fp32 copy)."""
    g = torch.Generator().manual_seed(V + 1)
    base = E.rows(V)["fp32"].bfloat16()
    coarse = ((torch.randn(V, generator=g) * 3 * 2).round() / 2).bfloat16()
    if V // 5:
        coarse[V - V // 5:] = -INF
    extra = [coarse, torch.full((V,), 1.25).bfloat16()]
    if V >= 40:
        ties = (torch.randn(V, generator=g) * 3).bfloat16()
        idx = torch.randperm(V, generator=g)[:36]
        ties[idx] = (100.0 - 0.5 * (torch.arange(36) // 3)).bfloat16()
        extra.append(ties)
    x = torch.cat([base, torch.stack(extra)])
    n, stride = x.shape[0], V + 1 + V % 2
    buf = torch.zeros(n * stride + 1, dtype=torch.bfloat16, device="cuda")
    lg = torch.as_strided(buf, (n, V), (stride, 1), 1)
    lg.copy_(x)
    assert lg.stride(0) % 2 == 1 and lg.data_ptr() % 4 == 2 and torch.equal(lg.cpu().float(), x.float())
    return lg, lg.float().contiguous()


def _same(a, b):
    if a.is_floating_point():
        return a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
    return a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("V", VS)
def test_samplers_draw_the_tokens_of_the_fp32_entry(V):
    from kivi_amd.sampling import RowSampler, Sampler, SamplingParams
    lg, lf = _rows(V)
    n = lg.shape[0]
    for t, k, p, mp in E.grid(V):
        a, b = Sampler(t, k, p, mp, seed=23), Sampler(t, k, p, mp, seed=23)
        for _ in range(2):
            assert torch.equal(a(lg), b(lf)), (t, k, p, mp)
    grid = E.grid(V)
    plain = [SamplingParams(i % 3 != 2, *grid[i % len(grid)], seed=40 + i) for i in range(n)]
    a, b = RowSampler(plain, "cuda", streams=list(range(n))), RowSampler(plain, "cuda", streams=list(range(n)))
    for _ in range(2):
        assert torch.equal(a(lg), b(lf))
    # a history table and penalties: the tokens, and the table with each token counted
    g = torch.Generator().manual_seed(V + 7)
    words = torch.tensor([0, 0, 0, 1, 5, 32767])[torch.randint(0, 6, (n, V), generator=g)]
    words = words | (torch.rand((n, V), generator=g) < 0.3).long() * E.PROMPT
    top = lf.cpu().topk(min(8, V), -1).indices                          # the candidates of every filter carry history
    for j, word in enumerate([1, E.PROMPT, E.PROMPT | 5, 32767, 0, 2, E.PROMPT, 1][: top.shape[1]]):
        words.scatter_(1, top[:, j: j + 1], torch.full((n, 1), word))
    table = torch.where(words >= 0x8000, words - 0x10000, words).to(torch.int16).cuda()
    pen = [SamplingParams(i % 3 != 2, *grid[(i + 1) % len(grid)], seed=60 + i, repetition_penalty=E.PENS[i % 4][0],
                          presence_penalty=E.PENS[i % 4][1], frequency_penalty=E.PENS[i % 4][2]) for i in range(n)]
    a, b = RowSampler(pen, "cuda", vocab_size=V), RowSampler(pen, "cuda", vocab_size=V)
    for rs in (a, b):
        rs.seen[:, :V].copy_(table)
    for _ in range(2):
        ta, tb = a(lg), b(lf)
        assert torch.equal(ta, tb) and torch.equal(a.seen, b.seen) and a.draw_index.tolist() == b.draw_index.tolist()
    assert not torch.equal(a.seen[:, :V], table)                         # (the draws were counted)
    # an allow mask, a bias list and min_new_tokens in force (its suppressed id: the row's unconstrained argmax)
    best = lf.argmax(-1).tolist()
    allowed = sorted(set(range(0, V, 3)) | set(top[:, :4].flatten().tolist()))
    con = []
    for i in range(n):
        bias = {int(top[i, j]): v for j, v in zip(range(top.shape[1]), (2.5, -INF, -1.75, 0.5))}
        con.append(SamplingParams(i % 3 != 2, *grid[(i + 2) % len(grid)], seed=80 + i, logit_bias=bias, allowed_token_ids=allowed,
                                  min_new_tokens=2 if V > 1 else 0, repetition_penalty=1.2 if i % 2 else 1.0))
    sup = [[best[i]] for i in range(n)]
    a, b = RowSampler(con, "cuda", vocab_size=V, suppress=sup), RowSampler(con, "cuda", vocab_size=V, suppress=sup)
    for s in range(3):                                                   # draws 0 and 1 suppressed, draw 2 not
        ta, tb = a(lg), b(lf)
        assert torch.equal(ta, tb) and torch.equal(a.seen, b.seen), s


@pytest.mark.parametrize("V", VS)
def test_scorers_give_the_bits_of_the_fp32_entry(V):
    from kivi_amd.scoring import token_logprobs, top_logprobs
    lg, lf = _rows(V)
    n = lg.shape[0]
    g = torch.Generator().manual_seed(V + 3)
    targets = torch.randint(0, V, (n,), generator=g)
    targets[0] = -100
    if V >= 40:
        targets[-1] = int(lf[-1].argmax())                                # a member of the top tie class
    targets = targets.cuda()
    for x, y in zip(token_logprobs(lg, targets, return_lse=True, return_rank=True),
                    token_logprobs(lf, targets, return_lse=True, return_rank=True)):
        assert _same(x, y)
    assert _same(token_logprobs(lg, targets), token_logprobs(lf, targets))
    for k in [k for k in (1, 5, 32) if k <= V]:
        for tg in (None, targets):
            a = top_logprobs(lg, k, tg, return_lse=True, return_rank=tg is not None)
            b = top_logprobs(lf, k, tg, return_lse=True, return_rank=tg is not None)
            for name, x, y in zip(a._fields, a, b):
                assert (x is None and y is None) or _same(x, y), (k, name)
        if V >= 40:                                                       # the cut goes through a tie class: ascending index decides
            ids = a.ids[-1].tolist()
            vals = lf[-1, ids].tolist()
            assert vals[-1] == lf[-1].topk(k + 1).values[-1].item() and vals == sorted(vals, reverse=True)
            assert all(i < j for i, j, u, v in zip(ids, ids[1:], vals, vals[1:]) if u == v)
        eq = a.ids[-2 if V >= 40 else -1].tolist()                        # the all-equal row: the k lowest indices
        assert eq == list(range(k))
    # (B, 1, V) views, as a decode step hands them over
    assert _same(token_logprobs(lg[:, None], targets[:, None]), token_logprobs(lf[:, None], targets[:, None]))
