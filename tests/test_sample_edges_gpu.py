"""GPU: general rows through the fused samplers against the fp64 reference at every vocabulary boundary of tests/sample_plan.py.

The method of tests/test_sample_gpu.py's _check_against_reference, at each V of sample_plan.VS instead of three sizes off every
boundary: fp16 rows (randn * 3, one coarse row of large tie classes) and fp32 rows (randn * 4), every row with a -inf stretch -- the
row's tail [V - V // 5, V) on row 0 --, the grid of the large-vocabulary test, the reference at the kernel's own u.  A token that is
not the reference's must be accepted by the rule of tests/sample_edges.py (five points up to V = 65536, the wide rule above), and
such draws number at most max(2, N // 1000) per test.  tests/test_sample_edges_cpu.py pins how many draws the reference alone
leaves open: at most one per test, so the cap binds the kernel.

1. kivi_sample (Sampler), fp16 and fp32; the fp32 copy of an fp16 row draws the same token.
2. kivi_sample_rows_pen (RowSampler with a history table) against reference_penalise on the CPU fed through the same acceptance:
   at these sizes this, not the identity with kivi_sample_rows on pre-penalised logits, is the evidence.  kivi_sample_rows on the
   reference's penalised logits draws the same tokens."""
import pytest
import torch

import sample_edges as E
from sample_plan import VS

pytestmark = pytest.mark.gpu


def _cap(n):
    return max(2, n // 1000)


@pytest.mark.parametrize("V", VS)
def test_rows_against_fp64(V):
    from kivi_amd.sampling import Sampler
    off = n = 0
    for name in ("fp16", "fp32"):
        lg = E.rows(V)[name].cuda()
        for (t, k, p, mp), acc in zip(E.grid(V), E.reference(V, name)):
            smp = Sampler(t, k, p, mp, seed=E.SEEDS[name])
            tok = smp(lg)[:, 0].cpu()
            ok = acc.ok(tok)
            assert bool(ok.all()), (name, t, k, p, mp, tok[~ok].tolist(), acc.nominal[~ok].tolist(), acc.five[~ok].tolist())
            off, n = off + int((tok != acc.nominal).sum()), n + len(tok)
            if name == "fp16":                       # the same values in fp32: the same tokens
                smp.reset(E.SEEDS[name])
                assert torch.equal(smp(lg.float())[:, 0].cpu(), tok)
    print(f"sample edges V={V}: kivi_sample off-nominal {off} of {n} draws (cap {_cap(n)})")
    assert off <= _cap(n), (off, n)


@pytest.mark.parametrize("V", VS)
def test_penalised_rows_against_fp64(V):
    from kivi_amd.sampling import RowSampler, SamplingParams
    lg, words = E.history(V)
    B = lg.shape[0]
    x, accs = E.pen_reference(V)
    lg, x = lg.cuda(), x.cuda()
    table = torch.where(words >= 0x8000, words - 0x10000, words).to(torch.int16)
    off = n = 0
    for (t, k, p, mp), acc in zip(E.grid(V), accs):
        base = [SamplingParams(True, t, k, p, mp, seed) for seed in E.PEN_SEEDS[:B]]
        pen = [SamplingParams(True, t, k, p, mp, seed, repetition_penalty=a, presence_penalty=b, frequency_penalty=c)
               for seed, (a, b, c) in zip(E.PEN_SEEDS, E.PENS[:B])]
        rs = RowSampler(pen, "cuda", streams=E.PEN_STREAMS[:B], vocab_size=V)
        rs.seen[:, :V].copy_(table)
        tok = rs(lg)[:, 0].cpu()
        ok = acc.ok(tok)
        assert bool(ok.all()), (t, k, p, mp, tok[~ok].tolist(), acc.nominal[~ok].tolist(), acc.five[~ok].tolist())
        off, n = off + int((tok != acc.nominal).sum()), n + B
        plain = RowSampler(base, "cuda", streams=E.PEN_STREAMS[:B])
        assert torch.equal(plain(x)[:, 0].cpu(), tok)                        # the two kernels agree on the reference's fp32 logits
        want = words.clone()
        for r, i in enumerate(tok.tolist()):
            want[r, i] += int(want[r, i] & E.COUNT != E.COUNT)                # counted where it was written, saturating
        assert torch.equal(rs.seen[:, :V].cpu().long() & 0xFFFF, want) and rs.draw_index.tolist() == [1] * B
    print(f"sample edges V={V}: kivi_sample_rows_pen off-nominal {off} of {n} draws (cap {_cap(n)})")
    assert off <= _cap(n), (off, n)
