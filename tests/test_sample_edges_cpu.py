"""CPU: the fp64 side of tests/test_sample_edges_gpu.py alone.  That file lets at most max(2, N // 1000) draws per test differ from the
reference's nominal token, each explained by a decision within EPS of its boundary.  The cap is a condition on the kernel only if
the reference itself leaves that little room: here the draws whose accepted set holds more than one token are counted and pinned,
per vocabulary, for the rows, seeds and grid that the GPU file uses.  No device, no kernel."""
import numpy as np
import pytest
import torch

import sample_edges as E
from sample_plan import VS

# V -> draws with more than one accepted token (five-point rule, the vocabulary's own rule); every V not named: (0, 0)
MAIN = {131072: (1, 1), 262144: (1, 1), 262145: (1, 1)}
PENALISED = {65536: (1, 1), 131072: (1, 1), 262144: (1, 1)}


def _cap(n):
    return max(2, n // 1000)


@pytest.mark.parametrize("V", VS)
def test_reference_alone_stays_inside_the_cap(V):
    five = own = n = 0
    for name in ("fp16", "fp32"):
        accs = E.reference(V, name)
        f, o, d = E.ambiguous(accs)
        five, own, n = five + f, own + o, n + d
        for a in accs:
            assert bool(a.ok(a.nominal).all()) and bool(((a.lo <= a.nominal) & (a.nominal <= a.hi)).all())
            assert a.wide == (V > 65536)
    assert n == 2 * 6 * E.batch(V)
    assert (five, own) == MAIN.get(V, (0, 0)) and own <= _cap(n)


@pytest.mark.parametrize("V", VS)
def test_penalised_reference_alone_stays_inside_the_cap(V):
    x, accs = E.pen_reference(V)
    assert x.dtype == torch.float32 and bool(torch.isfinite(x.max(-1).values).all())
    five, own, n = E.ambiguous(accs)
    assert n == 6 * E.batch(V)
    assert (five, own) == PENALISED.get(V, (0, 0)) and own <= _cap(n)


def test_rows_hold_what_the_edges_need():
    for V in (65, 1025, 65537):
        r = E.rows(V)
        assert r["fp16"].dtype == torch.float16 and r["fp32"].dtype == torch.float32
        for x in r.values():
            assert x.shape == (4, V) and bool(torch.isinf(x[0, V - V // 5:]).all()) and bool(torch.isfinite(x[0, : V - V // 5]).all())
            assert bool(torch.isinf(x).any(1).all()) and bool(torch.isfinite(x).any(1).all())
        assert len(r["fp16"][0].unique()) < len(r["fp16"][1].unique()) or V < 100      # the coarse row: large tie classes
        lg, w = E.history(V)
        top = lg.float().topk(8, -1).indices[:, :4]
        assert w.gather(1, top).tolist() == [[1, E.PROMPT, E.PROMPT | 5, 32767]] * 4


def test_five_point_rule_is_that_of_test_sample_gpu():
    """accepted().five restates tests/test_sample_gpu.py's _accepted with the kept sets shared between the probe points."""
    from kivi_amd.sampling import draw_u, reference_sample
    V = 1025
    lg = E.rows(V)["fp16"]
    u = draw_u(5, np.arange(4), 3)
    for t, k, p, mp in E.grid(V):
        runs = [(u, p, mp), (u, p * (1 - E.EPS), mp), (u, min(1.0, p * (1 + E.EPS)), mp), (np.clip(u - E.EPS, 0, None), p, mp),
                (np.minimum(u + E.EPS, 1 - 2 ** -24), p, mp)]
        if mp:
            runs += [(u, p, mp * (1 - E.EPS)), (u, p, mp * (1 + E.EPS))]
        want = torch.stack([reference_sample(lg, uu, t, k, pp, mm) for uu, pp, mm in runs], 1)
        assert torch.equal(E.accepted(lg, u, t, k, p, mp).five, want)
