"""The fp64 side of tests/test_sample_edges_gpu.py, shared with tests/test_sample_edges_cpu.py: general rows at every vocabulary of
tests/sample_plan.py, the parameter grid of tests/test_sample_gpu.py's large-vocabulary test, and which tokens a correct kernel may
return for a draw.  CPU only; nothing here touches a device.

The kernel carries fp32 scores and integer weights, the reference fp64, so a decision that lies within EPS = 1e-5 of its boundary
may fall either way.  Two rules say what that allows:
- five points (V <= 65536, the rule of tests/test_sample_gpu.py): the reference's token with one boundary moved by EPS -- top_p
  down / up, u down / up, min_p down / up -- or none;
- wide (V > 65536): with ~1e5 kept tokens an interval of 2 EPS of the kept mass holds several tokens, and three probe points step
  over some of them.  A token is accepted when it is kept under one of the EPS-shifted parameter sets and lies, in vocabulary
  order, between the lowest reference token at u - EPS and the highest at u + EPS over those sets.
`kept` is computed once per shifted parameter set and only u varies, which keeps V = 2^20 to a few seconds."""
import functools
from typing import NamedTuple

import numpy as np
import torch

from sample_plan import MAX_V

EPS = 1e-5
WIDE_ABOVE = 65536
PENS = [(0.5, -0.7, 0.0), (1.3, 0.6, 0.25), (1.3, -0.7, 0.25), (0.5, 0.6, 0.0)]      # (repetition, presence, frequency) per row
PEN_SEEDS, PEN_STREAMS = [31, 32, 33, 2 ** 64 - 34], [0, 3, 9, 2 ** 32 - 1]
PROMPT, COUNT = 0x8000, 0x7FFF
SEEDS = {"fp16": 21, "fp32": 22}


def batch(V):
    """Rows per test: the fp64 reference sorts every row five to seven times per grid entry."""
    return 4 if V <= 151936 else 2 if V < MAX_V else 1


def grid(V):
    return [(1.0, 50, 1.0, None), (0.7, 50, 0.9, None), (1.0, 0, 0.9, None), (1.3, 0, 0.5, 0.05), (1.0, 1, 1.0, None),
            (0.8, V + 5, 0.9, 0.05)]


def _stretches(x, V):
    """-inf stretches: the row's tail on row 0, its head, its middle, a comb -- never a whole row."""
    B = x.shape[0]
    if V // 5:
        x[0, V - V // 5:] = -float("inf")
    if B > 1:
        x[1, : V // 7] = -float("inf")
    if B > 2:
        x[2, V // 3: V // 3 + V // 4] = -float("inf")
    if B > 3 and V > 1:
        x[3, V // 2 + 1:: 7] = -float("inf")
    return x


@functools.lru_cache(maxsize=4)
def rows(V):
    """-> {"fp16": (B, V) fp16, row 0 coarse (large tie classes); "fp32": (B, V) fp32}, on the CPU."""
    B = batch(V)
    g = torch.Generator().manual_seed(V)
    lg16 = (torch.randn((B, V), generator=g) * 3).half()
    lg16[0] = (lg16[0].float() * 2).round().half() / 2
    lg32 = torch.randn((B, V), generator=g) * 4
    return {"fp16": _stretches(lg16, V), "fp32": _stretches(lg32, V)}


class Accepted(NamedTuple):
    nominal: torch.Tensor                # (B,) the reference's token at the nominal parameters and u
    five: torch.Tensor                   # (B, 5 or 7) the five-point rule's tokens
    union: torch.Tensor                  # (B, V) bool: kept under some shifted parameter set
    lo: torch.Tensor                     # (B,) the wide rule's range, inclusive
    hi: torch.Tensor
    wide: bool

    def ok(self, tok):
        """(B,) bool: the rule of this vocabulary accepts tok (B,)."""
        tok = tok.view(-1).cpu()
        if not self.wide:
            return (self.five == tok[:, None]).any(1)
        return self.union.gather(1, tok[:, None])[:, 0] & (self.lo <= tok) & (tok <= self.hi)

    def five_sizes(self):
        return torch.tensor([len(set(r.tolist())) for r in self.five])

    def sizes(self):
        """(B,) how many tokens the rule accepts."""
        if not self.wide:
            return self.five_sizes()
        idx = torch.arange(self.union.shape[1])[None]
        return (self.union & (self.lo[:, None] <= idx) & (idx <= self.hi[:, None])).sum(1)


def accepted(logits, u, t, k, p, mp) -> Accepted:
    """What a correct kernel may return for rows `logits` (B, V) at u (B,) under (temperature, top_k, top_p, min_p)."""
    from kivi_amd.sampling import reference_kept
    V = logits.shape[1]
    u = np.asarray(u, dtype=np.float64)
    ulo, uhi = np.clip(u - EPS, 0, None), np.minimum(u + EPS, 1 - 2 ** -24)
    sets = [(p, mp), (p * (1 - EPS), mp), (min(1.0, p * (1 + EPS)), mp)]
    if mp:
        sets += [(p, mp * (1 - EPS)), (p, mp * (1 + EPS))]
    keeps, cums, done = [], [], {}
    for pp, mm in sets:
        if (pp, mm) not in done:                     # (top_p = 1 moved up is top_p = 1 again)
            keep, e = reference_kept(logits, t, k, pp, mm)
            done[(pp, mm)] = (keep, torch.where(keep, e, torch.zeros_like(e)).cumsum(-1))
        keeps.append(done[(pp, mm)][0])
        cums.append(done[(pp, mm)][1])

    def token(cum, uu):                              # reference_sample's draw
        uu = torch.as_tensor(uu).reshape(-1, 1)
        return (cum <= uu * cum[:, -1:]).sum(-1).clamp(max=V - 1)

    at_u = [token(c, u) for c in cums]
    below, above = [token(c, ulo) for c in cums], [token(c, uhi) for c in cums]
    five = torch.stack(at_u[:3] + [below[0], above[0]] + at_u[3:], 1)
    union = functools.reduce(torch.logical_or, keeps)
    return Accepted(at_u[0], five, union, torch.stack(below).min(0).values, torch.stack(above).max(0).values, V > WIDE_ABOVE)


@functools.lru_cache(maxsize=8)
def reference(V, name):
    """The Accepted of every grid entry for rows(V)[name] at the u of Sampler(seed=SEEDS[name]), draw 0."""
    from kivi_amd.sampling import draw_u
    lg = rows(V)[name]
    u = draw_u(SEEDS[name], np.arange(lg.shape[0]), 0)
    return [accepted(lg, u, *entry) for entry in grid(V)]


# ------------------------------------------------------------------ penalised rows
@functools.lru_cache(maxsize=2)
def history(V):
    """-> (fp16 logits (B, V), history words (B, V) int64): prompt bits on 30 %, counts 0 / 1 / 5 / 32767, the eight largest logits
    of every row marked, so the candidates of every filter carry history."""
    lg = rows(V)["fp16"]
    B = lg.shape[0]
    g = torch.Generator().manual_seed(V + 7)
    w = torch.tensor([0, 0, 0, 1, 5, 32767])[torch.randint(0, 6, (B, V), generator=g)]
    w = w | (torch.rand((B, V), generator=g) < 0.3).long() * PROMPT
    top = lg.float().topk(min(8, V), -1).indices
    for j, word in enumerate([1, PROMPT, PROMPT | 5, 32767, 0, 2, PROMPT, 1][: top.shape[1]]):
        w.scatter_(1, top[:, j: j + 1], torch.full((B, 1), word))
    return lg, w


@functools.lru_cache(maxsize=2)
def pen_reference(V):
    """reference_penalise over history(V) with PENS per row, then the same acceptance: (penalised fp32 logits, [Accepted per grid
    entry]) at the u of RowSampler rows with PEN_SEEDS / PEN_STREAMS, draw 0."""
    from kivi_amd.sampling import draw_u_rows, reference_penalise
    lg, w = history(V)
    B = lg.shape[0]
    x = reference_penalise(lg, (w & PROMPT) != 0, w & COUNT, *[[pen[i] for pen in PENS[:B]] for i in range(3)])
    u = draw_u_rows(PEN_SEEDS[:B], PEN_STREAMS[:B], [0] * B)
    return x, [accepted(x, u, *entry) for entry in grid(V)]


def ambiguous(accs):
    """(draws whose five-point set holds more than one token, draws whose set under the vocabulary's own rule does, draws)."""
    five = sum(int((a.five_sizes() > 1).sum()) for a in accs)
    own = sum(int((a.sizes() > 1).sum()) for a in accs)
    return five, own, sum(len(a.nominal) for a in accs)
