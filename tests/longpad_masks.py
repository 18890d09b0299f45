"""Long left pads at decode time: the additive masks of tests/test_longpad_cpu.py and tests/test_longpad_gpu.py.

A short prompt admitted into a living cache of length L (continuous batching) is left-padded to L: its row's
first L - len(prompt) keys are masked at the fp16 minimum at every later decode step.  With L in the thousands the mask covers whole
512-token super-blocks, whole slices of the sliced one-launch form and often the entire packed K and V stores.  One pattern per
batch row; every pad stops before the new token (HF never masks the token it feeds), so no row is fully masked.

leadwalk_mask: the leads of tests/test_decode_lead_long_cpu.py and tests/test_decode_lead_long_gpu.py -- pads
placed by the walk of a row kernel that skips them, on rows long enough for a wave to walk two super-blocks behind a lead."""
import torch

FMIN = torch.finfo(torch.float16).min
SB = 512          # tokens per super-block of the matrix-pipe layout (kivi_amd/csrc/kivi_mfma_layout.h)
ROWS = 12


def longpad_mask(n, Tq, Tv, device, rows=None):
    """(B, 1, 1, n) fp16 additive mask of a decode step over n keys (the new token is key n - 1), B = 12 or len(rows).  Tq / Tv: the
    packed K / V lengths BEFORE the step, read off the reference 9-tuple (past[0].shape[-1] * fpi, past[4].shape[2]) -- never off the
    layer under test.  A pad of p keys is mask[b, ..., :min(p, n - 1)] = finfo(fp16).min.
      row 0        no mask (control)
      rows 1 2 3   p = 512, 513, 511: a whole super-block, one key over, one key short
      row 4        p = (Tq // 512) * 512: every whole K super-block
      row 5        p = Tq: the whole packed K; the fp16 residual and the new token are live
      row 6        p = max(Tq, Tv) + 1: both packed stores and a key more
      row 7        p = n - 2: the last cached key and the new token are live
      row 8        p = n - 1: only the new token
      row 9        p = 700, and -3.0 added at keys 800, 900 and n - 2
      row 10       no pad; a hole [512, 1024) at the minimum: a whole middle super-block (a whole slice of a sliced row)
      row 11       [512, n - 1) at the minimum: the first super-block and the new token are live
    `rows`: keep these pattern rows only, in this order (shapes that need few units)."""
    m = torch.zeros((ROWS, 1, 1, n), dtype=torch.float16)
    pads = {1: SB, 2: SB + 1, 3: SB - 1, 4: (Tq // SB) * SB, 5: Tq, 6: max(Tq, Tv) + 1, 7: n - 2, 8: n - 1, 9: 700}
    for b, p in pads.items():
        m[b, ..., : max(0, min(p, n - 1))] = FMIN
    for k in (800, 900, n - 2):
        if 0 <= k < n:
            m[9, ..., k] += -3.0
    m[10, ..., SB: min(2 * SB, n - 1)] = FMIN
    m[11, ..., SB: n - 1] = FMIN
    if rows is not None:
        m = m[list(rows)].contiguous()
    return m.to(device)


def leadwalk_pads(n, Tq, Tv, nw):
    """The twelve pads of leadwalk_mask, clamped to n - 1."""
    nsb = -(-Tq // SB)
    p = [0, 33, SB, SB * nw - 1, SB * nw, SB * nw + 1, SB * (nsb - nw) - 96, SB * (nsb - nw), SB * (nsb - 1), Tq, max(Tq, Tv) + 1, n - 1]
    return [max(0, min(x, n - 1)) for x in p]


def leadwalk_mask(n, Tq, Tv, nw, device):
    """Leading pads that follow the walk of a row kernel under a lead (kivi_amd/csrc/kivi_lead_plan.h) on rows of
    many super-blocks: (mask, lead), mask (12, 1, 1, n) fp16 with the fp16 minimum at keys [0, lead[b]) of row b, lead (12,) int32 =
    min(p, n - 1).  Tq / Tv as in longpad_mask, nsb = ceil(Tq / 512), nw the waves per row of the kernel under test (the packed K
    super-blocks from the first live one on are dealt round-robin to nw waves, the live 32-token V blocks in nw contiguous runs).
      row 0        p = 0: the lead form with nothing to skip -- the deal must equal the plain one
      row 1        p = 33: K nothing skipped; V first live block 1: every wave's run shifts by one block
      row 2        p = 512: first live super-block 1; waves walk two super-blocks, for one of them the second is the partial last
      rows 3 4 5   p = 512 nw - 1, 512 nw, 512 nw + 1: a whole round of the deal skipped, and the straddle either side of it
      row 6        p = 512 (nsb - nw) - 96: nw + 1 live super-blocks -- wave 0 walks the straddled one and the partial last; V starts
                   three blocks before a super-block boundary
      row 7        p = 512 (nsb - nw): exactly nw live, one per wave, the last wave on the partial one
      row 8        p = 512 (nsb - 1): only the partial last super-block, on wave 0 alone
      row 9        p = Tq: no packed K; V live where Tv > clamp
      row 10       p = max(Tq, Tv) + 1: both packed stores skipped whole
      row 11       p = n - 1: only the new token"""
    lead = leadwalk_pads(n, Tq, Tv, nw)
    m = torch.zeros((ROWS, 1, 1, n), dtype=torch.float16)
    for b, p in enumerate(lead):
        m[b, ..., :p] = FMIN
    return m.to(device), torch.tensor(lead, dtype=torch.int32, device=device)


def assert_leadwalk(pre, out, lead, what=""):
    """leadwalk_mask's patterns read off the REFERENCE's step (as assert_patterns): finite, no row fully masked, the keys under a row's
    lead -- and only those -- dead and within 32 of the clamp, row 11 left with exactly one live key.  Returns the (B, nh) live counts.
    (A dead key is fp16(score - 65504): a score of 48 or more would land it on -65440, off what a kernel that skips the key can write.)"""
    x = pre.detach().float().cpu()[:, :, 0]
    n = x.shape[-1]
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out.detach().float()).all()), (what, "the reference is not finite")
    live = x > -60000
    count = live.sum(-1)
    assert bool((count >= 1).all()), (what, "a fully masked row")
    dead = x[~live]
    assert bool(((dead >= -65504) & (dead <= -65472)).all()), (what, "a dead key off the clamp", dead.min().item(), dead.max().item())
    under = torch.arange(n)[None] < torch.as_tensor(lead).cpu().long()[:, None]
    assert torch.equal(live, (~under)[:, None, :].expand_as(live)), (what, "the dead keys are not the keys under the lead")
    assert bool((count[11] == 1).all()) and bool(live[11, :, n - 1].all()), (what, "row 11", count[11])
    return count


def assert_patterns(pre, out, Tq, rows=None, what=""):
    """The patterns still mean what they say, read off the REFERENCE's step (tests/torch_ref64.py: decode_step under longpad_mask):
    `pre` (B, nh, 1, n) the fp16 rows fed to its softmax, `out` its output, Tq the packed K length before the step.  Returns the
    (B, nh) counts of live keys."""
    rows = list(range(ROWS)) if rows is None else list(rows)
    x = pre.detach().float().cpu()[:, :, 0]
    n = x.shape[-1]
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out.detach().float()).all()), (what, "the reference is not finite")
    live = x > -60000
    count = live.sum(-1)
    assert bool((count >= 1).all()), (what, "a fully masked row")
    dead = x[~live]
    assert bool(((dead >= -65504) & (dead <= -65472)).all()), (what, "a dead key off the clamp", dead.min().item(), dead.max().item())
    first = {p: live[i].any(0).nonzero().min().item() for i, p in enumerate(rows)}       # first live key of each pattern row, any head
    for i, p in enumerate(rows):
        if p == 0:
            assert bool(live[i].all()), (what, "control row")
        if p == 7:
            assert bool((count[i] == 2).all()) and first[p] == n - 2, (what, "row 7", count[i])
        if p == 8:
            assert bool((count[i] == 1).all()) and first[p] == n - 1, (what, "row 8", count[i])
        if p in (4, 5, 6):
            assert first[p] >= min((Tq // SB) * SB, n - 1), (what, "row", p, "live below the whole K super-blocks", first[p])
        if p == 10:
            assert not bool(live[i][:, SB: min(2 * SB, n - 1)].any()) and bool(live[i][:, :SB].all()), (what, "row 10")
        if p == 11:
            assert bool((count[i] == SB + 1).all()), (what, "row 11", count[i])
    return count
