"""The lead patterns that follow the walk (tests/longpad_masks.py: leadwalk_mask) checked WITHOUT a GPU, before
tests/test_decode_lead_long_gpu.py relies on them:

1. Inputs mean what they say: a Python restatement of kivi_lead_k_wave / kivi_lead_v_wave (kivi_amd/csrc/kivi_lead_plan.h), and for the
   (Tq, Tv, waves per row) of every GPU shape at every step it runs -- some row has a wave that starts at a shifted super-block, walks
   at least two and ends on the partial last one; some row skips a whole round of the deal; some row's V range starts off a super-block
   boundary; row 8 leaves one wave with K work; the rows 2-8 reach different (first live super-block, first live V block).
   Rows 4 and 5 (512 nw and 512 nw + 1) cannot differ there -- both numbers are floors of p -- they differ in the mask at key 512 nw
   (live in row 4, dead in row 5: the straddle), which is what is asserted for them.
2. The mask's layout, key by key.
3. Patterns through the fp64 reference (tests/torch_ref64.py: decode_step on the CPU) at two of the shapes with few heads, every step:
   the reference finite, no row fully masked, row 11 left with exactly one live key, the dead keys exactly the keys under the lead and
   within 32 of the clamp, one K flush on the way."""
import pytest
import torch

import torch_ref64 as T64
from helpers import make_kv
from longpad_masks import FMIN, ROWS, SB, assert_leadwalk, leadwalk_mask, leadwalk_pads

# (Tq, Tv) before the first step, R, waves per row: the shapes of tests/test_decode_lead_long_gpu.py (T0 = Tv + R, T0 % R = R - 2)
WALKS = {"row_deep_2b": (5214, 32, 8), "row_deep_4b": (5214, 32, 8), "row_nw8_2b": (5214, 32, 8), "row_nw8_4b": (5214, 32, 8),
         "row_nw4_2b": (4510, 32, 4), "row_nw4_4b": (4510, 32, 4), "row4_r4_2b": (4478, 128, 4), "row4_r4_4b": (4510, 32, 4),
         "row4_r8_2b": (4062, 32, 4), "row4_three_2b": (4510, 32, 4)}
STEPS = 5


# ---- kivi_lead_plan.h, restated
def k_first(lead, Tq):
    p = min(max(lead, 0), Tq)
    return -(-Tq // SB) if p >= Tq else p // SB


def v_first(lead, Tv):
    p = min(max(lead, 0), Tv)
    return -(-Tv // 32) if p >= Tv else p // 32


def k_wave(sb_lo, nsb, Tq, wave, nw):
    """(sb_first, n_sb, ng_total) of kivi_lead_k_wave."""
    first = sb_lo + wave
    n_sb = (nsb - first + nw - 1) // nw if nsb > first else 0
    left = Tq // 32 - 16 * (first + (n_sb - 1) * nw)
    return first, n_sb, (16 * (n_sb - 1) + min(left, 16)) if n_sb > 0 else 0


def v_wave(vb_lo, vb_hi, wave, nw):
    """[b_lo, b_hi) of kivi_lead_v_wave."""
    nb = max(vb_hi - vb_lo, 0)
    base, rem = divmod(nb, nw)
    lo = vb_lo + wave * base + min(wave, rem)
    return lo, lo + base + (1 if wave < rem else 0)


def _lengths_at(T0, R, s):
    """(n, Tq, Tv) of step s of a run that starts with T0 cached keys: the reference's bookkeeping (K flushed when the residual is full,
    one token leaving the V window per step)."""
    kv = T0 + s
    return kv + 1, (kv // R) * R, kv - R


def test_the_restatement_covers_a_row_exactly_once():
    """The ten lines above against what they restate: every super-block (and every group of it) from the first live one on is walked by
    exactly one wave, the V runs tile [first live block, ceil(Tv / 32)) in wave order."""
    for Tq, Tv, nw in ((4352, 4350, 4), (4480, 4478, 4), (5184, 5182, 8), (5216, 5186, 8), (1088, 1070, 4)):
        nsb, nb = -(-Tq // SB), -(-Tv // 32)
        for lead in (0, 33, 512, 2047, 2048, 4095, 4097, Tq - 1, Tq, Tq + 5):
            k0, seen, groups = k_first(lead, Tq), [], 0
            for w in range(nw):
                first, n_sb, ng = k_wave(k0, nsb, Tq, w, nw)
                seen += [first + i * nw for i in range(n_sb)]
                groups += ng
            assert sorted(seen) == list(range(k0, nsb)) and groups == max(Tq // 32 - 16 * k0, 0)
            v0, at = v_first(lead, Tv), None
            for w in range(nw):
                lo, hi = v_wave(v0, nb, w, nw)
                assert lo == (v0 if at is None else at) and hi >= lo
                at = hi
            assert at == max(nb, v0) == nb


@pytest.mark.parametrize("name", list(WALKS))
def test_inputs_mean_what_they_say(name):
    T0, R, nw = WALKS[name]
    assert T0 % R == R - 2 and (R - T0 % R) + 3 == STEPS
    for s in range(STEPS):
        n, Tq, Tv = _lengths_at(T0, R, s)
        nsb, nb = -(-Tq // SB), -(-Tv // 32)
        assert Tq % SB != 0, "the last super-block is partial"
        # two super-blocks per wave behind a lead AND a whole round skipped: nsb >= 2 nw + 1 (nw = 4), nw + 3 (nw = 8) -- but for
        # nh / nh_kv = 8, whose block per row holds 8 super-blocks at the most (the plan's cap, 4608 keys, is on 512 nsb + R): nsb = 2 nw,
        # where 512 (nsb - nw) = 512 nw and pattern row 7 is row 4 again; everything asserted below is still reached
        tight = nsb == 2 * nw
        assert tight == (name == "row4_r8_2b") and (tight or nsb >= (2 * nw + 1 if nw == 4 else nw + 3))
        lead = leadwalk_pads(n, Tq, Tv, nw)
        starts = [(k_first(p, Tq), v_first(p, Tv)) for p in lead]
        walks = [[k_wave(k0, nsb, Tq, w, nw) for w in range(nw)] for k0, _ in starts]
        # a wave that starts at a shifted super-block, walks two or more, and ends on the partial last one
        assert any(k0 >= 1 and n_sb >= 2 and first + (n_sb - 1) * nw == nsb - 1 and ng < 16 * n_sb
                   for (k0, _), row in zip(starts, walks) for first, n_sb, ng in row), (name, s)
        assert any(k0 >= nw and k0 < nsb for k0, _ in starts), (name, s, "a whole round of the deal skipped")
        assert any(v0 % 16 and v0 < nb for _, v0 in starts), (name, s, "a V range that starts inside a super-block")
        assert any(v_wave(v0, nb, w, nw)[0] % 16 for _, v0 in starts for w in range(nw))
        # row 0: the plain deal; row 6: nw + 1 live super-blocks, V three blocks before a boundary; row 7: one per wave; row 8: wave 0 alone
        assert starts[0] == (0, 0) and starts[1] == (0, 1)
        assert nsb - starts[6][0] == nw + 1 and starts[6][1] % 16 == 13 and walks[6][0][1] == 2
        assert nsb - starts[7][0] == nw and all(n_sb == 1 for _, n_sb, _ in walks[7]) and walks[7][nw - 1][2] < 16
        assert [n_sb for _, n_sb, _ in walks[8]] == [1] + [0] * (nw - 1) and 0 < walks[8][0][2] < 16
        assert starts[9][0] == nsb and starts[9][1] == (nb if Tq >= Tv else Tq // 32)
        assert starts[10] == (nsb, nb) and starts[11] == (nsb, nb) and lead[11] == n - 1
        # rows 2-8 reach different units -- but for rows 4 and 5, whose units are the same by arithmetic and whose masks differ
        for skip in (4, 5):
            some = [starts[b] for b in range(2, 9) if b != skip and not (tight and b == 7)]
            assert len(set(some)) == len(some), (name, s, starts)
        assert starts[4] == starts[5] and lead[5] == lead[4] + 1 == SB * nw + 1 and (not tight or lead[7] == lead[4])
        assert len(set(lead[:10])) == (9 if tight else 10), "different leads (rows 10 and 11 meet row 9 at n - 1 on the step after the flush)"


def test_mask_layout():
    for n, Tq, Tv, nw in ((5215, 5184, 5182, 8), (4512, 4480, 4479, 4), (4481, 4480, 4352, 4)):
        m, lead = leadwalk_mask(n, Tq, Tv, nw, "cpu")
        assert m.shape == (ROWS, 1, 1, n) and m.dtype == torch.float16 and lead.shape == (ROWS,) and lead.dtype == torch.int32
        m = m[:, 0, 0]
        dead = m == FMIN
        assert bool(((m == 0) | dead).all()) and bool((m[:, n - 1] == 0).all()), "the new token is live in every row"
        nsb = -(-Tq // SB)
        want = [0, 33, 512, 512 * nw - 1, 512 * nw, 512 * nw + 1, 512 * (nsb - nw) - 96, 512 * (nsb - nw), 512 * (nsb - 1), Tq,
                max(Tq, Tv) + 1, n - 1]
        assert lead.tolist() == [min(p, n - 1) for p in want] == leadwalk_pads(n, Tq, Tv, nw)
        for b in range(ROWS):
            assert int(dead[b].sum()) == lead[b] and bool(dead[b, : lead[b]].all()), "a pad is one run from key 0"


@pytest.mark.parametrize("nh,nh_kv,T0,R,kind,bits,nw", [(4, 4, 5214, 32, "randn", 2, 8), (8, 2, 4478, 128, "outlier", 2, 4)])
def test_patterns_through_the_reference(nh, nh_kv, T0, R, kind, bits, nw):
    B, D, g = ROWS, 128, 32
    fpi = 32 // bits
    past = T64.prefill_cache(make_kv(1, B, nh_kv, T0, D, kind), make_kv(2, B, nh_kv, T0, D), bits, bits, g, R)
    flushes = 0
    for s in range(STEPS):
        q, kn, vn = make_kv(100 + s, B, nh, 1, D), make_kv(200 + s, B, nh_kv, 1, D, kind), make_kv(300 + s, B, nh_kv, 1, D)
        n = T0 + s + 1
        Tq, Tv = past[0].shape[-1] * fpi, past[4].shape[2]
        assert (n, Tq, Tv) == _lengths_at(T0, R, s)
        mask, lead = leadwalk_mask(n, Tq, Tv, nw, "cpu")
        ref, new_past, pre = T64.decode_step(q, kn, vn, past, bits, bits, g, R, attention_mask=mask)
        count = assert_leadwalk(pre, ref, lead, what=(s, n))
        assert bool((count == (n - lead.long())[:, None]).all()) and bool((count[0] == n).all()) and bool((count[11] == 1).all())
        flushes += new_past[0].shape[-1] * fpi > Tq
        past = new_past
    assert flushes == 1 and past[1] is not None and past[1].shape[2] == 3, "the run crosses exactly one K flush and three steps more"
