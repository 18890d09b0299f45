"""The long-left-pad mask patterns (tests/longpad_masks.py) through the fp64 reference on the CPU (tests/torch_ref64.py: decode_step),
at two of the shapes of tests/test_longpad_gpu.py and every step they run: the patterns must keep meaning what they say -- the
reference finite, no row fully masked, the rows that leave one or two keys leaving exactly those, no live key under a pad that covers
the whole K super-blocks, dead keys on the clamp -- or the GPU tests would silently test something else."""
import pytest
import torch

import torch_ref64 as T64
from helpers import make_kv
from longpad_masks import FMIN, ROWS, assert_patterns, longpad_mask


def test_mask_layout():
    """The table of the helper's docstring, key by key, at a step right after a K flush (Tq = n - 1 > Tv) and in the middle of a
    residual; the row subset; the clamp that keeps the new token live."""
    for n, Tq, Tv in ((1121, 1120, 1088), (1105, 1088, 1072), (2103, 2080, 2070)):
        m = longpad_mask(n, Tq, Tv, "cpu")
        assert m.shape == (ROWS, 1, 1, n) and m.dtype == torch.float16
        m = m[:, 0, 0]
        dead = m == FMIN
        assert bool((m[:, n - 1] == 0).all()), "the new token is live in every row"
        lead = [int(dead[b].int().cumprod(0).sum()) for b in range(ROWS)]        # length of the leading pad
        assert lead == [0, 512, 513, 511, (Tq // 512) * 512, Tq, min(max(Tq, Tv) + 1, n - 1), n - 2, n - 1, 700, 0, 0]
        for b in range(9):
            assert int(dead[b].sum()) == lead[b], "a pad is one run from key 0"
        assert m[9, 800] == -3.0 and m[9, 900] == -3.0 and m[9, n - 2] == -3.0 and int((m[9] != 0).sum()) == 703
        assert bool(dead[10, 512:1024].all()) and int(dead[10].sum()) == 512
        assert bool(dead[11, 512: n - 1].all()) and int(dead[11].sum()) == n - 1 - 512
        sub = longpad_mask(n, Tq, Tv, "cpu", rows=[0, 4, 8])
        assert sub.shape == (3, 1, 1, n) and torch.equal(sub[:, 0, 0], m[[0, 4, 8]])


@pytest.mark.parametrize("nh,nh_kv,T0,R,kind,bits,steps", [(8, 2, 1100, 128, "outlier", 2, 55), (4, 4, 1100, 32, "randn", 2, 23)])
def test_patterns_through_the_reference(nh, nh_kv, T0, R, kind, bits, steps):
    """Every step of two GPU shapes (one K flush each: at step 52 of 55 and at step 20 of 23).  Without the n - 1 clamp of the pads row
    6 would be fully masked on the step after the flush (Tq = n - 1 there); with "outlier" keys dead scores land on -65472 as well as
    on -65504, so dead keys are held to a window of 32, not to the minimum itself."""
    B, D, g = ROWS, 128, 32
    fpi = 32 // bits
    k0, v0 = make_kv(1, B, nh_kv, T0, D, kind), make_kv(2, B, nh_kv, T0, D)
    past = T64.prefill_cache(k0, v0, bits, bits, g, R)
    flushed = False
    for s in range(steps):
        q, kn, vn = make_kv(100 + s, B, nh, 1, D), make_kv(200 + s, B, nh_kv, 1, D, kind), make_kv(300 + s, B, nh_kv, 1, D)
        n = T0 + s + 1
        Tq, Tv = past[0].shape[-1] * fpi, past[4].shape[2]
        assert Tq >= 1024, "two whole K super-blocks under the pads"
        mask = longpad_mask(n, Tq, Tv, "cpu")
        ref, new_past, pre = T64.decode_step(q, kn, vn, past, bits, bits, g, R, attention_mask=mask)
        count = assert_patterns(pre, ref, Tq, what=(s, n))
        assert bool((count[5] == n - Tq).all()) and bool((count[0] == n).all())
        flushed |= new_past[0].shape[-1] * fpi > Tq
        if Tq == n - 1:                      # the step after the flush: the packed K is the whole cache
            assert bool((count[5] == 1).all()) and bool((count[6] == 1).all())
        past = new_past
    assert flushed and past[1] is not None and past[1].shape[2] == 3, "the run crosses one K flush and three steps more"
