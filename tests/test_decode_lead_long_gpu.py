"""GPU: the lead-aware row kernels on LONG rows, every instantiation, against the fp64 reference.

tests/test_decode_lead_gpu.py runs every lead at three super-blocks, where each wave of a row walks at most one.  Here a row holds 8, 9 or
11 super-blocks, the last one partial, so that behind a lead a wave starts at a shifted super-block and walks a second one (the partial
last among them), a whole round of the deal is skipped, and the V stream is primed in the middle of a super-block: the twelve patterns of
longpad_masks.leadwalk_mask, checked against the reference alone in tests/test_decode_lead_long_cpu.py.

1. Stages (test_decode_lead_gpu.lead_stages, the same loop and bars: stage A 1e-3 + 1 ulp, stage B 2e-3 + 1 ulp, against the mask alone
   1.5e-3 + 1 ulp, the 9-tuple and the product instantiation bit-identical) at the unit counts that select each of the ten lead
   instantiations -- the launch probe names the one that ran -- with, at every step, the control of the 1.5e-3 bar on these long rows
   (the two-launch form against the row form, both with the mask alone: two forms that shipped before the lead) and, at step 0, a clone
   whose whole K and V super-blocks under each lead hold NaNs: finite and bit-identical.
   T0 % R = R - 2: five steps, the K flush at step 1, three steps after it; every step flushes V.
   nh / nh_kv = 8 runs at 8 super-blocks (T0 = 4062), the most a block per row of that form holds: the launch plan sizes a block for its
   geometry class, 512 nsb + residual_length keys, against a cap of 4608, so 9 super-blocks take the two-launch form, which ignores the
   lead.  At nsb = 2 nw pattern rows 4 and 7 coincide; every property of the walk is still reached (tests/test_decode_lead_long_cpu.py).
   The many-unit shapes draw the prompt's (12, 4 heads) on the CPU and repeat them over the heads on the GPU, head h scaled by
   1 + h / 64: every unit is distinct, so a unit read at the wrong (batch row, kv head) is a wrong answer; the reference is built from the same tensors.
2. The replayed entry (kivi_mf_decode_layer_dyn_lead through MfStepDriver.enqueue, eagerly, the lengths device-resident, the lead buffer
   rewritten in place between steps) bit-identical to kivi_attention_decode(..., lead=) on a twin, both kernels."""
import pytest
import torch

from helpers import make_kv, same_bits
from longpad_masks import ROWS, assert_leadwalk, leadwalk_mask
from test_decode_lead_gpu import D, G32, _forced, lead_stages
from test_extend_gpu import _assert_same_state

pytestmark = pytest.mark.gpu


def _draw(seed, heads, T, kind="randn"):
    """make_kv on the GPU; the prompt's keys and values of more than 16 heads: (12, 4 heads) drawn, repeated over the heads, head h
    scaled by 1 + h / 64.  (The one-token inputs of a step are drawn whole: scaling the queries as well would square the growth of the
    scores, and a masked score of 48 or more leaves the reference's dead key above -65472, where no skipped slot can follow it.)"""
    if heads <= 16 or T == 1:
        return make_kv(seed, ROWS, heads, T, D, kind).cuda()
    assert heads % 4 == 0
    x = make_kv(seed, ROWS, 4, T, D, kind).cuda().repeat(1, heads // 4, 1, 1)
    scale = (1 + torch.arange(heads, device="cuda", dtype=torch.float32) / 64)[None, :, None, None]
    return (x.float() * scale).half()


def _three_blocks_kv_heads():
    """The smallest kv-head count whose 12 k units give the device three blocks per CU (256 CUs: 64)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return -(-3 * cus // ROWS)


ROW, ROW4 = "mf_row_kernel", "mf_row4_kernel"
# id: (nh, nh_kv, T0, R, bits, keys, waves per row, (kernel, template arguments: None = any))
SHAPES = {
    "row_deep_2b": (4, 4, 5214, 32, 2, "randn", 8, (ROW, (8, 8, 8, None, None, 2, 2, True))),
    "row_deep_4b": (4, 4, 5214, 32, 4, "outlier", 8, (ROW, (4, 4, 8, None, None, 2, 4, True))),
    "row_nw8_2b": (24, 24, 5214, 32, 2, "outlier", 8, (ROW, (2, 3, 8, None, None, 4, 2, True))),
    "row_nw8_4b": (24, 24, 5214, 32, 4, "randn", 8, (ROW, (2, 3, 8, None, None, 4, 4, True))),
    "row_nw4_2b": (48, 48, 4510, 32, 2, "randn", 4, (ROW, (2, 3, 4, None, None, 4, 2, True))),         # the headline's form
    "row_nw4_4b": (48, 48, 4510, 32, 4, "outlier", 4, (ROW, (2, 3, 4, None, None, 4, 4, True))),
    "row4_r4_2b": (8, 2, 4478, 128, 2, "outlier", 4, (ROW4, (4, 3, 4, None, True, 4, 2, 2, True, True))),
    "row4_r4_4b": (8, 2, 4510, 32, 4, "randn", 4, (ROW4, (4, 3, 4, None, True, 4, 4, 2, True, True))),
    "row4_r8_2b": (16, 2, 4062, 32, 2, "outlier", 4, (ROW4, (4, 2, 4, None, False, 8, 2, 2, True, True))),
    "row4_three_2b": (None, None, 4510, 32, 2, "randn", 4, (ROW4, (2, 2, 4, None, True, 4, 2, 3, True, True))),   # 4 k / k heads
}


def _shape(name):
    nh, nh_kv, T0, R, bits, kind, nw, expect = SHAPES[name]
    if nh is None:
        nh_kv = _three_blocks_kv_heads()
        nh = 4 * nh_kv
    assert T0 % R == R - 2
    return nh, nh_kv, T0, R, bits, kind, nw, expect


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_lead_instantiation_on_long_rows(name):
    nh, nh_kv, T0, R, bits, kind, nw, expect = _shape(name)

    def check(pre, ref, n, Tq, lead, s):
        assert_leadwalk(pre, ref, lead, what=(name, s))
    lead_stages(nh, nh_kv, T0, R, kind, bits, patterns=lambda n, Tq, Tv: leadwalk_mask(n, Tq, Tv, nw, "cuda"), check=check, draw=_draw,
                what=f"decode lead long {name}", split_control=True, poison=True, expect=expect)


@pytest.mark.parametrize("name", ["row_deep_2b", "row4_r4_2b"])
def test_replayed_entry_under_a_lead_bit_identical_to_eager(name):
    from kivi_amd import _lib
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    from kivi_amd.graph import MfStepDriver
    nh, nh_kv, T0, R, bits, kind, nw, _ = _shape(name)
    B, steps = ROWS, 5
    a = make_layer_cache(KiviConfig(bits, bits, G32, R), B, nh_kv, D, T0 + 8, "cuda", num_heads=nh)
    a.flags = _forced("row")
    a.prefill(_draw(1, nh_kv, T0, kind), _draw(2, nh_kv, T0))
    assert _lib.load().kivi_mf_launch_plan(B, nh, nh_kv, a.k_quant_len, a.k_res_len, R, a.flags, bits, 0) == 1
    b = a.clone()
    drv = MfStepDriver([b])
    pitch = ((T0 + steps + 8 + 7) // 8) * 8
    mask_buf = torch.zeros((B, 1, 1, pitch), dtype=torch.float16, device="cuda")
    lead_buf = torch.zeros((B,), dtype=torch.int32, device="cuda")
    out_b = torch.empty((B, nh, 1, D), dtype=torch.float16, device="cuda")
    seen = []
    for s in range(steps):
        q, kn, vn = _draw(100 + s, nh, 1), _draw(200 + s, nh_kv, 1, kind), _draw(300 + s, nh_kv, 1)
        n = T0 + s + 1
        mask, lead = leadwalk_mask(n, a.k_quant_len, a.v_quant_len, nw, "cuda")      # (the twin's lengths: pinned to the reference's in 1.)
        seen.append(lead.tolist())
        oa = kivi_attention_decode(q, kn, vn, a, attention_mask=mask, lead=lead)
        mask_buf.zero_()
        mask_buf[..., :n] = mask
        lead_buf.copy_(lead)                                                           # in place: what a replayed step reads
        drv.prepare()
        drv.enqueue(0, q, kn, vn, out_b, mask_buf, lead_buf)
        drv.finish()
        assert bool(torch.isfinite(oa).all()) and same_bits(oa, out_b), (name, s)
    assert len({tuple(x) for x in seen}) == steps, "the lead changes at every step"
    assert a.k_res_len == 3 and a.k_quant_len == (T0 // R + 1) * R, "the run crosses the K flush"
    _assert_same_state(a, b)
