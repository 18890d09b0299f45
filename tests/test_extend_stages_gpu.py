"""GPU: the multi-token extend stage by stage, on both cache layouts.

Matrix-pipe layout (mf_extend_kernel): the scores never leave the chip, so KIVI_GQA_DUMP_SCORES makes the kernel also write the fp16
row each chunk row's softmax consumes (include/kivi_hip.h, kivi_mf_extend_layer) and every extend is checked unit by unit
(`_extend_stages`):
  A. the dumped rows against the fp64 contract's rows (tests/test_extend_cpu.py: extend64) at the GEMV bar, 1e-3 + 1 ulp, over every
     key a row sees (keys masked at the fp16 minimum: within the 32-spacing that binade leaves);
  B. the output against extend64's attend half run ON THE DUMPED ROWS (scores_override) at 2e-3 + 1 ulp;
  E. the output against extend64 end to end (3e-3 + 1 ulp) -- asserted at the bar where tests/test_extend_gpu.py asserts it, elsewhere
     at the allowance of tools/fuzz_decode.py, per row: 3x the bar for scores below 4, doubling with every binade of the row's largest
     |score| above that (one fp16 ulp of a score moves its probability by that ulp, relative; the reference softmax's own sensitivity);
  the cache bit-identical to extend64's 9-tuple and, range words included, to Q decode steps on a clone; dump on and dump off give
  the same bits.
The edges of the kernel (empty K residual, no packed K, K flushes inside / at the end of the chunk, full and one-over 16-row tiles, a
ring that wraps more than once, nh_kv 1 / 8, B 1 / 5, growth across a super-block, rows of 130 key tiles, chained extends after decode
steps, masks on chunk keys) and the dynamic range of the hi / lo operand pair (magnitudes 1e-4 .. 3e4).

Hook-state layout (KiviLayerCache.extend, torch ops) at the shapes the matrix pipe refuses, against the same contract.
kivi_vt_pack_at directly: written tokens, untouched words, range words."""
import pytest
import torch

import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from test_extend_cpu import extend64
from test_extend_gpu import CASES, _assert_same_state, _kv
from test_mfma_gpu import _ranged

pytestmark = pytest.mark.gpu
D, G32 = 128, 32
FMIN = torch.finfo(torch.float16).min


def _visible(P0, Q):
    vis = torch.ones((Q, P0 + Q), dtype=torch.bool)
    vis[:, P0:] = ~torch.ones((Q, Q), dtype=torch.bool).triu(1)
    return vis


def _e2e_rows(out, ref, pre, vis):
    """Per row: (ratio against 3e-3 + 1 ulp -- gemv_close's bound --, the fuzz allowance of the row's largest visible |score|)."""
    g, r = out.detach().cpu().float(), ref.detach().cpu().float()
    rms = r.pow(2).mean(dim=-1, keepdim=True).sqrt()
    bound = 3e-3 * torch.maximum(r.abs(), rms)
    bound = torch.where(r.abs() < 2.0 ** -14, bound + 2.0 ** -24, bound)
    bound = bound + torch.finfo(torch.float16).eps * r.abs().clamp_min(2.0 ** -14)
    err = (g - r).abs()
    ratio = torch.where(g == r, torch.zeros_like(err), err / bound.clamp_min(2.0 ** -126)).amax(-1)
    s = pre.detach().cpu().float()
    smax = torch.where(vis & (s > -60000), s.abs(), torch.zeros_like(s)).amax(-1).clamp_min(1e-9)
    allow = 3.0 * torch.clamp(torch.exp2(torch.floor(torch.log2(smax)) - 10) / 2.0 ** -9, min=1.0)
    return ratio, allow


def _extend_stages(layer, past, q, kn, vn, bits, R, mask=None, e2e="allow", label=""):
    """One extend of `layer` (matrix-pipe layout; `past`: the reference 9-tuple of its state) checked unit by unit -- stages A, B, E
    and the cache as in the module docstring.  e2e == "bar": E at 3e-3 + 1 ulp; "allow": E per row at 3 x 2^max(0, e - 1) of it, e the
    binade of the row's largest |score| (e = 1 for scores in [2, 4)).  Returns (the output, extend64's 9-tuple, worst A / B / E ratios;
    E as a fraction of what was asserted)."""
    from kivi_amd.attention import kivi_attention_decode
    assert layer.layout == "mfma"
    B, nh, Q, _ = q.shape
    P0 = layer.kv_seq_len
    n = P0 + Q
    plain, steps = layer.clone(), layer.clone()
    dump = torch.full((B, nh, Q, n + 8), float("nan"), dtype=torch.float16, device="cuda")    # unwritten visible keys stay NaN
    out = layer.extend(q, kn, vn, mask, scores_dump=dump)
    out_plain = plain.extend(q, kn, vn, mask)
    assert same_bits(out, out_plain), "the score dump changes the output"
    _assert_same_state(layer, plain)
    assert torch.isfinite(out).all()
    ref, ref_past, pre = extend64(q, kn, vn, past, bits, bits, G32, R, mask, return_scores=True)
    assert torch.isfinite(ref.float()).all(), "test inputs must keep the reference finite"
    x, pre = dump[..., :n].cpu(), pre.cpu()
    vis = _visible(P0, Q).expand_as(x)
    assert not torch.isnan(x[vis]).any(), "a key the row sees was not dumped"
    assert bool(torch.isnan(x[~vis]).all()) and bool(torch.isnan(dump[..., n:]).all()), "the dump wrote a key the row does not see"
    # A: the rows the softmax consumed
    live = vis & (pre.float() > -60000)
    ok, ra = gemv_close(torch.where(live, x.float(), 0.0), torch.where(live, pre.float(), 0.0), rtol=1e-3, ulps=1)
    assert ok, (label, "stage A", ra)
    dead = vis & ~live                        # fp16(x + finfo.min) keeps x only to the 32-spacing of that binade
    assert bool((x.float()[dead] <= -60000).all()) and bool(((x.float() - pre.float()).abs()[dead] <= 32).all()), (label, "masked keys")
    # B: the attend half on the kernel's own rows
    ref_b, _ = extend64(q, kn, vn, past, bits, bits, G32, R, mask, scores_override=x.to(q.device))
    ok, rb = gemv_close(out, ref_b, rtol=2e-3, ulps=1)
    assert ok, (label, "stage B", rb)
    # E: end to end
    ok, re_ = gemv_close(out, ref, rtol=3e-3, ulps=1)
    if e2e == "bar":
        assert ok, (label, "end to end", re_)
        e = re_
    else:
        rows, allow = _e2e_rows(out, ref, pre, vis)
        e = (rows / allow).max().item()
        assert e <= 1.0, (label, "end to end", re_, "allowed", allow.flatten()[(rows / allow).flatten().argmax()].item())
    # the cache: the contract's 9-tuple, Q decode steps on a clone (range words too), the next step
    assert layer.kv_seq_len == n
    for a_, b_ in zip(layer.as_tuple()[:8], ref_past[:8]):
        assert (a_ is None and b_ is None) or same_bits(a_, b_), label
    for i in range(Q):
        m = None if mask is None else mask[:, :, i:i + 1, : P0 + i + 1]
        kivi_attention_decode(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], steps, attention_mask=m)
    _assert_same_state(layer, steps)
    print(f"{label}: stage A {ra:.3f} of 1e-3+1ulp, stage B {rb:.3f} of 2e-3+1ulp, end to end {re_:.3f} of 3e-3+1ulp"
          + ("" if e2e == "bar" else f" ({e:.3f} of the allowance)"))
    return out, ref_past, (ra, rb, e)


def _prefilled(bits, ratio, R, k0, v0, max_len=None):
    from kivi_amd.attention import KiviConfig, make_layer_cache
    B, nh_kv, T0, _ = k0.shape
    cfg = KiviConfig(bits, bits, G32, R)
    layer = make_layer_cache(cfg, B, nh_kv, D, T0 + 8 if max_len is None else max_len, "cuda", num_heads=nh_kv * ratio)
    assert layer.layout == "mfma"
    layer.prefill(k0.cuda(), v0.cuda())
    return layer, T64.prefill_cache(k0.cuda(), v0.cuda(), bits, bits, G32, R)


def _run(bits, ratio, R, T0, Q, kind="randn", B=2, nh_kv=2, e2e="allow", mask=None, max_len=None, label=""):
    k0, v0 = _kv(1, B, nh_kv, T0, kind), _kv(2, B, nh_kv, T0, kind)
    layer, past = _prefilled(bits, ratio, R, k0, v0, max_len)
    q = make_kv(10, B, nh_kv * ratio, Q, D).cuda()
    kn, vn = _kv(11, B, nh_kv, Q, kind).cuda(), _kv(12, B, nh_kv, Q, kind).cuda()
    return layer, _extend_stages(layer, past, q, kn, vn, bits, R, mask, e2e, label)


# ------------------------------------------------------------------ 1. the suite's cases and the three formerly open ones
@pytest.mark.parametrize("bits,ratio,R,T0,Q,kind", CASES)
def test_extend_stages_cases(bits, ratio, R, T0, Q, kind):
    _run(bits, ratio, R, T0, Q, kind, e2e="bar", label=f"case {bits} {ratio} {R} {T0} {Q} {kind}")


@pytest.mark.parametrize("bits,ratio,R,T0,Q,kind", [(4, 4, 128, 600, 5, "outlier"), (4, 4, 32, 90, 300, "x30")])
def test_extend_stages_formerly_open(bits, ratio, R, T0, Q, kind):
    """The two 4-bit nh / nh_kv = 4 cases that missed the end-to-end bar (1.003x and 2.11x): both stages hold, so the kernel computes
    what the contract computes from its own rows; the end-to-end difference is the reference softmax's sensitivity to one fp16 ulp of
    scores in the tens."""
    _run(bits, ratio, R, T0, Q, kind, label=f"open {bits} {ratio} {R} {T0} {Q} {kind}")


def test_extend_q1_against_the_contract_both_forms():
    """Q = 1 at 2 bits, nh / nh_kv = 4, R = 64, P0 = 700 (1.007x of 1.5e-3 + 1 ulp between the two forms): the extend and the decode
    step each against the contract, stage by stage."""
    from kivi_amd import _lib
    from kivi_amd.attention import kivi_attention_decode
    bits, ratio, R, T0, B, nh_kv = 2, 4, 64, 700, 2, 2
    k0, v0 = _kv(1, B, nh_kv, T0, "randn"), _kv(2, B, nh_kv, T0, "randn")
    layer, past = _prefilled(bits, ratio, R, k0, v0)
    other = layer.clone()
    q, kn, vn = make_kv(10, B, nh_kv * ratio, 1, D).cuda(), make_kv(11, B, nh_kv, 1, D).cuda(), make_kv(12, B, nh_kv, 1, D).cuda()
    a, _, _ = _extend_stages(layer, past, q, kn, vn, bits, R, label="q1 extend")
    other.flags |= _lib.GQA_DUMP_SCORES
    b = kivi_attention_decode(q, kn, vn, other)
    n = T0 + 1
    x = other._native[4][0][:B, : nh_kv * ratio, :, :n].cpu()
    ref, new_past, pre = T64.decode_step(q, kn, vn, past, bits, bits, G32, R)
    ok, ra = gemv_close(x, pre, rtol=1e-3, ulps=1)
    assert ok, ("decode stage A", ra)
    ref_b, _, _ = T64.decode_step(q, kn, vn, past, bits, bits, G32, R, scores_override=x.to(q.device))
    ok, rb = gemv_close(b, ref_b, rtol=2e-3, ulps=1)
    assert ok, ("decode stage B", rb)
    rows, allow = _e2e_rows(b, ref, pre, torch.ones((1, n), dtype=torch.bool))
    assert bool((rows <= allow).all()), ("decode end to end", rows.max().item())
    _, rf = gemv_close(a, b, rtol=1.5e-3, ulps=1)
    _assert_same_state(layer, other)
    print(f"decode step: stage A {ra:.3f}, stage B {rb:.3f}; extend vs decode {rf:.3f} of 1.5e-3+1ulp")


# ------------------------------------------------------------------ 2. edges of mf_extend_kernel
EDGES = [  # (bits, B, nh_kv, ratio, R, P0, Q)
    (2, 2, 2, 1, 32, 512, 7),       # empty K residual (P0 a multiple of R)
    (4, 2, 2, 1, 32, 512, 7),
    (2, 2, 2, 4, 64, 20, 9),        # no packed K (Tq = 0), no packed V
    (4, 2, 2, 4, 64, 20, 9),
    (2, 2, 2, 1, 32, 20, 50),       # ... and the first K flush inside the chunk
    (2, 2, 2, 8, 32, 40, 24),       # a K flush on the chunk's last token
    (2, 2, 2, 1, 32, 100, 16),      # Q * G = 16: one full tile
    (2, 2, 2, 1, 32, 100, 17),      # 17: a tile and one row
    (4, 2, 2, 1, 32, 100, 17),
    (2, 2, 2, 8, 32, 100, 2),       # G = 8: 16 rows
    (2, 2, 2, 8, 32, 100, 3),       # 24 rows
    (2, 2, 1, 1, 32, 70, 97),       # the ring wraps more than once; whole R-runs packed straight from the chunk
    (4, 2, 1, 1, 32, 70, 97),
    (2, 2, 1, 4, 32, 300, 33),      # nh_kv = 1
    (2, 2, 8, 1, 32, 300, 20),      # nh_kv = 8
    (4, 2, 8, 4, 64, 300, 20),
    (2, 1, 2, 4, 64, 200, 19),      # B = 1
    (2, 5, 2, 1, 32, 130, 11),      # B = 5
    (4, 5, 2, 4, 32, 130, 11),
    (2, 2, 2, 4, 32, 4100, 16),     # rows of 130 key tiles: 4 waves x 32 rounds
    (4, 2, 2, 4, 32, 4100, 16),
    (4, 2, 2, 1, 128, 4100, 16),
]


@pytest.mark.parametrize("bits,B,nh_kv,ratio,R,P0,Q", EDGES)
def test_extend_stages_edges(bits, B, nh_kv, ratio, R, P0, Q):
    _run(bits, ratio, R, P0, Q, B=B, nh_kv=nh_kv, label=f"edge {bits} {B} {nh_kv} {ratio} {R} {P0} {Q}")


@pytest.mark.parametrize("bits,ratio", [(2, 4), (4, 1)])
def test_extend_stages_growth(bits, ratio):
    """A layer built for 510 tokens extended by 5: ensure_room reallocates the stores, the chunk crosses the 512-token super-block."""
    layer, _ = _run(bits, ratio, 32, 510, 5, max_len=510, label=f"growth {bits} {ratio}")
    assert layer.n_sb == 2


@pytest.mark.parametrize("bits,ratio,R", [(2, 8, 32), (4, 4, 64), (2, 1, 32)])
def test_extend_stages_chained(bits, ratio, R):
    """extend -> 3 decode steps -> extend -> extend: the V window starts mid-buffer before the second and third calls; every extend
    stage by stage, and the cache after each one bit-identical to an all-decode clone."""
    from kivi_amd.attention import kivi_attention_decode
    B, nh_kv, T0 = 2, 2, 150
    nh = nh_kv * ratio
    layer, past = _prefilled(bits, ratio, R, make_kv(1, B, nh_kv, T0, D), make_kv(2, B, nh_kv, T0, D))
    alld = layer.clone()

    def chunk(seed, Q):
        return make_kv(seed, B, nh, Q, D).cuda(), make_kv(seed + 1, B, nh_kv, Q, D).cuda(), make_kv(seed + 2, B, nh_kv, Q, D).cuda()

    def decode_all(q, kn, vn):
        for i in range(q.shape[2]):
            kivi_attention_decode(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], alld)

    for call, (seed, Q) in enumerate([(10, 13), (None, 3), (20, R + 5), (30, 7)]):
        q, kn, vn = chunk(100 + call if seed is None else seed, Q)
        if seed is None:                                   # decode steps, on both
            for i in range(Q):
                kivi_attention_decode(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], layer)
                _, past, _ = T64.decode_step(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], past, bits, bits, G32, R)
            decode_all(q, kn, vn)
            assert layer.v_res_start != 0 or layer.v_res_len == 0
            continue
        _, past, _ = _extend_stages(layer, past, q, kn, vn, bits, R, label=f"chained {bits} {ratio} {R} call {call}")
        decode_all(q, kn, vn)
        _assert_same_state(layer, alld)


@pytest.mark.parametrize("bits,ratio", [(2, 4), (2, 1), (4, 4), (2, 8)])
def test_extend_stages_mask_on_chunk_keys(bits, ratio):
    """A full (B, 1, Q, P0 + Q) mask: batch row 0 masks its whole prefix at the fp16 minimum (row i sees only chunk tokens 0..i; the
    prefix keys are large, so the masked scores land on the clamp at the fp16 minimum), batch row 1 adds -3 to scattered prefix keys and masks chunk key 2 at the minimum for the rows after it."""
    B, nh_kv, R, T0, Q = 2, 2, 32, 140, 12
    k0, v0 = make_kv(1, B, nh_kv, T0, D, "outlier"), make_kv(2, B, nh_kv, T0, D, "outlier")
    k0[0] *= 7                                # scores of the masked prefix reach the hundreds: fp16(x + finfo.min) overflows to -inf
    layer, past = _prefilled(bits, ratio, R, k0, v0)
    mask = torch.zeros((B, 1, Q, T0 + Q), dtype=torch.float16)
    mask[0, :, :, :T0] = FMIN
    gen = torch.Generator().manual_seed(3)
    mask[1, :, :, torch.randint(0, T0, (9,), generator=gen)] = -3.0
    mask[1, :, 3:, T0 + 2] = FMIN
    mask[1, :, :, T0 + 5] = -1.5
    q = make_kv(10, B, nh_kv * ratio, Q, D).cuda()
    kn, vn = make_kv(11, B, nh_kv, Q, D, "outlier").cuda(), make_kv(12, B, nh_kv, Q, D, "outlier").cuda()
    _extend_stages(layer, past, q, kn, vn, bits, R, mask.cuda(), label=f"mask {bits} {ratio}")


# ------------------------------------------------------------------ 3. dynamic range of the hi / lo operand pair
@pytest.mark.parametrize("m0,m1", [(1e-4, 1e-4), (1e-4, 1.0), (1.0, 1e3), (1e3, 1.0), (3e4, 3e4)])
@pytest.mark.parametrize("bits,ratio", [(2, 1), (2, 4), (2, 8), (4, 4)])
def test_extend_stages_dynamic_range(bits, ratio, m0, m1):
    """Prompt of magnitude m0, chunk of magnitude m1 (K spread over channels, V over tokens: test_mf_decode_steps_dynamic_range's
    inputs), q scaled so that the reference stays finite; the chunk crosses two K flushes (the second on its last token).  Scales run
    from the fp16 subnormals (hi and lo both subnormal: the pair holds a value to 2^-25) to ~2e4.  The range words against Q decode
    steps (in _extend_stages) and set exactly where a scale >= 256 was written."""
    from kivi_amd.quant import mfma
    B, nh_kv, R, T0, Q = 2, 2, 32, 600, 40
    nh = nh_kv * ratio
    k0, v0 = _ranged(1, B, nh_kv, T0, m0, 3), _ranged(2, B, nh_kv, T0, m0, 2)
    layer, past = _prefilled(bits, ratio, R, k0, v0)
    qmag = min(1.0, 300.0 / max(m0, m1))
    q = (make_kv(10, B, nh, Q, D) * qmag).half().cuda()
    kn, vn = _ranged(11, B, nh_kv, Q, m1, 3).cuda(), _ranged(12, B, nh_kv, Q, m1, 2).cuda()
    _, ref_past, _ = _extend_stages(layer, past, q, kn, vn, bits, R, label=f"range {bits} {ratio} {m0:g} {m1:g}")
    for store, sc in ((layer.kt, ref_past[2]), (layer.vt, ref_past[6])):     # the contract's K_scale_T / V_scale, per unit
        sc = sc.float().flatten(2)
        assert torch.equal(mfma.range_big(store).cpu(), (sc >= 256).any(-1).cpu())
        assert torch.equal(mfma.range_small(store).cpu(), (sc < 2.0 ** -8).all(-1).cpu())
        if bits == 2:                          # 2-bit groups of magnitude 1e3 have scales above 256 (4-bit: ~130)
            assert bool(mfma.range_big(store).any()) == (max(m0, m1) >= 1e3)
        if max(m0, m1) <= 1e-4:
            assert bool(mfma.range_small(store).all())


# ------------------------------------------------------------------ 4. the hook-state layout at its own shapes
HOOK_SHAPES = [  # (k_bits, v_bits, g, D, nh / nh_kv, R)
    (2, 2, 64, 128, 1, 64),
    (2, 2, 64, 128, 4, 128),
    (2, 2, 128, 128, 1, 128),
    (2, 2, 32, 64, 4, 32),
    (2, 2, 32, 128, 2, 32),
    (4, 4, 32, 128, 8, 32),
    (2, 4, 32, 128, 4, 32),
    (2, 2, 32, 128, 1, 256),
]


HOOK_CASES = ([sh + (q, "randn") for sh in HOOK_SHAPES for q in ("1", "R-1", "2R+3")] + [(2, 2, 64, 128, 4, 128, "masked", "randn")]
              + [sh + ("2R+3", "outlier") for sh in HOOK_SHAPES])


@pytest.mark.parametrize("kb,vb,g,Dh,ratio,R,qsel,kind", HOOK_CASES)
def test_hook_state_extend_at_its_shapes(kb, vb, g, Dh, ratio, R, qsel, kind, monkeypatch):
    """KiviLayerCache.extend where the matrix pipe refuses the shape.  Its softmax input is caught on the way (torch.softmax), so the
    torch path is checked in stages too: A. those rows against extend64's at 1e-3 + 1 ulp; B. the output against extend64 on those
    rows at 2e-3 + 1 ulp; E. the output against extend64 at the allowance of _extend_stages.  The 3e-3 + 1 ulp bar the suite holds the
    matrix-pipe cases to is NOT met on this path: randn inputs measured up to 1.12 of it (g = 64, nh / nh_kv = 4, R = 128, Q = 127)
    with stage A at 0.74 and stage B at 0.61 of their bars, so the torch path computes what the contract computes from its own rows
    and the rest is the reference softmax's response to one fp16 ulp of a score.  The cache against extend64's 9-tuple and against Q
    decode steps on a clone bit for bit, and the next decode step (see below)."""
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, kivi_attention_extend, make_layer_cache
    B, nh_kv = 2, 2
    nh = nh_kv * ratio
    T0 = 2 * R + 5
    Q = {"1": 1, "R-1": R - 1, "2R+3": 2 * R + 3, "masked": R + 7}[qsel]
    cfg = KiviConfig(kb, vb, g, R)
    k0, v0 = make_kv(1, B, nh_kv, T0, Dh, kind).cuda(), make_kv(2, B, nh_kv, T0, Dh).cuda()
    layer = make_layer_cache(cfg, B, nh_kv, Dh, T0 + 8, "cuda", num_heads=nh)
    assert getattr(layer, "layout", "") != "mfma"
    layer.prefill(k0, v0)
    past = T64.prefill_cache(k0, v0, kb, vb, g, R)
    steps = layer.clone()
    q, kn, vn = make_kv(10, B, nh, Q, Dh).cuda(), make_kv(11, B, nh_kv, Q, Dh, kind).cuda(), make_kv(12, B, nh_kv, Q, Dh).cuda()
    mask = None
    if qsel == "masked":
        mask = torch.zeros((B, 1, Q, T0 + Q), dtype=torch.float16)
        mask[0, :, :, :9] = FMIN
        mask[1, :, 4:, T0 + 1] = FMIN
        mask[1, :, :, 20:30] = -2.0
        mask = mask.cuda()
    rows = []
    softmax = torch.softmax

    def spy(x, *args, **kw):
        rows.append(x.detach().clone())
        return softmax(x, *args, **kw)

    with monkeypatch.context() as m:
        m.setattr(torch, "softmax", spy)
        out = kivi_attention_extend(q, kn, vn, layer, attention_mask=mask)
    assert len(rows) == 1 and rows[0].shape == (B, nh, Q, T0 + Q)
    ref, ref_past, pre = extend64(q, kn, vn, past, kb, vb, g, R, mask, return_scores=True)
    x, pre = rows[0].cpu(), pre.cpu().float()
    vis = _visible(T0, Q).expand_as(x)
    live = vis & (pre > -60000)
    ok, ra = gemv_close(torch.where(live, x, 0.0), torch.where(live, pre, 0.0), rtol=1e-3, ulps=1)
    assert ok, ("stage A", ra)
    assert bool(((x - pre).abs()[vis & ~live] <= 32).all())
    ref_b, _ = extend64(q, kn, vn, past, kb, vb, g, R, mask, scores_override=rows[0].half())
    ok, rb = gemv_close(out, ref_b, rtol=2e-3, ulps=1)
    assert ok, ("stage B", rb)
    _, re_ = gemv_close(out, ref, rtol=3e-3, ulps=1)
    r, allow = _e2e_rows(out, ref, pre, vis)
    assert bool((r <= allow).all()), ("end to end", re_)
    print(f"hook {kb} {vb} {g} {Dh} {ratio} {R} Q={Q} {kind}: stage A {ra:.3f}, stage B {rb:.3f}, end to end {re_:.3f}")
    assert layer.kv_seq_len == T0 + Q
    for x_, y_ in zip(layer.as_tuple()[:8], ref_past[:8]):
        assert (x_ is None and y_ is None) or same_bits(x_, y_)
    for i in range(Q):
        mi = None if mask is None else mask[:, :, i:i + 1, : T0 + i + 1]
        kivi_attention_decode(q[:, :, i:i + 1], kn[:, :, i:i + 1], vn[:, :, i:i + 1], steps, attention_mask=mi)
    for j, (x_, y_) in enumerate(zip(layer.as_tuple()[:9], steps.as_tuple()[:9])):
        assert (x_ is None and y_ is None) or (same_bits(x_, y_) if torch.is_tensor(x_) else x_ == y_), ("9-tuple member", j)
    # the next step: the composed form (no fused launch, nothing that depends on the layer's history) gives the same bits on both
    qn, kk, vv = make_kv(50, B, nh, 1, Dh).cuda(), make_kv(51, B, nh_kv, 1, Dh).cuda(), make_kv(52, B, nh_kv, 1, Dh).cuda()
    assert same_bits(kivi_attention_decode(qn, kk, vv, layer.clone(), fused_kernels=False),
                     kivi_attention_decode(qn, kk, vv, steps.clone(), fused_kernels=False))
    # ... and so does the fused form wherever both layers take the same launches.  A layer whose K residual once passed what the
    # one-call step holds (R = 256: 136 keys) keeps the slower multi-launch form from then on (_drop_fusion), and that form rounds
    # differently: there the two outputs are two forms of one step (1.5e-3 + 1 ulp) and each holds the contract.
    a, b = kivi_attention_decode(qn, kk, vv, layer), kivi_attention_decode(qn, kk, vv, steps)
    if getattr(layer, "_attend_unfusable", False) == getattr(steps, "_attend_unfusable", False):
        assert same_bits(a, b)
    else:
        assert R > 128 and getattr(steps, "_attend_unfusable", False)
        ok, rf = gemv_close(a, b, rtol=1.5e-3, ulps=1)
        assert ok, ("two forms of the next step", rf)
        ref_n, _, _ = T64.decode_step(qn, kk, vv, ref_past, kb, vb, g, R)
        for o in (a, b):
            ok, rn = gemv_close(o, ref_n, rtol=3e-3, ulps=1)
            assert ok, ("next step against the contract", rn)


@pytest.mark.parametrize("fused", [True, False])
def test_hook_state_decode_steps_r256_match_chained_reference(fused):
    """The decode steps the R = 256 extend cases compare against, on their own: 270 steps from a 517-token prompt (the K residual
    passes the 136 keys the one-call step holds -- the layer drops to the multi-launch form -- then fills to 256 and flushes; V
    flushes every step), the 9-tuple bit-identical to chained torch_ref64.decode_step after EVERY step and the output within
    3e-3 + 1 ulp of it; fused launches and the composed form."""
    import warnings

    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    bits, g, R, B, nh_kv, Dh = 2, 32, 256, 2, 2, 128
    T0 = 2 * R + 5
    k0, v0 = make_kv(1, B, nh_kv, T0, Dh).cuda(), make_kv(2, B, nh_kv, T0, Dh).cuda()
    layer = make_layer_cache(KiviConfig(bits, bits, g, R), B, nh_kv, Dh, T0 + 8, "cuda", num_heads=nh_kv)
    assert getattr(layer, "layout", "") != "mfma"
    layer.prefill(k0, v0)
    past = T64.prefill_cache(k0, v0, bits, bits, g, R)
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # the performance warning of the drop to the multi-launch form
        for s in range(270):
            q, kn, vn = make_kv(100 + s, B, nh_kv, 1, Dh).cuda(), make_kv(200 + s, B, nh_kv, 1, Dh).cuda(), make_kv(300 + s, B, nh_kv, 1, Dh).cuda()
            out = kivi_attention_decode(q, kn, vn, layer, fused_kernels=fused)
            ref, past, _ = T64.decode_step(q, kn, vn, past, bits, bits, g, R)
            ok, r = gemv_close(out, ref, rtol=3e-3, ulps=1)
            assert ok, (s, r)
            worst = max(worst, r)
            for j, (x_, y_) in enumerate(zip(layer.as_tuple()[:9], past[:9])):
                assert (x_ is None and y_ is None) or (same_bits(x_, y_) if torch.is_tensor(x_) else x_ == y_), (s, "9-tuple member", j)
    assert layer.k_quant_len == 3 * R and layer.k_res_len == 19
    if fused:
        assert getattr(layer, "_attend_unfusable", False), "the steps must have reached the multi-launch form"
    print(f"R = 256 decode steps (fused={fused}): worst output ratio {worst:.3f} of 3e-3+1ulp")


def test_extend_ignores_the_decode_dump_flag():
    """A layer whose flags carry KIVI_GQA_DUMP_SCORES for its decode steps (as the full-size tests set it): extend does not dump into
    the decode scratch rows -- it runs for Q > 1 and gives the bits of a layer without the flag."""
    from kivi_amd import _lib
    B, nh_kv, ratio, R, T0, Q = 2, 2, 4, 32, 100, 9
    k0, v0 = make_kv(1, B, nh_kv, T0, D), make_kv(2, B, nh_kv, T0, D)
    layer, _ = _prefilled(2, ratio, R, k0, v0)
    other = layer.clone()
    layer.flags |= _lib.GQA_DUMP_SCORES
    q, kn, vn = make_kv(10, B, nh_kv * ratio, Q, D).cuda(), make_kv(11, B, nh_kv, Q, D).cuda(), make_kv(12, B, nh_kv, Q, D).cuda()
    assert same_bits(layer.extend(q, kn, vn), other.extend(q, kn, vn))
    _assert_same_state(layer, other)


# ------------------------------------------------------------------ 5. kivi_vt_pack_at directly
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("off,T,big", [(0, 5, False), (1, 40, True), (31, 3, False), (32, 70, True), (33, 1, False), (513, 100, True)])
def test_vt_pack_at_direct(bits, off, T, big):
    """Per-token V quantisation of T tokens at token offset `off` into a store pre-filled with random words: the written tokens equal
    torch_ref64.quant_pack_lastdim (read back through kivi_vt_relayout), every other bit of the store is untouched, and the range words
    are what per-token V flushes set (byte 2 always, byte 1 for a scale >= 2^-8, byte 0 for one >= 256: a x1e3 token) on words whose
    other bytes were already set: a mark never overwrites a non-zero byte."""
    from kivi_amd import _lib
    from kivi_amd.quant import mfma
    B, nh_kv, n_sb = 2, 3, 2
    end = off + T
    v = make_kv(7, B, nh_kv, T, D).cuda()
    if big:
        v[1, 2, T // 2] *= 1000
    store = mfma.alloc_store(B, nh_kv, n_sb, "cuda", bits)
    flat = torch.empty(0, dtype=torch.int32, device="cuda").set_(store.untyped_storage())
    main = store.numel()
    gen = torch.Generator(device="cuda").manual_seed(off * 7 + T)
    flat[:main] = torch.randint(-2 ** 31, 2 ** 31 - 1, (main,), dtype=torch.int32, device="cuda", generator=gen)
    pre = 0x07 if not big else 0x0700          # a byte the new tokens would not set / would set to 1: the marks keep what is there
    mfma.range_flags(store).fill_(pre)
    before = flat.clone()
    lib = _lib.load()
    rc = lib.kivi_vt_pack_at(v.data_ptr(), v.stride(0), v.stride(1), v.stride(2), *mfma._st(store, bits), off, B, nh_kv, T, D, 32, bits,
                             _lib.stream_ptr(v))
    _lib.check(rc, "kivi_vt_pack_at")
    torch.cuda.synchronize()
    # the written tokens
    code, scale, mn = mfma.vt_to_ref(store, end, D, 32, bits)
    rc_, rs, rm = T64.quant_pack_lastdim(v, 32, bits)
    assert torch.equal(code[:, :, off:], rc_) and same_bits(scale[:, :, off:], rs) and same_bits(mn[:, :, off:], rm)
    # the bits the tokens own: a zeroed store written with all-ones fields for tokens [off, end) and zeros before
    own = mfma.alloc_store(B, nh_kv, n_sb, "cuda", bits)
    c1 = torch.zeros((B, nh_kv, end, D // (32 // bits)), dtype=torch.int32, device="cuda")
    s1 = torch.zeros((B, nh_kv, end, D // 32), dtype=torch.int16, device="cuda")
    c1[:, :, off:] = -1
    s1[:, :, off:] = -1
    mfma.vt_from_ref(own, c1, s1.view(torch.float16), s1.view(torch.float16), 32, bits)
    w = torch.empty(0, dtype=torch.int32, device="cuda").set_(own.untyped_storage())[:main]
    assert int((w != 0).sum()) > 0
    changed = (flat[:main] ^ before[:main]) & ~w
    assert int((changed != 0).sum()) == 0, "words outside the new tokens' fields were modified"
    # the range words
    sc = rs.float().flatten(2)
    marks = 0x010000 + 0x100 * (sc >= 2.0 ** -8).any(-1).int() + (sc >= 256).any(-1).int()
    expect = torch.zeros_like(marks)
    for k in range(3):                         # a byte already non-zero stays as it was; a zero byte takes the mark
        pb, mb = (pre >> (8 * k)) & 0xFF, (marks >> (8 * k)) & 0xFF
        expect += (mb if pb == 0 else torch.full_like(mb, pb)) << (8 * k)
    assert torch.equal(mfma.range_flags(store), expect.int()), (mfma.range_flags(store), expect)
    assert bool((sc >= 256).any()) == big
