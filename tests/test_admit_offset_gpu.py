"""GPU: admission at an offset -- kivi_mf_store_admit, KiviCacheBase.admit_(offset=), LlamaForCausalLM_KIVI.admit_(offset=),
generate_continuous(short_admissions=True).

1. Bytes.  A destination prefilled at T0 and decoded to L (ring moved and wrapped, K flushes, stores grown, the native descriptor
   built) takes a source that is L - S tokens SHORTER.  Bit for bit: the admitted rows sliced at the offset are the source (9-tuple and
   range words), the lead of the packed stores is zero, every other row of every held tensor keeps its bytes, pointers / lengths /
   descriptor stay, an old checkpoint is stale, the source is only read, and a clone rebased by the offset IS the source in those rows.
2. Steps.  40 decode steps on the destination (the lead masked by the additive key row) and on the source (no mask) with the same
   inputs: the rebased clone of the destination equals the source bit for bit afterwards, and goes on like it; the outputs of the
   un-rebased destination are finite and held against tests/torch_ref64.py over the row's real tokens at the bars of
   tests/test_longpad_gpu.py (matrix-pipe layout: the rows the softmax consumed at 1e-3 + 1 ulp over the real keys, the keys under
   the lead at most -60000 and within 32 of the fp16 minimum, the attend half on those rows at 2e-3 + 1 ulp; hook-state layout: end
   to end per row at the allowance of test_extend_stages_gpu._e2e_rows).  The keys under the lead are cut off on both sides rather than
   filled: the reference runs over the real tokens only, so the rms term of the bar is that of the real keys, as the convention wants.
3. Model: per-layer caches after an admission at the scheduler's offset; generate_continuous(short_admissions=True) against a
   restatement (greedy, EOS, per-request sampling, compact=), graphed against eager with one capture; the semantic bar d1 <= 2 d0.
"""
import os

import pytest
import torch

import torch_ref64 as T64
from helpers import gemv_close, make_kv, same_bits
from test_admit_gpu import (LAYOUTS, _check_outputs, _decode_to, _held, _prefilled, _prompts, _range_words, _same_member,
                            _step_inputs)
from test_extend_gpu import _model
from test_extend_stages_gpu import _e2e_rows
from test_rebase_cpu import _sliced
from test_sample_gpu import _layouts

pytestmark = pytest.mark.gpu
D, R = 128, 32
LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len")


# ------------------------------------------------------------------ 1. bytes
def _lead_bytes(lc, rows, off):
    """Everything the packed K and V of rows `rows` hold for tokens [0, off), as a list of tensors (matrix-pipe layout: the store words
    of blocks [0, off / 32), read at the addresses kivi_mfma_layout.h gives; hook-state layout: the pages and the V triple)."""
    if not hasattr(lc, "kt"):
        kf, P = 32 // lc.cfg.k_bits, lc.page_tokens
        out = [x[rows][:, :, :off] for x in (lc.v_code, lc.v_scale, lc.v_mn)]
        for p in range((off + P - 1) // P):
            n = min(P, off - p * P)
            out += [lc.k_code[rows][:, :, p, :, : n // kf], lc.k_scale[rows][:, :, p, :, : n // 32], lc.k_mn[rows][:, :, p, :, : n // 32]]
        return out
    out = []
    for st, is_k in ((lc.kt, True), (lc.vt, False)):
        W = st.shape[3]
        BW, S0 = (W - 2048) // 16, W - 2048                # code words of a block; word offset of the scale region
        mine = st[rows]
        for j in range(off // 32):
            sb = mine[:, :, j // 16]                       # (n, nh_kv, W) int32
            g = j % 16
            out.append(sb[..., g * BW: (g + 1) * BW])
            for region in (0, 1):
                r0 = S0 + region * 1024
                if is_k:                                   # 16 pieces of 8 halves: halves (g >> 3) * 1024 + p * 64 + (g & 7) * 8
                    halves = sb[..., r0: r0 + 1024].contiguous().view(torch.int16)
                    out += [halves[..., (g >> 3) * 1024 + p * 64 + (g & 7) * 8:][..., :8] for p in range(16)]
                else:                                      # 256 bytes at g * 256
                    out.append(sb[..., r0 + g * 64: r0 + (g + 1) * 64])
    return out


def _admit_and_check(dst, src, rows, off):
    kf = 32 // dst.cfg.k_bits
    L = dst.kv_seq_len
    lengths = tuple(getattr(dst, n) for n in LENGTHS)
    before = {n: t.clone() for n, t in _held(dst).items()}
    ptrs = {n: t.data_ptr() for n, t in _held(dst).items()}
    nat, ck = dst._native, dst.checkpoint()
    want, want_range = tuple(None if x is None else x.clone() for x in src.as_tuple()[:8]), [t.clone() for t in _range_words(src)]
    idx = torch.tensor(rows, device="cuda", dtype=torch.int32 if len(rows) == 1 else torch.int64)
    assert dst.admit_(idx, src, offset=off) is dst
    got = dst.as_tuple()
    assert got[8] == L == src.kv_seq_len + off
    mine = tuple(None if x is None else x[rows] for x in got[:8]) + (L,)
    for i, (x, y) in enumerate(zip(_sliced(mine, off, kf)[:8], want)):             # (a)
        assert _same_member(x, y), i
    for x, y in zip(_range_words(dst), want_range):
        assert torch.equal(x[rows], y)
    for t in _lead_bytes(dst, rows, off):                                          # (b)
        assert t.numel() and not t.any()
    others = [b for b in range(dst.B) if b not in rows]
    for n, t in _held(dst).items():                                                # (c)
        assert t.data_ptr() == ptrs[n], n
        assert torch.equal(t[others].view(torch.uint8), before[n][others].view(torch.uint8)), n
    assert lengths == tuple(getattr(dst, n) for n in LENGTHS) and dst._native is nat
    with pytest.raises(ValueError, match="stale"):                                 # (d)
        dst.restore_(ck)
    for x, y in zip(src.as_tuple()[:8], want):                                     # (e)
        assert _same_member(x, y)
    for x, y in zip(_range_words(src), want_range):
        assert torch.equal(x, y)
    twin = dst.clone().rebase_(off)                                                # (f)
    assert twin.kv_seq_len == src.kv_seq_len
    for i, (x, y) in enumerate(zip(twin.as_tuple()[:8], want)):
        assert _same_member(None if x is None else x[rows], y), i
    for x, y in zip(_range_words(twin), want_range):
        assert torch.equal(x[rows], y)


@pytest.mark.parametrize("T0,L,S", [(40, 110, 46), (40, 109, 45), (500, 530, 82), (500, 530, 498), (40, 1100, 76)])
@pytest.mark.parametrize("layout,bits,ratio", LAYOUTS)
def test_offset_admitted_bytes(layout, bits, ratio, T0, L, S):
    off = L - S
    assert off == {(110, 46): 64, (109, 45): 64, (530, 82): 448, (530, 498): 32, (1100, 76): 1024}[(L, S)]
    dst = _decode_to(_prefilled(layout, bits, ratio, 3, T0, 1), L, ratio, 100)
    assert dst.kv_seq_len == L and (dst._native is not None or layout == "hook")
    twin = dst.clone()
    twin._desc(twin.nh, "cuda") if layout == "mfma" else twin._native_desc(twin.nh_kv * ratio)      # the descriptor a step would have built
    _admit_and_check(dst, _prefilled(layout, bits, ratio, 1, S, 7), [1], off)
    src = _decode_to(_prefilled(layout, bits, ratio, 2, S - 3, 11), S, ratio, 200)      # a source that has decoded itself: another phase
    if layout == "mfma" and S - 3 >= R:
        assert src.v_res_start == 3
    _admit_and_check(twin, src, [2, 0], off)


# ------------------------------------------------------------------ 2. steps
@pytest.mark.parametrize("layout,bits,ratio,extend", [("mfma", 2, 1, False), ("mfma", 2, 4, True), ("hook", 2, 1, False),
                                                      ("hook", 2, 4, False), ("mfma", 4, 4, False)])
def test_steps_after_offset_admission(layout, bits, ratio, extend):
    from kivi_amd import _lib
    from kivi_amd.attention import kivi_attention_decode, kivi_attention_extend
    rows, L, S, nh_kv, B = [2, 0, 1], 110, 46, 2, 3
    off, nh = L - S, nh_kv * ratio
    dst = _decode_to(_prefilled(layout, bits, ratio, B, 40, 1), L, ratio, 100)
    src = _prefilled(layout, bits, ratio, B, S, 5)
    past = T64.prefill_cache(make_kv(5, B, nh_kv, S, D).cuda(), make_kv(6, B, nh_kv, S, D, "outlier").cuda(), bits, bits, 32, R)
    dst.admit_(rows, src, offset=off)
    if layout == "mfma":                                                           # the rows the softmax consumes, as test_longpad_gpu
        dst.flags = src.flags = _lib.GQA_FORCE_ROW | _lib.GQA_DUMP_SCORES
    inv = torch.tensor(rows, device="cuda")
    low = torch.finfo(torch.float16).min

    def to_dst(x):
        y = torch.empty_like(x)
        y[inv] = x                                                                 # destination row rows[i] is source row i
        return y

    def lead_mask(q_len, n):
        m = torch.zeros((B, 1, q_len, n), dtype=torch.float16, device="cuda")
        m[..., :off] = low
        return m
    worst_a = worst_b = worst_e = 0.0
    for s in range(40):                                                            # K flushes at 128 (64 for the source), a V flush in every step
        q, k, v = _step_inputs(1000 + 3 * s, B, nh, nh_kv)
        n = L + s + 1
        if layout == "mfma":
            dst.ensure_room(1)
            dst._desc(nh, q.device)[4][0].fill_(float("nan"))                      # a stale score row must not pass
        a = kivi_attention_decode(q, k, v, src)
        b = kivi_attention_decode(to_dst(q), to_dst(k), to_dst(v), dst, attention_mask=lead_mask(1, n))[inv]
        assert torch.isfinite(b).all() and torch.isfinite(a).all(), s
        prev = past
        ref, past, pre = T64.decode_step(q, k, v, prev, bits, bits, 32, R)
        if layout == "mfma":
            x_gpu = dst._native[4][0][:B, :nh, :, :n][inv].clone()
            assert not torch.isnan(x_gpu).any(), ("a key of the row was not written", s)
            ok, ra = gemv_close(x_gpu[..., off:], pre, rtol=1e-3, ulps=1)
            assert ok, ("stage A", s, ra)
            xd = x_gpu[..., :off].float()
            assert bool((xd <= -60000).all()) and bool(((xd - low).abs() <= 32).all()), ("keys under the lead", s)
            ref_b, _, _ = T64.decode_step(q, k, v, prev, bits, bits, 32, R, scores_override=x_gpu[..., off:].contiguous())
            ok, rb = gemv_close(b, ref_b, rtol=2e-3, ulps=1)
            assert ok, ("stage B", s, rb)
            worst_a, worst_b = max(worst_a, ra), max(worst_b, rb)
        else:
            ratio_, allow = _e2e_rows(b, ref, pre, torch.ones((1, S + s + 1), dtype=torch.bool))
            assert bool((ratio_ <= allow).all()), ("end to end", s, (ratio_ / allow).max().item())
            worst_e = max(worst_e, (ratio_ / allow).max().item())
    assert src.kv_seq_len + off == dst.kv_seq_len == L + 40 and dst.k_quant_len == 128
    if extend:
        q, k, v = (make_kv(77 + i, B, h, 5, D).cuda() for i, h in enumerate((nh, nh_kv, nh_kv)))
        a = kivi_attention_extend(q, k, v, src)
        b = kivi_attention_extend(to_dst(q), to_dst(k), to_dst(v), dst, attention_mask=lead_mask(5, dst.kv_seq_len + 5))
        assert torch.isfinite(b).all() and torch.isfinite(a).all()
    twin = dst.clone().rebase_(off)                                                # (a clone keeps the flags)
    ta, tb = src.as_tuple(), twin.as_tuple()
    assert ta[8] == tb[8]
    for i, (x, y) in enumerate(zip(ta[:8], tb[:8])):
        assert _same_member(y if y is None else y[inv], x), i
    for x, y in zip(_range_words(src), _range_words(twin)):
        assert torch.equal(y[inv], x)
    q, k, v = _step_inputs(5000, B, nh, nh_kv)                                     # one further common step, no mask on either
    assert same_bits(kivi_attention_decode(to_dst(q), to_dst(k), to_dst(v), twin)[inv], kivi_attention_decode(q, k, v, src))
    print(f"offset admission {layout} {bits}-bit ratio {ratio}: worst ratio: scores {worst_a:.3f} of 1e-3+1ulp, attend {worst_b:.3f} of "
          f"2e-3+1ulp, end to end {worst_e:.3f} of the allowance, over 40 steps")


# ------------------------------------------------------------------ 3. model level
def _living(model, steps=12):
    """A padded batch of 3 (47, 40 and 7 tokens) at L = 84 decoded for `steps` more steps: (caches, their 2D mask, the token every
    row is about to be fed)."""
    from kivi_amd.llama import left_pad
    ids, mask = left_pad(_prompts(1, [47, 40, 7]), 0, "cuda", length=84)
    lg, past = model(ids, padding_mask=mask)
    for _ in range(steps):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(lg.argmax(-1), past, padding_mask=mask)
    return past, mask, lg.argmax(-1)


def _go_on(model, tok, past, mask, n):
    out = []
    for _ in range(n):
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(tok, past, padding_mask=mask)
        tok = lg.argmax(-1)
        out.append(tok)
    return torch.cat(out, 1)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_model_one_row_admitted_at_an_offset(layout, monkeypatch):
    from kivi_amd.llama import left_pad
    from kivi_amd.serving import admission_offset
    _layouts(monkeypatch, layout)
    model = _model(1, 71)
    past, mask, tok = _living(model)
    L = past[0][-1]
    assert L == 96 and getattr(past[0].layer, "layout", "hook") == layout
    off = admission_offset(L, 20, R, model.rebase_quantum(past))
    assert off == 64
    untouched = _go_on(model, tok, [p.layer.clone().as_tuple() for p in past], mask, 10)      # the run without admission
    ids, short = left_pad(_prompts(3, [20]), 0, "cuda", length=L - off)
    caches = [p.layer for p in past]
    lg, past2 = model.admit_(past, [1], ids, short, offset=off)
    assert [p.layer for p in past2] == caches and past2[0][-1] == L
    alone_lg, alone = model(ids, padding_mask=short)                               # the short pass alone
    assert same_bits(lg, alone_lg)
    twins = model.rebase_([p.layer.clone().as_tuple() for p in past2], off)
    for p, q in zip(twins, alone):
        for i, (x, y) in enumerate(zip(p.layer.as_tuple()[:8], q.layer.as_tuple()[:8])):
            assert _same_member(x if x is None else x[1:2], y), i
        for x, y in zip(_range_words(p.layer), _range_words(q.layer)):
            assert torch.equal(x[1:2], y)
    # rows 0 and 2 go on as in the run without admission; row 1 is fed its own first token under a mask whose lead is zero
    tok = tok.clone()
    tok[1] = lg.argmax(-1)[0]
    mask = mask.clone()
    mask[1, :off], mask[1, off:L] = 0, short[0]
    got = _go_on(model, tok, past2, mask, 10)
    assert torch.equal(got[[0, 2]], untouched[[0, 2]])


def _restate(model, prompts, limits, batch, compact=None, eos=None, pad=0, params=None):
    """The policy of kivi_amd/serving.py with short_admissions=True written out from forward(padding_mask=), admit_(offset=), rebase_,
    argmax and RowSampler.  -> (tokens per request, the (L, offset, rows) of every admission, the (L, drop) of every rebase)."""
    from kivi_amd.llama import left_pad
    from kivi_amd.sampling import RowSampler
    N, nb, L = len(prompts), min(batch, len(prompts)), max(len(p) for p in prompts)

    def draw(lg, reqs):
        return lg.argmax(-1) if params is None else RowSampler([params[r] for r in reqs], "cuda")(lg)
    ids, mask = left_pad(prompts[:nb], pad, "cuda", length=L)
    lg, past = model(ids, padding_mask=mask)
    rs = None if params is None else RowSampler(params[:nb], "cuda")
    tok = lg.argmax(-1) if rs is None else rs(lg)
    req, out, nxt, admissions, drops = list(range(nb)), [[] for _ in range(N)], nb, [], []
    lead = [L - len(prompts[r]) for r in range(nb)]

    def emit(b, t):
        r = req[b]
        out[r].append(t)
        if len(out[r]) == limits[r] or t == eos:
            req[b] = None
    while True:
        for b, t in enumerate(tok[:, 0].tolist()):
            if req[b] is not None:
                emit(b, t)
        if compact is not None:
            live = [lead[b] for b in range(nb) if req[b] is not None]
            room = min(min(live) if live else L, L - max([len(p) for p in prompts[nxt:]], default=0),
                       min(past[0].layer.k_quant_len, past[0].layer.v_quant_len))
            drop = room // 32 * 32
            if drop >= compact:
                past = model.rebase_(past, drop)
                mask = mask[:, drop:]
                drops.append((L, drop))
                L -= drop
                lead = [n - drop for n in lead]
        while nxt < N and None in req:
            free = [b for b in range(nb) if req[b] is None][: N - nxt]
            new = list(range(nxt, nxt + len(free)))
            nxt += len(free)
            short = max(max(len(prompts[r]) for r in new), R)                       # room for the longest prompt and one residual
            off = 0
            while off + 32 + short <= L:
                off += 32
            nids, nmask = left_pad([prompts[r] for r in new], pad, "cuda", length=L - off)
            lg, past = model.admit_(past, free, nids, nmask, offset=off)
            mask[free] = torch.cat([torch.zeros_like(mask[free][:, :off]), nmask], 1)
            admissions.append((L, off, free))
            first = draw(lg, new)
            tok[free] = first
            for b, r, t in zip(free, new, first[:, 0].tolist()):
                req[b], lead[b] = r, L - len(prompts[r])
                if rs is not None:
                    rs.set_row(b, params[r], draw_index=1)
                emit(b, t)
        if all(r is None for r in req):
            return out, admissions, drops
        for b in range(nb):
            if req[b] is None:
                tok[b] = pad
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
        lg, past = model(tok, past, padding_mask=mask)
        tok = lg.argmax(-1) if rs is None else rs(lg)
        L += 1


LENS, LIMITS = [66, 12, 9, 8, 30, 7, 11, 6, 9, 5], [3, 20, 24, 12, 26, 10, 9, 12, 1, 6]


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_short_admissions_greedy(layout, monkeypatch):
    _layouts(monkeypatch, layout)
    model = _model(4, 72)
    prompts = _prompts(6, LENS)
    want, admissions, _ = _restate(model, prompts, LIMITS, 3)
    assert len(admissions) >= 4 and all(off > 0 and off % 32 == 0 for _, off, _ in admissions)
    seen = []
    admit_ = model.admit_
    monkeypatch.setattr(model, "admit_", lambda past, rows, ids, m, offset=0: seen.append((past[0][-1], offset, list(rows))) or
                        admit_(past, rows, ids, m, offset=offset))
    out = model.generate_continuous(prompts, LIMITS, 3, short_admissions=True)
    _check_outputs(out, LIMITS)
    assert [o.tolist() for o in out] == want and seen == admissions
    model.release_graphs()
    graphed = model.generate_continuous(prompts, LIMITS, 3, short_admissions=True, graphed=True)
    assert [o.tolist() for o in graphed] == want
    # EOS: a token some request generated
    eos = want[2][9]
    out_e = model.generate_continuous(prompts, LIMITS, 3, eos_token_id=eos, pad_token_id=0, short_admissions=True)
    _check_outputs(out_e, LIMITS, eos)
    want_e, _, _ = _restate(model, prompts, LIMITS, 3, eos=eos)
    assert [o.tolist() for o in out_e] == want_e and len(out_e[2]) <= 10
    # compact=: the rebases of the restatement, the leading pads kept on the host as without offsets
    want_c, adm_c, drops_c = _restate(model, prompts, LIMITS, 3, compact=32)
    del seen[:]
    out_c = model.generate_continuous(prompts, LIMITS, 3, compact=32, short_admissions=True)
    assert [o.tolist() for o in out_c] == want_c and seen == adm_c and drops_c
    graphed = model.generate_continuous(prompts, LIMITS, 3, compact=32, short_admissions=True, graphed=True)
    assert [o.tolist() for o in graphed] == want_c


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_short_admissions_graphed_captures_once(layout, monkeypatch):
    """Graphed equals eager token for token; the admissions replay the captured step (no length or buffer changed)."""
    from kivi_amd import graph
    _layouts(monkeypatch, layout)
    model = _model(4, 73)
    prompts = _prompts(8, [40, 33, 36, 9, 12, 7, 10, 8])              # no pad-free start: the first pads are there from the prompt pass on
    limits = [6, 14, 9, 12, 8, 10, 5, 7]
    eager = model.generate_continuous(prompts, limits, 3, short_admissions=True)
    stats = []
    end = graph.DecodeGraphs.end
    monkeypatch.setattr(graph.DecodeGraphs, "end", lambda self: stats.append(self.stats) or end(self))
    model.release_graphs()
    graphed = model.generate_continuous(prompts, limits, 3, short_admissions=True, graphed=True)
    assert [o.tolist() for o in graphed] == [o.tolist() for o in eager]
    if layout == "mfma":
        assert len(stats) == 1 and stats[0][1] == 1, stats                         # (eager steps, captures, replays)


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_generate_continuous_short_admissions_sampling(layout, monkeypatch):
    from kivi_amd.sampling import SamplingParams
    _layouts(monkeypatch, layout)
    model = _model(4, 74)
    prompts = _prompts(7, LENS)
    params = [SamplingParams(temperature=0.8 + 0.05 * r, top_k=(0, 40, 25)[r % 3], top_p=(0.9, 1.0)[r % 2], seed=80 + r) if r % 4 else
              SamplingParams(do_sample=False) for r in range(len(LENS))]
    want, admissions, _ = _restate(model, prompts, LIMITS, 3, params=params)
    assert any(off > 0 for _, off, _ in admissions)
    out = model.generate_continuous(prompts, LIMITS, 3, sampling=params, short_admissions=True)
    _check_outputs(out, LIMITS)
    assert [o.tolist() for o in out] == want
    graphed = model.generate_continuous(prompts, LIMITS, 3, sampling=params, short_admissions=True, graphed=True)
    assert [o.tolist() for o in graphed] == want


@pytest.mark.parametrize("layout", ["mfma", "hook"])
def test_offset_admission_semantic_bar(layout, monkeypatch):
    """Three teacher-forced passes over the same fed tokens: A, the row admitted at the offset; B, the same prompt admitted L-padded
    (offset 0); C, the prompt alone as an unpadded batch of one.  d0 = max |B - C| compares two paths of the parent commit that
    differ the way the new one does (length, launch form, pads inside K groups); d1 = max |A - C| has to stay within 2 d0 (each is one
    draw of a maximum over the same kind of error)."""
    from kivi_amd.llama import left_pad
    from kivi_amd.serving import admission_offset
    _layouts(monkeypatch, layout)
    model = _model(4, 75)
    prompt = _prompts(9, [20])
    fed = torch.tensor(_prompts(10, [16])[0], device="cuda")

    def forced(past, mask, row):
        """16 steps on `past` feeding `fed` to row `row` (pad to the others) -> that row's logits (16, vocab) as float."""
        out = []
        for s in range(16):
            tok = torch.zeros((mask.shape[0], 1), dtype=torch.long, device="cuda")
            tok[row] = fed[s]
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], 1)
            lg, past = model(tok, past, padding_mask=mask)
            out.append(lg[row, 0].float())
        return torch.stack(out)
    logits = {}
    for name in ("A", "B"):
        past, mask, _ = _living(model)
        L = past[0][-1]
        off = admission_offset(L, 20, R, model.rebase_quantum(past)) if name == "A" else 0
        assert off == (64 if name == "A" else 0)
        ids, short = left_pad(prompt, 0, "cuda", length=L - off)
        _, past = model.admit_(past, [1], ids, short, offset=off)
        mask = mask.clone()
        mask[1, :off], mask[1, off:L] = 0, short[0]
        logits[name] = forced(past, mask, 1)
    ids = torch.tensor(prompt, device="cuda")
    _, past = model(ids, padding_mask=torch.ones_like(ids))
    logits["C"] = forced(past, torch.ones_like(ids), 0)
    d0, d1 = (logits["B"] - logits["C"]).abs().max().item(), (logits["A"] - logits["C"]).abs().max().item()
    line = f"offset admission parity {layout}: d0 = max|B - C| = {d0:.6f}, d1 = max|A - C| = {d1:.6f}, d1 / d0 = {d1 / max(d0, 1e-30):.3f}"
    print(line)
    log = os.environ.get("KIVI_PARITY_LOG")
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")
    assert d0 > 0, "the bar has collapsed: the two paths of the parent commit agree exactly"
    assert d1 <= 2 * d0, (d0, d1)
