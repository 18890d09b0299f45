"""Time the constrained row sampler (kivi_sample_rows_con) against kivi_sample_rows_pen and against the torch constraints a caller
composes around it; writes profiles/sample_constraint_time.log -- or, with --parent-lib, hold every fused form of the row sampler to
the parent commit's library, in what it draws and in what it costs; writes profiles/sample_fold_time.log.

    python tools/sample_constraint_time.py [--rounds N] [--iters N] [--shape B V] [--parent-lib PATH] [--out PATH]

For (B, V) in {(32, 32000), (64, 128256)}, fp16 logits, top_k 50 + top_p 0.9 in every record, neutral penalty records over an empty
history table, forms on the same logits:
  (a) kivi_sample_rows_pen         RowSampler with a table and no constraint state: what a call without constraints launches
  (b) kivi_sample_rows_con neutral RowSampler with constraint state, every record neutral: the path of (a) plus one record load per row
  (c) kivi_sample_rows_con         a mask that allows about half the tokens and 300 list entries (biases; a tenth of them -inf) per row
  (c') ... mask alone / (c'') ... list alone: the two parts of (c)
  (d) torch + kivi_sample_rows_pen what a caller does today: unpack the bitmask to (B, V) bools, masked_fill, index_add of the biases,
                                   then kivi_sample_rows_pen on the result
Each round times `iters` back-to-back calls of each form with device events, after one warm-up; rounds alternate the forms, and every
timed window starts from the same tables.  Two figures per form, medians (min, max) over the rounds: the CALL time (eager, Python
dispatch inside the window) and the DEVICE time (the same calls captured into one hipGraph and replayed).  Ratios are taken against
(a) on each.
`--parent-lib`: a libkivi_hip.so built from the parent commit.  Before anything is timed, both libraries draw 40 successive tokens
for a batch of four rows -- greedy, sampled, penalised over a marked table, mask + list + suppress_until = 5 -- at every vocabulary
size of tests/sample_plan.py from identical buffers: tokens, draw indices, history table and allow masks have to be equal word for
word.  Then seven fused forms are timed through both libraries by the same raw call (sample_rows_time.raw_call) on the same buffers:
  1 plain rows, no table            2 table, neutral records, about 500 marks per row     3 table, penalised records, the same marks
  4 constraint state, neutral records (= b)    5 mask + 300 entries (= c)    6 mask alone (= c')    7 list alone (= c'')
and each form's device-time median through this library may exceed the parent's by at most the larger of the parent's own min-max
spread in this run and 1 % of the parent's median; a form that misses is reported and the tool exits with status 1."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sample_rows_time import _events, _graph, other_lib, raw_call  # noqa: E402

SHAPES = [(32, 32000), (64, 128256)]
ENTRIES = 300
PEN = dict(repetition_penalty=1.3, presence_penalty=0.6, frequency_penalty=0.25)
SEEN_OUTPUT = 4
CALLS = 40


def _torch_form(logits, under, allowed, ids, values, out):
    """Form (d): the bitmask unpacked to booleans, a masked_fill, an index_add of the biases, then the sampler -- in the dtype of
    `logits` (fp16 as timed: the additions then round to fp16; on fp32 logits it is the rule of the fused kernel bit for bit)."""
    B, V = logits.shape
    shifts = torch.arange(32, device=logits.device, dtype=torch.int32)
    rows = torch.arange(B, device=logits.device)[:, None].expand_as(ids).reshape(-1)
    flat_ids = (rows * V + ids.reshape(-1))
    flat_values = values.reshape(-1).to(logits.dtype)

    def fn():
        bits = ((allowed[:, :, None] >> shifts) & 1).bool().reshape(B, -1)[:, :V]
        x = logits.masked_fill(~bits, float("-inf"))
        x.view(-1).index_add_(0, flat_ids, flat_values)
        under(x, out=out)
    return fn


def suppress_token(row: np.ndarray, allowed) -> int:
    """The allowed token with the largest logit of `row` (the lowest index among equals): the one id whose suppression for the first
    draws has to show in what is drawn.  From the logits on the host, so it is known before any device call that the id is in the
    vocabulary, is let through by the mask, and -- whenever the row allows more than one token -- leaves others to draw from."""
    allowed = np.asarray(sorted(allowed), dtype=np.int64)
    assert allowed.size and 0 <= allowed[0] and allowed[-1] < row.size
    return int(allowed[np.argmax(row[allowed].astype(np.float64))])


def equal_draws(this, parent, V):
    """40 successive calls through each library from identical buffers, a batch of four rows of V tokens; asserts equality."""
    from kivi_amd.sampling import RowSampler, SamplingParams
    rng = np.random.default_rng(V)
    host = (rng.standard_normal((4, V)) * 3).astype(np.float16)
    allowed = sorted(set(rng.choice(V, size=(V + 1) // 2, replace=False).tolist()))
    biased = np.sort(rng.choice(V, size=min(ENTRIES, V), replace=False))
    values = (rng.standard_normal(biased.size) * 2).tolist()
    values[::10] = [float("-inf")] * len(values[::10])
    sup = suppress_token(host[3], allowed)
    base = dict(top_k=50, top_p=0.9)
    rs = RowSampler([SamplingParams(do_sample=False), SamplingParams(**base, seed=11), SamplingParams(**base, seed=12, **PEN),
                     SamplingParams(**base, seed=13, allowed_token_ids=allowed, logit_bias=dict(zip(biased.tolist(), values)),
                                    min_new_tokens=5)], "cuda", vocab_size=V, constraints=True, suppress=[sup])
    rs.observe_prompt(torch.from_numpy(rng.integers(0, V, (4, 400))).cuda())
    rs._mark(SEEN_OUTPUT, torch.from_numpy(rng.integers(0, V, (4, 100))).cuda())
    logits, out = torch.from_numpy(host).cuda(), torch.empty((4, 1), dtype=torch.int64, device="cuda")
    state = (rs.draw_index, rs.seen, rs.allowed)
    first = [t.clone() for t in state]
    got = []
    for lib in (this, parent):
        for t, t0 in zip(state, first):
            t.copy_(t0)
        tokens = []
        for _ in range(CALLS):
            rc = raw_call(lib, rs, logits, out)
            assert rc == 0, rc
            tokens.append(out.clone())
        got.append([torch.cat(tokens, 1).cpu()] + [t.cpu().clone() for t in state])
    assert len(allowed) == 1 or (got[0][0][3, :5] != sup).all(), "the suppressed id was drawn before draw 5"
    for name, a, b in zip(("tokens", "draw_index", "history table", "allow masks"), got[0], got[1]):
        assert torch.equal(a, b), f"V={V}: {name} differ between the two libraries"
    assert torch.equal(got[0][1], first[0].cpu() + CALLS)


def rows(rounds, iters, shapes, parent_lib):
    from kivi_amd import _lib
    from kivi_amd.sampling import RowSampler, SamplingParams, allow_bitmask
    lines, missed = [], 0
    this, parent = _lib.load(), other_lib(parent_lib) if parent_lib else None
    if parent:
        from sample_plan import VS
        for V in VS:
            equal_draws(this, parent, V)
        lines.append(f"  equal through both libraries, word for word: tokens, draw indices, history table and allow masks of {CALLS} successive "
                     f"calls, four rows (greedy, sampled, penalised over a marked table, mask + list + suppress_until 5), V in {VS}")
        print(lines[-1], flush=True)
    for B, V in shapes:
        gen = torch.Generator("cuda").manual_seed(B + V)
        cpu = torch.Generator().manual_seed(B + V)
        logits = (torch.randn((B, V), device="cuda", generator=gen) * 3).half()
        out = torch.empty((B, 1), dtype=torch.int64, device="cuda")
        base = dict(top_k=50, top_p=0.9, seed=1)
        streams = list(range(B))
        ids = torch.stack([torch.randperm(V, generator=cpu)[:ENTRIES].sort().values for _ in range(B)])
        values = torch.randn((B, ENTRIES), generator=cpu) * 2
        values[:, ::10] = float("-inf")
        masks = [allow_bitmask((torch.rand(V, generator=cpu) < 0.5).nonzero().view(-1).tolist(), V) for _ in range(B)]

        def sampler(mask, lists, constraints=True):
            ps = [SamplingParams(**base, logit_bias=dict(zip(ids[b].tolist(), values[b].tolist())) if lists else None) for b in range(B)]
            rs = RowSampler(ps, "cuda", streams=streams, vocab_size=V, constraints=constraints)
            if mask:
                for b in range(B):
                    rs.set_allowed(b, masks[b])
            return rs
        plain = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
        neutral, both, mask_only, list_only = sampler(False, False), sampler(True, True), sampler(True, False), sampler(False, True)
        under = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
        assert neutral.constraint is not None and plain.constraint is None
        assert torch.equal(plain(logits), neutral(logits)), "neutral records have to draw kivi_sample_rows_pen's tokens"
        torch_form = _torch_form(logits, under, both.allowed, ids.cuda(), values.cuda(), out)
        want = both(logits).clone()
        _torch_form(logits.float(), under, both.allowed, ids.cuda(), values.cuda(), out)()
        assert torch.equal(out, want), "the torch composition (in fp32) has to draw the fused kernel's tokens"
        fns = [("(a) rows_pen", lambda: plain(logits, out=out)), ("(b) rows_con, neutral records", lambda: neutral(logits, out=out)),
               ("(c) rows_con, mask + 300 entries", lambda: both(logits, out=out)),
               ("(c') rows_con, mask alone", lambda: mask_only(logits, out=out)),
               ("(c'') rows_con, 300 entries alone", lambda: list_only(logits, out=out)),
               ("(d) torch mask + bias + rows_pen", torch_form)]
        samplers, gated = [plain, neutral, both, mask_only, list_only, under], len(fns)
        if parent:
            rows_only = RowSampler(SamplingParams(**base), "cuda", streams=streams)
            marked = [RowSampler(SamplingParams(**base, **pen), "cuda", streams=streams, vocab_size=V) for pen in ({}, PEN)]
            prompt = torch.randint(0, V, (B, 400), device="cuda", generator=gen)
            emitted = torch.randint(0, V, (B, 100), device="cuda", generator=gen)
            for rs in marked:
                rs.observe_prompt(prompt)
                rs._mark(SEEN_OUTPUT, emitted)
            samplers += marked
            fused = [("1 rows", rows_only), ("2 rows_pen neutral, marks", marked[0]), ("3 rows_pen penalised, marks", marked[1]),
                     ("4 rows_con neutral", neutral), ("5 rows_con mask + 300", both), ("6 rows_con mask alone", mask_only),
                     ("7 rows_con 300 alone", list_only)]
            for name, rs in fused:
                fns += [(name + ", this", lambda rs=rs: raw_call(this, rs, logits, out)),
                        (name + ", parent", lambda rs=rs: raw_call(parent, rs, logits, out))]
        tables = [rs.seen for rs in samplers]
        saved = [t.clone() for t in tables]

        def restore():
            """Every timed window starts from the same history tables (each call counts the token it draws)."""
            for t, t0 in zip(tables, saved):
                t.copy_(t0)
        replays = [_graph(fn, iters) for _, fn in fns]
        for _, fn in fns:                                                    # one warm-up of every form
            fn()
        call, dev = [[] for _ in fns], [[] for _ in fns]
        for _ in range(rounds):
            for i, (_, fn) in enumerate(fns):
                restore()
                call[i].append(_events(fn, iters))
            for i, rp in enumerate(replays):
                restore()
                dev[i].append(_events(rp, 1) / iters)
        mc, md = [statistics.median(t) for t in call], [statistics.median(t) for t in dev]
        for i, (name, _) in enumerate(fns):
            ratio = "" if i == 0 else f"   / (a): call {mc[i] / mc[0]:5.2f}x  device {md[i] / md[0]:5.2f}x"
            lines.append(f"  B={B:3d} V={V:6d} fp16  {name:34s} call {mc[i]:7.1f} us (min {min(call[i]):7.1f}, max {max(call[i]):7.1f})   "
                         f"device {md[i]:7.1f} us (min {min(dev[i]):7.1f}, max {max(dev[i]):7.1f}){ratio}")
            print(lines[-1], flush=True)
        for i in range(gated, len(fns), 2):                                  # (this, parent) pairs: the gate on the device medians
            margin = max(max(dev[i + 1]) - min(dev[i + 1]), 0.01 * md[i + 1])
            ok = md[i] <= md[i + 1] + margin
            missed += not ok
            lines.append(f"  B={B:3d} V={V:6d} gate  {fns[i][0][:-6]:28s} this / parent: device {md[i] / md[i + 1]:6.3f}  call "
                         f"{mc[i] / mc[i + 1]:6.3f}   this {md[i]:7.1f} us <= parent {md[i + 1]:7.1f} + {margin:4.1f} us: "
                         f"{'met' if ok else 'MISSED'}")
            print(lines[-1], flush=True)
    return lines, missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "V"), help="time this shape only")
    ap.add_argument("--parent-lib", help="a libkivi_hip.so of the parent commit: the equality check, then every fused form through both")
    ap.add_argument("--out", help="default: profiles/sample_constraint_time.log, or profiles/sample_fold_time.log with --parent-lib")
    args = ap.parse_args()
    if args.rounds < 7:
        raise SystemExit("at least 7 rounds: the medians are over them")
    if not torch.cuda.is_available():
        raise SystemExit("sample_constraint_time.py needs a GPU: nothing is timed without one")
    path = args.out or os.path.join(ROOT, "profiles", "sample_fold_time.log" if args.parent_lib else "sample_constraint_time.log")
    lines = [f"kivi_sample_rows_con against kivi_sample_rows_pen and against torch constraints around it; fp16 logits (B, V), top_k 50 + "
             f"top_p 0.9 in every record, neutral penalties over an empty table; constrained rows: a mask allowing about half the tokens "
             f"and {ENTRIES} list entries; median (min, max) of {args.rounds} alternating rounds of {args.iters} back-to-back calls "
             f"between device events after one warm-up: eager calls (call time, Python dispatch included) and the same calls replayed "
             f"from one captured graph (device time)"]
    if args.parent_lib:
        lines.append("forms 1-7: the same raw call on the same buffers through this library and through the parent commit's; forms 2 and 3 "
                     "over about 500 marked tokens per row, 3 with penalties (1.3, 0.6, 0.25); gate: this library's device median <= the "
                     "parent's + max(the parent's max - min in this run, 1 % of its median)")
    print("\n".join(lines), flush=True)
    more, missed = rows(args.rounds, args.iters, [tuple(args.shape)] if args.shape else SHAPES, args.parent_lib)
    lines += more
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)
    if missed:
        raise SystemExit(f"{missed} form(s) missed the gate")


if __name__ == "__main__":
    main()
