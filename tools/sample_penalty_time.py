"""Time the penalised row sampler (kivi_sample_rows_pen) against kivi_sample_rows and against the torch penalties a caller composes
around it; writes profiles/sample_penalty_time.log.

    python tools/sample_penalty_time.py [--rounds N] [--iters N] [--shape B V] [--parent-lib PATH] [--out PATH]

For (B, V) in {(32, 32000), (64, 128256)}, fp16 logits, top_k 50 + top_p 0.9 in every record, about 500 marked tokens per row
(400 prompt tokens, 100 emitted ones), four forms on the same logits:
  (a) kivi_sample_rows           RowSampler without a table: the instantiation every call without penalties launches
  (b) kivi_sample_rows_pen 1/0/0 RowSampler with a table, every record neutral: the unpenalised path of the new kernel + the count
  (c) kivi_sample_rows_pen       repetition 1.3, presence 0.6, frequency 0.25 in every record
  (d) torch + kivi_sample_rows   what a caller does without the entry: gather / where / scatter for the repetition penalty over
                                 the row's token list, two (B, V) passes for frequency and presence over a count tensor,
                                 kivi_sample_rows on the result, scatter_add_ of the new tokens into the counts
Each round times `iters` back-to-back calls of each form with device events, after one warm-up; rounds alternate the forms, and
every timed window starts from the same table and counts (a call adds the token it draws, so a window ends `iters` marks on).  Two
figures per form, medians (minimums) over the rounds: the CALL time (eager, Python dispatch inside the window) and the DEVICE time
(the same calls captured into one hipGraph and replayed).  Ratios are taken against (a) on each.
`--parent-lib`: a libkivi_hip.so built from the parent commit; kivi_sample_rows is then timed through both libraries by the same
raw ctypes call on the same buffers, alternating, to show that (a) is the instantiation it was."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sample_rows_time import _events, _graph, other_lib, raw_call  # noqa: E402

SHAPES = [(32, 32000), (64, 128256)]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.6, frequency_penalty=0.25)


def _torch_form(logits, plain, hist_ids, counts, out):
    """Form (d): HF's RepetitionPenaltyLogitsProcessor over the ids, OpenAI's two penalties over the counts, then the sampler."""
    theta, pres, freq = PEN["repetition_penalty"], PEN["presence_penalty"], PEN["frequency_penalty"]
    ones = torch.ones_like(out, dtype=counts.dtype)

    def fn():
        score = torch.gather(logits, 1, hist_ids)
        score = torch.where(score < 0, score * theta, score / theta)
        x = logits.scatter(1, hist_ids, score)
        x -= freq * counts.to(x.dtype)
        x -= pres * (counts > 0).to(x.dtype)
        plain(x, out=out)
        counts.scatter_add_(1, out, ones)
    return fn


def rows(rounds, iters, shapes, parent_lib):
    from kivi_amd import _lib
    from kivi_amd.sampling import RowSampler, SamplingParams
    lines = []
    for B, V in shapes:
        gen = torch.Generator("cuda").manual_seed(B + V)
        logits = (torch.randn((B, V), device="cuda", generator=gen) * 3).half()
        out = torch.empty((B, 1), dtype=torch.int64, device="cuda")
        base = dict(top_k=50, top_p=0.9, seed=1)
        streams = list(range(B))
        plain = RowSampler(SamplingParams(**base), "cuda", streams=streams)
        neutral = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
        pen = RowSampler(SamplingParams(**base, **PEN), "cuda", streams=streams, vocab_size=V)
        under = RowSampler(SamplingParams(**base), "cuda", streams=streams)
        prompt = torch.randint(0, V, (B, 400), device="cuda", generator=gen)
        emitted = torch.randint(0, V, (B, 100), device="cuda", generator=gen)
        for rs in (neutral, pen):
            rs.observe_prompt(prompt)
            rs._mark(4, emitted)                                             # KIVI_SEEN_OUTPUT
        hist_ids = torch.cat([prompt, emitted], 1)
        counts = torch.zeros((B, V), dtype=torch.int32, device="cuda").scatter_add_(1, emitted, torch.ones_like(emitted, dtype=torch.int32))
        assert torch.equal(plain(logits), neutral(logits)), "neutral records have to draw kivi_sample_rows' tokens"
        fns = [("(a) kivi_sample_rows", lambda: plain(logits, out=out)), ("(b) rows_pen, neutral records", lambda: neutral(logits, out=out)),
               ("(c) rows_pen, penalised", lambda: pen(logits, out=out)),
               ("(d) torch penalties + rows", _torch_form(logits, under, hist_ids, counts, out))]
        if parent_lib:
            this, other = _lib.load(), other_lib(parent_lib)
            raw = RowSampler(SamplingParams(**base), "cuda", streams=streams)
            fns += [("(a) raw call, this library", lambda: raw_call(this, raw, logits, out)),
                    ("(a) raw call, parent library", lambda: raw_call(other, raw, logits, out))]
        saved = [t.clone() for t in (neutral.seen, pen.seen, counts)]

        def restore():
            """Every timed window starts from the about 500 marked tokens (each call adds the token it draws)."""
            for t, s0 in zip((neutral.seen, pen.seen, counts), saved):
                t.copy_(s0)
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
            lines.append(f"  B={B:3d} V={V:6d} fp16  {name:30s} call {mc[i]:7.1f} us (min {min(call[i]):7.1f}, max {max(call[i]):7.1f})   "
                         f"device {md[i]:7.1f} us (min {min(dev[i]):7.1f}, max {max(dev[i]):7.1f}){ratio}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "V"), help="time this shape only")
    ap.add_argument("--parent-lib", help="a libkivi_hip.so of the parent commit: kivi_sample_rows through both libraries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_penalty_time.log"))
    args = ap.parse_args()
    if args.rounds < 7:
        raise SystemExit("at least 7 rounds: the medians are over them")
    if not torch.cuda.is_available():
        raise SystemExit("sample_penalty_time.py needs a GPU: nothing is timed without one")
    lines = [f"kivi_sample_rows_pen against kivi_sample_rows and against torch penalties around it; fp16 logits (B, V), top_k 50 + "
             f"top_p 0.9 in every record, about 500 marked tokens per row, penalised records (1.3, 0.6, 0.25); median (min, max) of "
             f"{args.rounds} alternating rounds of {args.iters} back-to-back calls between device events after one warm-up: eager "
             f"calls (call time, Python dispatch included) and the same calls replayed from one captured graph (device time)"]
    print(lines[0], flush=True)
    lines += rows(args.rounds, args.iters, [tuple(args.shape)] if args.shape else SHAPES, args.parent_lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
