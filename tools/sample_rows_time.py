"""Time the per-row sampler (kivi_sample_rows) against kivi_sample; writes profiles/sample_rows_time.log.

    python tools/sample_rows_time.py [--rounds N] [--iters N] [--shape B V] [--out PATH]

For (B, V) in {(32, 32000), (64, 128256)}, fp16 logits, three samplers on the same logits:
  kivi_sample            Sampler(top_k=50, top_p=0.9): the sampler launch + the one-thread launch that advances n
  kivi_sample_rows       RowSampler with the same parameters in every record: one launch
  kivi_sample_rows mixed a quarter of the rows greedy, a quarter temperature only, a quarter top_k = 50, a quarter top_k = 50 +
                         top_p = 0.9 (interleaved over the batch)
Each round times `iters` back-to-back calls of each with device events; rounds interleave the three.  Two figures per sampler, medians
(minimums) over the rounds: the CALL time (eager calls, Python dispatch inside the window -- at these sizes the host is most of it)
and the DEVICE time (the same `iters` calls captured into one hipGraph and replayed: launches back to back without the host).  The
ratio rows / sample is taken on each.  The uniform RowSampler draws the tokens of the Sampler (checked before timing)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 32000), (64, 128256)]


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _graph(fn, iters):
    """`iters` calls of fn captured into one graph; returns a callable that replays it."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    from kivi_amd.graph import no_gc_in_capture
    g = torch.cuda.CUDAGraph()
    with no_gc_in_capture(), torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def other_lib(path):
    """A second libkivi_hip.so (e.g. the parent commit's) with the signatures of the three row entries."""
    import ctypes
    from kivi_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ("kivi_sample_rows", "kivi_sample_rows_pen", "kivi_sample_rows_con"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    return lib


def raw_call(lib, rs, logits, out):
    """What RowSampler `rs` calls for `logits` and `out` -- its entry, its arguments, the current stream -- through `lib`, unchecked."""
    name, args = rs.entry(logits, out)
    return getattr(lib, name)(*args)


def rows(rounds, iters, shapes):
    from kivi_amd.sampling import RowSampler, Sampler, SamplingParams
    lines = []
    for B, V in shapes:
        gen = torch.Generator("cuda").manual_seed(B + V)
        logits = (torch.randn((B, V), device="cuda", generator=gen) * 3).half()
        out = torch.empty((B, 1), dtype=torch.int64, device="cuda")
        old = Sampler(top_k=50, top_p=0.9, seed=1)
        uni = RowSampler(SamplingParams(top_k=50, top_p=0.9, seed=1), "cuda", streams=list(range(B)))
        kinds = [SamplingParams(do_sample=False), SamplingParams(temperature=0.8, top_k=0), SamplingParams(top_k=50),
                 SamplingParams(top_k=50, top_p=0.9)]
        mix = RowSampler([kinds[b % 4] for b in range(B)], "cuda")
        assert torch.equal(old(logits), uni(logits)), "the uniform RowSampler has to draw kivi_sample's tokens"
        fns = [("kivi_sample", lambda: old(logits, out=out)), ("kivi_sample_rows", lambda: uni(logits, out=out)),
               ("kivi_sample_rows mixed", lambda: mix(logits, out=out))]
        replays = [_graph(fn, iters) for _, fn in fns]
        for _, fn in fns:
            for _ in range(3):
                fn()
        call, dev = [[] for _ in fns], [[] for _ in fns]
        for _ in range(rounds):
            for i, (_, fn) in enumerate(fns):
                call[i].append(_events(fn, iters))
            for i, rp in enumerate(replays):
                dev[i].append(_events(rp, 1) / iters)
        mc, md = [statistics.median(t) for t in call], [statistics.median(t) for t in dev]
        for i, (name, _) in enumerate(fns):
            ratio = "" if i == 0 else f"   / kivi_sample: call {mc[i] / mc[0]:5.2f}x  device {md[i] / md[0]:5.2f}x"
            lines.append(f"  B={B:3d} V={V:6d} fp16  {name:23s} call {mc[i]:7.1f} us (min {min(call[i]):7.1f})   device {md[i]:7.1f} us "
                         f"(min {min(dev[i]):7.1f}){ratio}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "V"), help="time this shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_rows_time.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_rows_time.py needs a GPU: nothing is timed without one")
    lines = [f"kivi_sample (top_k 50, top_p 0.9) vs kivi_sample_rows (the same parameters in every record; a mixed batch: greedy / "
             f"temperature only / top_k 50 / top_k 50 + top_p 0.9 by quarters), fp16 logits (B, V); median (min) of {args.rounds} "
             f"interleaved rounds of {args.iters} back-to-back calls between device events: eager calls (call time, Python dispatch "
             f"included) and the same calls replayed from one captured graph (device time)"]
    print(lines[0], flush=True)
    lines += rows(args.rounds, args.iters, [tuple(args.shape)] if args.shape else SHAPES)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
