"""Time the fused log-prob kernel (kivi_token_logprob) against the torch composition; writes profiles/score_time.log.

    python tools/score_time.py [--rounds N] [--iters N] [--shape N V] [--out PATH]

kivi_amd.scoring.token_logprobs against torch.log_softmax(logits.float(), -1).gather(-1, targets) on the same fp16 logits, for
(N, V) in {(4096, 32000), (4096, 128256), (32, 32000)}: the slab of a prefill score at both vocabulary sizes, and a decode step's
(B, V).  Each round times `iters` back-to-back calls of each with device events; rounds interleave the two.  Medians and minimums
over the rounds.  These are CALL times: the Python dispatch of each call is inside the window (it hides behind the device work at
N = 4096 and is most of the figure at N = 32).  The share of the HBM peak is taken from them: the bytes the algorithm needs (the
logits once -- the second sweep of a row is meant to hit the caches -- plus targets and outputs) over the call time, over HBM_PEAK
(the measured streaming-read rate of the chip, 6.29 TB/s).  For the kernel's own time run one shape under a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/score_time.py --shape 4096 32000 --rounds 2
and read token_logprob_kernel's average in DIR's kernel statistics."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 32000), (4096, 128256), (32, 32000)]
HBM_PEAK = 6.29e12


def composition(logits, targets):
    return torch.log_softmax(logits.float(), -1).gather(-1, targets.unsqueeze(-1)).squeeze(-1)


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def rows(rounds, iters, shapes):
    from kivi_amd.scoring import token_logprobs
    lines = []
    for N, V in shapes:
        gen = torch.Generator("cuda").manual_seed(N + V)
        logits = (torch.randn((N, V), device="cuda", generator=gen) * 3).half()
        targets = torch.randint(0, V, (N,), device="cuda", generator=gen)
        fused = lambda: token_logprobs(logits, targets)               # noqa: E731
        ref = lambda: composition(logits, targets)                    # noqa: E731
        err = (fused() - ref()).abs().max().item()
        for _ in range(3):
            fused(), ref()
        tf, tr = [], []
        for _ in range(rounds):
            tf.append(_events(fused, iters))
            tr.append(_events(ref, iters))
        mf, mr = statistics.median(tf), statistics.median(tr)
        need = N * V * 2 + N * (8 + 4)
        lines.append(f"  N={N:5d} V={V:6d} fp16   kivi_token_logprob {mf:9.1f} us (min {min(tf):9.1f})  {need / mf * 1e-6:6.2f} TB/s = "
                     f"{need / (mf * 1e-6) / HBM_PEAK * 100:5.1f}% of HBM peak   torch log_softmax + gather {mr:9.1f} us "
                     f"(min {min(tr):9.1f})   {mr / mf:5.2f}x   max |difference| {err:.2e}")
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("N", "V"), help="time this shape only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_time.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_time.py needs a GPU: nothing is timed without one")
    lines = [f"kivi_token_logprob vs torch.log_softmax(logits.float(), -1).gather, fp16 logits (N, V); median (min) of {args.rounds} "
             f"interleaved rounds of {args.iters} back-to-back calls, device events around the calls (call time, Python dispatch included); "
             f"share of HBM peak = (N * V * 2 + 12 N bytes) / call time / {HBM_PEAK / 1e12:.2f} TB/s"]
    print(lines[0], flush=True)
    lines += rows(args.rounds, args.iters, [tuple(args.shape)] if args.shape else SHAPES)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
