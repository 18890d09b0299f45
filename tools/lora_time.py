"""Time the LoRA side path of one linear; writes profiles/lora_time.log.

    python tools/lora_time.py [--rounds N] [--tokens 1,8,32,...] [--out PATH]

The two launches kivi_lora_shrink + kivi_lora_expand (lora.apply_kernels) against lora.apply_torch -- rows selected per distinct slot
on the host, two fp32 matmuls per slot -- at the shapes 4096 -> 4096 and 11008 -> 4096 (Llama-2-7B's attention projections and its
down_proj), r = 16 in tables of rank 16, with one and with four distinct adapters spread round-robin over the rows, N in
{1, 8, 32, 64, 128, 256, 1024} rows of one token, fp16 and bf16.  Both forms in the same run, alternating within every round, the first
round discarded, device events around each call, medians with p10 / p90.  Before timing the two are held to each other within twice
the contract's bound (tests/lora_ref.py).  Printed beside each kernel time: the floor, the bytes the launches must move (the
adapters' tables once per token, x, t, y twice) / 8 TB/s.  The last line names the largest measured power of two at which the
launches are no slower than apply_torch at both shapes, both dtypes and both adapter counts: lora.LORA_KERNEL_MAX_TOKENS.
The graphed decode step with and without adapters (section 34, "Open") is not timed here.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8e12
SHAPES = {"4096 -> 4096": (4096, 4096), "11008 -> 4096": (11008, 4096)}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--tokens", default="1,8,32,64,128,256,1024")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lora_time.py needs a GPU: nothing is timed without one")
    import lora_ref as R
    from kivi_amd import lora
    tokens = [int(t) for t in args.tokens.split(",")]
    dtypes = [dict(fp16=torch.float16, bf16=torch.bfloat16)[d] for d in args.dtypes.split(",")]
    r = Rk = 16
    out = [f"the LoRA side path of one linear on {torch.cuda.get_device_name(0)}: r = {r}, {args.rounds} alternating rounds (one more, the "
           f"first, discarded); device events, microseconds; floor = bytes moved / 8 TB/s"]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    ahead = {n: True for n in tokens}
    for name, (K, O) in SHAPES.items():
        for dtype in dtypes:
            for n_adapters in (1, 4):
                A, B, scale, ranks = R.tables(4, Rk, K, O, (r,) * 4, dtype, "cuda", K + n_adapters)
                out.append(f"{name}, {str(dtype).split('.')[-1]}, {n_adapters} distinct adapter(s)")
                for N in tokens:
                    g = torch.Generator().manual_seed(N)
                    x = torch.randn((N, 1, K), generator=g).to(dtype).cuda()
                    y0 = torch.randn((N, 1, O), generator=g).to(dtype).cuda()
                    host = [b % n_adapters for b in range(N)]
                    slots = torch.tensor(host, dtype=torch.int32, device="cuda")
                    sc, rk = scale.tolist(), ranks.tolist()
                    y = y0.clone()
                    forms = {"kernels": lambda: lora.apply_kernels(y, x, A, B, scale, ranks, slots),
                             "apply_torch": lambda: lora.apply_torch(y, x, A, B, sc, rk, host)}
                    got = lora.apply_kernels(y0.clone(), x, A, B, scale, ranks, slots)
                    ref = lora.apply_torch(y0.clone(), x, A, B, sc, rk, host)
                    y64, mag = R.statement64(y0, x, A, B, scale, host)
                    agree = R.worst_ratio(got, y0, ref.double().cpu(), mag, K, Rk, dtype, factor=2.0)
                    floor = (N * Rk * (K + O) * 2 + N * (K + 2 * O) * 2 + 2 * N * Rk * 4) / HBM_BYTES_PER_S * 1e6
                    times = {k: [] for k in forms}
                    for rnd in range(args.rounds + 1):
                        for k, f in forms.items():
                            t = timed(f)
                            if rnd:
                                times[k].append(t)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    ahead[N] = ahead[N] and med["kernels"] <= med["apply_torch"]
                    out.append(f"  N {N:5d}: floor {floor:7.2f} us | " + " | ".join(
                        f"{k} {med[k]:8.1f} (p10 {pct(times[k], 0.1):.1f}, p90 {pct(times[k], 0.9):.1f})" for k in forms)
                        + f" | apply_torch / kernels {med['apply_torch'] / med['kernels']:.2f}x | |kernels - apply_torch| / (2 bound) "
                        f"{agree:.3g}{'' if agree <= 1.0 else '  <-- DISAGREE'}")
                    print(out[-1], flush=True)
    pow2 = [n for n in tokens if n & (n - 1) == 0]
    best = max((n for n in pow2 if all(ahead[m] for m in tokens if m <= n)), default=0)
    out.append(f"crossover: the launches are no slower than apply_torch at every shape, dtype and adapter count up to N = {best} "
               f"(measured N: {tokens}; no slower at {[n for n in tokens if ahead[n]]})")
    print(out[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
