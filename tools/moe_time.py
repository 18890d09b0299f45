"""Time one call of the sparse expert block; writes profiles/moe_time.log.

    python tools/moe_time.py [--rounds N] [--tokens 1,8,32,...] [--out PATH]

One SparseMoeBlock call -- router GEMM, route, experts -- at the Mixtral-8x7B geometry (H 4096, I 14336, 8 experts, 2 per token) and
the Qwen3-30B-A3B one (H 2048, I 768, 128 experts, 8 per token, weights rounded), N in {1, 8, 32, 64, 256, 1024} tokens, fp16 and
bf16, random weights.  Three forms in the same run, alternating within every round, the first round discarded, device events around
each call, medians with p10 / p90:
  kernels   kivi_moe_route + kivi_moe_experts (moe.route / moe.experts)
  (a) loop  the HF-style per-expert loop (moe.route_torch / moe.experts_torch; nonzero / where synchronise)
  (b) bmm   the sync-free composition: gather K whole expert matrices per token (gate_up[idx], down[idx]) and multiply with bmm;
            left out where its temporaries would pass --bmm-limit-gib
Before timing, the three forms are held to each other: max |delta| of the outputs relative to the rms of the fp32-accumulated (b)
or (a) result.  Printed beside each kernel time: the floor, bytes of the ACTIVE experts' weights (3 H I elements per expert that
received a pair) / 8 TB/s, and the fraction of it reached.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
GEOMETRIES = {"Mixtral-8x7B": dict(H=4096, I=14336, E=8, K=2, norm=True, rnd=False),
              "Qwen3-30B-A3B": dict(H=2048, I=768, E=128, K=8, norm=True, rnd=True)}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def bmm_form(torch, x, logits, gate_up, down, K, norm, rnd):
    """out[n] = sum_k w[n, k] * down[e] (silu(gate[e] x[n]) * up[e] x[n]) with the experts' matrices gathered per pair."""
    from kivi_amd import moe
    plan = moe.route_torch(logits, K, norm, rnd)
    idx = plan.idx.long()
    N, H = x.shape
    I = down.shape[2]
    gu = torch.bmm(gate_up[idx.reshape(-1)], x.repeat_interleave(K, 0).unsqueeze(-1)).squeeze(-1)        # (N K, 2 I)
    a = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
    y = torch.bmm(down[idx.reshape(-1)], a.unsqueeze(-1)).squeeze(-1).view(N, K, H)
    return (y.float() * plan.w[..., None]).sum(1).to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", default="1,8,32,64,256,1024")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--bmm-limit-gib", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("moe_time.py needs a GPU: nothing is timed without one")
    from kivi_amd import moe
    tokens = [int(t) for t in args.tokens.split(",")]
    dtypes = [dict(fp16=torch.float16, bf16=torch.bfloat16)[d] for d in args.dtypes.split(",")]
    out = [f"one sparse expert block call on {torch.cuda.get_device_name(0)}: {args.rounds} alternating rounds (one more, the first, "
           f"discarded); device events, microseconds; floor = bytes of the active experts' weights / 8 TB/s"]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for name, geo in GEOMETRIES.items():
        H, I, E, K = geo["H"], geo["I"], geo["E"], geo["K"]
        for dtype in dtypes:
            g = torch.Generator("cuda").manual_seed(0)
            gate_w = (torch.randn((E, H), device="cuda", generator=g) * 0.05).to(dtype)
            gate_up = torch.empty((E, 2 * I, H), device="cuda", dtype=dtype)
            down = torch.empty((E, H, I), device="cuda", dtype=dtype)
            for e in range(E):                                      # expert by expert: no fp32 copy of the whole stack
                gate_up[e] = (torch.randn((2 * I, H), device="cuda", generator=g) * 0.02).to(dtype)
                down[e] = (torch.randn((H, I), device="cuda", generator=g) * 0.02).to(dtype)
            out.append(f"{name} (H {H}, I {I}, E {E}, K {K}), {str(dtype).split('.')[-1]}")
            for N in tokens:
                x = torch.randn((N, H), device="cuda", generator=g).to(dtype)

                def kernels():
                    logits = torch.nn.functional.linear(x, gate_w)
                    return moe.experts(x, moe.route(logits, K, geo["norm"], geo["rnd"]), gate_up, down)

                def loop():
                    logits = torch.nn.functional.linear(x, gate_w)
                    return moe.experts_torch(x, moe.route_torch(logits, K, geo["norm"], geo["rnd"]), gate_up, down)

                def bmm():
                    return bmm_form(torch, x, torch.nn.functional.linear(x, gate_w), gate_up, down, K, geo["norm"], geo["rnd"])
                forms = {"kernels": kernels, "(a) loop": loop}
                if N * K * 3 * H * I * 2 <= args.bmm_limit_gib * 2 ** 30:
                    forms["(b) bmm"] = bmm
                res = {k: f() for k, f in forms.items()}
                ref = res["(b) bmm" if "(b) bmm" in res else "(a) loop"].float()
                rms = ref.pow(2).mean().sqrt().item()
                agree = ", ".join(f"|{k} - ref| {((v.float() - ref).abs().max().item() / rms):.3g}" for k, v in res.items())
                bar = 0.02 if dtype == torch.float16 else 0.16           # a few roundings of the dtype on sums of K terms
                ok = all((v.float() - ref).abs().max().item() / rms <= bar for v in res.values())
                active = int(torch.unique(moe.route_torch(torch.nn.functional.linear(x, gate_w), K).idx).numel())
                floor = active * 3 * H * I * 2 / HBM_BYTES_PER_S * 1e6
                del res, ref
                times = {k: [] for k in forms}
                for r in range(args.rounds + 1):
                    for k, f in forms.items():
                        t = timed(f)
                        if r:
                            times[k].append(t)
                med = {k: statistics.median(v) for k, v in times.items()}
                out.append(f"  N {N:5d}: {active:3d} active experts, floor {floor:8.1f} us | " + " | ".join(
                    f"{k} {med[k]:9.1f} (p10 {pct(times[k], 0.1):.1f}, p90 {pct(times[k], 0.9):.1f})" for k in forms)
                    + f" | kernels reach {floor / med['kernels']:.2f} of the floor, {med['(a) loop'] / med['kernels']:.2f}x (a)"
                    + ("" if "(b) bmm" in forms else " | (b) left out: temporaries past the limit")
                    + f" | agree: {agree}{'' if ok else '  <-- DISAGREE'}")
                print(out[-1], flush=True)
                torch.cuda.empty_cache()
            del gate_up, down
            torch.cuda.empty_cache()
    print("\n".join(out[:1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
