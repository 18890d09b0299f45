"""Time one call of the sparse expert block over FP8 experts; writes profiles/moe_w8_time.log.

    python tools/moe_w8_time.py [--rounds N] [--tokens 1,8,32,...] [--dtypes fp16,bf16] [--out PATH]

One block call -- router GEMM, route, experts -- at the Mixtral-8x7B geometry (H 4096, I 14336, 8 experts, 2 per token; 1.4 GB of FP8
bytes) and the Qwen3-30B-A3B one (H 2048, I 768, 128 experts, 8 per token, weights rounded; 0.6 GB): neither fits the last-level
cache.  N in {1, 8, 32, 64, 256} tokens, random bytes over the 254 finite codes, block scales near 2^-11.  Three forms in the same
run, alternating within every round, the first round discarded, device events around each call, medians with p10 / p90:
  w8      kivi_moe_route + kivi_moe_experts_w8 over the FP8 buffers (moe.route / moe.experts_w8)
  fp16    kivi_moe_route + kivi_moe_experts over the 16-bit stacks that hold `dequant` of the same bytes (moe.experts)
  loop    the dequantising loop (moe.route_torch / moe.experts_w8_torch; nonzero / where synchronise)
Before timing, w8 and the loop are held to the fp16 kernels' result (max |delta| relative to its rms).  Printed beside each w8 time:
the floor, FP8 bytes of the ACTIVE experts (3 H I per expert that received a pair) / 8 TB/s, and the fraction of it reached.  The
last lines state the crossover against the loop, the rule kivi_amd.moe.FP8_KERNEL_MAX_TOKENS is set by.  Needs a GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tokens", default="1,8,32,64,256")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_w8_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("moe_w8_time.py needs a GPU: nothing is timed without one")
    from kivi_amd import moe
    tokens = [int(t) for t in args.tokens.split(",")]
    dtypes = [dict(fp16=torch.float16, bf16=torch.bfloat16)[d] for d in args.dtypes.split(",")]
    out = [f"one sparse expert block call over FP8 experts on {torch.cuda.get_device_name(0)}: {args.rounds} alternating rounds (one "
           f"more, the first, discarded); device events, microseconds; floor = FP8 bytes of the active experts / 8 TB/s"]
    ahead = {}                      # N -> [loop / w8 of every (geometry, dtype)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for name, geo in GEOMETRIES.items():
        H, I, E, K = geo["H"], geo["I"], geo["E"], geo["K"]
        g = torch.Generator("cuda").manual_seed(0)
        fp8 = moe.Fp8Experts(E, H, I).cuda()
        finite = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8, device="cuda")
        for e in range(E):          # expert by expert: no wide copy of the whole stack
            fp8.gate_up_proj[e] = finite[torch.randint(0, 254, (2 * I, H), device="cuda", generator=g)]
            fp8.down_proj[e] = finite[torch.randint(0, 254, (H, I), device="cuda", generator=g)]
        for buf in (fp8.gate_up_proj_scale_inv, fp8.down_proj_scale_inv):
            buf.copy_(((0.5 + torch.rand(buf.shape, device="cuda", generator=g)) * 2.0 ** -11).view(torch.int32))
        for dtype in dtypes:
            gate_w = (torch.randn((E, H), device="cuda", generator=g) * 0.05).to(dtype)
            gate_up = torch.empty((E, 2 * I, H), device="cuda", dtype=dtype)
            down = torch.empty((E, H, I), device="cuda", dtype=dtype)
            for e in range(E):
                fp8.dequant_expert(e, dtype, (gate_up[e], down[e]))
            out.append(f"{name} (H {H}, I {I}, E {E}, K {K}), {str(dtype).split('.')[-1]}")
            for N in tokens:
                x = torch.randn((N, H), device="cuda", generator=g).to(dtype)

                def w8():
                    logits = torch.nn.functional.linear(x, gate_w)
                    return moe.experts_w8(x, moe.route(logits, K, geo["norm"], geo["rnd"]), fp8)

                def fp16():
                    logits = torch.nn.functional.linear(x, gate_w)
                    return moe.experts(x, moe.route(logits, K, geo["norm"], geo["rnd"]), gate_up, down)

                def loop():
                    logits = torch.nn.functional.linear(x, gate_w)
                    return moe.experts_w8_torch(x, moe.route_torch(logits, K, geo["norm"], geo["rnd"]), fp8)
                forms = {"w8": w8, "fp16": fp16, "loop": loop}
                res = {k: f() for k, f in forms.items()}
                ref = res["fp16"].float()
                rms = ref.pow(2).mean().sqrt().item()
                agree = ", ".join(f"|{k} - fp16| {((v.float() - ref).abs().max().item() / rms):.3g}" for k, v in res.items() if k != "fp16")
                bar = 0.02 if dtype == torch.float16 else 0.16           # a few roundings of the dtype on sums of K terms
                ok = all((v.float() - ref).abs().max().item() / rms <= bar for v in res.values())
                active = int(torch.unique(moe.route_torch(torch.nn.functional.linear(x, gate_w), K).idx).numel())
                floor = active * 3 * H * I / HBM_BYTES_PER_S * 1e6
                del res, ref
                times = {k: [] for k in forms}
                for r in range(args.rounds + 1):
                    for k, f in forms.items():
                        t = timed(f)
                        if r:
                            times[k].append(t)
                med = {k: statistics.median(v) for k, v in times.items()}
                ahead.setdefault(N, []).append(med["loop"] / med["w8"])
                out.append(f"  N {N:5d}: {active:3d} active experts, floor {floor:8.1f} us | " + " | ".join(
                    f"{k} {med[k]:9.1f} (p10 {pct(times[k], 0.1):.1f}, p90 {pct(times[k], 0.9):.1f})" for k in forms)
                    + f" | w8 reaches {floor / med['w8']:.2f} of the floor, {med['fp16'] / med['w8']:.2f}x fp16, {med['loop'] / med['w8']:.2f}x "
                      f"loop | agree: {agree}{'' if ok else '  <-- DISAGREE'}")
                print(out[-1], flush=True)
                torch.cuda.empty_cache()
            del gate_up, down
            torch.cuda.empty_cache()
        del fp8
        torch.cuda.empty_cache()
    wins = [n for n in sorted(ahead) if min(ahead[n]) >= 1.0]
    first_loss = next((n for n in sorted(ahead) if min(ahead[n]) < 1.0), None)
    below = [n for n in wins if first_loss is None or n < first_loss]
    out.append(f"crossover: w8 is no slower than the dequantising loop at both geometries (every dtype run) at N in {wins}; the largest "
               f"such N below the first N at which it loses somewhere ({first_loss}): {max(below) if below else None}; worst loop / w8 per N: "
               + ", ".join(f"{n}: {min(ahead[n]):.2f}" for n in sorted(ahead)))
    print(out[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
