"""Time the FP8 weight path; writes profiles/w8_time.log.  The twin of tools/w4_time.py.

    python tools/w8_time.py [--rounds N] [--tokens 1,8,...] [--skip-step] [--layers N] [--context T] [--out PATH]

(a) Per projection, fp16, at the shapes of Llama-2-7B (4096 -> 4096, 4096 -> 2 x 11008 fused gate / up, 11008 -> 4096) and of
    Llama-3-8B / Mistral-7B (4096 -> 1024, 4096 -> 2 x 14336, 14336 -> 4096), N in {1, 8, 32, 64, 96, 256, 1024} tokens:
      kernel      kivi_w8_linear, or kivi_w8_gate_up for the fused pair (writes silu(g) * u)
      fp16        F.linear on the dense fp16 weight -- what the model does without fp8_weights; the pair: two F.linear, silu, product
      dequant     kivi_w8_dequant into a scratch + F.linear (the pair: twice, then silu and the product): the path above kernel_max_tokens
      w4          kivi_w4_linear / kivi_w4_gate_up on the same shape at group 128, for the table
    A decode step reads every weight once, from HBM.  So that a repeated call does not find its weight in the 256 MiB last-level
    cache, each form walks `copies` distinct weights, enough for 512 MiB of FP8 bytes, inside one hipGraph of `copies` calls;
    device events around the replay, per call.  Forms alternate within every round, the first round is discarded, medians with
    p10 / p90.  floor = FP8 bytes / 8 TB/s.  The last lines name the crossover: the largest measured N at which the kernel beats
    dequant + F.linear on every shape, and every (shape, N <= 32) at which the kernel loses to fp16 F.linear.
(b) One graphed decode step of a Llama-2-7B-shaped model with random weights, B = 32 after a 2048-token prompt: fp8_weights off
    against on, weight_bits=4 beside them, alternating, host clock to a device synchronise over 50 steps; the bytes the weights take.
Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S = 8e12
GROUP, STEPS, B = 128, 50, 32
SHAPES = [("llama-2-7b q/k/v/o 4096->4096", 4096, 4096, False), ("llama-2-7b gate+up 4096->2x11008", 11008, 4096, True),
          ("llama-2-7b down 11008->4096", 4096, 11008, False), ("llama-3-8b k/v 4096->1024", 1024, 4096, False),
          ("llama-3-8b gate+up 4096->2x14336", 14336, 4096, True), ("llama-3-8b down 14336->4096", 4096, 14336, False)]


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def graphed(torch, calls):
    """calls: a list of callables -> a function that replays them all from one hipGraph and returns microseconds per call."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls[0]()
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        for f in calls:
            f()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cg.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / len(calls)
    return run


def projections(torch, args, out):
    import torch.nn.functional as F
    from kivi_amd import wfp8, wquant
    tokens = [int(t) for t in args.tokens.split(",")]
    beats = {n: True for n in tokens}
    behind_fp16 = []
    for name, O, K, pair in SHAPES:
        n_w = 2 if pair else 1
        packed = wfp8._lib.load().kivi_w8_bytes(O, K) * n_w
        copies = max(2, -(-(512 << 20) // packed))
        g = torch.Generator("cuda").manual_seed(O + K)
        dense, fp8, w4 = [], [], []
        for _ in range(copies):
            ws = [(torch.randn((O, K), device="cuda", generator=g) * 0.02).half() for _ in range(n_w)]
            dense.append(ws)
            fp8.append([tuple(t if t.dtype == torch.uint8 else t.view(torch.int32) for t in wfp8.quantize(w)) for w in ws])
            w4.append([wquant.pack(w, GROUP) for w in ws])
        scratch = [torch.empty((O, K), dtype=torch.float16, device="cuda") for _ in range(n_w)]
        floor = packed / HBM_BYTES_PER_S * 1e6
        out.append(f"{name}: O {O}, K {K}, {copies} weights per replay, FP8 {packed / 2 ** 20:.1f} MiB (fp16 {O * K * 2 * n_w / 2 ** 20:.1f} "
                   f"MiB), floor {floor:.1f} us")
        print(out[-1], flush=True)
        for N in tokens:
            x = torch.randn((N, K), device="cuda", generator=g).half()
            if pair:
                kern = [lambda q=q: wfp8.gate_up(x, q[0], q[1]) for q in fp8]
                fp16 = [lambda w=w: F.silu(F.linear(x, w[0])) * F.linear(x, w[1]) for w in dense]
                deq = [lambda q=q: F.silu(F.linear(x, wfp8.dequant(*q[0], out=scratch[0]))) * F.linear(x, wfp8.dequant(*q[1], out=scratch[1]))
                       for q in fp8]
                four = [lambda q=q: wquant.gate_up(x, q[0], q[1]) for q in w4]
            else:
                kern = [lambda q=q: wfp8.linear(x, *q[0]) for q in fp8]
                fp16 = [lambda w=w: F.linear(x, w[0]) for w in dense]
                deq = [lambda q=q: F.linear(x, wfp8.dequant(*q[0], out=scratch[0])) for q in fp8]
                four = [lambda q=q: wquant.linear(x, *q[0]) for q in w4]
            ref = fp16[0]().float()
            rms = ref.pow(2).mean().sqrt().item()
            agree = max((f().float() - ref).abs().max().item() / rms for f in (kern[0], deq[0]))      # FP8 against fp16: quantisation error
            forms = {"kernel": graphed(torch, kern), "fp16": graphed(torch, fp16), "dequant": graphed(torch, deq), "w4": graphed(torch, four)}
            times = {k: [] for k in forms}
            for r in range(args.rounds + 1):
                for k, f in forms.items():
                    t = f()
                    if r:
                        times[k].append(t)
            med = {k: statistics.median(v) for k, v in times.items()}
            beats[N] = beats[N] and med["kernel"] < med["dequant"]
            if N <= 32 and med["kernel"] >= med["fp16"]:
                behind_fp16.append(f"{name} at N {N} ({med['fp16'] / med['kernel']:.2f}x fp16, {floor / med['kernel']:.2f} of the floor)")
            out.append(f"  N {N:5d}: " + " | ".join(f"{k} {med[k]:8.1f} (p10 {pct(times[k], 0.1):.1f}, p90 {pct(times[k], 0.9):.1f})" for k in forms)
                       + f" | kernel reaches {floor / med['kernel']:.2f} of the floor, {med['fp16'] / med['kernel']:.2f}x fp16, "
                       f"{med['dequant'] / med['kernel']:.2f}x dequant, {med['w4'] / med['kernel']:.2f}x w4 | |FP8 - fp16| / rms {agree:.3g}")
            print(out[-1], flush=True)
        del dense, fp8, w4, scratch
        torch.cuda.empty_cache()
    ahead = [n for n in tokens if beats[n]]
    out.append(f"crossover: the kernel beats dequant + F.linear on every shape at N in {ahead}; the largest such N below the first N at "
               f"which it loses on some shape: {max([n for n in ahead if all(beats[m] for m in tokens if m <= n)], default=0)}")
    print(out[-1], flush=True)
    out.append("behind fp16 F.linear at N <= 32: " + ("; ".join(behind_fp16) if behind_fp16 else "nowhere"))
    print(out[-1], flush=True)


def step(torch, args, out):
    from kivi_amd import wfp8, wquant
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    geo = dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, intermediate_size=11008, num_hidden_layers=args.layers,
               vocab_size=32000)
    T = args.context
    ids = torch.randint(0, 32000, (B, T), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    models = {}
    for name, kw in (("fp8_weights=False", {}), ("fp8_weights=True", dict(fp8_weights=True)),
                     ("weight_bits=4", dict(weight_bits=4, weight_group=GROUP))):
        torch.manual_seed(0)
        torch.set_default_dtype(torch.float16)
        with torch.device("cuda"):
            model = LlamaForCausalLM_KIVI(make_config(geo, residual_length=32, **kw))
        torch.set_default_dtype(torch.float32)
        for p in model.parameters():
            if p.dim() > 1:
                p.data.normal_(0.0, 0.02)
        for m in model.modules():                               # one dense weight at a time: the fp16 model never exists beside it
            if isinstance(m, wquant.QuantLinear):
                m.pack_((torch.randn((m.out_features, m.in_features), device="cuda") * 0.02).half())
            elif isinstance(m, wfp8.Fp8Linear):
                m.quantize_((torch.randn((m.out_features, m.in_features), device="cuda") * 0.02).half())
        models[name] = model.eval()
        tensors = list(model.parameters()) + list(model.buffers())
        total = sum(t.numel() * t.element_size() for t in tensors)
        layers = sum(t.numel() * t.element_size() for t in list(model.model.layers.parameters()) + list(model.model.layers.buffers()))
        out.append(f"  {name}: weights {total / 1e9:.2f} GB on the device, {layers / 1e9:.2f} GB of them in the decoder layers")
        print(out[-1], flush=True)

    def run(model):
        logits, pasts = model(ids)
        tok = logits.argmax(-1)
        model.decode_graphed(tok, pasts, T, 8)
        tok = model.graphs.tok.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.decode_graphed(tok, pasts, T + 8, STEPS)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert model.graphs.whole
        model.graphs.end()
        del pasts
        torch.cuda.empty_cache()
        return dt * 1e3 / STEPS
    times = {k: [] for k in models}
    for r in range(args.step_rounds + 1):
        for k, m in models.items():
            t = run(m)
            if r:
                times[k].append(t)
    for k, v in times.items():
        out.append(f"  {k}: one decode step {statistics.median(v):7.3f} ms (min {min(v):.3f}, max {max(v):.3f} over {len(v)} runs of {STEPS} steps)")
        print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--tokens", default="1,8,32,64,96,256,1024")
    ap.add_argument("--skip-step", action="store_true", help="leave part (b) out")
    ap.add_argument("--skip-projections", action="store_true", help="leave part (a) out")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--context", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w8_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("w8_time.py needs a GPU: nothing is timed without one")
    out = [f"FP8 weights on {torch.cuda.get_device_name(0)}: fp16 activations, [128, 128] blocks; {args.rounds} alternating rounds (one "
           f"more, the first, discarded)"]
    if not args.skip_projections:
        out.append("(a) one projection call, microseconds per call: hipGraph over distinct weights, device events")
        with torch.no_grad():
            projections(torch, args, out)
    if not args.skip_step:
        out.append(f"(b) one decode step of a Llama-2-7B-shaped model ({args.layers} layers, random weights), B = {B} after a "
                   f"{args.context}-token prompt; decode_graphed (whole-step hipGraph), host clock to a device synchronise, milliseconds")
        step(torch, args, out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
