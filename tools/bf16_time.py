"""Time the bf16 boundary and the bf16 logits path; writes profiles/bf16_time.log.

    python tools/bf16_time.py [--rounds N] [--context T] [--layers N] [--skip-models] [--out PATH]

(a) One layer's way into the attention at B = 32, one decode step: kivi_qkv_rope_bf16 (bf16 projections -> fp16 q / k / v, one
    launch) against what an fp16 model pays for the same tensors, kivi_qk_rope plus the copy of v into its static buffer, at the head
    counts of Llama-3-8B (32 / 8, no norm, no padding) and Qwen3-14B (40 / 8, head norm, groups of 5 padded to 8).  Two clocks:
    `eager`, a host clock around 200 calls ending in a device synchronise, and `graph`, the same 200 calls captured in one hipGraph
    and replayed.
(b) kivi_sample_rows (top-k 50, top-p 0.9, temperature 0.8) and kivi_token_top_logprobs (k = 5) on a (32, 151936) row block: bf16,
    fp16, and fp32 after a .float() copy of the bf16 block that is part of the measured time.  Graph clock, 50 calls per replay.
(c) One decode_graphed step of `--layers` layers of the Qwen2.5-7B geometry (ratio 7, padded to 8, whole-step graph) with random
    weights, B = 32 after a `--context`-token prompt: the model in bf16 against the model in fp16.
Forms alternate within every round; the first round is discarded; medians with p10 / p90.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, D, CALLS, LOGIT_CALLS, STEPS, V = 32, 128, 200, 50, 50, 151936


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def line(name, xs, unit="us"):
    return f"  {name:44s} median {statistics.median(xs):9.2f}  p10 {pct(xs, 0.1):9.2f}  p90 {pct(xs, 0.9):9.2f} {unit}"


def rounds(forms, n):
    """forms: name -> callable returning one measurement.  Alternating, round 0 discarded."""
    times = {k: [] for k in forms}
    for r in range(n + 1):
        for k, f in forms.items():
            t = f()
            if r:
                times[k].append(t)
    return times


def eager(torch, fn, calls):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls
    return run


def graphed(torch, fn, calls):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        for _ in range(calls):
            fn()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        cg.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / calls
    return run


def boundary_forms(torch, nh, nh_kv, norm, rp):
    from kivi_amd.qkrope import qk_rope, qkv_rope_bf16
    g = torch.Generator("cuda").manual_seed(0)
    width = (nh + 2 * nh_kv) * D
    proj = torch.randn((B, 1, width), device="cuda", generator=g)
    ang = torch.rand((1, 1, D), device="cuda", generator=g) * 6
    w = [(1 + 0.1 * torch.randn(D, device="cuda", generator=g)) for _ in range(2)] if norm else [None, None]
    q_out = torch.empty((B, nh_kv * rp, 1, D), dtype=torch.float16, device="cuda")
    k_out, v_out = (torch.empty((B, nh_kv, 1, D), dtype=torch.float16, device="cuda") for _ in range(2))

    def views(t):
        q, k, v = t.split([nh * D, nh_kv * D, nh_kv * D], dim=-1)
        return q.unflatten(-1, (nh, D)), k.unflatten(-1, (nh_kv, D)), v.unflatten(-1, (nh_kv, D))
    qb, kb, vb = views(proj.bfloat16())
    qh, kh, vh = views(proj.half())
    cos32, sin32 = ang.cos(), ang.sin()
    cos16, sin16 = cos32.half(), sin32.half()
    wb = [None if t is None else t.bfloat16() for t in w]
    wh = [None if t is None else t.half() for t in w]

    def bf16():
        qkv_rope_bf16(qb, kb, vb, cos32, sin32, rp, wb[0], wb[1], 1e-6, q_out, k_out, v_out)

    def fp16():                                     # graph.py's pre() of an fp16 model with the option on
        v_out.copy_(vh.transpose(1, 2))
        qk_rope(qh, kh, cos16, sin16, rp, wh[0], wh[1], 1e-6, q_out, k_out)
    return {"fp16: kivi_qk_rope + v copy, eager": eager(torch, fp16, CALLS), "bf16: kivi_qkv_rope_bf16, eager": eager(torch, bf16, CALLS),
            "fp16: kivi_qk_rope + v copy, graph": graphed(torch, fp16, CALLS), "bf16: kivi_qkv_rope_bf16, graph": graphed(torch, bf16, CALLS)}


def logits_forms(torch):
    from kivi_amd.sampling import RowSampler, SamplingParams
    from kivi_amd.scoring import score_into
    g = torch.Generator("cuda").manual_seed(1)
    x = torch.randn((B, 1, V), device="cuda", generator=g) * 4
    xb, xh = x.bfloat16(), x.half()
    rs = RowSampler([SamplingParams(temperature=0.8, top_k=50, top_p=0.9, seed=5 + i) for i in range(B)], "cuda")
    tok = torch.zeros((B, 1), dtype=torch.long, device="cuda")
    lp = torch.zeros((B, 1), dtype=torch.float32, device="cuda")
    ids, top = torch.zeros((B, 1, 5), dtype=torch.long, device="cuda"), torch.zeros((B, 1, 5), dtype=torch.float32, device="cuda")
    forms = {}
    for name, fn in (("kivi_sample_rows", lambda t: rs(t, out=tok)), ("kivi_token_top_logprobs k=5", lambda t: score_into(t, tok, lp, ids, top))):
        forms[f"{name}, bf16"] = graphed(torch, lambda fn=fn: fn(xb), LOGIT_CALLS)
        forms[f"{name}, fp16"] = graphed(torch, lambda fn=fn: fn(xh), LOGIT_CALLS)
        forms[f"{name}, bf16 -> .float() -> fp32"] = graphed(torch, lambda fn=fn: fn(xb.float()), LOGIT_CALLS)
    return forms


GEOMETRY = dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944)


def model_forms(torch, T, layers):
    from kivi_amd.llama import Qwen2ForCausalLM_KIVI, make_config
    geo = dict(GEOMETRY, num_hidden_layers=layers, vocab_size=32000, head_dim=128)
    ids = torch.randint(0, 32000, (B, T), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    forms = {}
    for name, dt in (("fp16 model", torch.float16), ("bf16 model", torch.bfloat16)):
        cfg = make_config(geo, residual_length=128, qk_kernel=True)
        torch.manual_seed(0)
        torch.set_default_dtype(dt)
        with torch.device("cuda"):
            model = Qwen2ForCausalLM_KIVI(cfg)
        torch.set_default_dtype(torch.float32)
        for p in model.parameters():
            if p.dim() > 1:
                p.data.normal_(0.0, 0.02)

        def run(model=model):
            logits, pasts = model(ids)
            tok = logits.argmax(-1)
            model.decode_graphed(tok, pasts, T, 8)
            tok = model.graphs.tok.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.decode_graphed(tok, pasts, T + 8, STEPS)
            torch.cuda.synchronize()
            dt_ = time.perf_counter() - t0
            assert model.graphs.whole
            model.graphs.end()
            del pasts
            return dt_ * 1e6 / STEPS
        forms[f"{name} (ratio 7 padded to 8, whole-step graph)"] = run
    return forms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--skip-models", action="store_true", help="leave part (c) out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bf16_time.py needs a GPU: nothing is timed without one")
    out = [f"bf16 boundary and bf16 logits on {torch.cuda.get_device_name(0)}: B={B}, {args.rounds} alternating rounds "
           f"(one more, the first, discarded); microseconds"]
    for title, nh, nh_kv, norm, rp in (("Llama-3-8B heads (32 / 8), RoPE", 32, 8, False, 4),
                                       ("Qwen3-14B heads (40 / 8), head norm + RoPE + pad to 8", 40, 8, True, 8)):
        out.append(f"(a) q / k / v of one layer of a decode step made ready for the attention, {title}; per call, {CALLS} calls per "
                   f"measurement")
        out += [line(k, v) for k, v in rounds(boundary_forms(torch, nh, nh_kv, norm, rp), args.rounds).items()]
    out.append(f"(b) one call on a ({B}, {V}) row block; hipGraph of {LOGIT_CALLS} calls, device events, per call")
    out += [line(k, v) for k, v in rounds(logits_forms(torch), args.rounds).items()]
    torch.cuda.empty_cache()
    if not args.skip_models:
        out.append(f"(c) one decode step of {args.layers} layers, hidden {GEOMETRY['hidden_size']}, {GEOMETRY['num_key_value_heads']} kv "
                   f"heads, random weights, after a {args.context}-token prompt; decode_graphed, host clock to a device synchronise over "
                   f"{STEPS} steps, per step")
        out += [line(k, v) for k, v in rounds(model_forms(torch, args.context, args.layers), max(3, args.rounds // 2)).items()]
    print("\n".join(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
