"""Time kivi_qk_rope and the padded query groups; writes profiles/qk_rope_time.log.

    python tools/qk_rope_time.py [--rounds N] [--context T] [--layers N] [--out PATH]

(a) The per-layer q / k preparation of a decode step at B = 32, from the projections' outputs to q (B, heads, 1, D) and k: the torch
    chain the attention modules run without the option (`t * cos + rotate_half(t) * sin` twice; with a head norm its chain in front)
    against one kivi_qk_rope launch, at the head counts of Llama-3-8B (32 / 8, no norm, no padding) and Qwen3-14B (40 / 8, head norm,
    groups of 5 padded to 8).  Two clocks: `eager`, a host clock around 200 calls ending in a device synchronise (what a step pays
    when the host is the slower side), and `graph`, the same 200 calls captured in one hipGraph and replayed (what the GPU needs).
(b) The attention of one decode step of one layer, B = 32 over `--context` cached tokens (kivi_attention_decode, 2 bits, group 32,
    residual 128): a group ratio of 7 (28 / 4 heads, Qwen2.5-7B) and of 5 (40 / 8, Qwen2.5-14B) on the matrix-pipe layout padded to
    8, on the hook-state layout, and a true ratio-8 cache of the same kv heads.  Device events around 50 steps.
(c) One whole decode step of `--layers` layers of the Qwen2.5-7B (ratio 7) and Qwen2.5-14B (ratio 5) geometries with random weights,
    B = 32 after a `--context`-token prompt, through decode_graphed: qk_kernel on (padded matrix-pipe caches, whole-step graph)
    against off (hook-state caches, per-layer graphs), and a Llama-shaped model of the same widths with nh = 8 nh_kv.
Forms alternate within every round; the first round is discarded; medians with p10 / p90.  Needs a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, D, CALLS, STEPS = 32, 128, 200, 50


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def line(name, xs, unit="us"):
    return f"  {name:34s} median {statistics.median(xs):9.2f}  p10 {pct(xs, 0.1):9.2f}  p90 {pct(xs, 0.9):9.2f} {unit}"


def rounds(forms, n):
    """forms: name -> callable returning one measurement.  Alternating, round 0 discarded."""
    times = {k: [] for k in forms}
    for r in range(n + 1):
        for k, f in forms.items():
            t = f()
            if r:
                times[k].append(t)
    return times


def prep_forms(torch, nh, nh_kv, norm, rp):
    from kivi_amd.qkrope import qk_rope, qk_rope_torch
    g = torch.Generator("cuda").manual_seed(0)
    q_in = torch.randn((B, 1, nh * D), device="cuda", generator=g).half().view(B, 1, nh, D)
    k_in = torch.randn((B, 1, nh_kv * D), device="cuda", generator=g).half().view(B, 1, nh_kv, D)
    ang = torch.rand((1, 1, D), device="cuda", generator=g) * 6
    cos, sin = ang.cos().half(), ang.sin().half()
    qw = kw = None
    if norm:
        qw, kw = (1 + 0.1 * torch.randn(D, device="cuda", generator=g)).half(), (1 + 0.1 * torch.randn(D, device="cuda", generator=g)).half()
    q_out = torch.empty((B, nh_kv * rp, 1, D), dtype=torch.float16, device="cuda")
    k_out = torch.empty((B, nh_kv, 1, D), dtype=torch.float16, device="cuda")
    q_dst, k_dst = torch.empty((B, nh, 1, D), dtype=torch.float16, device="cuda"), torch.empty_like(k_out)

    def chain():                                    # what graph.py's pre() runs without the option: into static buffers
        q, k = qk_rope_torch(q_in, k_in, cos, sin, qw, kw, 1e-6)
        q_dst.copy_(q), k_dst.copy_(k)

    def kernel():
        qk_rope(q_in, k_in, cos, sin, rp, qw, kw, 1e-6, q_out, k_out)

    def eager(fn):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / CALLS
        return run

    def graphed(fn):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()
        torch.cuda.current_stream().wait_stream(s)
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            for _ in range(CALLS):
                fn()

        def run():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            cg.replay()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / CALLS
        return run
    return {"torch chain, eager": eager(chain), "kivi_qk_rope, eager": eager(kernel),
            "torch chain, graph": graphed(chain), "kivi_qk_rope, graph": graphed(kernel)}


def attend_forms(torch, nh_kv, ratio, T):
    from kivi_amd.attention import KiviConfig, KiviLayerCache, KiviLayerCacheMF, kivi_attention_decode
    from kivi_amd.cache_mf import padded_heads
    cfg = KiviConfig(2, 2, 32, 128)
    g = torch.Generator("cuda").manual_seed(1)
    k0 = torch.randn((B, nh_kv, T, D), device="cuda", generator=g).half()
    v0 = torch.randn((B, nh_kv, T, D), device="cuda", generator=g).half()
    nhp = padded_heads(cfg, D, nh_kv * ratio, nh_kv)
    forms = {}
    for name, heads, mk in ((f"ratio {ratio} padded to {nhp // nh_kv}, matrix pipe", nhp, "mf"), (f"ratio {ratio}, hook-state", nh_kv * ratio, "hook"),
                            ("true ratio 8, matrix pipe", nh_kv * 8, "mf")):
        if mk == "mf":
            base = KiviLayerCacheMF(cfg, B, nh_kv, D, T + 2 * STEPS + 256, "cuda", num_heads=heads)
        else:
            base = KiviLayerCache(cfg, B, nh_kv, D, T + 2 * STEPS + 256, "cuda")
        base.prefill(k0, v0)
        q = torch.randn((B, heads, 1, D), device="cuda", generator=g).half()
        if name.startswith("ratio") and mk == "mf":             # the pad heads, as kivi_qk_rope leaves them
            q.view(B, nh_kv, heads // nh_kv, 1, D)[:, :, ratio:] = 0
        kn, vn = torch.randn((B, nh_kv, 1, D), device="cuda", generator=g).half(), torch.randn((B, nh_kv, 1, D), device="cuda", generator=g).half()

        def run(base=base, q=q, kn=kn, vn=vn):
            layer = base.clone()
            for _ in range(4):
                kivi_attention_decode(q, kn, vn, layer)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(STEPS):
                kivi_attention_decode(q, kn, vn, layer)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / STEPS
        forms[name] = run
    return forms


GEOMETRIES = {7: dict(hidden_size=3584, num_attention_heads=28, num_key_value_heads=4, intermediate_size=18944),
              5: dict(hidden_size=5120, num_attention_heads=40, num_key_value_heads=8, intermediate_size=13824)}


def model_forms(torch, ratio, T, layers):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, Qwen2ForCausalLM_KIVI, make_config
    geo = dict(GEOMETRIES[ratio], num_hidden_layers=layers, vocab_size=32000, head_dim=128)
    ids = torch.randint(0, 32000, (B, T), device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    forms = {}
    for name, cls, d, on in ((f"ratio {ratio}, qk_kernel on (padded, whole-step graph)", Qwen2ForCausalLM_KIVI, geo, True),
                             (f"ratio {ratio}, qk_kernel off (hook-state, per-layer graphs)", Qwen2ForCausalLM_KIVI, geo, False),
                             ("true ratio 8 (Llama-shaped, whole-step graph)", LlamaForCausalLM_KIVI,
                              dict(geo, num_attention_heads=8 * geo["num_key_value_heads"]), False)):
        cfg = make_config(d, residual_length=128, qk_kernel=on)
        torch.manual_seed(0)
        torch.set_default_dtype(torch.float16)
        with torch.device("cuda"):
            model = cls(cfg)
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
            dt = time.perf_counter() - t0
            model.graphs.end()
            del pasts
            return dt * 1e6 / STEPS
        forms[name] = run
    return forms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--context", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--skip-models", action="store_true", help="leave part (c) out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_rope_time.log"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("qk_rope_time.py needs a GPU: nothing is timed without one")
    out = [f"kivi_qk_rope and padded query groups on {torch.cuda.get_device_name(0)}: B={B}, {args.rounds} alternating rounds "
           f"(one more, the first, discarded); microseconds"]
    for title, nh, nh_kv, norm, rp in (("Llama-3-8B heads (32 / 8), RoPE", 32, 8, False, 4), ("Qwen3-14B heads (40 / 8), head norm + RoPE + pad to 8", 40, 8, True, 8)):
        out.append(f"(a) q / k preparation of one layer of a decode step, {title}; per call, {CALLS} calls per measurement")
        out += [line(k, v) for k, v in rounds(prep_forms(torch, nh, nh_kv, norm, rp), args.rounds).items()]
    for nh_kv, ratio in ((4, 7), (8, 5)):
        out.append(f"(b) attention of one decode step of one layer, {nh_kv} kv heads, {args.context} cached tokens, 2 bits, residual 128; per step, "
                   f"device events around {STEPS} steps")
        out += [line(k, v) for k, v in rounds(attend_forms(torch, nh_kv, ratio, args.context), args.rounds).items()]
        torch.cuda.empty_cache()
    if not args.skip_models:
        for ratio in (7, 5):
            g = GEOMETRIES[ratio]
            out.append(f"(c) one decode step of {args.layers} layers, hidden {g['hidden_size']}, {g['num_key_value_heads']} kv heads, random weights, "
                       f"after a {args.context}-token prompt; decode_graphed, host clock to a device synchronise over {STEPS} steps, per step")
            out += [line(k, v) for k, v in rounds(model_forms(torch, ratio, args.context, args.layers), max(3, args.rounds // 2)).items()]
            torch.cuda.empty_cache()
    print("\n".join(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
