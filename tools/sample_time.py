"""Time the fused sampler (kivi_sample) and the sampled graphed decode step; writes profiles/sample_time.log.

    python tools/sample_time.py [--rounds N] [--iters N] [--no-step] [--out PATH]

1. kivi_sample against the torch composition of transformers' warpers on the same fp16 logits (TemperatureLogitsWarper,
   TopKLogitsWarper, TopPLogitsWarper -- the sort / softmax / cumsum / scatter / masked_fill of transformers v5, restated here --,
   then softmax and torch.multinomial), for (B, V) in {(1, 32000), (32, 32000), (1, 128256), (64, 128256)} and top_k = 50 / 0
   with top_p = 0.9.  Each round times `iters` back-to-back calls of each with device events; rounds interleave the two.
2. The graphed decode step at the Llama-2-7B shape (random weights, B = 32, prompt 2048, 512 new tokens, 2-bit g = 32 R = 32, the
   whole step replayed from one hipGraph): decode_graphed greedy against decode_graphed with a Sampler (top_k 50, top_p 0.9),
   interleaved rounds, ms per step over the 512 steps (the eager and capture steps included, the same number in both).
Medians and minimums over the rounds."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 32000), (32, 32000), (1, 128256), (64, 128256)]
PARAMS = [(50, 0.9), (0, 0.9)]


def hf_torch(logits, temperature, top_k, top_p):
    """transformers v5's Temperature -> TopK -> TopP warpers, softmax and multinomial, in torch."""
    scores = logits.float() / temperature
    if top_k:
        kth = torch.topk(scores, min(top_k, scores.shape[-1]))[0][..., -1, None]
        scores = scores.masked_fill(scores < kth, -float("inf"))
    if top_p < 1.0:
        sorted_logits, sorted_indices = torch.sort(scores, descending=False)
        cum = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= (1 - top_p)
        remove[..., -1:] = 0
        scores = scores.masked_fill(remove.scatter(1, sorted_indices, remove), -float("inf"))
    return torch.multinomial(torch.softmax(scores, -1), num_samples=1)


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def sampler_rows(rounds, iters):
    from kivi_amd.sampling import Sampler
    lines = []
    for B, V in SHAPES:
        logits = (torch.randn((B, 1, V), device="cuda", generator=torch.Generator("cuda").manual_seed(B + V)) * 3).half()
        for k, p in PARAMS:
            smp = Sampler(1.0, k, p, seed=1)
            out = torch.empty((B, 1), dtype=torch.int64, device="cuda")
            fused = lambda: smp(logits, out=out)                      # noqa: E731
            ref = lambda: hf_torch(logits[:, 0], 1.0, k, p)           # noqa: E731
            for _ in range(3):
                fused(), ref()
            tf, tr = [], []
            for _ in range(rounds):
                tf.append(_events(fused, iters))
                tr.append(_events(ref, iters))
            mf, mr = statistics.median(tf), statistics.median(tr)
            lines.append(f"  B={B:3d} V={V:6d} top_k={k:2d} top_p={p}   kivi_sample {mf:8.1f} us (min {min(tf):7.1f})   "
                         f"torch warpers + multinomial {mr:8.1f} us (min {min(tr):7.1f})   {mr / mf:5.1f}x")
            print(lines[-1], flush=True)
    return lines


def step_rows(rounds, gen=512, prompt=2048, B=32):
    from kivi_amd.llama import LlamaForCausalLM_KIVI
    from kivi_amd.sampling import Sampler
    cfg = SimpleNamespace(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, num_hidden_layers=32,
                          intermediate_size=11008, vocab_size=32000, max_position_embeddings=prompt + gen + 1, rope_theta=10000.0,
                          rms_norm_eps=1e-5, tie_word_embeddings=False, k_bits=2, v_bits=2, group_size=32, residual_length=32,
                          kivi_max_cache_len=prompt + gen + 1, attention_bias=False, rope_scaling=None, head_dim=None,
                          sliding_window=None)
    torch.manual_seed(0)
    with torch.device("cuda"):
        torch.set_default_dtype(torch.float16)
        model = LlamaForCausalLM_KIVI(cfg)
        torch.set_default_dtype(torch.float32)
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.02)
    ids = torch.randint(0, 32000, (B, prompt), device="cuda")
    res = {"greedy": [], "sampled": []}
    for r in range(rounds):
        for mode in ("greedy", "sampled"):
            logits, pasts = model(ids)
            smp = Sampler(1.0, 50, 0.9, seed=r) if mode == "sampled" else None
            tok = logits.argmax(-1) if smp is None else smp(logits)
            torch.cuda.synchronize()
            t0 = time.time()
            model.decode_graphed(tok, pasts, prompt, gen, sampler=smp)
            torch.cuda.synchronize()
            res[mode].append((time.time() - t0) * 1e3 / gen)
            print(f"  round {r} {mode}: {res[mode][-1]:.3f} ms/step  graph stats {model.graphs.stats}", flush=True)
            del pasts
            model.release_graphs()
    g, s = statistics.median(res["greedy"]), statistics.median(res["sampled"])
    return [f"  greedy  {g:7.3f} ms/step (min {min(res['greedy']):.3f})",
            f"  sampled {s:7.3f} ms/step (min {min(res['sampled']):.3f})   sampled / greedy {s / g:.4f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_time.log"))
    args = ap.parse_args()
    lines = [f"kivi_sample vs the torch composition of transformers' warpers, fp16 logits (B, 1, V), temperature 1; median (min) of "
             f"{args.rounds} interleaved rounds of {args.iters} back-to-back calls, device events"]
    print(lines[0], flush=True)
    lines += sampler_rows(args.rounds, args.iters)
    if not args.no_step:
        lines.append(f"graphed decode step, Llama-2-7B shape (random weights), B=32, prompt 2048 + 512 new tokens, 2-bit g=32 R=32, "
                     f"whole-step hipGraph; median (min) of {args.step_rounds} interleaved rounds, ms per step over 512 steps")
        print(lines[-1], flush=True)
        lines += step_rows(args.step_rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
