"""End to end: generate_continuous against static waves on a Llama-shaped model with random weights (the recipe of
examples/mem_spd_test.py: Llama-2-7B architecture, k = v = 2 bit, g = 32, R = 32; the tokens mean nothing, time does).

    python tools/continuous_bench.py [--requests 96] [--batch 32] [--reps 3]

Requests: prompt lengths uniform in [32, 160]; output lengths 8 + floor(Exp(mean 96)), capped at 512 -- a skewed distribution (the
median is ~75 tokens, the longest of a wave of 32 is typically beyond 300); numpy seed 0.  No EOS: every request runs to its length.
  static waves   generate() on `batch` requests at a time (left-padded), each wave until its longest request ends;
  continuous     generate_continuous(batch_size=batch), eager and graphed: finished rows take the waiting requests.
Tokens per second count the tokens the requests asked for, over the wall time of the whole queue (host clock around work that ends
in a device synchronise).  One warm-up of every mode, then `reps` repetitions with the modes alternating; the spread is printed.
The admission share is measured in a run of its own: the wall time inside admit_ (synchronised on both sides) over the total."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=96)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--intermediate", type=int, default=11008)
    ap.add_argument("--vocab", type=int, default=32000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = SimpleNamespace(hidden_size=args.hidden, num_attention_heads=args.heads, num_key_value_heads=args.heads,
                          num_hidden_layers=args.layers, intermediate_size=args.intermediate, vocab_size=args.vocab,
                          max_position_embeddings=8192, rope_theta=10000.0, rms_norm_eps=1e-5, tie_word_embeddings=False,
                          k_bits=2, v_bits=2, group_size=32, residual_length=32, kivi_max_cache_len=None, attention_bias=False)
    torch.manual_seed(0)
    from kivi_amd.llama import LlamaForCausalLM_KIVI, left_pad
    with torch.device(dev):
        torch.set_default_dtype(torch.float16)
        model = LlamaForCausalLM_KIVI(cfg)
        torch.set_default_dtype(torch.float32)
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.02)
    rng = np.random.default_rng(0)
    N, B = args.requests, args.batch
    prompts = [rng.integers(1, args.vocab, size=int(n)).tolist() for n in rng.integers(32, 161, size=N)]
    limits = [int(min(512, 8 + np.floor(rng.exponential(96.0)))) for _ in range(N)]
    asked = sum(limits)

    def static_waves():
        steps = 0
        for w in range(0, N, B):
            ids, mask = left_pad(prompts[w: w + B], 0, dev)
            n = max(limits[w: w + B])
            model.generate(ids, n, attention_mask=mask)
            steps += n
        return steps

    def continuous(graphed):
        out = model.generate_continuous(prompts, limits, B, graphed=graphed)
        assert [o.numel() for o in out] == limits
        return None

    modes = [("static waves (generate)", static_waves), ("continuous, eager", lambda: continuous(False)),
             ("continuous, graphed", lambda: continuous(True))]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        extra = fn()
        torch.cuda.synchronize()
        return time.time() - t0, extra

    times = {name: [] for name, _ in modes}
    wave_steps = None
    for rep in range(args.reps + 1):                       # repetition 0 warms every mode up
        for name, fn in modes:
            t, extra = timed(fn)
            wave_steps = extra if extra is not None else wave_steps
            if rep:
                times[name].append(t)
    # the admission share, in a run of its own (the synchronisations around admit_ would perturb the timed runs)
    spent, calls = [0.0], [0]
    inner = model.admit_

    def admit_timed(*a, **k):
        torch.cuda.synchronize()
        t0 = time.time()
        res = inner(*a, **k)
        torch.cuda.synchronize()
        spent[0] += time.time() - t0
        calls[0] += 1
        return res
    model.admit_ = admit_timed
    total, _ = timed(lambda: continuous(False))
    model.admit_ = inner
    res = {"model": f"llama-shaped random weights: L={args.layers} h={args.hidden} nh={args.heads} ffn={args.intermediate}, 2-bit g=32 R=32",
           "requests": N, "batch": B, "prompt_tokens": "uniform [32, 160], numpy seed 0",
           "output_tokens": "8 + floor(Exp(mean 96)) capped at 512, numpy seed 0",
           "tokens_asked_for": asked, "longest_output": max(limits), "median_output": int(np.median(limits)),
           "static_wave_steps": wave_steps, "ideal_steps": -(-asked // B), "repetitions": args.reps,
           "admission": {"calls": calls[0], "seconds": round(spent[0], 3), "share_of_total": round(spent[0] / total, 4),
                         "total_seconds_instrumented": round(total, 3)}}
    for name, _ in modes:
        ts = times[name]
        res[name] = {"seconds": [round(t, 3) for t in ts], "median_seconds": round(sorted(ts)[len(ts) // 2], 3),
                     "tokens_per_s": round(asked / sorted(ts)[len(ts) // 2], 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
