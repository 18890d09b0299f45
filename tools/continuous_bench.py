"""End to end: generate_continuous against static waves on a Llama-shaped model with random weights (the recipe of
examples/mem_spd_test.py: Llama-2-7B architecture, k = v = 2 bit, g = 32, R = 32; the tokens mean nothing, time does).

    python tools/continuous_bench.py [--requests 96] [--batch 32] [--reps 3] [--compact N [N ...] | --short]

Requests: prompt lengths uniform in [32, 160]; output lengths 8 + floor(Exp(mean 96)), capped at 512 -- a skewed distribution (the
median is ~75 tokens, the longest of a wave of 32 is typically beyond 300); numpy seed 0.  No EOS: every request runs to its length.
  static waves   generate() on `batch` requests at a time (left-padded), each wave until its longest request ends;
  continuous     generate_continuous(batch_size=batch), eager and graphed: finished rows take the waiting requests.
Tokens per second count the tokens the requests asked for, over the wall time of the whole queue (host clock around work that ends
in a device synchronise).  One warm-up of every mode, then `reps` repetitions with the modes alternating; the spread is printed.
The admission share is measured in a run of its own: the wall time inside admit_ (synchronised on both sides) over the total.
`--compact N [N ...]`: the modes are generate_continuous with compact=None -- the behaviour without it, the
comparison -- and with compact=N for every N given, eager and graphed, alternating; no static waves.  Per mode also the decode steps,
the kv length at the end and the number of rebases (host-side counters around model methods, no synchronisation); the share of time
in rebase_ comes from a synchronised run of its own per N, like the admission share.
`--short`: generate_continuous with short_admissions=False -- the behaviour without it, the comparison -- and
True, eager and graphed, alternating; no static waves.  Per mode also the admissions, the tokens their prompt passes ran over and
the offsets (host-side counters around admit_); the admission share of each form comes from a synchronised eager run of its own.
The two forms may pick other tokens; every request runs to its length, so the work is the same."""
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
    ap.add_argument("--compact", type=int, nargs="+", default=None, metavar="N",
                    help="compare generate_continuous(compact=None) with compact=N for every N (no static waves)")
    ap.add_argument("--short", action="store_true",
                    help="compare generate_continuous(short_admissions=False) with True (no static waves)")
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

    def continuous(graphed, compact=None, short=False):
        out = model.generate_continuous(prompts, limits, B, graphed=graphed, compact=compact, short_admissions=short)
        assert [o.numel() for o in out] == limits
        return None

    modes = [("static waves (generate)", static_waves), ("continuous, eager", lambda: continuous(False)),
             ("continuous, graphed", lambda: continuous(True))]
    if args.compact:
        return compact_modes(args, model, continuous, asked)
    if args.short:
        return short_modes(args, model, continuous, asked)

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


def compact_modes(args, model, continuous, asked):
    """--compact: compact=None against compact=N, eager and graphed (see the module docstring)."""
    seen = {"steps": 0, "rebases": 0, "dropped": 0, "last": 0}
    forward_, graphed_, rebase_ = model._forward, model.decode_graphed, model.rebase_

    def forward(ids, past=None, *a, **k):
        if past is not None:
            seen["steps"] += 1
            seen["last"] = past[0].layer.kv_seq_len + 1
        return forward_(ids, past, *a, **k)

    def decode_graphed(tok, past, position, steps, *a, **k):
        seen["steps"] += steps
        seen["last"] = past[0].layer.kv_seq_len + steps
        return graphed_(tok, past, position, steps, *a, **k)

    def rebase(past, drop):
        seen["rebases"] += 1
        seen["dropped"] += drop
        return rebase_(past, drop)
    model._forward, model.decode_graphed, model.rebase_ = forward, decode_graphed, rebase
    modes = [(f"{'graphed' if g else 'eager'}, compact={c}", g, c) for c in [None] + list(args.compact) for g in (False, True)]
    runs = {name: [] for name, _, _ in modes}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        return time.time() - t0
    for rep in range(args.reps + 1):                       # repetition 0 warms every mode up
        for name, g, c in modes:
            seen.update(steps=0, rebases=0, dropped=0, last=0)
            t = timed(lambda: continuous(g, c))
            if rep:
                runs[name].append((t, dict(seen)))
    res = {"requests": args.requests, "batch": args.batch, "tokens_asked_for": asked, "repetitions": args.reps, "layers": args.layers}
    for name, _, _ in modes:
        ts = sorted(t for t, _ in runs[name])
        med, counters = ts[len(ts) // 2], runs[name][0][1]
        res[name] = {"seconds": [round(t, 3) for t, _ in runs[name]], "median_seconds": round(med, 3), "tokens_per_s": round(asked / med, 1),
                     "spread": round((ts[-1] - ts[0]) / med, 3), "steps": counters["steps"], "final_kv_length": counters["last"],
                     "rebases": counters["rebases"], "tokens_dropped": counters["dropped"]}
    # the share of rebase_ (and admit_), in synchronised runs of their own
    admit_ = model.admit_
    for c in args.compact:
        spent = {"rebase": 0.0, "admit": 0.0}

        def synced(fn, key):
            def run(*a, **k):
                torch.cuda.synchronize()
                t0 = time.time()
                out = fn(*a, **k)
                torch.cuda.synchronize()
                spent[key] += time.time() - t0
                return out
            return run
        model.rebase_, model.admit_ = synced(rebase, "rebase"), synced(admit_, "admit")
        seen.update(steps=0, rebases=0, dropped=0, last=0)
        total = timed(lambda: continuous(False, c))
        model.rebase_, model.admit_ = rebase, admit_
        res[f"instrumented eager, compact={c}"] = {"total_seconds": round(total, 3), "rebases": seen["rebases"],
                                                   "rebase_seconds": round(spent["rebase"], 4), "rebase_share": round(spent["rebase"] / total, 5),
                                                   "admit_seconds": round(spent["admit"], 3), "admit_share": round(spent["admit"] / total, 4)}
    model._forward, model.decode_graphed, model.rebase_ = forward_, graphed_, rebase_
    print(json.dumps(res))


def short_modes(args, model, continuous, asked):
    """--short: short_admissions=False against True, eager and graphed (see the module docstring)."""
    seen = {"admissions": 0, "pass_tokens": 0, "offset_tokens": 0, "rows": 0}
    admit_ = model.admit_

    def counted(past, rows, ids, mask, offset=0):
        seen["admissions"] += 1
        seen["rows"] += ids.shape[0]
        seen["pass_tokens"] += ids.shape[0] * ids.shape[1]
        seen["offset_tokens"] += ids.shape[0] * offset
        return admit_(past, rows, ids, mask, offset=offset)
    model.admit_ = counted
    modes = [(f"{'graphed' if g else 'eager'}, short_admissions={s}", g, s) for s in (False, True) for g in (False, True)]
    runs = {name: [] for name, _, _ in modes}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        return time.time() - t0
    for rep in range(args.reps + 1):                       # repetition 0 warms every mode up
        for name, g, s in modes:
            seen.update(admissions=0, pass_tokens=0, offset_tokens=0, rows=0)
            t = timed(lambda: continuous(g, None, s))
            if rep:
                runs[name].append((t, dict(seen)))
    res = {"requests": args.requests, "batch": args.batch, "tokens_asked_for": asked, "repetitions": args.reps, "layers": args.layers}
    for name, _, _ in modes:
        ts = sorted(t for t, _ in runs[name])
        med, counters = ts[len(ts) // 2], runs[name][0][1]
        res[name] = {"seconds": [round(t, 3) for t, _ in runs[name]], "median_seconds": round(med, 3), "tokens_per_s": round(asked / med, 1),
                     "spread": round((ts[-1] - ts[0]) / med, 3), "admissions": counters["admissions"], "rows_admitted": counters["rows"],
                     "prompt_pass_tokens": counters["pass_tokens"], "tokens_under_offsets": counters["offset_tokens"]}
    for s in (False, True):                                # the share of admit_, in synchronised runs of their own
        spent = [0.0]

        def synced(*a, **k):
            torch.cuda.synchronize()
            t0 = time.time()
            out = counted(*a, **k)
            torch.cuda.synchronize()
            spent[0] += time.time() - t0
            return out
        model.admit_ = synced
        total = timed(lambda: continuous(False, None, s))
        model.admit_ = counted
        res[f"instrumented eager, short_admissions={s}"] = {"total_seconds": round(total, 3), "admit_seconds": round(spent[0], 3),
                                                            "admit_share": round(spent[0] / total, 4)}
    model.admit_ = admit_
    print(json.dumps(res))


if __name__ == "__main__":
    main()
