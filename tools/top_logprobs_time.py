"""Time the fused top-k log-prob kernel (kivi_token_top_logprobs); writes profiles/top_logprobs_time.log.

    python tools/top_logprobs_time.py [--rounds N] [--shape N V] [--parent-lib PATH] [--out PATH]

fp16 logits (N, V) in {(32, 32000), (64, 128256), (4096, 32000), (4096, 128256)}, k = 5 and 20, three forms on the same tensors:
  (a) kivi_token_logprob alone (kivi_amd.scoring.token_logprobs) -- with --parent-lib also through that library (the parent commit's
      build) at the first 4096-row shape, to show the existing kernel is unchanged;
  (b) kivi_token_top_logprobs with targets (kivi_amd.scoring.top_logprobs);
  (c) what a caller composes from torch: log_softmax(logits.float(), -1), .topk(k), .gather(targets).
The method of tools/score_time.py: device events around back-to-back calls (call times, Python dispatch included), one warm-up, 7
rounds that alternate the forms, medians.  Reported: (b) / (c) and (b) / (a); the second is the price of the lists, the row's extra
cache-resident passes.  Then one end-to-end line: generate_graphed on the tiny model of the tests with and without
return_logprobs / top_logprobs, in steps per second (wall clock around the call, synchronised)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 32000), (64, 128256), (4096, 32000), (4096, 128256)]
KS = (5, 20)


def composition(logits, targets, k):
    lp = torch.log_softmax(logits.float(), -1)
    top = lp.topk(k)
    return lp.gather(-1, targets.unsqueeze(-1)).squeeze(-1), top.indices, top.values


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def _parent_form(path, logits, targets):
    """kivi_token_logprob of another build of the library on the same tensors (its own handle: nothing of this build runs)."""
    from kivi_amd import _lib
    lib = ctypes.CDLL(path)
    res, args = _lib.SIGNATURES["kivi_token_logprob"]
    lib.kivi_token_logprob.restype, lib.kivi_token_logprob.argtypes = res, args
    N, V = logits.shape
    out = torch.empty(N, dtype=torch.float32, device="cuda")

    def call():
        rc = lib.kivi_token_logprob(_lib.ptr(logits), 16, V, N, V, _lib.ptr(targets), 1, -100, _lib.ptr(out), None, None,
                                    _lib.stream_ptr(logits))
        assert rc == 0, rc
        return out
    return call


def rows(rounds, shapes, parent_lib):
    from kivi_amd.scoring import token_logprobs, top_logprobs
    lines = []
    for N, V in shapes:
        iters = 100 if N * V < 10 ** 7 else 20
        gen = torch.Generator("cuda").manual_seed(N + V)
        logits = (torch.randn((N, V), device="cuda", generator=gen) * 3).half()
        targets = torch.randint(0, V, (N,), device="cuda", generator=gen)
        forms = {"a": lambda: token_logprobs(logits, targets)}
        for k in KS:
            forms[f"b{k}"] = lambda k=k: top_logprobs(logits, k, targets)
            forms[f"c{k}"] = lambda k=k: composition(logits, targets, k)
        if parent_lib and (N, V) == next((s for s in shapes if s[0] >= 4096), shapes[-1]):
            forms["parent"] = _parent_form(parent_lib, logits, targets)
            assert torch.equal(forms["parent"]().view(torch.int32), forms["a"]().view(torch.int32)), "the parent build gives other bits"
        same = all(torch.equal(forms[f"b{k}"]().ids, forms[f"c{k}"]()[1]) for k in KS)        # (ties may order differently in torch)
        for fn in forms.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in forms}
        for _ in range(rounds):
            for name, fn in forms.items():
                times[name].append(_events(fn, iters))
        med = {name: statistics.median(t) for name, t in times.items()}
        line = f"  N={N:5d} V={V:6d} fp16  (a) kivi_token_logprob {med['a']:9.1f} us"
        if "parent" in med:
            line += f" [parent build {med['parent']:9.1f} us, same bits]"
        for k in KS:
            b, c = med[f"b{k}"], med[f"c{k}"]
            line += f" | k={k:2d}: (b) fused {b:9.1f} us  (c) torch {c:9.1f} us  (b)/(c) {b / c:5.2f}  (b)/(a) {b / med['a']:5.2f}"
        line += f" | ids equal torch's: {same}"
        lines.append(line)
        print(line, flush=True)
    return lines


def end_to_end(steps=200):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    torch.manual_seed(0)
    cfg = make_config(dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=4, num_hidden_layers=2,
                           intermediate_size=1024, vocab_size=320), residual_length=32)
    model = LlamaForCausalLM_KIVI(cfg).half().cuda()
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.05)
    ids = torch.randint(0, 320, (4, 21), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    forms = (("plain", {}), ("return_logprobs", dict(return_logprobs=True)),
             ("return_logprobs, top_logprobs=5", dict(return_logprobs=True, top_logprobs=5)))
    rates = {name: [] for name, _ in forms}
    for rnd in range(6):                                    # alternating; round 0 warms up (every call captures its own graphs)
        for name, kw in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate_graphed(ids, steps, **kw)
            torch.cuda.synchronize()
            if rnd:
                rates[name].append(steps / (time.perf_counter() - t0))
    out = [f"{name}: {statistics.median(r):7.0f} steps/s" for name, r in rates.items()]
    return (f"  generate_graphed, tiny model (2 layers, hidden 512, vocab 320), B=4, {steps} steps per call (captures included), median "
            f"of 5 alternating calls: " + "; ".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("N", "V"), help="time this shape only")
    ap.add_argument("--parent-lib", help="libkivi_hip.so of the parent commit: form (a) through it at one shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_logprobs_time.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("top_logprobs_time.py needs a GPU: nothing is timed without one")
    lines = [f"kivi_token_top_logprobs: fp16 logits (N, V); median of {args.rounds} alternating rounds of back-to-back calls (100, or 20 "
             f"from 10^7 logits on), device events around the calls (call time, Python dispatch included)"]
    print(lines[0], flush=True)
    lines += rows(args.rounds, [tuple(args.shape)] if args.shape else SHAPES, args.parent_lib)
    lines.append(end_to_end())
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
