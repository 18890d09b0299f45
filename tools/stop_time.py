"""Time the finish tracker inside the graphed decode step (kivi_stop_rows); writes profiles/stop_time.log.

    python tools/stop_time.py [--shape tiny|wide] [--rounds N] [--steps N] [--parent-tree DIR] [--out PATH] [--append]

--shape tiny (default), the shape of tools/top_logprobs_time.py's end-to-end line: the tiny model of the tests (2 layers, hidden 512,
4 heads, vocab 320, the matrix-pipe cache layout, so the WHOLE step is one graph), B = 4, a 21-token prompt; the host needs longer
to enqueue such a step than the GPU to run it.  --shape wide: 8 layers of the Llama-2-7B geometry with random weights, B = 8, where
the GPU is the slower side, as it is for a model a user would run.  One measurement is one request: the prompt pass,
8 graphed steps that settle the step (one eager, one captured, replays), then `--steps` timed replays through decode_graphed -- a host
clock around them, ending in a device synchronise -- reported in microseconds per step.  The stops can never match (an id no logits
hold), so every step runs.  Forms, alternating within every round:
  parent    decode_graphed of the parent commit's tree (--parent-tree: a built checkout of it; left out without)
  plain     decode_graphed of this tree without a tracker
  tracker   with a StopRows, never polled (sync_every=None): the price of the launch in the captured step
  every=N   with a StopRows polled before every N-th step, N in 1, 2, 4, 8, 16, 32
Every form runs in a worker process of its own tree (this file, --worker), all alive for the whole run and driven round-robin, so the
forms see the same machine state.  (a) the tracker's cost: median(tracker) - median(plain) against the spread of repeated runs of the
parent (p10 to p90; of `plain` without a parent tree).  (b) the default of sync_every: the smallest N whose median lies within that
spread of the never-polled form's."""
import argparse
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYNCS = (1, 2, 4, 8, 16, 32)
T, WARM = 21, 8
# tiny: the model of the tests, a step the host cannot enqueue as fast as the GPU runs it; wide: 8 layers of the Llama-2-7B geometry,
# random weights, a step of the size a user would run, where the GPU is the slower side
SHAPES = {"tiny": dict(B=4, std=0.05, cfg=dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=4, num_hidden_layers=2,
                                               intermediate_size=1024, vocab_size=320)),
          "wide": dict(B=8, std=0.02, cfg=dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, num_hidden_layers=8,
                                               intermediate_size=11008, vocab_size=32000))}


def worker(tree: str, steps: int, shape: str) -> None:
    """Serve measurements over stdin / stdout: a line `plain`, `tracker` or `every=N` in, microseconds per step out."""
    sys.path.insert(0, tree)
    import torch
    from kivi_amd.llama import LlamaForCausalLM_KIVI, make_config
    B, std = SHAPES[shape]["B"], SHAPES[shape]["std"]
    cfg = make_config(SHAPES[shape]["cfg"], residual_length=32)
    NEVER = cfg.vocab_size - 1
    torch.manual_seed(0)
    torch.set_default_dtype(torch.float16)
    with torch.device("cuda"):
        model = LlamaForCausalLM_KIVI(cfg)
    torch.set_default_dtype(torch.float32)
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, std)
    model.lm_head.weight.data[NEVER].zero_()                # the logit of token NEVER is 0: no argmax among the random ones (asserted below)
    ids = torch.randint(0, NEVER, (B, T), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    stopper = None
    print("ready", flush=True)
    for line in sys.stdin:
        form = line.strip()
        if not form:
            break
        kw = {}
        logits, pasts = model(ids)
        tok = logits.argmax(-1)
        if form != "plain":
            from kivi_amd.stopping import StopParams, StopRows
            if stopper is None:
                stopper = StopRows(StopParams([NEVER]), "cuda", B=B)
            stopper.reset()
            stopper(tok)
            kw = dict(stopper=stopper, sync_every=None if form == "tracker" else int(form.split("=")[1]))
        model.decode_graphed(tok, pasts, T, WARM, **kw)
        tok = model.graphs.tok.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.decode_graphed(tok, pasts, T + WARM, steps, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert out.shape == (B, steps) and not bool((out == NEVER).any()), "a stop matched: not every step ran"
        assert model.graphs.stats[2] >= steps - 2, model.graphs.stats      # replays (a geometry class may change once)
        model.graphs.end()
        print(f"{dt * 1e6 / steps:.3f}", flush=True)


class Worker:
    def __init__(self, tree: str, steps: int, shape: str):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--steps", str(steps), "--shape", shape],
                                  stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
        assert self.p.stdout.readline().strip() == "ready", f"the worker of {tree} did not start"

    def measure(self, form: str) -> float:
        self.p.stdin.write(form + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline().strip()
        assert line, f"the worker died on {form!r}"
        return float(line)

    def close(self) -> None:
        self.p.stdin.close()
        self.p.wait(timeout=60)


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, max(0, round(q * (len(xs) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=448)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="tiny")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit: its decode_graphed is timed in the same rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stop_time.log"))
    ap.add_argument("--append", action="store_true", help="append to --out (a second shape into the same log)")
    ap.add_argument("--worker", metavar="TREE", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.steps, args.shape)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stop_time.py needs a GPU: nothing is timed without one")
    here = Worker(ROOT, args.steps, args.shape)
    parent = Worker(os.path.abspath(args.parent_tree), args.steps, args.shape) if args.parent_tree else None
    forms = ([("parent", parent, "plain")] if parent else []) + [("plain", here, "plain"), ("tracker", here, "tracker")] + \
            [(f"every={n}", here, f"every={n}") for n in SYNCS]
    times = {name: [] for name, _, _ in forms}
    order = random.Random(0)
    for rnd in range(args.rounds + 1):                       # round 0 warms every form up
        order.shuffle(forms)                                 # no form always follows the same one
        for name, w, form in forms:
            t = w.measure(form)
            if rnd:
                times[name].append(t)
    here.close()
    if parent:
        parent.close()
    med = {name: statistics.median(t) for name, t in times.items()}
    base = "parent" if parent else "plain"
    lo, hi = pct(times[base], 0.1), pct(times[base], 0.9)
    spread = hi - lo
    c = SHAPES[args.shape]["cfg"]
    lines = [f"finish tracker in the graphed decode step: {args.shape} model ({c['num_hidden_layers']} layers, hidden {c['hidden_size']}, "
             f"vocab {c['vocab_size']}, whole-step graph), B={SHAPES[args.shape]['B']}, "
             f"{args.steps} timed replays per request after {WARM} settling steps, host clock to a device synchronise, "
             f"{args.rounds} alternating rounds (one more, the first, discarded); microseconds per step",
             f"  spread of `{base}`: p10 {lo:.2f}  median {med[base]:.2f}  p90 {hi:.2f}  -> p10-p90 spread {spread:.2f} us"]
    for name in times:
        t = times[name]
        lines.append(f"  {name:9s} median {med[name]:8.2f}  p10 {pct(t, 0.1):8.2f}  p90 {pct(t, 0.9):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}")
    d = med["tracker"] - med["plain"]
    lines.append(f"  (a) tracker - plain = {d:+.2f} us per step ({'within' if abs(d) <= spread else 'EXCEEDS'} the spread of {spread:.2f} us)"
                 + (f"; plain - parent = {med['plain'] - med['parent']:+.2f} us" if parent else "; no parent tree given"))
    lines.append("  (b) sync_every sweep, median - median(never polled = `tracker`): " +
                 "  ".join(f"{n}: {med[f'every={n}'] - med['tracker']:+.2f}" for n in SYNCS))
    ok = [n for n in SYNCS if med[f"every={n}"] - med["tracker"] <= spread]
    lines.append(f"      smallest sync_every within the spread of never: {ok[0] if ok else 'none of ' + str(SYNCS)}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
