"""Time the constrained row sampler (kivi_sample_rows_con) against kivi_sample_rows_pen and against the torch constraints a caller
composes around it; writes profiles/sample_constraint_time.log.

    python tools/sample_constraint_time.py [--rounds N] [--iters N] [--shape B V] [--parent-lib PATH] [--out PATH]

For (B, V) in {(32, 32000), (64, 128256)}, fp16 logits, top_k 50 + top_p 0.9 in every record, neutral penalty records over an empty
history table, forms on the same logits:
  (a) kivi_sample_rows_pen         RowSampler with a table and no constraint state: what a call without constraints launches
  (b) kivi_sample_rows_con neutral RowSampler with constraint state, every record neutral: the path of (a) inside the new kernel
                                   plus one record load per row
  (c) kivi_sample_rows_con         a mask that allows about half the tokens and 300 list entries (biases; a tenth of them -inf) per row
  (c') ... mask alone / (c'') ... list alone: the two parts of (c)
  (d) torch + kivi_sample_rows_pen what a caller does today: unpack the bitmask to (B, V) bools, masked_fill, index_add of the biases,
                                   then kivi_sample_rows_pen on the result
Each round times `iters` back-to-back calls of each form with device events, after one warm-up; rounds alternate the forms.  Two
figures per form, medians (min, max) over the rounds: the CALL time (eager, Python dispatch inside the window) and the DEVICE time
(the same calls captured into one hipGraph and replayed).  Ratios are taken against (a) on each.
`--parent-lib`: a libkivi_hip.so built from the parent commit; kivi_sample_rows_pen is then timed through both libraries by the same
raw ctypes call on the same buffers, alternating: the spread of (a) against itself, and whether (a) is the code it was."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sample_rows_time import _events, _graph  # noqa: E402

SHAPES = [(32, 32000), (64, 128256)]
ENTRIES = 300


def _torch_form(logits, under, allowed, ids, values, out):
    """Form (d): the bitmask unpacked to booleans, a masked_fill, an index_add of the biases, then the sampler -- in the dtype of
    `logits` (fp16 as timed: the additions then round to fp16; on fp32 logits it is the rule of the fused kernel bit for bit)."""
    B, V = logits.shape
    shifts = torch.arange(32, device=logits.device, dtype=torch.int32)
    rows = torch.arange(B, device=logits.device)[:, None].expand_as(ids).reshape(-1)
    flat_ids = (rows * V + ids.reshape(-1))
    flat_values = values.reshape(-1).to(logits.dtype)

    def fn():
        bits = ((allowed[:, :, None] >> shifts) & 1).bool().reshape(B, -1)[:, :V]
        x = logits.masked_fill(~bits, float("-inf"))
        x.view(-1).index_add_(0, flat_ids, flat_values)
        under(x, out=out)
    return fn


def _raw_pen(lib, logits, rs, out):
    from kivi_amd import _lib
    B, V = logits.shape
    args = (_lib.ptr(logits), 16, logits.stride(0), B, V, _lib.ptr(rs.records), _lib.ptr(rs.draw_index), _lib.ptr(rs.penalties),
            _lib.ptr(rs.seen), rs.seen.stride(0), _lib.ptr(out), 1)
    return lambda: lib.kivi_sample_rows_pen(*args, _lib.stream_ptr(logits))


def rows(rounds, iters, shapes, parent_lib):
    from kivi_amd import _lib
    from kivi_amd.sampling import RowSampler, SamplingParams, allow_bitmask
    lines = []
    for B, V in shapes:
        gen = torch.Generator("cuda").manual_seed(B + V)
        cpu = torch.Generator().manual_seed(B + V)
        logits = (torch.randn((B, V), device="cuda", generator=gen) * 3).half()
        out = torch.empty((B, 1), dtype=torch.int64, device="cuda")
        base = dict(top_k=50, top_p=0.9, seed=1)
        streams = list(range(B))
        ids = torch.stack([torch.randperm(V, generator=cpu)[:ENTRIES].sort().values for _ in range(B)])
        values = torch.randn((B, ENTRIES), generator=cpu) * 2
        values[:, ::10] = float("-inf")
        masks = [allow_bitmask((torch.rand(V, generator=cpu) < 0.5).nonzero().view(-1).tolist(), V) for _ in range(B)]

        def sampler(mask, lists, constraints=True):
            ps = [SamplingParams(**base, logit_bias=dict(zip(ids[b].tolist(), values[b].tolist())) if lists else None) for b in range(B)]
            rs = RowSampler(ps, "cuda", streams=streams, vocab_size=V, constraints=constraints)
            if mask:
                for b in range(B):
                    rs.set_allowed(b, masks[b])
            return rs
        plain = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
        neutral, both, mask_only, list_only = sampler(False, False), sampler(True, True), sampler(True, False), sampler(False, True)
        under = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
        assert neutral.constraint is not None and plain.constraint is None
        assert torch.equal(plain(logits), neutral(logits)), "neutral records have to draw kivi_sample_rows_pen's tokens"
        torch_form = _torch_form(logits, under, both.allowed, ids.cuda(), values.cuda(), out)
        want = both(logits).clone()
        _torch_form(logits.float(), under, both.allowed, ids.cuda(), values.cuda(), out)()
        assert torch.equal(out, want), "the torch composition (in fp32) has to draw the fused kernel's tokens"
        fns = [("(a) rows_pen", lambda: plain(logits, out=out)), ("(b) rows_con, neutral records", lambda: neutral(logits, out=out)),
               ("(c) rows_con, mask + 300 entries", lambda: both(logits, out=out)),
               ("(c') rows_con, mask alone", lambda: mask_only(logits, out=out)),
               ("(c'') rows_con, 300 entries alone", lambda: list_only(logits, out=out)),
               ("(d) torch mask + bias + rows_pen", torch_form)]
        if parent_lib:
            other = ctypes.CDLL(parent_lib)
            other.kivi_sample_rows_pen.restype, other.kivi_sample_rows_pen.argtypes = _lib.SIGNATURES["kivi_sample_rows_pen"]
            raw = RowSampler(SamplingParams(**base), "cuda", streams=streams, vocab_size=V)
            fns += [("(a) raw call, this library", _raw_pen(_lib.load(), logits, raw, out)),
                    ("(a) raw call, parent library", _raw_pen(other, logits, raw, out))]
        tables = [rs.seen for rs in (plain, neutral, both, mask_only, list_only, under)] + ([raw.seen] if parent_lib else [])

        def restore():
            """Every timed window starts from an empty history table (each call counts the token it draws)."""
            for t in tables:
                t.zero_()
        replays = [_graph(fn, iters) for _, fn in fns]
        for _, fn in fns:                                                    # one warm-up of every form
            fn()
        call, dev = [[] for _ in fns], [[] for _ in fns]
        for _ in range(rounds):
            for i, (_, fn) in enumerate(fns):
                restore()
                call[i].append(_events(fn, iters))
            for i, rp in enumerate(replays):
                restore()
                dev[i].append(_events(rp, 1) / iters)
        mc, md = [statistics.median(t) for t in call], [statistics.median(t) for t in dev]
        for i, (name, _) in enumerate(fns):
            ratio = "" if i == 0 else f"   / (a): call {mc[i] / mc[0]:5.2f}x  device {md[i] / md[0]:5.2f}x"
            lines.append(f"  B={B:3d} V={V:6d} fp16  {name:34s} call {mc[i]:7.1f} us (min {min(call[i]):7.1f}, max {max(call[i]):7.1f})   "
                         f"device {md[i]:7.1f} us (min {min(dev[i]):7.1f}, max {max(dev[i]):7.1f}){ratio}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=2, metavar=("B", "V"), help="time this shape only")
    ap.add_argument("--parent-lib", help="a libkivi_hip.so of the parent commit: kivi_sample_rows_pen through both libraries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_constraint_time.log"))
    args = ap.parse_args()
    if args.rounds < 7:
        raise SystemExit("at least 7 rounds: the medians are over them")
    if not torch.cuda.is_available():
        raise SystemExit("sample_constraint_time.py needs a GPU: nothing is timed without one")
    lines = [f"kivi_sample_rows_con against kivi_sample_rows_pen and against torch constraints around it; fp16 logits (B, V), top_k 50 + "
             f"top_p 0.9 in every record, neutral penalties over an empty table; constrained rows: a mask allowing about half the tokens "
             f"and {ENTRIES} list entries; median (min, max) of {args.rounds} alternating rounds of {args.iters} back-to-back calls "
             f"between device events after one warm-up: eager calls (call time, Python dispatch included) and the same calls replayed "
             f"from one captured graph (device time)"]
    print(lines[0], flush=True)
    lines += rows(args.rounds, args.iters, [tuple(args.shape)] if args.shape else SHAPES, args.parent_lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
