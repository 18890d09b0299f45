"""Time ONE admission into living caches in both forms with device events: the prompt pass and the row
movement separately.

    python tools/admit_offset_time.py [--rounds N] [--batch B] [--layers N]

Model: the Llama-2-7B-shaped random model of tools/continuous_bench.py (2-bit, g = 32, R = 32; the tokens mean nothing, time does).
Living caches of `batch` rows at L in {1024, 4096}; n in {1, 8} prompts of 128 tokens are admitted
  at an offset   admit_(offset=admission_offset(L, 128, R, quantum)): the prompt pass over L - offset tokens, then per layer two
                 kivi_mf_store_admit launches and one kivi_cache_admit for the fp16 residual and window;
  L-padded       admit_(offset=0), the code path without offsets: the prompt pass over L tokens, then per layer one kivi_cache_admit.
Per round and form, between device events: forward(input_ids, padding_mask=) and the loop of KiviCacheBase.admit_ over the layers
(the two halves of LlamaForCausalLM_KIVI.admit_); for the new kernel alone also the loop of its launches over the layers, with
moved_bytes / time as a fraction of 8 TB/s.  One warm-up of both forms, then `rounds` rounds with the forms alternating; medians.
The device is idle (synchronised) before every timed item."""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
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
    from kivi_amd import admit
    from kivi_amd.llama import LlamaForCausalLM_KIVI, left_pad
    from kivi_amd.serving import admission_offset
    with torch.device(dev):
        torch.set_default_dtype(torch.float16)
        model = LlamaForCausalLM_KIVI(cfg)
        torch.set_default_dtype(torch.float32)
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.02)
    B, P, R = args.batch, 128, cfg.residual_length
    g = torch.Generator().manual_seed(0)

    def events(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3, out

    print(f"one admission into living caches: {args.layers} layers, h = {args.hidden}, {args.heads} / {args.heads} heads, 2-bit g = 32 R = {R}, "
          f"{B} rows, prompts of {P} tokens; medians of {args.rounds} alternating rounds, microseconds", flush=True)
    with torch.no_grad():
        for L in (1024, 4096):
            ids = torch.randint(1, args.vocab, (B, L), generator=g).to(dev)
            _, past = model.forward(ids, padding_mask=torch.ones_like(ids))
            caches = [p.layer for p in past]
            quantum = model.rebase_quantum(past)
            for n in (1, 8):
                prompts = [torch.randint(1, args.vocab, (P,), generator=g).tolist() for _ in range(n)]
                rows = (torch.arange(n, device=dev) * (B // n if B >= 2 * n else 1)).to(torch.int64)
                forms = [("at an offset", admission_offset(L, P, R, quantum)), ("L-padded (offset=0)", 0)]
                inputs = {name: left_pad(prompts, 0, dev, length=L - off) for name, off in forms}

                def one(name, off):
                    t_pass, (_, fresh) = events(lambda: model.forward(inputs[name][0], padding_mask=inputs[name][1]))
                    t_move, _ = events(lambda: [c.admit_(rows, t.layer, check=False, offset=off) for c, t in zip(caches, fresh)])
                    t_store = moved = 0
                    if off:
                        def stores():
                            for c, t in zip(caches, fresh):
                                admit.admit_store(c.kt, t.layer.kt, rows, 2, True, -(-t.layer.k_quant_len // 32), off // 32)
                                admit.admit_store(c.vt, t.layer.vt, rows, 2, False, -(-t.layer.v_quant_len // 32), off // 32)
                        t_store, _ = events(stores)
                        t0 = fresh[0].layer
                        moved = len(caches) * (admit.store_moved_bytes(t0.kt, n, -(-t0.k_quant_len // 32), off // 32) +
                                               admit.store_moved_bytes(t0.vt, n, -(-t0.v_quant_len // 32), off // 32))
                    return t_pass, t_move, t_store, moved
                for name, off in forms:
                    one(name, off)
                ts = {name: [] for name, _ in forms}
                for _ in range(args.rounds):
                    for name, off in forms:
                        ts[name].append(one(name, off))
                print(f"  L = {L}, n = {n} rows (offset {forms[0][1]}, prompt pass over {L - forms[0][1]} tokens):")
                med = {}
                for name, off in forms:
                    t_pass, t_move, t_store = (_median([t[i] for t in ts[name]]) for i in range(3))
                    med[name] = t_pass + t_move
                    line = f"    {name:22s} prompt pass {t_pass:11.1f}   row movement {t_move:9.1f}   together {t_pass + t_move:11.1f}"
                    if off:
                        moved = ts[name][0][3]
                        line += (f"\n    {'':22s} kivi_mf_store_admit alone ({2 * len(caches)} launches): {t_store:9.1f}   {moved / 1e6:.2f} MB read + "
                                 f"written   {moved / (t_store * 1e-6) / 8e12:6.3f} of 8 TB/s")
                    print(line)
                print(f"    at an offset / L-padded: {med[forms[0][0]] / med[forms[1][0]]:6.3f}x", flush=True)
            del past, caches
    return 0


if __name__ == "__main__":
    sys.exit(main())
