"""Time the prompt pass's attention: kivi_prefill_attention against what the code without it runs for the same call, in the same
process, with device events.

    python tools/prefill_attn_time.py [--rounds N] [--no-model]

Per shape -- Llama-2-7B heads (32 / 32) and Llama-3-8B heads (32 / 8), D = 128, B in {1, 8}, T in {512, 2048, 4096} -- q, k, v are
seeded fp16 tensors in the layout the attention modules hold them in (transposed views of (B, T, heads, D)):
  unpadded   kernel(lead = None)                 against   repeat_interleave of K / V (32 / 8 only) + SDPA(is_causal=True)
  padded     kernel(lead), leads drawn uniformly in [0, T - 32]
                                                 against   repeat_interleave + SDPA(attn_mask = the (B, 1, T, T) fp16 mask)
The (B, 1, T, T) mask is built once per pass and read by every layer: padding_prompt_mask is timed on its own and stated
separately, as its share per layer of a 32-layer pass.  A timed item is `reps` back-to-back calls between two device events on an
idle device; one warm-up of every form, then `rounds` rounds with the forms alternating; medians, microseconds per call.  The
kernel's rate is 4 * D * (live pairs) * nh * B FLOP over its time.  At every timed size the two outputs are compared on the live rows.

Then one end-to-end line: model.forward of the Llama-2-7B-shaped random model (32 layers, 2-bit, g = 32, R = 32) on B = 8, T = 2048
left-padded prompts with the option off (eager class: the masked path) and on, with torch.cuda.max_memory_allocated of each pass."""
import argparse
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 128


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def events(fn, reps=1):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, out


def shapes(dev, rounds):
    from kivi_amd import prefill
    from kivi_amd.generation import padding_prompt_mask
    g = torch.Generator().manual_seed(0)
    print(f"prompt-pass attention, D = {D}, fp16; medians of {rounds} alternating rounds, microseconds per call", flush=True)
    print(f"{'heads':>7s} {'B':>2s} {'T':>5s} {'pads':>6s} | {'kernel':>9s} {'TFLOP/s':>8s} | {'parent':>10s} {'mask/32':>9s} | "
          f"{'kernel/parent':>13s} {'with mask':>10s} | max |diff|")
    for nh, nh_kv in ((32, 32), (32, 8)):
        G = nh // nh_kv
        for B in (1, 8):
            for T in (512, 2048, 4096):
                q, k, v = (torch.randn((B, T, h, D), generator=g).half().to(dev).transpose(1, 2) for h in (nh, nh_kv, nh_kv))
                reps = 10 if B * T <= 4096 else 3
                for padded in (False, True):
                    lead = torch.randint(0, T - 31, (B,), generator=g).to(torch.int32).to(dev) if padded else None
                    live = T - (lead.long() if padded else torch.zeros(B, dtype=torch.long, device=dev))
                    flop = 4.0 * D * nh * float((live * (live + 1) // 2).sum())
                    mask2d = (torch.arange(T, device=dev)[None] >= (T - live)[:, None]).long()
                    t_mask, mask4 = events(lambda: padding_prompt_mask(mask2d)) if padded else (0.0, None)

                    def parent():
                        kr, vr = (k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)) if G > 1 else (k, v)
                        if mask4 is None:
                            return F.scaled_dot_product_attention(q, kr, vr, is_causal=True)
                        return F.scaled_dot_product_attention(q, kr, vr, attn_mask=mask4)

                    def kernel():
                        return prefill.attention_kernel(q, k, v, lead)
                    o_new, o_old = kernel(), parent()                       # warm-up of both forms
                    rows = mask2d.bool()[:, None, :].expand(-1, nh, -1)
                    diff = (o_new[rows].float() - o_old[rows].float()).abs().max().item()
                    del o_new, o_old
                    if padded:
                        t_mask = _median([events(lambda: padding_prompt_mask(mask2d))[0] for _ in range(rounds)])
                    ts = {"kernel": [], "parent": []}
                    for _ in range(rounds):
                        ts["kernel"].append(events(kernel, reps)[0])
                        ts["parent"].append(events(parent, reps)[0])
                    tk, tp = _median(ts["kernel"]), _median(ts["parent"])
                    print(f"{nh:>4d}/{nh_kv:<2d} {B:>2d} {T:>5d} {'leads' if padded else 'none':>6s} | {tk:9.1f} {flop / tk / 1e6:8.1f} | "
                          f"{tp:10.1f} {t_mask / 32:9.1f} | {tk / tp:13.3f} {tk / (tp + t_mask / 32):10.3f} | {diff:.2e}", flush=True)
                    del mask4
                del q, k, v
                torch.cuda.empty_cache()


def model_line(dev, rounds):
    from kivi_amd.llama import LlamaForCausalLM_KIVI, left_pad
    cfg = SimpleNamespace(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, num_hidden_layers=32,
                          intermediate_size=11008, vocab_size=32000, max_position_embeddings=8192, rope_theta=10000.0,
                          rms_norm_eps=1e-5, tie_word_embeddings=False, k_bits=2, v_bits=2, group_size=32, residual_length=32,
                          kivi_max_cache_len=None, attention_bias=False, kivi_prefill_kernel=False)
    torch.manual_seed(0)
    with torch.device(dev):
        torch.set_default_dtype(torch.float16)
        model = LlamaForCausalLM_KIVI(cfg)
        torch.set_default_dtype(torch.float32)
    for p in model.parameters():
        if p.dim() > 1:
            p.data.normal_(0.0, 0.02)
    B, T = 8, 2048
    g = torch.Generator().manual_seed(1)
    lens = [T] + torch.randint(32, T + 1, (B - 1,), generator=g).tolist()
    ids, mask = left_pad([torch.randint(1, 32000, (n,), generator=g).tolist() for n in lens], 0, dev)

    def option(on):                                        # the same weights for both forms: the option is flipped in place
        cfg.kivi_prefill_kernel = on
        for layer in model.model.layers:
            layer.self_attn.prefill_kernel = on

    def one(on):
        option(on)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t, (lg, _) = events(lambda: model.forward(ids, padding_mask=mask))
        return t, torch.cuda.max_memory_allocated() - base, lg
    with torch.no_grad():
        lg_on, lg_off = one(True)[2], one(False)[2]
        ts = {True: [], False: []}
        for _ in range(rounds):
            for on in (True, False):
                t, peak, _ = one(on)
                ts[on].append((t, peak))
    print(f"model.forward, Llama-2-7B shape (32 layers, 32 / 32 heads), B = {B}, T = {T} left-padded (prompts of {min(lens)} .. {max(lens)} "
          f"tokens); medians of {rounds} alternating rounds")
    for on in (False, True):
        t = _median([x[0] for x in ts[on]])
        print(f"  option {'on ' if on else 'off'}: {t / 1e3:9.2f} ms   peak memory above the weights {max(x[1] for x in ts[on]) / 2 ** 20:9.1f} MiB")
    print(f"  on / off: {_median([x[0] for x in ts[True]]) / _median([x[0] for x in ts[False]]):.3f}x   last-token logits max |diff| "
          f"{(lg_on.float() - lg_off.float()).abs().max().item():.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    with torch.no_grad():
        shapes(dev, args.rounds)
    if not args.no_model:
        model_line(dev, max(3, args.rounds // 2))
    return 0


if __name__ == "__main__":
    sys.exit(main())
