"""Time kivi_mf_extend_layer (one attention launch + the K / V flushes) against the decode step it replaces, with device events.

    python tools/extend_time.py [--iters N]

Shapes: the headline shape (B = 32, 32 / 32 heads, 4k prompt, 2-bit, R = 32) and BASELINE config 4 (Llama-3-8B: B = 64, 32 / 8
heads, 8k).  For every Q: microseconds per extend, the algorithmic bytes (the cache as it stands + the chunk's q / k / v / out),
the fraction of 8 TB/s, and the ratio to Q x the decode step (kivi_mf_decode_layer) measured in the same run.  Each timed call
starts from the same lengths (they are restored after the call), so every repetition does the same work on the same buffers."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("headline", 32, 32, 32, 4096), ("config4", 64, 32, 8, 8192)]
QS = [1, 4, 16, 64, 256]
LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len")


def _time(fn, layer, iters):
    saved = [getattr(layer, n) for n in LENGTHS]
    def run():
        fn()
        for n, v in zip(LENGTHS, saved):
            setattr(layer, n, v)
    for _ in range(3):
        run()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, kivi_attention_extend, make_layer_cache
    dev = "cuda"
    torch.manual_seed(0)
    for name, B, nh, nh_kv, T0 in SHAPES:
        cfg = KiviConfig(2, 2, 32, 32)
        layer = make_layer_cache(cfg, B, nh_kv, 128, T0 + max(QS) + 64, dev, num_heads=nh)
        k0 = torch.randn((B, nh_kv, T0, 128), device=dev, dtype=torch.float16)
        layer.prefill(k0, torch.randn_like(k0))
        del k0
        cache_bytes = layer.nbytes()
        q1 = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
        k1 = torch.randn((B, nh_kv, 1, 128), device=dev, dtype=torch.float16)
        dec = _time(lambda: kivi_attention_decode(q1, k1, k1, layer), layer, args.iters)
        print(f"{name}: B={B} nh={nh} nh_kv={nh_kv} P0={T0} 2-bit R=32  cache {cache_bytes / 1e6:.1f} MB  decode step {dec:.1f} us", flush=True)
        for Q in QS:
            q = torch.randn((B, nh, Q, 128), device=dev, dtype=torch.float16)
            k = torch.randn((B, nh_kv, Q, 128), device=dev, dtype=torch.float16)
            us = _time(lambda: kivi_attention_extend(q, k, k, layer), layer, args.iters)
            nbytes = cache_bytes + 2 * (2 * q.numel() + 2 * k.numel())
            print(f"  Q={Q:4d}  extend {us:9.1f} us  bytes {nbytes / 1e6:8.1f} MB  {nbytes / (us * 1e-6) / 8e12:6.3f} of 8 TB/s  "
                  f"extend / (Q x decode) {us / (Q * dec):6.3f}", flush=True)
        del layer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
