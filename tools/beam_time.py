"""Time the per-step cache reorder of beam search (kivi_cache_reorder through KiviLayerCacheMF.reorder_) with device events.

    python tools/beam_time.py [--iters N]

Shape: Llama-2-7B geometry, 8 requests x 4 beams = 32 rows, 32 / 32 heads, 2-bit g = 32 R = 32, a 4096-token prompt forked into
the beams, then 128 generated tokens.  Reported per layer: reorder_(idx, group=4, from_token=4096) with every row moved (each beam
takes its neighbour's history), the same cache's decode step (kivi_mf_decode_layer), a torch index_select + copy_ of every member
(what the reference's _reorder_cache costs when done in place), and the reorder's fraction of 8 TB/s on its algorithmic bytes
(read + write of the moved suffixes).  The moved suffixes (~20 MB) fit the 256 MiB Infinity Cache, so back-to-back repetitions of
the reorder are partly served from it; the decode step reads the whole ~410 MB cache."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTHS = ("k_quant_len", "k_res_len", "v_quant_len", "v_res_start", "v_res_len", "kv_seq_len")


def _time(fn, iters, restore=None):
    for _ in range(3):
        fn()
        if restore:
            restore()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
        if restore:
            restore()
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from kivi_amd import reorder
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    from kivi_amd.quant import mfma
    dev = "cuda"
    torch.manual_seed(0)
    req, nb, nh, T0, gen = 8, 4, 32, 4096, 128
    B = req * nb
    cfg = KiviConfig(2, 2, 32, 32)
    src = make_layer_cache(cfg, req, nh, 128, T0 + gen + 64, dev, num_heads=nh)
    k0 = torch.randn((req, nh, T0, 128), device=dev, dtype=torch.float16)
    src.prefill(k0, torch.randn_like(k0))
    del k0
    layer = src.index_select(torch.arange(req, device=dev).repeat_interleave(nb))
    del src
    for _ in range(gen):
        q = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
        kivi_attention_decode(q, torch.randn_like(q), torch.randn_like(q), layer)
    torch.cuda.synchronize()
    idx = (torch.arange(B, device=dev) // nb) * nb + (torch.arange(B, device=dev) + 1) % nb
    idx = idx.to(torch.int32)
    slabs = layer._reorder_slabs(T0)
    moved = reorder.moved_bytes(slabs, B)
    us_reorder = _time(lambda: layer.reorder_(idx, group=nb, from_token=T0, check=False), args.iters)

    saved = [getattr(layer, n) for n in LENGTHS]

    def restore():
        for n, v in zip(LENGTHS, saved):
            setattr(layer, n, v)
    q1 = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
    k1 = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
    us_decode = _time(lambda: kivi_attention_decode(q1, k1, k1, layer), args.iters, restore)

    li = idx.long()
    members = [layer.kt, layer.vt, layer.k_res, layer.v_res, mfma.range_flags(layer.kt), mfma.range_flags(layer.vt)]
    whole = sum(x.numel() * x.element_size() for x in members)
    us_torch = _time(lambda: [x.copy_(x.index_select(0, li)) for x in members], max(args.iters // 5, 5))

    print(f"beam reorder, one layer: {req} requests x {nb} beams = {B} rows, nh = nh_kv = {nh}, D = 128, 2-bit g = 32 R = 32, "
          f"prompt {T0}, {gen} generated tokens (kv length {layer.kv_seq_len}), every row moved", flush=True)
    print(f"  slabs {len(slabs)}, moved suffix {moved / 2 / B / 1e6:.3f} MB per row, algorithmic traffic {moved / 1e6:.1f} MB "
          f"(read + write)")
    print(f"  reorder_ (kivi_cache_reorder)        {us_reorder:9.1f} us   {moved / (us_reorder * 1e-6) / 8e12:6.3f} of 8 TB/s")
    print(f"  decode step (kivi_mf_decode_layer)   {us_decode:9.1f} us   reorder / decode {us_reorder / us_decode:6.3f}")
    print(f"  torch index_select + copy_ of every member ({whole / 1e6:.1f} MB allocated)  {us_torch:9.1f} us   "
          f"{us_torch / us_reorder:6.1f}x the reorder")


if __name__ == "__main__":
    main()
