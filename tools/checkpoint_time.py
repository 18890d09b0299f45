"""Time checkpoint() and restore_() of one layer's cache (kivi_cache_snapshot) with device events.

    python tools/checkpoint_time.py [--rounds N]

Shape: Llama-2-7B geometry, B = 32 rows, 32 / 32 heads, 2-bit g = 32 R = 32, a 4096-token prompt + 31 decode steps, so the K
residual is as full as it gets (31 keys).  Per round, in this order and each between two device events: checkpoint(), the same
bytes saved member by member with torch (clone of the live k_res rows, the V ring, both stores' range words -- what can be done
without the snapshot kernel), restore_(), the torch copy_ of those members back, clone() of the layer (the only rollback there was)
and the decode step of the cache.  Medians over the rounds.  Two modes:
  cold    a 512 MiB buffer is cleared before every timed item, which evicts the Infinity Cache (256 MiB) and keeps the device busy
          while the host enqueues the item: the item's launches are queued back to back;
  warm    the device is idle (synchronised) before every timed item and the ~17 MB it moves were touched by the item before it, so they
          are served from the Infinity Cache, and a multi-launch item shows the host's enqueue gaps.
The one condition (both modes): checkpoint() and restore_() are each no slower than their torch counterparts in the same run.
The fraction of 8 TB/s is on the moved bytes (read + write)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    from kivi_amd import checkpoint
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    from kivi_amd.quant import mfma
    dev = "cuda"
    torch.manual_seed(0)
    B, nh, T0, steps = 32, 32, 4096, 31
    layer = make_layer_cache(KiviConfig(2, 2, 32, 32), B, nh, 128, T0 + steps + 64, dev, num_heads=nh)
    k0 = torch.randn((B, nh, T0, 128), device=dev, dtype=torch.float16)
    layer.prefill(k0, torch.randn_like(k0))
    del k0
    for _ in range(steps):
        q = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
        kivi_attention_decode(q, torch.randn_like(q), torch.randn_like(q), layer)
    torch.cuda.synchronize()
    assert layer.k_res_len == 31 and layer.kv_seq_len == T0 + steps

    moved = 2 * B * checkpoint.row_bytes(layer._checkpoint_slabs())
    members = lambda: [layer.k_res[:, :, : layer.k_res_len], layer.v_res, mfma.range_flags(layer.kt), mfma.range_flags(layer.vt)]   # noqa: E731
    base = layer.checkpoint()
    saved = [x.clone() for x in members()]
    q1 = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
    k1 = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    held = {}

    def decode():
        kivi_attention_decode(q1, k1, k1, layer)

    items = [("checkpoint()              (kivi_cache_snapshot, gather)", lambda: held.__setitem__("ck", layer.checkpoint()), None),
             ("torch clone of the members (4 copies)", lambda: held.__setitem__("t", [x.clone() for x in members()]), None),
             ("restore_()                (kivi_cache_snapshot, scatter)", lambda: layer.restore_(base), None),
             ("torch copy_ of the members back (4 copies)", lambda: [x.copy_(s) for x, s in zip(members(), saved)], None),
             ("clone() of the layer", lambda: held.__setitem__("c", layer.clone()), lambda: held.pop("c")),
             ("decode step (kivi_mf_decode_layer)", decode, lambda: layer.restore_(base))]

    def one(fn, after, cold):
        if cold:
            flush.zero_()
        else:
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if after:
            after()
        return a.elapsed_time(b) * 1e3

    results = {}
    for cold in (True, False):
        for fn_name, fn, after in items:          # warm-up of every item
            one(fn, after, cold)
        ts = {name: [] for name, _, _ in items}
        for _ in range(args.rounds):
            for name, fn, after in items:
                ts[name].append(one(fn, after, cold))
        results[cold] = {name: _median(v) for name, v in ts.items()}

    whole = layer.allocated_bytes()
    print(f"checkpoint / restore, one layer: B = {B}, nh = nh_kv = {nh}, D = 128, 2-bit g = 32 R = 32, prompt {T0} + {steps} steps "
          f"(kv length {layer.kv_seq_len}, {layer.k_res_len} residual keys), medians of {args.rounds} interleaved rounds", flush=True)
    print(f"  a checkpoint holds {base.nbytes() / 1e6:.2f} MB; the layer's cache {whole / 1e6:.1f} MB allocated, "
          f"{layer.nbytes() / 1e6:.1f} MB in use; moved per call {moved / 1e6:.1f} MB (read + write)")
    names = [n for n, _, _ in items]
    ok = True
    for cold in (True, False):
        r = results[cold]
        print(f"  {'cold (Infinity Cache evicted, launches queued)' if cold else 'warm (device idle before, bytes in the Infinity Cache)'}:")
        for n in names:
            extra = f"   {moved / (r[n] * 1e-6) / 8e12:6.3f} of 8 TB/s" if n in names[:4] else ""
            print(f"    {n:58s} {r[n]:9.1f} us{extra}")
        for mine, theirs in ((names[0], names[1]), (names[2], names[3])):
            verdict = "holds" if r[mine] <= r[theirs] else "MISSED"
            ok = ok and r[mine] <= r[theirs]
            print(f"    {mine.split('(')[0].strip()} vs torch: {r[mine] / r[theirs]:6.3f}x   (condition: no slower -- {verdict})")
        print(f"    clone() / checkpoint() {r[names[4]] / r[names[0]]:6.1f}x   checkpoint() / decode step {r[names[0]] / r[names[5]]:6.3f}   "
              f"restore_() / decode step {r[names[2]] / r[names[5]]:6.3f}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
