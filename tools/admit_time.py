"""Time admit_() of one layer's cache (kivi_cache_admit) with device events, next to the torch composition of the same move.

    python tools/admit_time.py [--rounds N]

Shape: Llama-2-7B geometry, a living cache of B = 32 rows, 32 / 32 heads, 2-bit g = 32 R = 32 at L = 4096 (a 4091-token prompt + 5
decode steps, so its ring window stands at phase 5), and a source of n = 1 and n = 8 rows from a prompt pass at 4096 (phase 0).
Per round, each between two device events: admit_() (ONE launch for all stores), and the same move composed from torch -- one
index_copy_ per buffer on the rows (the super-blocks in use of both stores, their range words, the live K residual rows) and an
indexed assignment of the window tokens rotated from the source's ring phase to the destination's.  Medians over the rounds.  Two modes:
  cold    a 512 MiB buffer is cleared before every timed item, which evicts the Infinity Cache (256 MiB) and keeps the device busy
          while the host enqueues the item: the item's launches are queued back to back;
  warm    the device is idle (synchronised) before every timed item and the bytes it moves were touched by the item before it.
The expectation: the launch is no slower than the composition in the same run.  The fraction of 8 TB/s is on 2 x the bytes moved
(read + write)."""
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
    from kivi_amd import admit
    from kivi_amd.attention import KiviConfig, kivi_attention_decode, make_layer_cache
    from kivi_amd.quant import mfma
    dev = "cuda"
    torch.manual_seed(0)
    B, nh, L, steps = 32, 32, 4096, 5
    cfg = KiviConfig(2, 2, 32, 32)

    def prompt_cache(rows, T):
        lc = make_layer_cache(cfg, rows, nh, 128, L + 64, dev, num_heads=nh)
        k0 = torch.randn((rows, nh, T, 128), device=dev, dtype=torch.float16)
        lc.prefill(k0, torch.randn_like(k0))
        return lc
    dst = prompt_cache(B, L - steps)
    for _ in range(steps):
        q = torch.randn((B, nh, 1, 128), device=dev, dtype=torch.float16)
        kivi_attention_decode(q, torch.randn_like(q), torch.randn_like(q), dst)
    torch.cuda.synchronize()
    assert dst.kv_seq_len == L and dst.v_res_start == steps
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    R1 = dst.v_res.shape[2]

    def one(fn, cold):
        if cold:
            flush.zero_()
        else:
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    print(f"admission into one layer: B = {B}, nh = nh_kv = {nh}, D = 128, 2-bit g = 32 R = 32, kv length {L} (destination ring phase "
          f"{dst.v_res_start}, source phase 0), medians of {args.rounds} interleaved rounds", flush=True)
    ok = True
    for n in (1, 8):
        src = prompt_cache(n, L)
        rows = torch.arange(n, device=dev) * 3 + 1                     # rows 1, 4, 7, ...
        slabs = admit.live(dst._admit_slabs(src))
        moved = admit.moved_bytes(slabs, n)
        used_k, used_v = -(-dst.k_quant_len // 512), -(-dst.v_quant_len // 512)
        ring = (dst.v_res_start + torch.arange(dst.v_res_len, device=dev)) % R1

        def launch():
            dst.admit_(rows, src, check=False)

        def composed():
            dst.kt[:, :, :used_k].index_copy_(0, rows, src.kt[:, :, :used_k])
            dst.vt[:, :, :used_v].index_copy_(0, rows, src.vt[:, :, :used_v])
            mfma.range_flags(dst.kt).index_copy_(0, rows, mfma.range_flags(src.kt))
            mfma.range_flags(dst.vt).index_copy_(0, rows, mfma.range_flags(src.vt))
            if dst.k_res_len:
                dst.k_res[:, :, : dst.k_res_len].index_copy_(0, rows, src.k_res[:, :, : dst.k_res_len])
            dst.v_res[rows[:, None], :, ring[None, :]] = src.v_res_view().transpose(1, 2)

        def in_use(c):
            return [c.kt[:, :, :used_k], c.vt[:, :, :used_v], c.k_res[:, :, : c.k_res_len], c.v_res[:, :, ring],
                    mfma.range_flags(c.kt), mfma.range_flags(c.vt)]
        composed()
        want = [t.clone() for t in in_use(dst)]
        dst.kt[rows], dst.vt[rows], dst.v_res[rows] = 0, 0, 0          # the launch has to put them back
        launch()
        same = all(torch.equal(a, b) for a, b in zip(in_use(dst), want))
        print(f"  n = {n} rows: {len(slabs)} slabs, {moved / 2e6:.2f} MB per admission ({moved / 1e6:.2f} MB read + write); "
              f"launch and composition leave the same bytes: {same}")
        ok = ok and same
        items = [("admit_()  (kivi_cache_admit, one launch)", launch), ("torch composition (index_copy_ per buffer + ring assignment)", composed)]
        for cold in (True, False):
            for _, fn in items:
                one(fn, cold)
            ts = {name: [] for name, _ in items}
            for _ in range(args.rounds):
                for name, fn in items:
                    ts[name].append(one(fn, cold))
            r = {name: _median(v) for name, v in ts.items()}
            print(f"    {'cold (Infinity Cache evicted, launches queued)' if cold else 'warm (device idle before)'}:")
            for name, _ in items:
                print(f"      {name:62s} {r[name]:9.1f} us   {moved / (r[name] * 1e-6) / 8e12:6.3f} of 8 TB/s")
            a, b = r[items[0][0]], r[items[1][0]]
            print(f"      admit_() vs torch: {a / b:6.3f}x   (expectation: no slower -- {'holds' if a <= b else 'MISSED'})")
            ok = ok and a <= b
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
