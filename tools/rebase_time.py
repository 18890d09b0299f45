"""Time the rebase of one layer's cache (two kivi_mf_store_shift launches) with device events, next to the
out-of-place torch composition of the same move.

    python tools/rebase_time.py [--rounds N]

Shape: Llama-2-7B geometry, a living cache of B = 32 rows, 32 / 32 heads, 2-bit g = 32 R = 32; drops of 512 and of 2048 tokens at
kv length 4096 and of 32 tokens at 700.  Per round, each between two device events: the cache's `_rebase_buffers(drop)` at fixed
lengths (what rebase_ enqueues: per store the range words zeroed and ONE launch), and the same move composed from torch, out of
place: per store a clone of the kept super-blocks copied back and the vacated ones zeroed (a drop of whole super-blocks), or the
blocks in use gathered into a new tensor, shifted and copied back (any other drop).  The composition does not recompute the range
words.  Medians over the rounds.  Two modes, as tools/admit_time.py defines them:
  cold    a 512 MiB buffer is cleared before every timed item, which evicts the Infinity Cache (256 MiB) and keeps the device busy
          while the host enqueues the item: the item's launches are queued back to back;
  warm    the device is idle (synchronised) before every timed item and the bytes it moves were touched by the item before it.
The expectation: the launches are no slower than the composition in the same run.  The fraction of 8 TB/s is on the bytes read +
written (every kept block once each way, the vacated blocks written).  The launch needs no second copy of the store: the bytes the
composition allocates for its clone are printed."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def _block_views(st, is_k, n_sb):
    """The codes and the scale / zero-point pieces of the first n_sb super-blocks as (B, h, n_sb, 16, ...) views indexed by block."""
    B, h, _, W = st.shape
    C = W - 2048
    st = st[:, :, :n_sb]
    codes = st[..., :C].view(B, h, n_sb, 16, C // 16)
    sm = st[..., C:]
    if is_k:       # word (region, g >> 3, p, g & 7, 4 words) of the 2048 (kt_sm_half): block g = (g >> 3, g & 7)
        sm = sm.view(B, h, n_sb, 2, 2, 16, 8, 4).permute(0, 1, 2, 4, 6, 3, 5, 7)
    else:          # word (region, g, 64 words)
        sm = sm.view(B, h, n_sb, 2, 16, 64).permute(0, 1, 2, 4, 3, 5)
    return codes, sm


def composed_shift(st, is_k, n_blocks, shift):
    """Blocks [shift, n_blocks) -> [0, n_blocks - shift), the vacated ones zeroed, out of place.  -> bytes of the temporary."""
    B, h = st.shape[:2]
    n_sb, keep = -(-n_blocks // 16), n_blocks - shift
    if shift % 16 == 0:
        s, k = shift // 16, -(-keep // 16)
        tmp = st[:, :, s: s + k].clone()
        st[:, :, :k].copy_(tmp)
        st[:, :, k: n_sb].zero_()
        return tmp.numel() * 4
    extra = 0
    for x in _block_views(st, is_k, n_sb):
        flat = x.reshape(B, h, n_sb * 16, -1)                      # the copy: x is not contiguous over the super-blocks
        new = torch.zeros_like(flat)
        new[:, :, :keep] = flat[:, :, shift: n_blocks]
        new[:, :, n_blocks:] = flat[:, :, n_blocks:]
        x.copy_(new.view(x.shape))
        extra += 2 * flat.numel() * 4
    return extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    from kivi_amd import rebase
    from kivi_amd.attention import KiviConfig, make_layer_cache
    dev = "cuda"
    torch.manual_seed(0)
    B, nh = 32, 32
    cfg = KiviConfig(2, 2, 32, 32)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

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

    print(f"rebase of one layer: B = {B}, nh = nh_kv = {nh}, D = 128, 2-bit g = 32 R = 32, medians of {args.rounds} interleaved rounds",
          flush=True)
    ok = True
    caches = {}
    for L, drop in ((4096, 512), (4096, 2048), (700, 32)):
        if L not in caches:
            caches.clear()
            lc = make_layer_cache(cfg, B, nh, 128, L + 64, dev, num_heads=nh)
            k0 = torch.randn((B, nh, L, 128), device=dev, dtype=torch.float16)
            lc.prefill(k0, torch.randn_like(k0))
            del k0
            caches[L] = (lc, lc.kt.clone(), lc.vt.clone())
        lc, kt0, vt0 = caches[L]
        stores = [(lc.kt, True, -(-lc.k_quant_len // 32)), (lc.vt, False, -(-lc.v_quant_len // 32))]
        shift = drop // 32
        moved = sum(rebase.moved_bytes(st, 2, n, shift) for st, _, n in stores)

        def launch():
            lc._rebase_buffers(drop)

        def composed():
            return sum(composed_shift(st, is_k, n, shift) for st, is_k, n in stores)
        # the same bytes first, from the same start
        lc.kt.copy_(kt0), lc.vt.copy_(vt0)
        tmp_bytes = composed()
        want = [lc.kt.clone(), lc.vt.clone()]
        lc.kt.copy_(kt0), lc.vt.copy_(vt0)
        launch()
        same = torch.equal(lc.kt, want[0]) and torch.equal(lc.vt, want[1])
        del want
        print(f"  drop {drop} of {L}: K {stores[0][2]} blocks, V {stores[1][2]} blocks, {shift} blocks down; {moved / 1e6:.2f} MB read + "
              f"written; launch and composition leave the same stores: {same}; the composition's temporaries: {tmp_bytes / 1e6:.2f} MB, "
              f"the launch's: 0", flush=True)
        ok = ok and same
        items = [("_rebase_buffers  (kivi_mf_store_shift, one launch per store)", launch), ("torch composition, out of place", composed)]
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
                print(f"      {name:62s} {r[name]:9.1f} us   {moved / (r[name] * 1e-6) / 8e12:6.3f} of 8 TB/s   "
                      f"({moved / (r[name] * 1e-6) / 6.29e12:5.3f} of the 6.29 TB/s float4 copy)")
            a, b = r[items[0][0]], r[items[1][0]]
            print(f"      launches vs torch: {a / b:6.3f}x   (expectation: no slower -- {'holds' if a <= b else 'MISSED'})", flush=True)
            ok = ok and a <= b
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
