"""Time one decode layer step with and without the per-row lead: kivi_gqa_decode_lead against kivi_gqa_decode --
the parent's call -- on the same cache, in the same process, with device events.

    python tools/decode_lead_time.py [--rounds N] [--reps N] [--log PATH]

Shapes: the headline (32 / 32 heads, B = 32, 4080 cached keys, 2 bits, residual 32: mf_row_kernel) and BASELINE config 4 (32 / 8
heads, B = 64, 8064 keys, 2 bits, residual 128: mf_row4_kernel, a block per row).  Per shape three settings of the leads:
  zero      0 in every row (the lead form must cost what the mask alone costs);
  uniform   drawn uniformly in [0, n - 64];
  short     three quarters of the rows at n - 64, the rest at 0: a batch of short requests beside long ones.
The additive mask holds the fp16 minimum under every row's lead in all forms.  The step is the stateless kivi_gqa_decode[_lead] on the
cache's own buffers (the lengths do not advance, so every call does the same work: the K append and the V flush rewrite the same
rows).  A timed item is `reps` back-to-back calls between two device events; one warm-up of every form, then `rounds` rounds with
the forms alternating -- mask alone, mask + lead, mask alone again (the spread of the two mask-only series is the noise floor of the
comparison); medians, microseconds per call.  `live` is the share of the packed K and V bytes of the launch that lie in units the
lead form walks (kivi_lead_plan.h): what a memory-bound kernel's time ratio should approach.  Lines go to stdout and to --log
(default profiles/decode_lead_time.log)."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, G32, SB = 128, 32, 512
FMIN = torch.finfo(torch.float16).min


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def events(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def step_args(layer, nh, q, kn, vn, mask, out):
    """kivi_gqa_decode_args of the NEXT step of `layer` (what kivi_mf_decode_layer builds, kivi_layer.hip: mf_decode_args)."""
    from kivi_amd import _lib
    d, hs = layer._desc(nh, q.device)[0], layer.host_step()
    return _lib.GqaDecodeArgs(
        B=d.B, nh=nh, nh_kv=d.nh_kv, D=d.D, group_size=d.group_size, bits=d.bits, inv_scale=d.inv_scale,
        q=q.data_ptr(), q_sb=q.stride(0), q_sh=q.stride(1), mask=mask.data_ptr(), mask_sb=mask.stride(0),
        kt=d.kt, kt_sb=d.kt_sb, kt_sh=d.kt_sh, kt_ss=d.kt_ss, Tq=hs.Tq,
        kres=d.k_res, kres_sb=d.kr_sb, kres_sh=d.kr_sh, kres_st=d.kr_st, knew=kn.data_ptr(), knew_sb=kn.stride(0), knew_sh=kn.stride(1),
        k_res_len=hs.k_res_len,
        vt=d.vt, vt_sb=d.vt_sb, vt_sh=d.vt_sh, vt_ss=d.vt_ss, Tv=hs.Tv,
        vres=d.v_res, vres_sb=d.vr_sb, vres_sh=d.vr_sh, vres_st=d.vr_st, v_win_start=hs.v_win_start, v_res_len=hs.v_res_len,
        vnew=vn.data_ptr(), vnew_sb=vn.stride(0), vnew_sh=vn.stride(1), v_flush=hs.v_flush,
        scores=d.scores, s_sb=d.s_sb, s_sh=d.s_sh, stats=d.stats, stats_bytes=d.stats_bytes,
        workspace=d.workspace, workspace_bytes=d.workspace_bytes, out=out.data_ptr(), out_sb=out.stride(0), out_sh=out.stride(1),
        residual_length=d.residual_length, v_window_rows=d.v_window_rows, kt_superblocks=d.cap // SB, vt_superblocks=d.cap // SB,
        flags=d.flags, kt_range=d.kt_range, vt_range=d.vt_range, dyn_step=None)


def live_share(lead, Tq, Tv):
    """share of the packed K (512-token super-blocks) and V (32-token blocks) tokens in units the lead form walks"""
    k = v = 0
    for p in lead:
        pk, pv = min(max(p, 0), Tq), min(max(p, 0), Tv)
        k += 0 if pk >= Tq else Tq - pk // SB * SB
        v += 0 if pv >= Tv else Tv - pv // 32 * 32
    return (k + v) / (len(lead) * (Tq + Tv))


def shape(say, dev, name, B, nh, nh_kv, T0, R, bits, rounds, reps):
    from kivi_amd import _lib
    from kivi_amd.attention import KiviConfig, make_layer_cache
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    layer = make_layer_cache(KiviConfig(bits, bits, G32, R), B, nh_kv, D, T0 + 8, dev, num_heads=nh)
    layer.prefill(torch.randn((B, nh_kv, T0, D), device=dev, dtype=torch.float16), torch.randn((B, nh_kv, T0, D), device=dev, dtype=torch.float16))
    layer.ensure_room(1)
    n = T0 + 1
    q, kn, vn = (torch.randn((B, h, 1, D), generator=g).half().to(dev) for h in (nh, nh_kv, nh_kv))
    out = torch.empty((B, nh, 1, D), dtype=torch.float16, device=dev)
    Tq, Tv = layer.k_quant_len, layer.v_quant_len
    plan = lib.kivi_mf_launch_plan(B, nh, nh_kv, Tq, layer.k_res_len, R, layer._flags(), bits, 0)
    say(f"{name}: {nh} / {nh_kv} heads, B = {B}, n = {n} keys (Tq = {Tq}, Tv = {Tv}), {bits} bits, residual {R}; launch plan {plan}; "
        f"medians of {rounds} alternating rounds of {reps} calls, microseconds per layer step")
    say(f"  {'leads':>8s} {'live':>6s} | {'mask (a)':>9s} {'mask (b)':>9s} {'spread':>7s} | {'mask+lead':>9s} {'lead/mask':>9s} | max |diff|")
    settings = (("zero", [0] * B), ("uniform", torch.randint(0, n - 63, (B,), generator=g).tolist()),
                ("short", [n - 64 if b % 4 else 0 for b in range(B)]))
    stream = _lib.stream_ptr(q)
    for label, lead_list in settings:
        lead = torch.tensor(lead_list, dtype=torch.int32, device=dev)
        mask = torch.zeros((B, 1, 1, n), dtype=torch.float16, device=dev)
        mask.masked_fill_((torch.arange(n, device=dev)[None] < lead[:, None].long())[:, None, None, :], FMIN)
        a = step_args(layer, nh, q, kn, vn, mask, out)

        def plain():
            _lib.check(lib.kivi_gqa_decode(ctypes.byref(a), stream), "kivi_gqa_decode")

        def led():
            _lib.check(lib.kivi_gqa_decode_lead(ctypes.byref(a), lead.data_ptr(), stream), "kivi_gqa_decode_lead")
        plain()                                                  # warm-up of both forms, and what they compute
        o_mask = out.clone()
        led()
        diff = (out.float() - o_mask.float()).abs().max().item()
        assert bool(torch.isfinite(out).all())
        ts = {"a": [], "lead": [], "b": []}
        for _ in range(rounds):
            ts["a"].append(events(plain, reps))
            ts["lead"].append(events(led, reps))
            ts["b"].append(events(plain, reps))
        ta, tb, tl = _median(ts["a"]), _median(ts["b"]), _median(ts["lead"])
        tm = 0.5 * (ta + tb)
        say(f"  {label:>8s} {live_share(lead_list, Tq, Tv):6.3f} | {ta:9.1f} {tb:9.1f} {abs(ta - tb) / tm:7.3f} | {tl:9.1f} {tl / tm:9.3f} | {diff:.2e}")
    del layer
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "decode_lead_time.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing is measured", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f, torch.no_grad():
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        say("one decode layer step, the mask alone against the mask and the per-row lead (tools/decode_lead_time.py)")
        shape(say, dev, "headline", 32, 32, 32, 4080, 32, 2, args.rounds, args.reps)
        shape(say, dev, "BASELINE config 4", 64, 32, 8, 8064, 128, 2, args.rounds, args.reps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
