"""What the three row movers (reorder.py, checkpoint.py, admit.py) do with a slab list before their library call.  A slab is the tuple
reorder.slab returns, (base, row stride, [(count, stride)], run), or the two-sided one of admit.slab, (dst base, dst row stride,
[dst strides], src base, src row stride, [src strides], [counts], run)."""
from __future__ import annotations

from . import _lib


def row_bytes(s) -> int:
    """Bytes of one row the slab names: the run times its three level counts."""
    if len(s) == 8:
        return s[7] * s[6][0] * s[6][1] * s[6][2]
    return s[3] * s[2][0][0] * s[2][1][0] * s[2][2][0]


def live(slabs):
    """The slabs that move something (a positive run and positive counts): the others take no descriptor (and no room in a snapshot
    buffer row)."""
    return [s for s in slabs if s[-1] > 0 and (min(s[6]) if len(s) == 8 else min(s[2])[0]) > 0]


def arrays(slabs):
    """The live slabs as ReorderSlab / AdmitSlab arrays of at most KIVI_REORDER_MAX_SLABS, one library call each."""
    slabs, out = live(slabs), []
    for i in range(0, len(slabs), _lib.REORDER_MAX_SLABS):
        part = slabs[i: i + _lib.REORDER_MAX_SLABS]
        arr = ((_lib.ReorderSlab if len(part[0]) == 4 else _lib.AdmitSlab) * len(part))()
        for d, s in zip(arr, part):
            if len(s) == 4:
                d.base, d.row_stride, levels, d.run = s
                for k, (n, st) in enumerate(levels):
                    d.n[k], d.stride[k] = n, st
            else:
                d.dst_base, d.dst_row_stride, dst, d.src_base, d.src_row_stride, src, cnt, d.run = s
                for k in range(3):
                    d.dst_stride[k], d.src_stride[k], d.n[k] = dst[k], src[k], cnt[k]
        out.append(arr)
    return out
