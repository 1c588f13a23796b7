"""The rule of ``a3d_point_index_nearest`` (include/agile3d_hip.h) restated in numpy as the brute force it is defined by, for the
host tests (CPU) and the GPU tests of the label transfer.  Nothing of the index appears here: no cells, no keys, no table.

For query q, over every source row p whose three coordinates are finite: d2 = ((px-qx)^2 + (py-qy)^2) + (pz-qz)^2 in
``np.float32`` operations, one rounding each (``pick_rule.fp32_rule_argmin``'s arithmetic); r2 = fl32(r) * fl32(r) rounded
once; the answer is the FIRST arg-min of d2 among the rows with d2 <= r2, else -1 with d2 = +inf; a query that is not finite
gets -1.  The first arg-min is taken over the keys (bits of d2, row): d2 >= +0 and never NaN, so its bits order as it does,
and a row out of reach has a key above every real one -- an accepted d2 of +inf (r2 = +inf) still wins over no row at all.
"""
import numpy as np

F32 = np.float32
MAX_CELLS = 1 << 20
UNKEYABLE = 1                # the bit of the summary's error word


def nearest(src, queries, max_distance, labels=None, fill=0, chunk=256):
    """dict: ``nearest`` int32 [m], ``d2`` fp32 [m], ``labels`` int32 [m] or None, and the summary's counts ``matched``,
    ``unmatched``, ``nonfinite``, ``source_left_out``."""
    src = np.ascontiguousarray(src, F32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, F32).reshape(-1, 3)
    r = F32(max_distance)
    with np.errstate(all="ignore"):
        r2 = F32(r * r)
    finite = np.isfinite(src).all(1)
    sound = np.isfinite(q).all(1)
    rows = np.arange(len(src), dtype=np.uint64)
    out = np.full(len(q), -1, np.int32)
    d2_out = np.full(len(q), np.inf, F32)
    with np.errstate(all="ignore"):
        for a in range(0, len(q), chunk):
            if not len(src):
                break
            d = src[None, :, :] - q[a:a + chunk, None, :]
            s = d * d
            d2 = (s[..., 0] + s[..., 1]) + s[..., 2]
            ok = finite[None, :] & (d2 <= r2) & sound[a:a + chunk, None]
            key = np.where(ok, d2.view(np.uint32).astype(np.uint64) << np.uint64(32) | rows[None, :], np.uint64(2 ** 64 - 1))
            best = key.argmin(1)
            hit = ok[np.arange(len(best)), best]
            out[a:a + chunk] = np.where(hit, best, -1)
            d2_out[a:a + chunk] = np.where(hit, d2[np.arange(len(best)), best], F32(np.inf))
    lab = None
    if labels is not None:
        labels = np.asarray(labels, np.int32)
        lab = np.where(out >= 0, labels[np.maximum(out, 0)] if len(labels) else fill, fill).astype(np.int32)
    matched = int((out >= 0).sum())
    return dict(nearest=out, d2=d2_out, labels=lab, matched=matched, unmatched=int(sound.sum()) - matched,
                nonfinite=int((~sound).sum()), source_left_out=int((~finite).sum()))


def unkeyable(src, cell_size):
    """True when a finite source row lies beyond 2^20 cells on some axis: |floor(fl32(x / cell_size))| > 2^20."""
    src = np.ascontiguousarray(src, F32).reshape(-1, 3)
    src = src[np.isfinite(src).all(1)]
    with np.errstate(all="ignore"):
        return bool((np.abs(np.floor(src / F32(cell_size))) > MAX_CELLS).any())
