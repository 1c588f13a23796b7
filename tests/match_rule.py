"""The rule of ``a3d_feature_prototypes`` and ``a3d_feature_match`` (include/agile3d_hip.h) restated on the host,
independently of the package (not collected; numpy only, no import of ``agile3d_amd``): fixed-point sums in int64, the caller's
prototype step, the 128-step loops in float64 with one accumulator each, one scan over the prototypes in ascending order with
the division-free comparisons, the score.  Every decision is exact, so the kernels are held to these bit for bit; the score is
a double rounded once to fp32, and the kernels are held to it within one fp32 ulp."""
import numpy as np

CHANNELS = 128
QUANTUM = 2.0 ** -20
LIMIT = 2.0 ** 40
MAX_ROWS = 1 << 22
MAX_PROTOTYPES = 256
BAD_CLASS, BAD_INDEX, BAD_PROTOTYPE = 1, 2, 4
F32, F64 = np.float32, np.float64


def prototypes(feats, classes, n_classes=MAX_PROTOTYPES):
    """``dict(sums int64 [n_classes, 128], count int32 [n_classes], examples, examples_left_out, err)``."""
    f = np.asarray(feats, F32).reshape(-1, CHANNELS)
    cls = np.asarray(classes, np.int64).reshape(-1)
    assert len(f) == len(cls) < MAX_ROWS and 1 <= n_classes <= MAX_PROTOTYPES
    sums, count = np.zeros((n_classes, CHANNELS), np.int64), np.zeros(n_classes, np.int32)
    bad = (cls < -1) | (cls >= n_classes)
    rows = np.flatnonzero((cls >= 0) & ~bad)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(f[rows].astype(F64) / QUANTUM)                       # (the quotient is exact; to nearest even)
        ok = (np.abs(x) <= LIMIT).all(1)                                 # (a NaN fails the comparison)
    for r, xr in zip(rows[ok], x[ok]):
        sums[cls[r]] += xr.astype(np.int64)
        count[cls[r]] += 1
    return dict(sums=sums, count=count, examples=int(ok.sum()), examples_left_out=int((~ok).sum()), err=BAD_CLASS if bad.any() else 0)


def prototype_table(sums, count):
    """``{class: fp32 [128]}`` for the classes with ``count > 0``: ``float32((float64(sum) / float64(count)) * quantum)``."""
    return {c: ((sums[c].astype(F64) / F64(count[c])) * QUANTUM).astype(F32) for c in range(len(count)) if count[c] > 0}


def _ordered_sum(a, b):
    """sum over the last axis of a * b in float64, one accumulator, ascending (the products of fp32 values are exact)."""
    acc = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], F64)
    for i in range(CHANNELS):
        acc = acc + a[..., i] * b[..., i]
    return acc


def match(feats, protos, proto_class, cos_min, candidate=None, inverse_map=None):
    """The outputs of ``a3d_feature_match`` as a dict of numpy arrays and ints.  With ``inverse_map``: ``match_full`` and
    ``score_full``, entries with an index outside the rows left at the sentinels -7 / -7.0, and the ``BAD_INDEX`` bit."""
    f32 = np.asarray(feats, F32).reshape(-1, CHANNELS)
    p32 = np.asarray(protos, F32).reshape(-1, CHANNELS)
    cls = np.asarray(proto_class, np.int64).reshape(-1)
    n, k = len(f32), len(p32)
    assert 1 <= k <= MAX_PROTOTYPES and len(cls) == k and 0.0 <= cos_min <= 1.0
    c2 = F64(cos_min) * F64(cos_min)
    f, p = f32.astype(F64), p32.astype(F64)
    err = 0
    with np.errstate(all="ignore"):
        nn, pp = _ordered_sum(f, f), _ordered_sum(p, p)
        dot = _ordered_sum(f[:, None, :], p[None, :, :])                 # [n, k]
        odd = ~np.isfinite(f32).all(1)
        can = ~odd & (nn > 0)
        if candidate is not None:
            can &= np.asarray(candidate).reshape(-1) != 0
        best, match_ = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        b_dot, b_d2, b_pp = np.zeros(n), np.zeros(n), np.ones(n)
        m_d2, m_pp = np.zeros(n), np.ones(n)
        for c in range(k):
            if not pp[c] < np.inf:
                err |= BAD_PROTOTYPE
            if not 0 <= cls[c] < MAX_PROTOTYPES:
                err |= BAD_CLASS
            if not 0.0 < pp[c] < np.inf:
                continue
            d = dot[:, c]
            d2 = d * d
            sa, sb = np.sign(d), np.sign(b_dot)
            left, right = d2 * b_pp, b_d2 * pp[c]
            beats = np.where(sa != sb, sa > sb, np.where(sa > 0, left > right, np.where(sa < 0, left < right, False)))
            take = can & ((best < 0) | beats)
            best[take], b_dot[take], b_d2[take], b_pp[take] = c, d[take], d2[take], pp[c]
            passes = can & (d > 0) & (d2 >= c2 * (nn * pp[c]))
            take = passes & ((match_ < 0) | (d2 * m_pp > m_d2 * pp[c]))
            match_[take], m_d2[take], m_pp[take] = c, d2[take], pp[c]
        score = np.where(best >= 0, (b_dot / np.sqrt(nn * b_pp)).astype(F32), F32(0.0)).astype(F32)
    match_qv = np.where(match_ >= 0, cls[np.maximum(match_, 0)], -1).astype(np.int32)
    counted = match_qv[(match_ >= 0) & (match_qv >= 0) & (match_qv < MAX_PROTOTYPES)]
    out = dict(match_qv=match_qv, best_qv=best.astype(np.int32), score_qv=score, rows_nonfinite=int(odd.sum()),
               matched=np.bincount(counted, minlength=MAX_PROTOTYPES).astype(np.int64))
    if inverse_map is not None:
        inv = np.asarray(inverse_map, np.int64).reshape(-1)
        valid = (inv >= 0) & (inv < n)
        out["match_full"], out["score_full"] = np.full(len(inv), -7, np.int32), np.full(len(inv), -7.0, F32)
        out["match_full"][valid], out["score_full"][valid] = match_qv[inv[valid]], score[inv[valid]]
        if not valid.all():
            err |= BAD_INDEX
    out["err"] = err
    return out


def ulps(a, b):
    """The distance of two fp32 arrays in units in the last place (finite values of one sign, or zeros)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
