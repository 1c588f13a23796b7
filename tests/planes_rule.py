"""The rule of ``a3d_find_planes`` (include/agile3d_hip.h) restated on the host, independently of the package (not collected;
numpy only, no import of ``agile3d_amd``).  What many rows meet in is numpy int64 -- exact under the call's own bound
n 2^(2 bits) <= 2^62 -- or Python integers (the recentring, ``off``, the 128-bit sum of squared distances); the solve is
``normals_rule.stage_b``, float64 scalars one operation at a time; the tests a row passes are exact products in float64 and
int64.  The kernels are held to this bit for bit."""
import numpy as np

import normals_rule as NR

G, D, SCALE_BITS, MAX_PLANES = 16, 1024, 20, 16
SCALE = 1 << SCALE_BITS
OUT_CANDIDATE, OUT_NONFINITE, OUT_ZERO, OUT_FRAME, OUT_BINS = range(5)
LEFT_OUT = ("candidate", "nonfinite", "zero_normal", "frame", "bins")
BAD_INDEX = 1
F64, F32 = np.float64, np.float32
PLANE = np.dtype([("normal", "<f4", (3,)), ("offset", "<f4"), ("inliers", "<i4"), ("score", "<i4"), ("round", "<i4"), ("bin", "<i4"),
                  ("count", "<i8"), ("sum", "<i8", (3,)), ("mom", "<i8", (6,)), ("off", "<i8"), ("N", "<i4", (3,)), ("rms", "<f4")])


def direction_table():
    """int32 [3 G G, 3]: llrint(2^20 x the unit vector along e_a + u e_b + v e_c), u = (2 iu + 1 - G) / G, v likewise."""
    t = np.zeros((3, G, G, 3), F64)
    for a in range(3):
        for iu in range(G):
            for iv in range(G):
                d = np.zeros(3, F64)
                d[a], d[(a + 1) % 3], d[(a + 2) % 3] = 1.0, (2 * iu + 1 - G) / G, (2 * iv + 1 - G) / G
                t[a, iu, iv] = d / np.sqrt(d @ d)
    return np.rint(t * F64(SCALE)).astype(np.int32).reshape(-1, 3)


def settings(quantum, offset_bin, normal_deg, dist_tol):
    """``(bin_width, dist_tol_units, cos_min)``: world units -> 2^-20 quanta, rounded once each; the cosine rounded once."""
    to_units = lambda x: int(np.rint(F64(x) / F64(quantum) * F64(SCALE)))
    return to_units(offset_bin), to_units(dist_tol), min(max(float(np.cos(np.radians(F64(normal_deg)))), 0.0), 1.0)


def direction_cell(v):
    """``cell`` int64 [n] of fp32 normals [n, 3] (finite, not zero): the axis of largest magnitude (the lowest of equals), the
    canonical sign, and per other component the number of boundaries t_j = (j - G/2) / (G/2) with n_b >= t_j n_a."""
    v = np.asarray(v, F32).reshape(-1, 3)
    mag = np.abs(v)
    ax = np.zeros(len(v), np.int64)
    ax[mag[:, 1] > mag[np.arange(len(v)), ax]] = 1
    ax[mag[:, 2] > mag[np.arange(len(v)), ax]] = 2
    rows = np.arange(len(v))
    sign = np.where(v[rows, ax] < 0, F32(-1), F32(1))
    na, nb, nc = [(sign * v[rows, (ax + s) % 3]).astype(F64) for s in range(3)]
    t = (np.arange(1, G) - G // 2).astype(F64) * F64(2.0 / G)
    iu = (nb[:, None] >= t[None, :] * na[:, None]).sum(1)
    iv = (nc[:, None] >= t[None, :] * na[:, None]).sum(1)
    return (ax * G + iu) * G + iv


def admit(normals, positions, candidate, origin, quantum, bits, table, bin_width):
    """``(bin int64 [n] (-1: left out), X int64 [n, 3], reason int64 [n] (-1: admitted))``."""
    v, p = np.asarray(normals, F32).reshape(-1, 3), np.asarray(positions, F32).reshape(-1, 3)
    n = len(v)
    reason = np.full(n, -1, np.int64)
    X, in_frame = NR.fixed_point(p, origin, quantum, bits)
    finite = np.isfinite(v).all(1) & np.isfinite(p).all(1)
    with np.errstate(invalid="ignore"):
        zero = (v == 0).all(1)
    tests = [(OUT_CANDIDATE, np.zeros(n, bool) if candidate is None else np.asarray(candidate).reshape(-1) == 0),
             (OUT_NONFINITE, ~finite), (OUT_ZERO, zero), (OUT_FRAME, ~in_frame)]
    for code, failed in tests:
        reason[(reason < 0) & failed] = code
    ok = reason < 0
    bins = np.full(n, -1, np.int64)
    if ok.any():
        cell = direction_cell(v[ok])
        d = (np.asarray(table, np.int64)[cell] * X[ok]).sum(1)
        k = d // int(bin_width) + D // 2                    # (numpy's // on integers is the floor)
        inside = (k >= 0) & (k < D)
        at = np.flatnonzero(ok)
        reason[at[~inside]] = OUT_BINS
        bins[at[inside]] = cell[inside] * D + k[inside]
    return bins, X, reason


def sums_of(X):
    """``(cnt, S [3], M [6])`` as Python ints of int64 rows X [m, 3]."""
    S = [int(X[:, a].sum()) for a in range(3)]
    M = [int((X[:, a] * X[:, b]).sum()) for a, b in NR.MOMENT_PAIRS]
    return len(X), S, M


def fit(cnt, S, M):
    """``(normal fp32 [3], N [3] Python ints, off)`` of the plane through rows with these sums, or ``None`` (an invalid fit)."""
    normal, _, valid = NR.stage_b(cnt, S, M, (0.0, 0.0, 0.0), 1.0, None)
    if not valid:
        return None
    N = [int(np.rint(F64(normal[a]) * F64(SCALE))) for a in range(3)]
    R = [S[a] // cnt for a in range(3)]
    off = sum(N[a] * R[a] for a in range(3)) + sum(N[a] * (S[a] - cnt * R[a]) for a in range(3)) // cnt
    return normal, N, off


def inliers(plane, remaining, v64, X, cos_min, tol):
    normal, N, off = plane
    n64 = normal.astype(F64)
    dot = (n64[0] * v64[:, 0] + n64[1] * v64[:, 1]) + n64[2] * v64[:, 2]
    e = (X * np.array(N, np.int64)).sum(1) - np.int64(off)
    return remaining & (np.abs(dot) >= F64(cos_min)) & (np.abs(e) <= np.int64(tol))


def squared_distances(N, off, cnt, S, M):
    """The exact integer sum over the rows of (N . X - off)^2 from their sums."""
    NS = sum(N[a] * S[a] for a in range(3))
    NMN = sum((1 if a == b else 2) * N[a] * N[b] * M[k] for k, (a, b) in enumerate(NR.MOMENT_PAIRS))
    return NMN - 2 * off * NS + cnt * off * off


def record_floats(normal, off, cnt, E, origin, quantum):
    """``(offset fp32, rms fp32)`` of the header, every double operation rounded on its own."""
    n = normal.astype(F64)
    o = [F64(x) for x in origin]
    unit = F64(quantum) * F64(1.0 / SCALE)
    offset = F32(((n[0] * o[0] + n[1] * o[1]) + n[2] * o[2]) + F64(off) * unit)
    Ed = F64(E >> 64) * F64(2.0 ** 64) + F64(E & ((1 << 64) - 1))
    return offset, F32(np.sqrt(Ed / F64(cnt)) * unit)


def find_planes(normals, positions, origin, quantum, bits, bin_width, dist_tol, cos_min, min_voxels, max_planes, candidate=None,
                inverse_map=None, plane_full=None, table=None):
    """Everything ``a3d_find_planes`` writes, as a dict: ``plane_qv`` int32 [n], ``plane_full`` (with ``inverse_map``; entries
    of an index out of range keep what ``plane_full`` held, default -2), ``records`` (``PLANE``), ``summary``."""
    table = direction_table() if table is None else table
    v = np.asarray(normals, F32).reshape(-1, 3)
    n = len(v)
    assert n << (2 * bits) <= 1 << 62
    bins, X, reason = admit(v, positions, candidate, origin, quantum, bits, table, bin_width)
    with np.errstate(invalid="ignore"):
        v64 = np.where(np.isfinite(v), v, 0).astype(F64)
    H = np.bincount(bins[bins >= 0], minlength=3 * G * G * D).astype(np.int64).reshape(-1, D)
    plane_qv = np.full(n, -1, np.int32)
    records = np.zeros(MAX_PLANES, PLANE)
    n_planes = rounds = spent = 0
    stop = max(3, min_voxels // 4)
    for rnd in range(2 * max_planes if n else 0):
        score = H.copy()
        score[:, 1:] += H[:, :-1]
        score[:, :-1] += H[:, 1:]
        peak = int(np.argmax(score))                        # (the first of equals: the lowest flat bin)
        best = int(score.reshape(-1)[peak])
        if best < stop:
            break
        remaining = bins >= 0
        seeds = remaining & (bins // D == peak // D) & (np.abs(bins - peak) <= 1)
        assert int(seeds.sum()) == best
        plane = fit(*sums_of(X[seeds]))
        final = None
        for _ in range(2):
            if plane is None:
                break
            plane = fit(*sums_of(X[inliers(plane, remaining, v64, X, cos_min, dist_tol)]))
        if plane is not None:
            final = inliers(plane, remaining, v64, X, cos_min, dist_tol)
        rounds += 1
        if final is not None and int(final.sum()) >= min_voxels:
            cnt, S, M = sums_of(X[final])
            normal, N, off = plane
            r = records[n_planes]
            r["normal"], r["N"], r["off"], r["inliers"], r["count"], r["sum"], r["mom"] = normal, N, off, cnt, cnt, S, M
            r["score"], r["bin"], r["round"] = best, peak, rnd
            r["offset"], r["rms"] = record_floats(normal, off, cnt, squared_distances(N, off, cnt, S, M), origin, quantum)
            plane_qv[final] = n_planes
            n_planes += 1
            leave = final
        else:
            spent += 1
            leave = seeds
        np.subtract.at(H.reshape(-1), bins[leave], 1)
        bins[leave] = -1
        if n_planes >= max_planes:
            break
    out = dict(plane_qv=plane_qv, records=records[:n_planes].copy(),
               summary=dict(n_planes=n_planes, rounds=rounds, spent=spent, admitted=int((reason < 0).sum()), err=0,
                            left_out={name: int((reason == code).sum()) for code, name in enumerate(LEFT_OUT)}))
    if inverse_map is not None:
        rows = np.asarray(inverse_map, np.int64).reshape(-1)
        full = np.full(len(rows), -2, np.int32) if plane_full is None else np.array(plane_full, np.int32)
        inside = (rows >= 0) & (rows < n)
        full[inside] = plane_qv[rows[inside]]
        out["plane_full"] = full
        if not inside.all():
            out["summary"]["err"] |= BAD_INDEX
    return out
