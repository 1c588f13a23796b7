"""The rules of ``a3d_estimate_normals`` and ``a3d_cull_points`` (include/agile3d_hip.h) restated on the host, independently
of the package (not collected; numpy only, no import of ``agile3d_amd``).  Stage A and the recentring are Python integers;
stage B is numpy float64 SCALARS, one operation at a time in the header's order, so that every intermediate is rounded once
as the kernel rounds it.  The kernels are held to these bit for bit.  ``estimate`` is that restatement; ``estimate_large`` forms
the integer sums with numpy int64 instead (exact under the call's own overflow bound) so that a scene of a quarter of a
million voxels takes seconds -- ``test_normals_host.py`` holds it to ``estimate``."""
import math

import numpy as np

RANGE, BAD_INDEX = 1, 2
SWEEPS = 6
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))          # (p, q, the third index)
MOMENT_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
CULL_BACK, CULL_FRONT = 1, 2
F64, F32 = np.float64, np.float32


def fixed_point(xyz, origin, quantum, bits):
    """``(X int64 [n, 3], ok bool [n])``: X_a = llrint(((double)x_a - origin[a]) / quantum), ok = |X_a| <= 2^bits on every axis
    (a NaN or an infinity fails)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((np.asarray(xyz, F32).astype(F64) - np.asarray(origin, F64)) / F64(quantum))
        ok = (np.abs(r) <= F64(2.0 ** bits)).all(1)
    return np.where(ok[:, None], r, 0.0).astype(np.int64), ok


def stage_a(n, xyz, inverse_map, origin, quantum, bits):
    """``(words: list of n lists of 10 Python ints (cnt, X, Y, Z, XX, XY, XZ, YY, YZ, ZZ), counted, err)``."""
    X, ok = fixed_point(xyz, origin, quantum, bits)
    rows = np.arange(len(X)) if inverse_map is None else np.asarray(inverse_map, np.int64)
    words = [[0] * 10 for _ in range(n)]
    counted = err = 0
    for i, row in enumerate(rows.tolist()):
        inside = 0 <= row < n
        if not inside:
            err |= BAD_INDEX
        if not ok[i]:
            err |= RANGE
        if not (inside and ok[i]):
            continue
        x = [int(v) for v in X[i]]
        w = words[row]
        w[0] += 1
        for a in range(3):
            w[1 + a] += x[a]
        for k, (a, b) in enumerate(MOMENT_PAIRS):
            w[4 + k] += x[a] * x[b]
        counted += 1
    return words, counted, err


def neighbourhoods(coords4):
    """Per row the rows of the 27 cells around it that exist in the same batch sample (itself included)."""
    c = np.asarray(coords4, np.int64).reshape(-1, 4).tolist()
    where = {tuple(p): i for i, p in enumerate(c)}
    out = []
    for b, x, y, z in c:
        out.append([j for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
                    if (j := where.get((b, x + dx, y + dy, z + dz))) is not None])
    return out


def recentre(N, S, M):
    """``(R, s, m)`` in Python integers: R_a = floor(S_a / N), s_a = S_a - N R_a, m_ab = M_ab - R_a S_b - R_b S_a + N R_a R_b
    (m in the order of MOMENT_PAIRS)."""
    R = [S[a] // N for a in range(3)]
    s = [S[a] - N * R[a] for a in range(3)]
    m = [M[k] - R[a] * S[b] - R[b] * S[a] + N * R[a] * R[b] for k, (a, b) in enumerate(MOMENT_PAIRS)]
    return R, s, m


def jacobi(C):
    """SWEEPS cyclic sweeps over PAIRS on the symmetric 3 x 3 list-of-lists ``C`` of float64 scalars (changed in place);
    returns V, whose columns are the vectors.  Every line is one rounded operation or a sequence of them in the order written."""
    one, zero, two = F64(1.0), F64(0.0), F64(2.0)
    V = [[one if i == j else zero for j in range(3)] for i in range(3)]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(SWEEPS):
            for p, q, r in PAIRS:
                apq = C[p][q]
                if apq == zero:
                    continue
                app, aqq = C[p][p], C[q][q]
                theta = (aqq - app) / (two * apq)
                t = one / (np.abs(theta) + np.sqrt(theta * theta + one))
                if theta < zero:
                    t = -t
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                C[p][p] = app - h
                C[q][q] = aqq + h
                C[p][q] = C[q][p] = zero
                arp, arq = C[r][p], C[r][q]
                C[r][p] = C[p][r] = c * arp - s * arq
                C[r][q] = C[q][r] = s * arp + c * arq
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return V


def stage_b(N, S, M, origin, quantum, viewpoint=None):
    """``(normal fp32 [3], variation fp32, valid)`` of one neighbourhood from its integer sums."""
    v, variation, valid = stage_b_double(N, S, M, origin, quantum, viewpoint)
    return np.array([F32(x) for x in v], F32), F32(variation), valid


def stage_b_double(N, S, M, origin, quantum, viewpoint=None):
    """``stage_b`` before its last step, the rounding to fp32: ``(v: three float64, variation float64, valid)``."""
    nothing = ([F64(0.0)] * 3, F64(0.0), False)
    if N < 3:
        return nothing
    R, s, m = recentre(N, S, M)
    n64 = F64(N)
    sd = [F64(v) for v in s]
    md = [F64(v) for v in m]
    C = [[None] * 3 for _ in range(3)]
    for k, (a, b) in enumerate(MOMENT_PAIRS):
        C[a][b] = C[b][a] = md[k] - (sd[a] * sd[b]) / n64
    V = jacobi(C)
    d = [C[0][0], C[1][1], C[2][2]]
    imin = 0
    if d[1] < d[imin]:
        imin = 1
    if d[2] < d[imin]:
        imin = 2
    imax = 0
    if d[1] > d[imax]:
        imax = 1
    if d[2] > d[imax]:
        imax = 2
    dmid = d[3 - imin - imax] if imin != imax else d[imin]
    with np.errstate(over="ignore", invalid="ignore"):
        if not (dmid * F64(1048576.0) > d[imax] and d[imax] < F64(np.inf)):
            return nothing
    v = [V[0][imin], V[1][imin], V[2][imin]]
    if viewpoint is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            mean = [F64(origin[a]) + F64(quantum) * (F64(R[a]) + sd[a] / n64) for a in range(3)]
            g = (v[0] * (F64(viewpoint[0]) - mean[0]) + v[1] * (F64(viewpoint[1]) - mean[1])) + v[2] * (F64(viewpoint[2]) - mean[2])
        flip = bool(g < 0)
    else:
        big = 0
        if np.abs(v[1]) > np.abs(v[big]):
            big = 1
        if np.abs(v[2]) > np.abs(v[big]):
            big = 2
        flip = bool(v[big] < 0)
    if flip:
        v = [-x for x in v]
    total = (d[0] + d[1]) + d[2]
    variation = (d[imin] if d[imin] > 0 else F64(0.0)) / total if total > 0 else F64(0.0)
    return v, variation, True


def estimate(coords4, xyz, inverse_map, origin, quantum, bits, viewpoint=None):
    """Everything ``a3d_estimate_normals`` writes, as a dict: ``moments_qv`` int64 [n, 10], ``count_qv`` int32 [n],
    ``normal_qv`` fp32 [n, 3], ``variation_qv`` fp32 [n], ``normal_full`` fp32 [n_full, 3], ``summary`` (a dict).  Python
    integers throughout (``stage_a``, ``neighbourhoods``): for scenes of a few thousand voxels."""
    n = len(coords4)
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    words, counted, err = stage_a(n, xyz, inverse_map, origin, quantum, bits)
    totals = [[sum(words[j][k] for j in hood) for k in range(10)] for hood in neighbourhoods(coords4)]
    return _finish(n, xyz, inverse_map, np.array(words, np.int64).reshape(n, 10), totals, counted, err, origin, quantum, viewpoint)


def _finish(n, xyz, inverse_map, words, totals, counted, err, origin, quantum, viewpoint):
    normal, variation, count = np.zeros((n, 3), F32), np.zeros(n, F32), np.zeros(n, np.int32)
    n_valid = 0
    for i, tot in enumerate(totals):
        count[i] = tot[0]
        if tot[0] >= 3:
            normal[i], variation[i], valid = stage_b(tot[0], tot[1:4], tot[4:], origin, quantum, viewpoint)
            n_valid += valid
    rows = np.arange(len(xyz)) if inverse_map is None else np.asarray(inverse_map, np.int64)
    inside = (rows >= 0) & (rows < n)
    full = np.zeros((len(xyz), 3), F32)
    full[inside] = normal[rows[inside]]
    return dict(moments_qv=words, count_qv=count, normal_qv=normal, variation_qv=variation, normal_full=full,
                summary=dict(counted=counted, valid=n_valid, invalid=n - n_valid, err=err))


def estimate_large(coords4, xyz, inverse_map, origin, quantum, bits, viewpoint=None):
    """``estimate`` for scenes of hundreds of thousands of voxels: stage A and the neighbourhood sums in numpy int64 -- exact
    under the call's own bound n_full 2^(2 bits) <= 2^62, asserted here -- and stage B, unchanged, where N >= 3.  The host
    test holds it to ``estimate``."""
    n = len(coords4)
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    assert len(xyz) << (2 * bits) <= 1 << 62
    X, ok = fixed_point(xyz, origin, quantum, bits)
    rows = np.arange(len(X)) if inverse_map is None else np.asarray(inverse_map, np.int64)
    inside = (rows >= 0) & (rows < n)
    err = (0 if inside.all() else BAD_INDEX) | (0 if ok.all() else RANGE)
    take = inside & ok
    Xc, at = X[take], rows[take]
    words = np.zeros((n, 10), np.int64)
    np.add.at(words[:, 0], at, 1)
    for a in range(3):
        np.add.at(words[:, 1 + a], at, Xc[:, a])
    for k, (a, b) in enumerate(MOMENT_PAIRS):
        np.add.at(words[:, 4 + k], at, Xc[:, a] * Xc[:, b])
    # the rows of the 27 cells, by a sorted key of (batch, x, y, z) shifted to be non-negative
    c = np.asarray(coords4, np.int64).reshape(-1, 4)
    lo = c[:, 1:].min(0) - 1
    span = c[:, 1:].max(0) - lo + 2
    key = lambda b, p: ((b * span[0] + (p[:, 0] - lo[0])) * span[1] + (p[:, 1] - lo[1])) * span[2] + (p[:, 2] - lo[2])
    own = key(c[:, 0], c[:, 1:])
    order = np.argsort(own)
    sorted_keys = own[order]
    padded = np.concatenate([words, np.zeros((1, 10), np.int64)])
    totals = np.zeros((n, 10), np.int64)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                want = key(c[:, 0], c[:, 1:] + (dx, dy, dz))
                pos = np.minimum(np.searchsorted(sorted_keys, want), n - 1)
                row = np.where(sorted_keys[pos] == want, order[pos], n)
                totals += padded[row]
    return _finish(n, xyz, inverse_map, words, totals.tolist(), int(take.sum()), err, origin, quantum, viewpoint)


def cull(xyz, normals, eye, mode):
    """``(xyz_out fp32 [n, 3], hidden uint8 [n], count)`` of ``a3d_cull_points``: g = (Nx (x - ex) + Ny (y - ey)) + Nz (z - ez)
    in fp32, one operation at a time; BACK hides g > 0, FRONT hides g < 0; a hidden vertex's coordinates become the NaN 0x7fc00000."""
    p, nn, e = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(normals, F32).reshape(-1, 3), np.asarray(eye, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        w = p - e
        g = (nn[:, 0] * w[:, 0] + nn[:, 1] * w[:, 1]) + nn[:, 2] * w[:, 2]
        hidden = g > 0 if mode == CULL_BACK else g < 0
    out = p.copy()
    out.view(np.uint32)[hidden] = 0x7fc00000
    return out, hidden.astype(np.uint8), int(hidden.sum())


def angle(a, b):
    """The angle between the LINES along a and b, in float64 (atan2 of |a x b| and |a . b|: accurate near 0)."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return math.atan2(float(np.linalg.norm(np.cross(a, b))), abs(float(a @ b)))
