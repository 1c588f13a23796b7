"""The rules of ``a3d_measure_objects`` and ``a3d_object_extents`` (include/agile3d_hip.h) restated on the host, independently
of the package (not collected; numpy only, no import of ``agile3d_amd``): int64 arithmetic for the moments, float64 one
operation at a time for the faces, float32 one operation at a time for the projections.  Everything the kernels accumulate
is an integer or a minimum / maximum, so they are held to these exactly."""
import numpy as np

MOMENTS = np.dtype([("vertices", "<i8"), ("voxels", "<i8"), ("sum", "<i8", (3,)), ("mom", "<i8", (6,)), ("area_thirds", "<i8"),
                    ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("reserved_", "<i4", (2,))])
RANGE, BAD_LABEL = 1, 2
MAX_BITS, MAX_Q, MAX_FACES = 20, 1 << 38, 1 << 23
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # XX, XY, XZ, YY, YZ, ZZ


def order_key(values):
    """uint32 keys that order like the TOTAL order of the fp32 bit patterns (-0 below +0)."""
    b = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(b >> 31 == 1, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_value(keys):
    k = np.asarray(keys, np.uint32)
    return np.where(k >> 31 == 1, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).reshape(k.shape).view(np.float32)


def total_min_max(values):
    """(min, max) of fp32 ``values`` [k, ...] along axis 0 by the total order of bit patterns; (+inf, -inf) when k = 0."""
    v = np.ascontiguousarray(values, np.float32)
    if len(v) == 0:
        shape = v.shape[1:]
        return np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    k = order_key(v)
    return key_value(k.min(0)), key_value(k.max(0))


def fixed_point(xyz, origin, quantum, bits):
    """``(X int64 [n, 3], ok bool [n])``: X = rint((double(x) - origin) / quantum), ok where |X| <= 2^bits on every axis (a NaN
    or an infinity is not ok; X is 0 there)."""
    with np.errstate(all="ignore"):
        r = np.rint((np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64) - np.asarray(origin, np.float64)) / float(quantum))
        ok = (np.abs(r) <= float(2 ** bits)).all(1)
    return np.where(ok[:, None], r, 0.0).astype(np.int64), ok


def face_quanta(xyz, faces, area_quantum):
    """``(Q int64 [m], ok bool [m])`` of faces whose indices are all valid: Q = rint(|e1 x e2| / area_quantum) in float64, every
    operation on its own; ok where the quotient is at most MAX_Q (a NaN is not)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
        e1, e2 = b - a, c - a
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        q = np.rint(np.sqrt((nx * nx + ny * ny) + nz * nz) / float(area_quantum))
        ok = q <= float(MAX_Q)
    return np.where(ok, q, 0.0).astype(np.int64), ok


def measure_numpy(xyz, labels, origin, quantum, bits, n_classes, labels_qv=None, faces=None, area_quantum=None):
    """``(records MOMENTS [n_classes], err)`` by the header's rule."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64).reshape(-1)
    n = len(labels)
    rec = np.zeros(n_classes, MOMENTS)
    err = 0
    X, in_range = fixed_point(xyz, origin, quantum, bits)
    in_label = (labels >= 0) & (labels < n_classes)
    if (~in_range).any():
        err |= RANGE
    if (~in_label).any():
        err |= BAD_LABEL
    counts = in_range & in_label
    for k in range(n_classes):
        rows = counts & (labels == k)
        rec["vertices"][k] = rows.sum()
        rec["sum"][k] = X[rows].sum(0)
        rec["mom"][k] = [(X[rows, a] * X[rows, b]).sum() for a, b in PAIRS]
        rec["lo"][k], rec["hi"][k] = total_min_max(xyz[rows])[0], total_min_max(xyz[rows])[1]
    if labels_qv is not None:
        qv = np.asarray(labels_qv, np.int64).reshape(-1)
        good = (qv >= 0) & (qv < n_classes)
        if (~good).any():
            err |= BAD_LABEL
        rec["voxels"] = np.bincount(qv[good], minlength=n_classes)
    if faces is not None and len(faces):
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        f = f[((f >= 0) & (f < n)).all(1)]                      # a corner index outside: skipped silently
        good = in_label[f].all(1)
        if (~good).any():
            err |= BAD_LABEL
        f = f[good]
        Q, ok = face_quanta(xyz, f, area_quantum)
        if (~ok).any():
            err |= RANGE
        for corner in range(3):
            np.add.at(rec["area_thirds"], labels[f[ok, corner]], Q[ok])
    return rec, err


def extents_numpy(xyz, labels, axes):
    """``(out fp32 [n_classes, 3, 2], err)``: per object and axis the (min, max) of p = (a_x*x + a_y*y) + a_z*z in float32, every
    operation on its own."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64).reshape(-1)
    axes = np.asarray(axes, np.float32).reshape(-1, 3, 3)
    n_classes = len(axes)
    out = np.empty((n_classes, 3, 2), np.float32)
    out[..., 0], out[..., 1] = np.inf, -np.inf
    err = 0
    in_label = (labels >= 0) & (labels < n_classes)
    finite = np.isfinite(xyz).all(1)
    if (~in_label).any():
        err |= BAD_LABEL
    if (~finite).any():
        err |= RANGE
    for k in range(n_classes):
        p = xyz[in_label & finite & (labels == k)]
        for j in range(3):
            a = axes[k, j]
            with np.errstate(all="ignore"):
                proj = (a[0] * p[:, 0] + a[1] * p[:, 1]) + a[2] * p[:, 2]
            assert proj.dtype == np.float32
            if np.isnan(proj).any():
                err |= RANGE
            out[k, j] = total_min_max(proj[~np.isnan(proj)])
    return out, err
