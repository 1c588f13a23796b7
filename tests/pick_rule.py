"""The session's search and pick rules restated in numpy, for the host tests (CPU) and the GPU tests of the session family;
``render_rule.py`` and ``shade_rule.py`` build on them.  Rule modules import numpy and each other, nothing else.

``fp32_rule_argmin``  a3d_nearest_rows: the fp32 distance from the differences, first arg-min.
``pick_rule_f64``     a3d_pick_ray in float64, with the margins a test needs to know whether float64 can speak for fp32.
``mesh_rule_f64``     a3d_pick_mesh in float64, Moeller-Trumbore form (NOT the kernel's arithmetic: an independent statement).
``mesh_rule_f32``     the kernel's arithmetic in numpy float32, one operation at a time, the double fallback included.
``paint_numpy``       a3d_session_paint.

The mesh pick rule (include/agile3d_hip.h, a3d_pick_mesh): among the faces a ray crosses at a finite t > 0 the one with the
smallest t, ties -> the lower face index; double-sided, edges inclusive; faces with det == 0, a repeated index, a NaN
coordinate or an index outside [0, n) are skipped.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32


def fp32_rule_argmin(rows, q):
    """The header's rule one fp32 operation at a time: (dx*dx + dy*dy) + dz*dz from the differences, first arg-min."""
    d = rows.astype(np.float32) - q.astype(np.float32)
    s = d * d
    return int(((s[:, 0] + s[:, 1]) + s[:, 2]).argmin())



def pick_rule_f64(xyz, o, d, r):
    """The pick rule in float64: (index or -1, margin in t between the first two candidates, smallest distance of any
    point in front of / near the origin plane to the cylinder surface, smallest |t| of a point inside the cylinder)."""
    v = xyz.astype(np.float64) - o.astype(np.float64)
    d = d.astype(np.float64)
    t = v @ d
    perp = np.linalg.norm(v - t[:, None] * d, axis=1)
    cand = np.flatnonzero((t > 0) & (perp <= r))
    surface = np.abs(perp[t > -1e-3] - r).min() if (t > -1e-3).any() else np.inf
    plane = np.abs(t[perp <= r + 1e-3]).min() if (perp <= r + 1e-3).any() else np.inf
    if len(cand) == 0:
        return -1, np.inf, surface, plane
    order = cand[np.lexsort((cand, perp[cand], t[cand]))]
    gap = t[order[1]] - t[order[0]] if len(order) > 1 else np.inf
    return int(order[0]), gap, surface, plane



# ------------------------------------------------------------------------------------------- the rule, twice
def _valid_faces(faces, n):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < n)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return np.where(in_range[:, None], f, 0), in_range, in_range & distinct


def mesh_rule_f64(xyz, faces, o, d):
    """Per face, in float64: t (inf = no crossing), the weights u, v of the face's second and third vertex, and whether
    an index was out of range.  The fp32 inputs are exact in float64; its own rounding (1e-16) is nothing here."""
    f, in_range, ok = _valid_faces(faces, len(xyz))
    x = np.asarray(xyz, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        p = np.cross(d, e2)
        det = (e1 * p).sum(1)
        tv = o - a
        q = np.cross(tv, e1)
        u = (tv * p).sum(1) / det
        v = (q * d).sum(1) / det
        t = (e2 * q).sum(1) / det
        hit = ok & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & np.isfinite(t)
    return np.where(hit, t, np.inf), u, v, bool((~in_range).any())


def first_of(t):
    """(face or -1, t, gap to the next larger t) of a per-face t array under the order (t, face index)."""
    if len(t) == 0 or not np.isfinite(t).any():
        return -1, np.inf, np.inf
    best = int(np.argmin(t))                       # the first of equals: the lower index
    rest = np.delete(t, best)
    return best, float(t[best]), (float(rest.min()) - float(t[best]) if len(rest) else np.inf)


def shear_of(d32):
    """What a3d_pick_mesh derives from the unit direction on the host, in fp32: (kx, ky, kz, sx, sy, sz)."""
    d32 = np.asarray(d32, F32)
    kz = 0
    if abs(d32[1]) > abs(d32[kz]):
        kz = 1
    if abs(d32[2]) > abs(d32[kz]):
        kz = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d32[kz] < 0:
        kx, ky = ky, kx
    return kx, ky, kz, F32(d32[kx] / d32[kz]), F32(d32[ky] / d32[kz]), F32(F32(1.0) / d32[kz])


def mesh_rule_f32(xyz32, faces, o32, d32):
    """The kernel's arithmetic, every fp32 operation rounded on its own, in the kernel's order.  Returns
    (face or -1, t as fp32, flags, (u, v, point) of the hit in fp32 or None)."""
    xyz32, o32 = np.asarray(xyz32, F32), np.asarray(o32, F32)
    f, in_range, ok = _valid_faces(faces, len(xyz32))
    flags = int((~in_range).any())
    if len(f) == 0:
        return -1, F32(0), flags, None
    kx, ky, kz, sx, sy, sz = shear_of(d32)
    with np.errstate(all="ignore"):
        a, b, c = xyz32[f[:, 0]] - o32, xyz32[f[:, 1]] - o32, xyz32[f[:, 2]] - o32      # translate (fp32 arrays: fp32 results)
        ax, ay = a[:, kx] - sx * a[:, kz], a[:, ky] - sy * a[:, kz]                      # permute and shear
        bx, by = b[:, kx] - sx * b[:, kz], b[:, ky] - sy * b[:, kz]
        cx, cy = c[:, kx] - sx * c[:, kz], c[:, ky] - sy * c[:, kz]
        uu = cx * by - cy * bx
        vv = ax * cy - ay * cx
        ww = bx * ay - by * ax
        assert uu.dtype == F32 and ax.dtype == F32
        z = (uu == 0) | (vv == 0) | (ww == 0)                                            # the double fallback
        if z.any():
            D = np.float64
            uu = np.where(z, (cx.astype(D) * by.astype(D) - cy.astype(D) * bx.astype(D)).astype(F32), uu)
            vv = np.where(z, (ax.astype(D) * cy.astype(D) - ay.astype(D) * cx.astype(D)).astype(F32), vv)
            ww = np.where(z, (bx.astype(D) * ay.astype(D) - by.astype(D) * ax.astype(D)).astype(F32), ww)
        mixed = ((uu < 0) | (vv < 0) | (ww < 0)) & ((uu > 0) | (vv > 0) | (ww > 0))
        det = (uu + vv) + ww
        az, bz, cz = sz * a[:, kz], sz * b[:, kz], sz * c[:, kz]
        tt = ((uu * az + vv * bz) + ww * cz) / det
        assert tt.dtype == F32
        hit = ok & ~mixed & (det != 0) & (tt > 0) & (tt < np.inf)
    if not hit.any():
        return -1, F32(0), flags, None
    key = np.where(hit, (tt.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(f), dtype=np.uint64),
                   np.uint64(0xffffffffffffffff))
    best = int(np.argmin(key))
    with np.errstate(all="ignore"):
        u, v = F32(vv[best] / det[best]), F32(ww[best] / det[best])
        w = F32(F32(F32(1.0) - u) - v)
        pa, pb, pc = xyz32[f[best, 0]], xyz32[f[best, 1]], xyz32[f[best, 2]]
        point = (w * pa + u * pb) + v * pc
    assert point.dtype == F32
    return best, tt[best], flags, (u, v, point)


def paint_numpy(labels_qv, inverse_map, xyz32, colors32, palette, cubes, cube_size):
    lab = labels_qv[inverse_map]
    n = len(palette)
    entry = np.where(lab < n, lab, 1 + (lab - 1) % (n - 1))
    col = np.where((lab > 0)[:, None], palette[entry], colors32).astype(np.float32)
    for c in cubes:
        inside = (np.abs(xyz32 - c[:3].astype(np.float32)) < np.float32(cube_size)).all(1)
        col[inside] = c[3:]
    return lab, col

