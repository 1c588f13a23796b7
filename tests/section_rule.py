"""The section rule (include/agile3d_hip.h, ``a3d_section``) restated in numpy float32, one operation at a time, for
``test_section_host.py`` (CPU) and ``test_gpu_section.py``; built on ``pick_rule.py`` and ``render_rule.py``, whose
arithmetic of the two exact tests it reuses.  Like them it imports numpy and the other rule modules, nothing else.

A section here is ``(planes fp32 [k, 4], cull)``: rows ``(nx, ny, nz, c)`` keeping ``n . p >= c``; ``cull`` 0 none, 1 back,
2 front.

``ray_interval``          the interval [t_lo, t_hi] and the empty flag of one ray: what ``a3d_section_ray`` returns.
``front``                 the facing of a crossing from the test's det alone: det > 0 is FRONT.
``mesh_section_rule``     ``a3d_pick_mesh_section`` for one ray; ``render_mesh_section_rule`` folds it into images.
``keeps``                 the vertex rule; ``points_section_rule`` / ``render_points_section_rule`` the cloud's pick and view.
``room`` / ``grid_cloud`` / ``exact_crossing`` / ``facing_rays``  the small scenes both test files use.
"""
import numpy as np

from pick_rule import F32
from render_rule import camera_fields, face_pass_f32, pixel_rays, point_pass_f32

CULL_NONE, CULL_BACK, CULL_FRONT = 0, 1, 2
INF = F32(np.inf)


# ------------------------------------------------------------------------------------------- the ray's interval
def ray_interval(planes, o32, d32):
    """(t_lo fp32, t_hi fp32, empty) of the ray (o, d): den = (nx dx + ny dy) + nz dz, so = (nx ox + ny oy) + nz oz;
    den > 0: q = (c - so) / den, t_lo = q if q > t_lo else t_lo; den < 0: t_hi = q if q < t_hi else t_hi; else empty
    unless so >= c.  (The comparison, not fmax / fmin: a NaN q and a zero of the other sign leave the bound as it is.)"""
    o, d = np.asarray(o32, F32), np.asarray(d32, F32)
    t_lo, t_hi, empty = F32(0.0), INF, False
    with np.errstate(all="ignore"):
        for nx, ny, nz, c in np.asarray(planes, F32).reshape(-1, 4):
            den = (nx * d[0] + ny * d[1]) + nz * d[2]
            so = (nx * o[0] + ny * o[1]) + nz * o[2]
            assert den.dtype == F32 and so.dtype == F32
            if den > 0:
                q = (c - so) / den
                t_lo = q if q > t_lo else t_lo
            elif den < 0:
                q = (c - so) / den
                t_hi = q if q < t_hi else t_hi
            elif not so >= c:
                empty = True
    assert t_lo.dtype == F32 and t_hi.dtype == F32
    return t_lo, t_hi, empty


def front(det):
    """The facing from the crossing test's det = (U + V) + W: > 0 is FRONT (the vertices appear counter-clockwise from the
    ray's origin, g . d < 0 for g = (b - a) x (c - a)), < 0 is BACK."""
    return det > 0


def counts(hit, tt, det, planes, cull, o32, d32):
    """Which of the crossings ``hit`` (per face, from ``face_pass_f32``) count under the section."""
    t_lo, t_hi, empty = ray_interval(planes, o32, d32)
    with np.errstate(all="ignore"):
        ok = hit & (not empty) & (tt >= t_lo) & (tt <= t_hi)
    if cull == CULL_BACK:
        ok &= front(det)
    elif cull == CULL_FRONT:
        ok &= ~front(det)
    return ok


# ------------------------------------------------------------------------------------------- meshes
def mesh_section_rule(xyz32, faces, o32, d32, planes, cull):
    """``a3d_pick_mesh_section`` for one ray: (face or -1, t fp32, u, v, point fp32 [3] or None) -- among the crossings
    that count the smallest (t bits, face); u, v and the point as ``mesh_rule_f32`` computes them."""
    xyz32 = np.asarray(xyz32, F32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return -1, F32(0), F32(0), F32(0), None
    hit, tt, vv, ww, det = face_pass_f32(xyz32, f, o32, d32)
    ok = counts(hit, tt, det, planes, cull, o32, d32)
    if not ok.any():
        return -1, F32(0), F32(0), F32(0), None
    key = np.where(ok, (tt.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(f), dtype=np.uint64),
                   np.uint64(0xffffffffffffffff))
    best = int(np.argmin(key))
    with np.errstate(all="ignore"):
        u, v = F32(vv[best] / det[best]), F32(ww[best] / det[best])
        w = F32(F32(F32(1.0) - u) - v)
        pa, pb, pc = xyz32[f[best, 0]], xyz32[f[best, 1]], xyz32[f[best, 2]]
        point = (w * pa + u * pb) + v * pc
    assert point.dtype == F32
    return best, tt[best], u, v, point


def render_mesh_section_rule(xyz32, faces, cam, planes, cull):
    """(face int32 [h, w], t fp32 (+inf = nothing), u, v fp32): ``mesh_section_rule`` per pixel."""
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    h, w = d.shape[:2]
    face, t = np.full((h, w), -1, np.int32), np.full((h, w), np.inf, F32)
    u, v = np.zeros((h, w), F32), np.zeros((h, w), F32)
    for j in range(h):
        for i in range(w):
            got, tt, uu, vv, _ = mesh_section_rule(xyz32, faces, o, d[j, i], planes, cull)
            if got >= 0:
                face[j, i], t[j, i], u[j, i], v[j, i] = got, tt, uu, vv
    return face, t, u, v


# ------------------------------------------------------------------------------------------- clouds
def keeps(planes, xyz32):
    """bool [n]: (nx x + ny y) + nz z >= c for every plane; a NaN fails."""
    p = np.asarray(xyz32, F32).reshape(-1, 3)
    keep = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        for nx, ny, nz, c in np.asarray(planes, F32).reshape(-1, 4):
            side = (nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2]
            assert side.dtype == F32
            keep &= side >= c
    return keep


def points_section_rule(xyz32, o32, d32, r, planes):
    """``a3d_pick_ray_section`` for one ray: (index or -1, t fp32) -- ``k_pick_ray``'s key over the vertices that show."""
    xyz32 = np.asarray(xyz32, F32).reshape(-1, 3)
    if len(xyz32) == 0:
        return -1, INF
    ok, tt, p2 = point_pass_f32(xyz32, o32, d32, r)
    ok &= keeps(planes, xyz32)
    if not ok.any():
        return -1, INF
    c = np.flatnonzero(ok)
    best = c[np.lexsort((c, p2[c].view(np.uint32), tt[c].view(np.uint32)))[0]]
    return int(best), tt[best]


def render_points_section_rule(xyz32, r, cam, planes):
    """(index int32 [h, w], t fp32 [h, w]): ``points_section_rule`` per pixel."""
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    h, w = d.shape[:2]
    index, t = np.full((h, w), -1, np.int32), np.full((h, w), np.inf, F32)
    for j in range(h):
        for i in range(w):
            index[j, i], t[j, i] = points_section_rule(xyz32, o, d[j, i], r, planes)
    return index, t


# ------------------------------------------------------------------------------------------- scenes
INNER = 12                                    # the face of ``room`` that stands inside it


def room():
    """(xyz fp32 [11, 3], faces int32 [13, 3]): the closed box [-1, 1]^3 of 12 triangles, every one wound to FACE INWARDS
    (g = (b - a) x (c - a) points to the centre), and face 12, a triangle in the plane y = 0 inside it whose g is (0, -1, 0):
    it faces a camera on the -y side.  Coordinates are powers of two or their halves: exact in fp32."""
    corner = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    index = lambda p: int(np.flatnonzero((corner == p).all(1))[0])
    faces = []
    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for side in (-1.0, 1.0):
            quad = []
            for s1, s2 in ((-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)):
                p = np.empty(3)
                p[axis], p[a1], p[a2] = side, s1, s2
                quad.append(index(p))
            for tri in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
                a, b, c = corner[list(tri)]
                g = np.cross(b - a, c - a)
                faces.append(tri if g[axis] * side < 0 else (tri[0], tri[2], tri[1]))
    xyz = np.concatenate([corner, [[-0.5, 0.0, -0.5], [0.5, 0.0, -0.5], [0.0, 0.0, 0.5]]])
    faces.append((8, 9, 10))
    return xyz.astype(F32), np.asarray(faces, np.int32)


def grid_cloud():
    """fp32 [125, 3]: the 5 x 5 x 5 lattice of the coordinates -0.5, -0.25, 0, 0.25, 0.5 (exact in fp32), x fastest."""
    g = np.array([-0.5, -0.25, 0.0, 0.25, 0.5])
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)


def exact_crossing():
    """(xyz, faces, o, d, t): one triangle in the plane z = 2 and the ray from (0.25, 0.25, -2) along +z.  Every value of
    the crossing test is a dyadic number of few bits, so the ray meets the face at t = 4 EXACTLY, and the planes z >= 2 and
    z <= 2 give (c - so) / den = 4 exactly as well: the crossing sits on both ends of an interval."""
    xyz = np.array([[0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0]], F32)
    return xyz, np.array([[0, 1, 2]], np.int32), np.array([0.25, 0.25, -2.0], F32), np.array([0.0, 0.0, 1.0], F32), F32(4.0)


def facing_rays():
    """Twelve (xyz, faces, o, d): one oblique triangle in both windings, met through its centroid by rays whose dominant
    axis is x, y, z with either sign of d[kz].  |g . d| / |g| is 0.3 or more for every one of them."""
    tri = np.array([[1.0, 0.1, -0.2], [-0.1, 1.2, 0.1], [0.2, -0.1, 1.1]], F32)
    centre = tri.astype(np.float64).mean(0)
    out = []
    for winding in ((0, 1, 2), (0, 2, 1)):
        for axis in range(3):
            for sign in (1.0, -1.0):
                d = np.full(3, 0.15)
                d[(axis + 1) % 3] = -0.1
                d[axis] = sign
                d /= np.linalg.norm(d)
                o = (centre - 3.0 * d).astype(F32)
                out.append((tri, np.array([winding], np.int32), o, d.astype(F32)))
    return out
