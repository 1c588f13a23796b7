"""The rendered view's rule and bound, restated in numpy for ``test_render_host.py`` (CPU) and ``test_gpu_render.py``.

THE RULE (include/agile3d_hip.h): the image is, pixel by pixel, what the picks return for the ray through the pixel's
centre.  ``pixel_rays`` restates the camera's fp32 ray formula one operation at a time; ``face_pass_f32`` and
``point_pass_f32`` restate the two exact tests for ONE ray against all primitives (the arithmetic of
``pick_rule.mesh_rule_f32`` and of ``k_pick_ray``), ``render_mesh_rule`` / ``render_points_rule`` fold them into
images by brute force, ``shade_rule`` restates the colour image.

THE BOUND (csrc/session.hip: render_rect_face, render_rect_point, render_rect_tiles): ``camera_bounds``, ``rect_face``,
``rect_point`` restate in float64 which pixels a primitive can reach: ("none" | "every" | "rect", (px0, py0, px1, py1)), the
rectangle in whole pixels before it is widened to tiles of 16.
"""
import numpy as np

from pick_rule import F32, U, mesh_rule_f32, shear_of

TILE = 16
MAX_RECT_TILES = 256


def camera_fields(cam):
    """(o, d00, du, dv) as fp32 arrays, width, height of a ``lib.Camera``."""
    return (np.array(cam.o[:], F32), np.array(cam.d00[:], F32), np.array(cam.du[:], F32), np.array(cam.dv[:], F32),
            int(cam.width), int(cam.height))


def pixel_rays(cam):
    """fp32 [h, w, 3] unit directions: x = (d00 + u du) + v dv per component, len = sqrt((xx + yy) + zz), d = x / len."""
    o, d00, du, dv, w, h = camera_fields(cam)
    u = np.arange(w, dtype=F32)[None, :]
    v = np.arange(h, dtype=F32)[:, None]
    with np.errstate(all="ignore"):
        x, y, z = ((d00[k] + u * du[k]) + v * dv[k] for k in range(3))
        assert x.dtype == F32 and x.shape == (h, w)
        ln = np.sqrt((x * x + y * y) + z * z)
        d = np.stack([x / ln, y / ln, z / ln], -1)
    assert d.dtype == F32
    return d


# ------------------------------------------------------------------------------------------- the exact tests, one ray
def face_pass_f32(xyz32, faces, o32, d32):
    """(hit mask [m], t fp32 [m], vv, ww, det) of ONE ray against every face: mesh_rule_f32's arithmetic, kept per face."""
    xyz32, o32 = np.asarray(xyz32, F32), np.asarray(o32, F32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(xyz32)
    in_range = ((f >= 0) & (f < n)).all(1)
    ok = in_range & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = np.where(in_range[:, None], f, 0)
    kx, ky, kz, sx, sy, sz = shear_of(d32)
    with np.errstate(all="ignore"):
        a, b, c = xyz32[f[:, 0]] - o32, xyz32[f[:, 1]] - o32, xyz32[f[:, 2]] - o32
        ax, ay = a[:, kx] - sx * a[:, kz], a[:, ky] - sy * a[:, kz]
        bx, by = b[:, kx] - sx * b[:, kz], b[:, ky] - sy * b[:, kz]
        cx, cy = c[:, kx] - sx * c[:, kz], c[:, ky] - sy * c[:, kz]
        uu, vv, ww = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        z = (uu == 0) | (vv == 0) | (ww == 0)
        if z.any():
            D = np.float64
            uu = np.where(z, (cx.astype(D) * by.astype(D) - cy.astype(D) * bx.astype(D)).astype(F32), uu)
            vv = np.where(z, (ax.astype(D) * cy.astype(D) - ay.astype(D) * cx.astype(D)).astype(F32), vv)
            ww = np.where(z, (bx.astype(D) * ay.astype(D) - by.astype(D) * ax.astype(D)).astype(F32), ww)
        mixed = ((uu < 0) | (vv < 0) | (ww < 0)) & ((uu > 0) | (vv > 0) | (ww > 0))
        det = (uu + vv) + ww
        tt = ((uu * (sz * a[:, kz]) + vv * (sz * b[:, kz])) + ww * (sz * c[:, kz])) / det
        hit = ok & ~mixed & (det != 0) & (tt > 0) & (tt < np.inf)
    assert tt.dtype == F32
    return hit, tt, vv, ww, det


def point_pass_f32(xyz32, o32, d32, r):
    """(pass mask [n], t fp32 [n], perpendicular distance^2 fp32 [n]) of ONE ray against every point: k_pick_ray's test."""
    xyz32, o32, d32 = np.asarray(xyz32, F32), np.asarray(o32, F32), np.asarray(d32, F32)
    r2 = F32(r) * F32(r)
    with np.errstate(all="ignore"):
        v = xyz32 - o32
        tt = (v[:, 0] * d32[0] + v[:, 1] * d32[1]) + v[:, 2] * d32[2]
        px, py, pz = v[:, 0] - tt * d32[0], v[:, 1] - tt * d32[1], v[:, 2] - tt * d32[2]
        p2 = (px * px + py * py) + pz * pz
        ok = (tt > 0) & (p2 <= r2)
    assert tt.dtype == F32 and p2.dtype == F32
    return ok, tt, p2


# ------------------------------------------------------------------------------------------- the images by brute force
def render_mesh_rule(xyz32, faces, cam):
    """(face int32 [h, w], t fp32 [h, w] (+inf = nothing), u, v fp32 [h, w], flags) -- mesh_rule_f32 per pixel."""
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    h, w = d.shape[:2]
    face = np.full((h, w), -1, np.int32)
    t = np.full((h, w), np.inf, F32)
    u, v = np.zeros((h, w), F32), np.zeros((h, w), F32)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    flags = 0
    for j in range(h):
        for i in range(w):
            got, tt, fl, hit = mesh_rule_f32(xyz32, faces, o, d[j, i])
            flags |= fl
            if got >= 0:
                face[j, i], t[j, i], u[j, i], v[j, i] = got, tt, hit[0], hit[1]
    return face, t, u, v, flags


def render_points_rule(xyz32, r, cam):
    """(index int32 [h, w], t fp32 [h, w]): per pixel the smallest (t bits, distance^2 bits, row) among the passing points."""
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    h, w = d.shape[:2]
    index = np.full((h, w), -1, np.int32)
    t = np.full((h, w), np.inf, F32)
    if len(xyz32) == 0:
        return index, t
    rows = np.arange(len(xyz32))
    for j in range(h):
        for i in range(w):
            ok, tt, p2 = point_pass_f32(xyz32, o, d[j, i], r)
            if ok.any():
                c = np.flatnonzero(ok)
                best = c[np.lexsort((rows[c], p2[c].view(np.uint32), tt[c].view(np.uint32)))[0]]
                index[j, i], t[j, i] = best, tt[best]
    return index, t


def quantise(c):
    q = np.minimum(np.maximum(c, F32(0)), F32(1)) * F32(255) + F32(0.5)
    assert q.dtype == F32
    return q.astype(np.uint8)


def base_colors(ids, u, v, faces, colors32, background):
    """(fp32 [h, w, 3] unquantised colours, the mask of pixels that are not background) as a3d_render_shade computes them:
    the vertex's colour (faces None) or ((1 - u - v) c0 + u c1) + v c2 in fp32, background where id < 0."""
    colors32 = np.asarray(colors32, F32)
    h, w = ids.shape
    c = np.empty((h, w, 3), F32)
    c[:] = np.asarray(background, F32)
    hit = ids >= 0
    if faces is None:
        c[hit] = colors32[ids[hit]]
    else:
        f = np.asarray(faces, np.int64).reshape(-1, 3)[ids[hit]]
        uu, vv = u[hit][:, None], v[hit][:, None]
        ww = (F32(1.0) - uu) - vv
        c[hit] = (ww * colors32[f[:, 0]] + uu * colors32[f[:, 1]]) + vv * colors32[f[:, 2]]
    assert c.dtype == F32
    return c, hit


def shade_rule(ids, u, v, faces, colors32, background):
    """uint8 [h, w, 3]: the base colours quantised as (uint8)(min(max(c, 0), 1) * 255 + 0.5)."""
    return quantise(base_colors(ids, u, v, faces, colors32, background)[0])


# ------------------------------------------------------------------------------------------- the bound
def camera_bounds(cam):
    """float64: (inv [3, 3] = rows of [du dv d00]^-1, their norms [3], dmax) -- what a3d_render_camera_bounds returns."""
    o, d00, du, dv, w, h = camera_fields(cam)
    m = np.stack([du, dv, d00], 1).astype(np.float64)
    inv = np.linalg.inv(m)
    corners = [d00.astype(np.float64) + u * du.astype(np.float64) + v * dv.astype(np.float64)
               for u in (0, w - 1) for v in (0, h - 1)]
    dmax = max(np.linalg.norm(c) for c in corners) * (1 + 1e-6)
    return inv, np.linalg.norm(inv, axis=1), dmax


def _rect_pixels(x0, x1, y0, y1, w, h):
    if not (x0 <= x1 and y0 <= y1):
        return "every", None
    if x1 < 0 or y1 < 0 or x0 > w - 1 or y0 > h - 1:
        return "none", None
    px0, px1 = int(np.floor(max(x0, 0.0))), int(np.ceil(min(x1, w - 1.0)))
    py0, py1 = int(np.floor(max(y0, 0.0))), int(np.ceil(min(y1, h - 1.0)))
    if (px1 // TILE - px0 // TILE + 1) * (py1 // TILE - py0 // TILE + 1) > MAX_RECT_TILES:
        return "every", None
    return "rect", (px0, py0, px1, py1)


def rect_face(cam, bounds, A, B, C):
    """The pixels a face with fp32 vertices A, B, C can reach (indices assumed valid and distinct)."""
    o, _, _, _, w, h = camera_fields(cam)
    inv, (na, nb, nc), dmax = bounds
    with np.errstate(all="ignore"):
        p = np.stack([A, B, C]).astype(np.float64) - o.astype(np.float64)
        if np.isnan(p).any():
            return "none", None
        lo, hi = p.min(0), p.max(0)
        R = max(np.abs(lo).max(), np.abs(hi).max())
        g = np.sqrt((np.maximum(0.0, np.maximum(lo, -hi)) ** 2).sum())
        if not R < 1e30 or not g > R / 1024.0:
            return "every", None
        c_lo, eta = 0.98 * g / dmax, 32.0 * U * R
        a, b, c = (p @ inv.T).T
        xs, ys = [], []
        for k in range(3):
            j = (k + 1) % 3
            if c[k] >= c_lo:
                xs.append(a[k] / c[k]); ys.append(b[k] / c[k])
            if (c[k] >= c_lo) != (c[j] >= c_lo):
                s = (c_lo - c[k]) / (c[j] - c[k])
                xs.append((a[k] + s * (a[j] - a[k])) / c_lo); ys.append((b[k] + s * (b[j] - b[k])) / c_lo)
        if not xs:
            return "none", None
        mx = 1 / 128 + (na + 8192 * nc) * eta / c_lo
        my = 1 / 128 + (nb + 8192 * nc) * eta / c_lo
        return _rect_pixels(min(xs) - mx, max(xs) + mx, min(ys) - my, max(ys) + my, w, h)


def rect_point(cam, bounds, P, r):
    """The pixels a point P with radius r can reach."""
    o, _, _, _, w, h = camera_fields(cam)
    inv, (na, nb, nc), dmax = bounds
    with np.errstate(all="ignore"):
        p = np.asarray(P, F32).astype(np.float64) - o.astype(np.float64)
        n2 = (p * p).sum()
        if not n2 < 1e60:
            return "none", None
        ln = np.sqrt(n2)
        reff = r * (1 + 1 / 1024) + 128 * U * (ln + r)
        if not ln > reff * (1 + 1 / 1024):
            return "every", None
        t0 = np.sqrt(n2 - reff * reff)
        a, b, c = inv @ p
        ha, hb, hc = reff * na, reff * nb, reff * nc
        c_lo, c_hi = max(c - hc, 0.98 * t0 / dmax), c + hc
        if not c_hi >= c_lo:
            return "none", None
        x0, x1 = min((a - ha) / c_lo, (a - ha) / c_hi), max((a + ha) / c_lo, (a + ha) / c_hi)
        y0, y1 = min((b - hb) / c_lo, (b - hb) / c_hi), max((b + hb) / c_lo, (b + hb) / c_hi)
        return _rect_pixels(x0 - 1 / 128, x1 + 1 / 128, y0 - 1 / 128, y1 + 1 / 128, w, h)


def covers(verdict, i, j):
    """Whether pixel (column i, row j) lies inside a bound: its tile is one of the rectangle's tiles."""
    kind, rect = verdict
    if kind == "every":
        return True
    if kind == "none":
        return False
    return rect[0] // TILE <= i // TILE <= rect[2] // TILE and rect[1] // TILE <= j // TILE <= rect[3] // TILE
