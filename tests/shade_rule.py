"""The lighting rules restated in numpy float32, one operation at a time, for ``test_shade_host.py`` (CPU) and
``test_gpu_shade.py``: vertex normals (``a3d_vertex_normals``), the lit colour image of a mesh (``a3d_render_shade_lit``)
and the depth-shaded one of a cloud (``a3d_render_shade_depth``).  The rules are stated in include/agile3d_hip.h; every
product, sum, difference, quotient and square root below is one fp32 operation, in the header's order, so the kernels
must give these bits.  The base colours and the quantisation are ``render_rule``'s.
"""
import numpy as np

from pick_rule import F32
from render_rule import base_colors, pixel_rays, quantise


def vertex_normals_rule(xyz32, faces, offsets, corners):
    """fp32 [n, 3]: per vertex the sequential sum of its list's face normals, normalised (0 where there is none)."""
    xyz32 = np.asarray(xyz32, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n, m = len(xyz32), len(f)
    ok = ((f >= 0) & (f < n)).all(1)
    fs = np.where(ok[:, None], f, 0)
    with np.errstate(all="ignore"):
        pa, pb, pc = xyz32[fs[:, 0]], xyz32[fs[:, 1]], xyz32[fs[:, 2]]
        e1, e2 = pb - pa, pc - pa
        g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        assert g.dtype == F32
        ok &= np.isfinite(g).all(1)
        out = np.zeros((n, 3), F32)
        for v in range(n):
            s = np.zeros(3, F32)
            for c in corners[max(int(offsets[v]), 0):min(int(offsets[v + 1]), 3 * m)]:
                if 0 <= c < 3 * m and ok[c // 3]:
                    s = s + g[c // 3]
            l2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
            if l2 > 0 and np.isfinite(l2):
                out[v] = s / np.sqrt(l2)
    assert out.dtype == F32
    return out


def lit_factor(ids, u, v, faces, normals32, cam, ambient):
    """fp32 [h, w] each: k of every pixel (1 where the pixel shows nothing), k0, and the signed Nn . d (0 where nothing)."""
    normals32 = np.asarray(normals32, F32)
    hit = ids >= 0
    f = np.asarray(faces, np.int64).reshape(-1, 3)[ids[hit]]
    d = pixel_rays(cam)[hit]
    uu, vv = u[hit][:, None], v[hit][:, None]
    with np.errstate(all="ignore"):
        ww = (F32(1.0) - uu) - vv
        nn = (ww * normals32[f[:, 0]] + uu * normals32[f[:, 1]]) + vv * normals32[f[:, 2]]
        l2 = (nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]
        dot = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
        k0 = np.where((l2 > 0) & np.isfinite(l2), np.fmin(np.abs(dot) / np.sqrt(l2), F32(1)), F32(1)).astype(F32)
        a = F32(ambient)
        k = a + (F32(1) - a) * k0
    assert nn.dtype == F32 and k.dtype == F32
    full, full0, full_dot = np.ones(ids.shape, F32), np.ones(ids.shape, F32), np.zeros(ids.shape, F32)
    full[hit], full0[hit], full_dot[hit] = k, k0, dot
    return full, full0, full_dot


def lit_rule(ids, u, v, faces, colors32, normals32, cam, ambient, background):
    """uint8 [h, w, 3]: a3d_render_shade_lit."""
    c, hit = base_colors(ids, u, v, faces, colors32, background)
    k = lit_factor(ids, u, v, faces, normals32, cam, ambient)[0]
    c[hit] = c[hit] * k[hit][:, None]
    return quantise(c)


def depth_factor(ids, t, strength):
    """fp32 [h, w]: k = 1 / (1 + strength s), s the four neighbours' relative depth steps in left, right, up, down order."""
    h, w = ids.shape
    shows = ids >= 0
    s = np.zeros((h, w), F32)
    with np.errstate(all="ignore"):
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            tq = np.full((h, w), np.inf, F32)
            there = np.zeros((h, w), bool)
            src = (slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0)))
            dst = (slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0)))
            tq[dst], there[dst] = t[src], shows[src]
            r = np.where(there & shows, np.fmax(t - tq, F32(0)) / t, F32(0)).astype(F32)
            s = s + r
        k = F32(1) / (F32(1) + F32(strength) * s)
    assert k.dtype == F32
    return np.where(shows, k, F32(1)).astype(F32)


def depth_rule(ids, t, u, v, faces, colors32, strength, background):
    """uint8 [h, w, 3]: a3d_render_shade_depth."""
    c, hit = base_colors(ids, u, v, faces, colors32, background)
    k = depth_factor(ids, t, strength)
    c[hit] = c[hit] * k[hit][:, None]
    return quantise(c)
