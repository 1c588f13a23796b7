"""The rules of correcting a labelling by hand (include/agile3d_hip.h: ``a3d_region_mask``, ``a3d_select_vertices``,
``a3d_session_overlay``) restated in numpy float32, one operation at a time, for ``test_region_host.py`` (CPU),
``test_gpu_region.py`` and ``test_gpu_session_region.py``.  Like the other rule modules it imports numpy and rule modules,
nothing else: ``render_rule.pixel_rays`` is the ray of a pixel, ``section_rule.keeps`` the vertex rule of a section.

``polygon_cover`` / ``stroke_cover``   bool [h, w]: the pixels a shape covers.
``region_mask``                       the mask after a call: REPLACE, ADD or SUBTRACT of a shape.
``select``                            which vertices a camera sees inside a mask, and the summary's counts.
``overlay``                           the manual layer after a call, the labels and colours laid out, the summary's sums.
"""
import numpy as np

from pick_rule import F32
from render_rule import camera_fields, pixel_rays
from section_rule import keeps

POLYGON, STROKE = 0, 1
REPLACE, ADD, SUBTRACT = 0, 1, 2
NONE, PAINT, ERASE = 0, 1, 2
NOT_FINITE = 1


def _pixels(w, h):
    return np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]


def polygon_cover(points, w, h):
    """Even-odd: the parity of the edges a = P[j], b = P[(j + 1) % k] with (a.y > p.y) != (b.y > p.y) and
    p.x < ((b.x - a.x) * (p.y - a.y)) / (b.y - a.y) + a.x."""
    P = np.asarray(points, F32).reshape(-1, 2)
    px, py = _pixels(w, h)
    inside = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for j in range(len(P)):
            (ax, ay), (bx, by) = P[j], P[(j + 1) % len(P)]
            straddles = (ay > py) != (by > py)
            num = (bx - ax) * (py - ay)
            xi = num / (by - ay) + ax
            assert xi.dtype == F32
            inside ^= straddles & (px < xi)
    return inside


def stroke_cover(points, radius, w, h):
    """Within the radius of a segment: e = b - a, w = p - a, L = e.x e.x + e.y e.y, h = 0 unless L > 0, else (w . e) / L clamped
    by q < 0 ? 0 : (q > 1 ? 1 : q); d = w - h e; d.x d.x + d.y d.y <= r r.  One point: the segment a = b = P[0]."""
    P = np.asarray(points, F32).reshape(-1, 2)
    px, py = _pixels(w, h)
    r2 = F32(radius) * F32(radius)
    covered = np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for j in range(max(len(P) - 1, 1)):
            (ax, ay), (bx, by) = P[j], P[min(j + 1, len(P) - 1)]
            ex, ey = bx - ax, by - ay
            wx, wy = px - ax, py - ay
            L = ex * ex + ey * ey
            if L > 0:
                q = (wx * ex + wy * ey) / L
                hh = np.where(q < 0, F32(0), np.where(q > 1, F32(1), q))
            else:
                hh = np.zeros((h, w), F32)
            dx, dy = wx - hh * ex, wy - hh * ey
            d2 = dx * dx + dy * dy
            assert d2.dtype == F32 and d2.shape == (h, w)
            covered |= d2 <= r2
    return covered


def region_mask(shape, points, w, h, radius=None, mode=REPLACE, mask=None):
    """uint8 [h, w]: ``mask`` (any byte that is not 0 counts as 1) after the call; the values written are 0 or 1."""
    covered = polygon_cover(points, w, h) if shape == POLYGON else stroke_cover(points, radius, w, h)
    old = np.zeros((h, w), bool) if mask is None else np.asarray(mask) != 0
    if mode == REPLACE:
        return covered.astype(np.uint8)
    return ((old | covered) if mode == ADD else (old & ~covered)).astype(np.uint8)


def select(xyz32, cam, rows32, mask, t=None, slack=0.0, planes=()):
    """dict: ``selected`` uint8 [n], ``in_view`` bool [n], the summary's ``n_selected``, ``n_in_view`` and ``flags``, and the
    pixel ``u``, ``v`` int64 [n] of each vertex (0 where it is not in the image), ``tt`` fp32 [n] or None.
    ``rows32``: fp32 [9], the rows of [du dv d00]^-1; ``t``: fp32 [h, w] or None (select through everything)."""
    p = np.asarray(xyz32, F32).reshape(-1, 3)
    o, _, _, _, w, h = camera_fields(cam)
    R = np.asarray(rows32, F32).reshape(9)
    mask = np.asarray(mask).reshape(h, w)
    with np.errstate(all="ignore"):
        wx, wy, wz = p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2]
        a = (R[0] * wx + R[1] * wy) + R[2] * wz
        b = (R[3] * wx + R[4] * wy) + R[5] * wz
        c = (R[6] * wx + R[7] * wy) + R[8] * wz
        x, y = a / c, b / c
        xr, yr = np.floor(x + F32(0.5)), np.floor(y + F32(0.5))
        assert xr.dtype == F32 and c.dtype == F32
        in_image = (xr >= 0) & (xr < F32(w)) & (yr >= 0) & (yr < F32(h))
        in_view = (c > 0) & in_image & keeps(planes, p)
        u = np.where(in_image, xr, F32(0)).astype(np.int64)
        v = np.where(in_image, yr, F32(0)).astype(np.int64)
        sel = in_view & (mask[v, u] != 0)
        tt = None
        if t is not None:
            d = pixel_rays(cam)[v, u]
            tt = (wx * d[:, 0] + wy * d[:, 1]) + wz * d[:, 2]
            assert tt.dtype == F32
            sel &= tt - np.asarray(t, F32).reshape(h, w)[v, u] <= F32(slack)
    flags = NOT_FINITE if len(p) and not np.isfinite(p).all() else 0
    return dict(selected=sel.astype(np.uint8), in_view=in_view, n_selected=int(sel.sum()), n_in_view=int(in_view.sum()),
                flags=flags, u=u, v=v, tt=tt)


def palette_colors(labels, colors32, palette32):
    """fp32 [n, 3] by ``a3d_session_paint``'s rule: the palette entry of a label > 0 (labels >= n_palette wrap over the
    entries 1..n_palette-1), the vertex's own colour for label 0."""
    lab = np.asarray(labels, np.int64)
    pal = np.asarray(palette32, F32).reshape(-1, 3)
    entry = np.where(lab < len(pal), lab, 1 + (lab - 1) % (len(pal) - 1))
    return np.where((lab > 0)[:, None], pal[np.clip(entry, 0, len(pal) - 1)], np.asarray(colors32, F32).reshape(-1, 3))


def overlay(labels_in, on, obj, selected=None, op=NONE, value=0, colors32=None, palette32=None):
    """dict: the layer ``on`` uint8 [n] / ``obj`` int32 [n] after the call, ``labels`` int32 [n] and ``colors`` fp32 [n, 3] (None
    without ``colors32``), ``written`` bool [n] (False: a label outside 0..255, the outputs keep what they held), and the
    summary's ``changed``, ``overridden``, ``differing``, ``err``."""
    model = np.asarray(labels_in, np.int32)
    was_on, was_obj = np.asarray(on) != 0, np.asarray(obj, np.int32)
    now_on, now_obj = was_on.copy(), was_obj.copy()
    on_bytes = np.asarray(on, np.uint8).copy()
    if op != NONE and selected is not None:
        s = np.asarray(selected) != 0
        if op == PAINT:
            altered = s & (~was_on | (was_obj != value))
            now_on[s], now_obj[s] = True, value
            on_bytes[s & ~was_on] = 1
        else:
            altered = s & was_on
            now_on[s] = False
            on_bytes[altered] = 0
    else:
        altered = np.zeros(len(model), bool)
    lab = np.where(now_on, now_obj, model)
    written = (lab >= 0) & (lab <= 255)
    colors = None if colors32 is None else palette_colors(np.where(written, lab, 0), colors32, palette32)
    return dict(on=on_bytes, obj=now_obj, labels=lab.astype(np.int32), colors=colors, written=written,
                changed=int(altered.sum()), overridden=int(now_on.sum()), differing=int((now_on & (now_obj != model)).sum()),
                err=int(not written.all()))
