"""The lit colour image of a point cloud (``a3d_render_shade_lit_points``) restated in numpy float32, one operation at a time,
beside ``shade_rule.py``: the rule is stated in include/agile3d_hip.h; every product, sum, quotient and square root below is
one fp32 operation, in the header's order, so the kernel must give these bits.  The pixel rays and the quantisation are
``render_rule``'s.
"""
import numpy as np

from pick_rule import F32
from render_rule import pixel_rays, quantise


def lit_points_factor(ids, normals32, cam, ambient):
    """fp32 [h, w]: k of every pixel whose id lies in 0..n-1 (1 elsewhere): k0 = min(|N . d| / |N|, 1), or 1 where |N|^2 is 0
    or not finite; k = ambient + (1 - ambient) k0."""
    normals32 = np.asarray(normals32, F32).reshape(-1, 3)
    hit = (ids >= 0) & (ids < len(normals32))
    nn = normals32[ids[hit]]
    d = pixel_rays(cam)[hit]
    with np.errstate(all="ignore"):
        l2 = (nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]
        dot = (nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1]) + nn[:, 2] * d[:, 2]
        k0 = np.where((l2 > 0) & np.isfinite(l2), np.fmin(np.abs(dot) / np.sqrt(l2), F32(1)), F32(1)).astype(F32)
        a = F32(ambient)
        k = a + (F32(1) - a) * k0
    assert k.dtype == F32
    full = np.ones(ids.shape, F32)
    full[hit] = k
    return full


def lit_points_rule(ids, colors32, normals32, cam, ambient, background):
    """uint8 [h, w, 3]: the vertex's colour times k where 0 <= id < n, else the background, unshaded; then the quantisation."""
    colors32 = np.asarray(colors32, F32).reshape(-1, 3)
    h, w = ids.shape
    c = np.empty((h, w, 3), F32)
    c[:] = np.asarray(background, F32)
    hit = (ids >= 0) & (ids < len(colors32))
    k = lit_points_factor(ids, normals32, cam, ambient)
    c[hit] = colors32[ids[hit]] * k[hit][:, None]
    assert c.dtype == F32
    return quantise(c)


def flat_points_rule(ids, colors32, background):
    """uint8 [h, w, 3]: ``a3d_render_shade`` on a cloud, ids outside 0..n-1 as the background."""
    colors32 = np.asarray(colors32, F32).reshape(-1, 3)
    c = np.empty((*ids.shape, 3), F32)
    c[:] = np.asarray(background, F32)
    hit = (ids >= 0) & (ids < len(colors32))
    c[hit] = colors32[ids[hit]]
    return quantise(c)
