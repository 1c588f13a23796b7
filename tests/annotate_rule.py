"""The annotation rules restated in numpy float32, one operation at a time, for ``test_annotate_host.py`` (CPU) and
``test_gpu_annotate.py``: the label image (``a3d_render_labels``) and the outlines and click markers composed over a
colour image (``a3d_render_annotate``).  The rules are stated in include/agile3d_hip.h; every difference, product and sum
below is one fp32 operation, in the header's order, so the kernels must give these bits.  The quantisation is
``render_rule``'s.
"""
import numpy as np

from pick_rule import F32
from render_rule import quantise


def corner_rule(u, v):
    """int [..]: the heaviest corner of a face for the weights ``u``, ``v`` (fp32): with w = (1 - u) - v, corner 0 if
    w >= u and w >= v, else 1 if u >= v, else 2 -- ties to the lower corner, NaN weights to corner 2."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    with np.errstate(all="ignore"):
        w = (F32(1.0) - u) - v
        assert w.dtype == F32
        return np.where((w >= u) & (w >= v), 0, np.where(u >= v, 1, 2))


def labels_rule(ids, u, v, faces, labels):
    """int32 [h, w]: a3d_render_labels.  ``faces`` None: ``labels[id]`` for 0 <= id < n.  Else the label of the heaviest
    corner of face ``id`` for 0 <= id < m with its three indices in [0, n); -1 everywhere else."""
    ids = np.asarray(ids, np.int64)
    labels = np.asarray(labels, np.int32).reshape(-1)
    n = len(labels)
    out = np.full(ids.shape, -1, np.int32)
    if faces is None:
        ok = (ids >= 0) & (ids < n)
        out[ok] = labels[ids[ok]]
        return out
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = (ids >= 0) & (ids < len(f))
    tri = f[np.where(ok, ids, 0)] if len(f) else np.zeros(ids.shape + (3,), np.int64)
    ok &= ((tri >= 0) & (tri < n)).all(-1)
    corner = corner_rule(u, v)
    vertex = np.take_along_axis(tri, corner[..., None], -1)[..., 0]
    out[ok] = labels[vertex[ok]]
    return out


def outline_mask(label):
    """bool [h, w]: pixels with a label >= 1 that have a 4-neighbour INSIDE the image whose label differs."""
    label = np.asarray(label)
    h, w = label.shape
    differs = np.zeros((h, w), bool)
    differs[:, 1:] |= label[:, 1:] != label[:, :-1]         # left
    differs[:, :-1] |= label[:, :-1] != label[:, 1:]        # right
    differs[1:, :] |= label[1:, :] != label[:-1, :]         # up
    differs[:-1, :] |= label[:-1, :] != label[1:, :]        # down
    return (label >= 1) & differs


def marker_cover(t, markers, radius, inner_radius, depth_slack):
    """(hit int [h, w]: the LAST marker of the table that covers the pixel, -1 for none; inner bool [h, w]: whether the pixel
    lies within that marker's inner radius).  A row with a NaN field covers nothing."""
    t = np.asarray(t, F32)
    h, w = t.shape
    markers = np.asarray(markers, F32).reshape(-1, 6)
    fx, fy = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    r2, i2, slack = F32(radius) * F32(radius), F32(inner_radius) * F32(inner_radius), F32(depth_slack)
    hit, inner = np.full((h, w), -1), np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        for k, row in enumerate(markers):
            if np.isnan(row).any():
                continue
            dx, dy = fx - row[0], fy - row[1]
            d2 = dx * dx + dy * dy
            assert d2.dtype == F32 and d2.shape == (h, w)
            cover = (d2 <= r2) & (row[2] - t <= slack)
            hit[cover], inner[cover] = k, (d2 <= i2)[cover]
    return hit, inner


def annotate_rule(rgb, label, t, markers, radius, inner_radius, depth_slack, outline, border):
    """uint8 [h, w, 3]: a3d_render_annotate.  ``outline`` None: no outlines (``label`` is then not looked at); ``markers``
    fp32 [k, 6], possibly empty."""
    out = np.array(rgb, np.uint8)
    if outline is not None:
        out[outline_mask(label)] = quantise(np.asarray(outline, F32))
    markers = np.zeros((0, 6), F32) if markers is None else np.asarray(markers, F32).reshape(-1, 6)
    hit, inner = marker_cover(t, markers, radius, inner_radius, depth_slack)
    rim = (hit >= 0) & ~inner
    out[rim] = quantise(np.asarray(border, F32))
    core = (hit >= 0) & inner
    out[core] = quantise(markers[hit[core], 3:])
    return out
