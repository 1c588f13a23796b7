"""CPU: ``view.marker_table`` (the projection of click points to the marker rows ``a3d_render_annotate`` draws) and the
numpy restatement of the annotation rules itself (``annotate_rule.py``), which ``test_gpu_annotate.py`` holds the kernels to.
"""
import numpy as np
import pytest

from agile3d_amd.view import marker_table
from annotate_rule import annotate_rule, corner_rule, labels_rule, marker_cover, outline_mask
from pick_rule import F32
from render_rule import camera_fields
from session_kit import FAR, camera_of

EPS = 2.0 ** -24


def _camera(shift):
    return camera_of(shift + [0.0, -1.0, 0.6], shift + [0.0, 3.0, 0.0], 60.0, (37, 29))


@pytest.mark.parametrize("shift", [np.zeros(3), FAR], ids=["near", "50 m out"])
def test_marker_table_projects_a_point_of_a_pixels_ray_to_that_pixel(shift):
    """A point P = o + s (d00 + u du + v dv) =: o + s D, formed in float64 from the camera's fp32 fields, lies on the ray of
    the position (u, v) at t = s |D|.  ``marker_table`` is handed p = fp32(P), as the session's click table holds it, so
    p = P + e with |e_i| <= 2^-24 |P_i|, |e| <= 2^-24 |P|.  With ra, rb, rc the rows of [du dv d00]^-1:
    (a, b, c) = (s u + ra.e, s v + rb.e, s + rc.e), hence
        |x - u| = |ra.e - u rc.e| / (s + rc.e) <= (|ra| + |u| |rc|) |e| / (s - |rc| |e|)        (likewise y with rb, v)
        |t - s |D|| <= |e|
    to which the one rounding of the result to fp32 adds 2^-24 |x| (2^-24 t).  The float64 arithmetic itself (a 3 x 3 solve
    of condition ~ the focal length in pixels) stays 8 orders below that; 1 % on the bound and 1e-9 absolute cover it.  50 m
    out |P| grows from ~3 to ~70, and the bound with it: for the nearest point (s = 0.5) at the position farthest outside
    the image it reaches 1.2e-3 of a pixel, which is why the last line only asks that it stay below 1e-2."""
    cam = _camera(shift)
    o, d00, du, dv, w, h = (np.asarray(f, np.float64) if np.ndim(f) else f for f in camera_fields(cam))
    inv = np.linalg.inv(np.stack([du, dv, d00], 1))
    ra, rb, rc = np.linalg.norm(inv, axis=1)
    uv = [(0.0, 0.0), (18.0, 14.0), (36.0, 28.0), (12.25, 7.75), (-3.5, 40.25), (100.0, -60.0)]
    rows, want = [], []
    for s in (0.5, 3.0, 20.0):
        for u, v in uv:
            D = d00 + u * du + v * dv
            rows.append(o + s * D)
            want.append((u, v, s, np.linalg.norm(D)))
    p32 = np.asarray(rows).astype(F32)
    col = np.random.default_rng(1).uniform(0, 1, (len(rows), 3)).astype(F32)
    got = marker_table(cam, p32, col)
    assert got.dtype == F32 and got.shape == (len(rows), 6) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got[:, 3:], col)
    worst = 0.0
    for (x, y, t), p, (u, v, s, ld) in zip(got[:, :3].astype(np.float64), p32.astype(np.float64), want):
        e = EPS * np.linalg.norm(p) * (1 + EPS)
        bx = 1.01 * (ra + abs(u) * rc) * e / (s - rc * e) + EPS * abs(x) + 1e-9
        by = 1.01 * (rb + abs(v) * rc) * e / (s - rc * e) + EPS * abs(y) + 1e-9
        bt = 1.01 * e + EPS * t + 1e-9
        assert abs(x - u) <= bx and abs(y - v) <= by and abs(t - s * ld) <= bt, (u, v, s, x, y, t, bx, by, bt)
        worst = max(worst, bx, by)
    assert worst < 1e-2, worst


def test_marker_table_drops_what_lies_behind_the_camera_and_keeps_the_order():
    cam = _camera(np.zeros(3))
    o, d00, du, dv, w, h = (np.asarray(f, np.float64) if np.ndim(f) else f for f in camera_fields(cam))
    ahead = [o + s * (d00 + u * du + v * dv) for s, u, v in ((2.0, 3.0, 4.0), (1.0, 30.0, 2.0), (5.0, 10.0, 20.0))]
    behind = o - 2.0 * (d00 + 5.0 * du + 5.0 * dv)
    pts = np.array([ahead[0], behind, ahead[1], o, [np.nan, 0.0, 0.0], ahead[2], [np.inf, 0.0, 1.0]])
    col = np.arange(21, dtype=np.float64).reshape(7, 3) / 32
    got = marker_table(cam, pts, col)
    assert got.shape == (3, 6) and np.array_equal(got[:, 3:], col[[0, 2, 5]].astype(F32))     # (o itself has c = 0)
    assert np.allclose(got[:, :2], [[3.0, 4.0], [30.0, 2.0], [10.0, 20.0]], atol=1e-4)
    nan_colour = marker_table(cam, pts[[0, 2]], [[0.1, np.nan, 0.2], [0.3, 0.4, 0.5]])
    assert nan_colour.shape == (1, 6) and np.array_equal(nan_colour[0, 3:], F32([0.3, 0.4, 0.5]))
    assert marker_table(cam, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 6)
    with pytest.raises(ValueError):
        marker_table(cam, pts, col[:3])


# ------------------------------------------------------------------------------------------- the restatement itself
def _random_view(seed, h=29, w=37):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    label = rng.integers(-1, 3, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.int32)   # 4 x 4 patches
    t = np.where(label < 0, np.inf, rng.uniform(1.0, 5.0, (h, w))).astype(F32)
    return rgb, label, t


def test_rule_without_outline_and_marker_returns_the_image():
    rgb, label, t = _random_view(0)
    assert np.array_equal(annotate_rule(rgb, label, t, None, 5.0, 4.0, 0.1, None, (1, 1, 1)), rgb)
    assert np.array_equal(annotate_rule(rgb, None, t, np.zeros((0, 6)), 5.0, 4.0, 0.1, None, (1, 1, 1)), rgb)
    nan_rows = np.full((3, 6), 0.5, F32)
    nan_rows[0, 0] = nan_rows[1, 2] = nan_rows[2, 5] = np.nan                       # a NaN anywhere in a row: it covers nothing
    assert np.array_equal(annotate_rule(rgb, label, t, nan_rows, 50.0, 40.0, 1e9, None, (1, 1, 1)), rgb)


def test_rule_outlines_only_objects_and_never_along_the_image_edge():
    rgb, label, t = _random_view(1)
    rgb[...] = 200
    out = annotate_rule(rgb, label, t, None, 5.0, 4.0, 0.1, (0.0, 0.0, 0.0), (1, 1, 1))
    changed = (out != rgb).any(-1)
    assert changed.any() and (label[changed] >= 1).all() and np.array_equal(changed, outline_mask(label))
    # object 1 fills the left half up to the image's edge, object 2 the right half; below them background and nothing
    small = np.array([[1, 1, 2, 2],
                      [1, 1, 2, 2],
                      [1, 1, 2, 2],
                      [0, 0, -1, -1],
                      [0, 0, -1, -1]], np.int32)
    want = np.array([[0, 1, 1, 0],          # both sides of the border between 1 and 2; nothing along the top, left, right
                     [0, 1, 1, 0],
                     [1, 1, 1, 1],          # against the background and against nothing
                     [0, 0, 0, 0],          # background and nothing are never outlined, not even against each other
                     [0, 0, 0, 0]], bool)
    assert np.array_equal(outline_mask(small), want)
    assert not outline_mask(np.full((1, 1), 3, np.int32)).any() and not outline_mask(np.full((4, 5), 3, np.int32)).any()


def test_rule_markers_cover_by_distance_and_depth_and_the_last_wins():
    t = np.full((21, 21), 2.0, F32)
    t[:, 15:] = np.inf                                                              # the right columns show nothing
    rgb = np.zeros((21, 21, 3), np.uint8)
    markers = F32([[10, 10, 2.0, 1, 0, 0], [14, 10, 2.0, 0, 1, 0]])
    hit, inner = marker_cover(t, markers[:1], 5.0, 3.0, 0.1)
    assert hit[14, 13] == 0 and not inner[14, 13] and hit[15, 13] == -1             # 3^2 + 4^2 == 5^2 exactly; 3^2 + 5^2 is outside
    assert inner[10, 13] and not inner[10, 14] and inner[10, 10]
    hit, inner = marker_cover(t, markers, 5.0, 3.0, 0.1)
    assert hit[10, 10] == 1 and not inner[10, 10] and hit[10, 8] == 0 and hit[10, 17] == 1   # the later one wins where both cover
    hidden = marker_cover(t, F32([[10, 10, 2.11, 1, 0, 0]]), 5.0, 3.0, 0.1)[0]
    assert (hidden[:, :15] == -1).all() and (hidden[10, 15] == 0)                   # behind the surface, seen where nothing is
    assert (marker_cover(t, F32([[10, 10, 2.09, 1, 0, 0]]), 5.0, 3.0, 0.1)[0][10, 10]) == 0
    out = annotate_rule(rgb, None, t, markers, 5.0, 3.0, 0.1, None, (1.0, 1.0, 1.0))
    assert out[10, 12].tolist() == [0, 255, 0] and out[10, 7].tolist() == [255, 0, 0] and out[10, 5].tolist() == [255, 255, 255]


def test_corner_rule_partitions_a_face():
    """Every weight pair goes to exactly one corner, the heaviest; u == w goes to corner 0, u == v above w to corner 1."""
    g = np.arange(0, 65, dtype=np.float64) / 64
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    u, v = u[u + v <= 1], v[u + v <= 1]
    w = 1 - u - v                                                                   # (exact: multiples of 1/64)
    got = corner_rule(u.astype(F32), v.astype(F32))
    weights = np.stack([w, u, v], 1)
    assert np.array_equal(got, weights.argmax(1))                                   # argmax: the first of equal maxima, the lower corner
    assert set(got.tolist()) == {0, 1, 2}
    assert corner_rule(F32(0.375), F32(0.25)) == 0                                  # u == w > v
    assert corner_rule(F32(0.375), F32(0.375)) == 1                                 # u == v > w
    assert corner_rule(F32(0.25), F32(0.5)) == 2 and corner_rule(F32(0.25), F32(0.25)) == 0
    for u_, v_ in ((np.nan, 0.2), (0.2, np.nan), (np.nan, np.nan)):
        assert corner_rule(F32(u_), F32(v_)) == 2
    # the label image takes that corner's label; out-of-range ids and face indices show nothing
    faces = np.array([[0, 1, 2], [2, 1, 7], [-1, 0, 1]], np.int32)
    ids = np.array([[0, 0, 0, 1, 2, 3, -1]], np.int32)
    uu, vv = F32([[0.1, 0.8, 0.1, 0.1, 0.1, 0.1, 0.0]]), F32([[0.1, 0.1, 0.8, 0.1, 0.1, 0.1, 0.0]])
    assert labels_rule(ids, uu, vv, faces, [5, 6, 7]).tolist() == [[5, 6, 7, -1, -1, -1, -1]]
    assert labels_rule(ids, None, None, None, [5, 6, 7]).tolist() == [[5, 5, 5, 6, 7, -1, -1]]
    assert (labels_rule(ids, uu, vv, np.zeros((0, 3), np.int32), [5, 6, 7]) == -1).all()
