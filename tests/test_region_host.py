"""Host side of correcting by hand (no GPU): properties of the region rule itself (``region_rule.py``), what the three
entry points of ``csrc/session_region.hip`` refuse before they touch a GPU, and ``view.camera_rows``.
``test_gpu_region.py`` holds the kernels to the same restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import region_rule as R
from pick_rule import F32

NAN, INF = float("nan"), float("inf")


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def _f32p(values):
    return np.ascontiguousarray(values, F32).ctypes.data_as(C.POINTER(C.c_float))


def _camera(lib, w=33, h=17):
    """A camera whose inverse is exact in fp32: pixel (u, v) looks along (u / 64 - 0.25, v / 64 - 0.25, 1)."""
    cam = lib.Camera()
    cam.o[:], cam.d00[:], cam.du[:], cam.dv[:] = [0, 0, 0], [-0.25, -0.25, 1], [1 / 64, 0, 0], [0, 1 / 64, 0]
    cam.width, cam.height = w, h
    return cam


# ------------------------------------------------------------------------------------------- the polygon rule
MARGIN = 2.0 ** -7


def _even_odd_f64(P, w, h):
    """(inside bool [h, w], distance float64 [h, w] of every pixel to the nearest edge) of the fp32 points in float64."""
    P = np.asarray(P, F32).astype(np.float64)
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    inside, dist = np.zeros((h, w), bool), np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for j in range(len(P)):
            (ax, ay), (bx, by) = P[j], P[(j + 1) % len(P)]
            straddles = (ay > py) != (by > py)
            inside ^= straddles & (px < (bx - ax) * (py - ay) / (by - ay) + ax)
            ex, ey, L = bx - ax, by - ay, (bx - ax) ** 2 + (by - ay) ** 2
            s = np.clip(((px - ax) * ex + (py - ay) * ey) / L, 0, 1) if L > 0 else 0.0
            dist = np.minimum(dist, np.hypot(px - ax - s * ex, py - ay - s * ey))
    return inside, dist


@pytest.mark.parametrize("seed", range(6))
def test_polygon_agrees_with_float64_away_from_the_edges(seed):
    """THE MARGIN, from the rule's roundings.  The straddle test compares fp32 values and is the same in both precisions, so
    a pixel can only be classified differently through the crossing xi = ((bx - ax) * (py - ay)) / (by - ay) + ax of an edge
    that straddles its row.  With |coordinates| <= 8192 = 2^13 every difference is at most 2^14 in size.  The two numerator
    differences, the product, the denominator's difference and the quotient are five roundings of relative size 2^-24 each;
    where the edge straddles, |py - ay| <= |by - ay|, so the quotient is at most 2^14 in size (but for those roundings) and
    off by at most 5 * 2^-24 * 2^14 = 5 * 2^-10.  The final sum is at most 2^14 + 2^13 < 2^15 and adds one rounding of at most
    2^-24 * 2^15 = 2 * 2^-10.  In all |xi - X| <= 7 * 2^-10 < 2^-7 (second-order terms are 2^-24 of that).  A pixel whose
    Euclidean distance to every edge exceeds 2^-7 is farther than that from every crossing on its row: the rule and float64
    agree on it."""
    rng = np.random.default_rng(seed)
    w, h = 96, 64
    k = int(rng.integers(3, 40))
    if seed % 2:                                                # a star around the image's centre whose long spikes reach out to
        k += k % 2                                              # the bound of the derivation: its edges cross the image
        radius = np.where(np.arange(k) % 2, rng.uniform(3.0, 40.0, k), rng.uniform(3000.0, 8100.0, k))
        angle = np.sort(rng.uniform(0, 2 * np.pi, k))
        P = (np.stack([np.cos(angle), np.sin(angle)], 1) * radius[:, None] + [w / 2, h / 2]).astype(F32)
        assert np.abs(P).max() <= 8192
    else:                                                       # vertices near the image
        P = (rng.uniform(-200.0, 200.0, (k, 2)) + [w / 2, h / 2]).astype(F32)
    if seed == 2:
        P = np.round(P * 4) / 4                                 # quarter pixels: many edges through or close to pixel centres
    got = R.polygon_cover(P, w, h)
    want, dist = _even_odd_f64(P, w, h)
    far = dist > MARGIN
    assert far.mean() > 0.9 and np.array_equal(got[far], want[far])
    assert got.any() and not got.all()


def test_rectangle_through_pixel_centres():
    """Edges exactly through pixel centres: the `>` of the straddle test keeps the row of the smaller y and drops the row of
    the larger, the `<` of the crossing test keeps the left column and drops the right one -- whichever way the rectangle is
    wound and wherever its list starts."""
    w, h = 12, 10
    want = np.zeros((h, w), bool)
    want[2:7, 3:9] = True                                       # rows 2..6 of y in [2, 7], columns 3..8 of x in [3, 9]
    corners = [(3, 2), (9, 2), (9, 7), (3, 7)]
    for pts in (corners, corners[::-1], corners[2:] + corners[:2]):
        assert np.array_equal(R.polygon_cover(pts, w, h), want)
    # two rectangles that share the edge x = 9 tile the plane: every pixel of the column belongs to exactly one
    right = R.polygon_cover([(9, 2), (11, 2), (11, 7), (9, 7)], w, h)
    assert not (right & want).any() and right[2:7, 9:11].all() and right.sum() == 10


def test_bow_tie_parity():
    """(0, 0) (10, 10) (10, 0) (0, 10): two triangles that meet at (5, 5).  Even-odd fills both and nothing else."""
    w, h = 11, 11
    got = R.polygon_cover([(0, 0), (10, 10), (10, 0), (0, 10)], w, h)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    left, right = (u < v) & (u < 10 - v), (u > v) & (u > 10 - v) & (u < 10)      # (x = 10: the polygon lies to the left)
    assert got[left].all() and left.sum() == 25 and got[right].all() and right.sum() == 16
    strict = (np.abs(u - v) > 0) & (np.abs(u + v - 10) > 0)     # off the two diagonals the parity is the geometry's
    assert np.array_equal(got[strict], (left | right)[strict])
    # a polygon traced twice covers nothing; the rule handles self-intersection by parity alone
    square = [(2, 2), (8, 2), (8, 8), (2, 8)]
    assert R.polygon_cover(square, w, h).sum() == 36 and not R.polygon_cover(square + square, w, h).any()


def test_one_point_stroke_is_a_disc():
    w, h = 21, 17
    c, r = (9.25, 7.5), 4.3
    got = R.stroke_cover([c], r, w, h)
    u, v = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    dx, dy = u - F32(c[0]), v - F32(c[1])
    assert np.array_equal(got, dx * dx + dy * dy <= F32(r) * F32(r)) and 50 < got.sum() < 70
    assert np.array_equal(R.stroke_cover([c, c], r, w, h), got)             # L == 0: the same disc
    assert np.array_equal(R.stroke_cover([c, c, c], r, w, h), got)
    # a segment: the discs at its ends and the band between them
    band = R.stroke_cover([(4, 8), (15, 8)], 2.0, w, h)
    assert band[6:11, 4:16].all() and band[8, 2] and band[8, 17] and not band[8, 1] and not band[5, 10] and not band[6, 2]
    assert np.array_equal(R.stroke_cover([(4, 8), (10, 8), (15, 8)], 2.0, w, h), band)


def test_add_then_subtract_restores_a_mask():
    w, h = 40, 30
    rng = np.random.default_rng(3)
    poly = rng.uniform(-5, 45, (7, 2))
    base = R.region_mask(R.STROKE, [(5, 5), (30, 20)], w, h, 3.0)
    shape = R.polygon_cover(poly, w, h)
    assert shape.any() and base.any()
    disjoint = (base.astype(bool) & ~shape).astype(np.uint8)    # a mask that does not meet the shape
    added = R.region_mask(R.POLYGON, poly, w, h, mode=R.ADD, mask=disjoint)
    assert np.array_equal(added.astype(bool), disjoint.astype(bool) | shape)
    assert np.array_equal(R.region_mask(R.POLYGON, poly, w, h, mode=R.SUBTRACT, mask=added), disjoint)
    # and the other way round on a mask that holds the shape; bytes that are not 0 count as 1, the bytes written are 0 or 1
    holds = (base.astype(bool) | shape).astype(np.uint8) * 200
    cut = R.region_mask(R.POLYGON, poly, w, h, mode=R.SUBTRACT, mask=holds)
    back = R.region_mask(R.POLYGON, poly, w, h, mode=R.ADD, mask=cut)
    assert set(np.unique(back)) == {0, 1} and np.array_equal(back.astype(bool), holds.astype(bool))
    assert np.array_equal(R.region_mask(R.POLYGON, poly, w, h, mode=R.REPLACE, mask=holds), shape.astype(np.uint8))


# ------------------------------------------------------------------------------------------- refusals (no GPU needed)
def test_struct_layouts():
    lib, _ = _lib()
    assert C.sizeof(lib.SelectSummary) == 24 and C.sizeof(lib.OverlaySummary) == 32
    assert C.sizeof(lib.SelectArgs) == 152 and lib.SelectArgs.camera.offset == 16 and lib.SelectArgs.rows.offset == 72
    assert lib.SelectArgs.slack.offset == 108 and lib.SelectArgs.mask_dev.offset == 112 and lib.SelectArgs.summary_dev.offset == 144
    assert C.sizeof(lib.SessionOverlayArgs) == 96 and lib.SessionOverlayArgs.op.offset == 80
    assert lib.A3D_REGION_MAX_POINTS == 256


FAKE = 0x1000                                                   # a "device pointer" no refused call ever follows

MASK_BAD = {
    "width 0": dict(width=0),
    "height 4097": dict(height=4097),
    "a shape that is none": dict(shape=2),
    "a negative shape": dict(shape=-1),
    "mode 3": dict(mode=3),
    "mode -1": dict(mode=-1),
    "a polygon of 2 points": dict(points=[(0, 0), (1, 1)]),
    "a polygon of 257 points": dict(points=[(i, i % 7) for i in range(257)]),
    "a stroke of no point": dict(shape=1, points=[], radius=1.0),
    "a stroke of 257 points": dict(shape=1, points=[(i, 0) for i in range(257)], radius=1.0),
    "a NaN point": dict(points=[(0, 0), (4, NAN), (0, 4)]),
    "an infinite point": dict(shape=1, points=[(0, 0), (INF, 1)], radius=1.0),
    "the last of 256 points NaN": dict(points=[(i, i % 5) for i in range(255)] + [(NAN, 0)]),
    "a stroke of radius 0": dict(shape=1, points=[(1, 1)], radius=0.0),
    "a stroke of negative radius": dict(shape=1, points=[(1, 1)], radius=-1.0),
    "a stroke of NaN radius": dict(shape=1, points=[(1, 1)], radius=NAN),
    "a stroke of infinite radius": dict(shape=1, points=[(1, 1)], radius=INF),
    "no points": dict(points=None),
    "no mask": dict(mask=None),
}


@pytest.mark.parametrize("name", sorted(MASK_BAD))
def test_region_mask_refuses(name):
    lib, L = _lib()
    a = dict(width=8, height=8, shape=0, points=[(0, 0), (4, 0), (0, 4)], radius=0.0, mode=0, mask=FAKE)
    a.update(MASK_BAD[name])
    pts = None if a["points"] is None else _f32p(np.asarray(a["points"], F32).reshape(-1, 2))
    k = 3 if a["points"] is None else len(a["points"])
    assert L.a3d_region_mask(a["width"], a["height"], a["shape"], pts, k, a["radius"], a["mode"], a["mask"], None) == lib.A3D_ERR_INVALID
    assert "a3d_region_mask" in L.a3d_last_error().decode()


def _select_args(lib, **kw):
    a = lib.SelectArgs()
    a.xyz_dev, a.n, a.camera = FAKE, 4, _camera(lib)
    a.rows[:] = [64, 0, 16, 0, 64, 16, 0, 0, 1]
    a.slack, a.mask_dev, a.t_dev, a.selected_dev, a.summary_dev = 0.0, FAKE, None, FAKE, FAKE
    keep = []
    for name, value in kw.items():
        if name == "section":
            keep.append(value)
            a.section = C.pointer(value)
        elif name == "rows":
            a.rows[:] = value
        elif name == "camera":
            a.camera = value
        else:
            setattr(a, name, value)
    return a, keep


def _section(lib, planes=(), cull=0, n_planes=None):
    s = lib.Section()
    s.n_planes, s.cull = len(planes) if n_planes is None else n_planes, cull
    for k, p in enumerate(planes):
        s.planes[k][:] = [float(x) for x in p]
    return s


def test_select_vertices_refuses():
    lib, L = _lib()
    flat, big, nan_cam = _camera(lib), _camera(lib, 4097, 4), _camera(lib)
    flat.d00[:] = [1, 1, 0]                                     # du, dv, d00 in one plane: no camera
    nan_cam.o[0] = NAN
    bad = {
        "a camera in one plane": dict(camera=flat), "a camera too wide": dict(camera=big), "a NaN camera": dict(camera=nan_cam),
        "9 planes": dict(section=_section(lib, n_planes=9)), "a zero normal": dict(section=_section(lib, [(0, 0, 0, 0)])),
        "a NaN plane": dict(section=_section(lib, [(0, 0, 1, NAN)])), "cull 3": dict(section=_section(lib, cull=3)),
        "a negative slack": dict(slack=-1e-3), "a NaN slack": dict(slack=NAN), "an infinite slack": dict(slack=INF),
        "n < 0": dict(n=-1), "n = 2^31": dict(n=1 << 31),
        "no vertices": dict(xyz_dev=None), "no mask": dict(mask_dev=None), "no selection": dict(selected_dev=None),
        "no summary": dict(summary_dev=None),
        "a NaN row": dict(rows=[64, 0, 16, 0, NAN, 16, 0, 0, 1]), "an infinite row": dict(rows=[64, 0, 16, 0, 64, 16, 0, 0, INF]),
    }
    for name, kw in bad.items():
        a, keep = _select_args(lib, **kw)
        assert L.a3d_select_vertices(C.byref(a), None) == lib.A3D_ERR_INVALID, name
        assert "a3d_select_vertices" in L.a3d_last_error().decode(), name
    assert L.a3d_select_vertices(None, None) == lib.A3D_ERR_INVALID


def _overlay_args(lib, **kw):
    a = lib.SessionOverlayArgs()
    a.labels_in_dev, a.n, a.manual_on_dev, a.manual_obj_dev, a.selected_dev = FAKE, 4, FAKE, FAKE, FAKE
    a.colors_full_dev, a.palette_dev, a.labels_out_dev, a.colors_out_dev, a.summary_dev = FAKE, FAKE, FAKE, FAKE, FAKE
    a.op, a.obj, a.n_palette = 1, 3, 8
    for name, value in kw.items():
        setattr(a, name, value)
    return a


def test_session_overlay_refuses():
    lib, L = _lib()
    bad = {
        "n < 0": dict(n=-1), "n = 2^31": dict(n=1 << 31), "op 3": dict(op=3), "op -1": dict(op=-1), "obj 256": dict(obj=256),
        "obj -1": dict(obj=-1), "no labels": dict(labels_in_dev=None), "no on": dict(manual_on_dev=None),
        "no obj": dict(manual_obj_dev=None), "no summary": dict(summary_dev=None),
        "labels out alone": dict(colors_out_dev=None), "colours out alone": dict(labels_out_dev=None),
        "outputs without colours": dict(colors_full_dev=None), "outputs without a palette": dict(palette_dev=None),
        "a palette of 1": dict(n_palette=1), "a palette of 257": dict(n_palette=257),
    }
    for name, kw in bad.items():
        assert L.a3d_session_overlay(C.byref(_overlay_args(lib, **kw)), None) == lib.A3D_ERR_INVALID, name
        assert "a3d_session_overlay" in L.a3d_last_error().decode(), name
    assert L.a3d_session_overlay(None, None) == lib.A3D_ERR_INVALID


# ------------------------------------------------------------------------------------------- camera_rows
def test_camera_rows_against_numpy():
    lib, _ = _lib()
    from agile3d_amd import view as V
    from session_kit import camera_of
    assert V.camera_rows(_camera(lib)).tolist() == [64, 0, 16, 0, 64, 16, 0, 0, 1]
    for eye, target, fov, size in (([0.0, -1.0, 0.6], [0.0, 3.0, 0.0], 60.0, (37, 29)), ([50.3, -48.7, 3.0], [52.0, -45.0, 1.2], 35.0, (1024, 768)),
                                   ([1.0, 2.0, 3.0], [-4.0, 0.5, 0.0], 100.0, (4096, 16))):
        cam = camera_of(eye, target, fov, size)
        rows = V.camera_rows(cam)
        assert rows.dtype == np.float32 and rows.shape == (9,)
        m = np.stack([np.array(cam.du[:], np.float64), np.array(cam.dv[:], np.float64), np.array(cam.d00[:], np.float64)], 1)
        want = np.linalg.inv(m).reshape(9)
        assert np.all(np.abs(rows - want) <= 1e-6 * np.abs(want).max())          # relative to the matrix: an entry that
                                                                                 # cancels to nearly 0 has no digits of its own
    flat = _camera(lib)
    flat.d00[:] = [1, 1, 0]
    with pytest.raises(ValueError):
        V.camera_rows(flat)
