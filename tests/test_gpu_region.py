"""-m gpu: correcting by hand, the three kernels of csrc/session_region.hip through ``agile3d_amd.view``, bit for bit against
the numpy restatement of their rules (``region_rule.py``).

1  region_mask: polygons and strokes, vertices outside the image, 1 / 2 / 3 / 4 / 256 points, the three modes, odd sizes
2  select_vertices: vertices behind the camera, on c == 0, NaN and infinite, projected beyond 1e9 pixels, exactly on the image's
   borders; visible and through, slack 0 and > 0, +inf in the t image, sections of 0, 1 and 8 planes; the summary's counts;
   and, on a rendered cloud, that everything the id image shows is selected
3  session_overlay: paint, erase and none, no selection, the palette's wrap, a label of 256, a pure layer update, determinism
"""
import ctypes as C

import numpy as np
import pytest
import torch

import region_rule as R
from agile3d_amd import lib as L
from agile3d_amd import view as V
from pick_rule import F32
from session_kit import DEV, _dev, bits, camera_of, cloud_scene, render

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (17, 33), (64, 48))                            # (width, height): one pixel, odd strips, whole strips


# ---------------------------------------------------------------------------------------------------- 1
def _shapes(w, h):
    """name -> (shape, points, radius) for a w x h image."""
    rng = np.random.default_rng(w * 100 + h)
    ring = np.linspace(0, 2 * np.pi, 256, endpoint=False)
    wobble = 1 + 0.35 * np.sin(7 * ring)
    star = np.stack([w / 2 + 0.7 * w * wobble * np.cos(ring), h / 2 + 0.7 * h * wobble * np.sin(ring)], 1)
    path = np.stack([np.linspace(-3, w + 2, 256), h / 2 + 0.4 * h * np.sin(np.linspace(0, 9, 256))], 1)
    return {
        "a triangle with a vertex outside": ("polygon", [(-4.5, 0.25 * h), (1.2 * w, -2.0), (0.6 * w, 1.5 * h)], None),
        "a quad through pixel centres": ("polygon", [(0, 0), (w // 2, 0), (w // 2, h // 2), (0, h // 2)], None),
        "a bow tie": ("polygon", [(0, 0), (w, h), (w, 0), (0, h)], None),
        "256 points, a star beyond the image": ("polygon", star, None),
        "a random polygon": ("polygon", rng.uniform(-0.5 * w, 1.5 * w, (9, 2)), None),
        "a disc": ("stroke", [(0.4 * w, 0.6 * h)], 0.3 * (w + h)),
        "a disc of a repeated point": ("stroke", [(0.4 * w, 0.6 * h)] * 2, 0.3 * (w + h)),
        "a segment from outside": ("stroke", [(-5.0, 0.2 * h), (0.8 * w, 0.9 * h)], 1.75),
        "a stroke of 256 points": ("stroke", path, 0.08 * h + 0.5),
        "a hair": ("stroke", [(0.0, 0.0), (w - 1.0, h - 1.0)], 1e-3),
    }


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_region_mask_against_the_rule(size):
    w, h = size
    rng = np.random.default_rng(w)
    before = (rng.integers(0, 3, (h, w)) * 100).astype(np.uint8)             # 0, 100 and 200: a byte that is not 0 counts as 1
    n_set = 0
    for name, (shape, points, radius) in _shapes(w, h).items():
        code = R.POLYGON if shape == "polygon" else R.STROKE
        got = V.region_mask(shape, points, w, h, radius, device=DEV)
        want = R.region_mask(code, points, w, h, radius)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w)
        assert np.array_equal(got.cpu().numpy(), want), name
        n_set += int(want.sum())
        for mode, mode_code in (("replace", R.REPLACE), ("add", R.ADD), ("subtract", R.SUBTRACT)):
            mask = _dev(before, np.uint8)
            assert V.region_mask(shape, points, w, h, radius, mode, mask) is mask
            assert np.array_equal(mask.cpu().numpy(), R.region_mask(code, points, w, h, radius, mode_code, before)), (name, mode)
    assert n_set > 0


def test_region_mask_wrapper_refuses():
    mask = torch.zeros((8, 8), dtype=torch.uint8, device=DEV)
    tri = [(0, 0), (4, 0), (0, 4)]
    for bad in (lambda: V.region_mask("circle", tri, 8, 8, device=DEV), lambda: V.region_mask("polygon", tri[:2], 8, 8, device=DEV),
                lambda: V.region_mask("polygon", tri, 8, 8, radius=1.0, device=DEV), lambda: V.region_mask("stroke", tri, 8, 8, device=DEV),
                lambda: V.region_mask("stroke", tri, 8, 8, radius=0.0, device=DEV), lambda: V.region_mask("polygon", tri, 8, 8, mode="xor", device=DEV),
                lambda: V.region_mask("polygon", tri, 8, 8, mode="add", device=DEV), lambda: V.region_mask("polygon", tri, 9, 8, mask=mask),
                lambda: V.region_mask("polygon", [(0, 0), (np.nan, 1), (2, 2)], 8, 8, device=DEV),
                lambda: V.region_mask("polygon", tri, 8, 8, mask=mask.to(torch.int32)), lambda: V.region_mask("polygon", tri, 0, 8, device=DEV)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------- 2
W, H = 33, 17
COUNTS = (0, 1, 63, 64, 65, 257, 1025, 5000)                 # (1025: one vertex beyond a workgroup of 1024)


def exact_camera(w=W, h=H):
    """Pixel (u, v) looks along (u / 64 - 0.25, v / 64 - 0.25, 1) from the origin: the rows of the inverse are (64, 0, 16),
    (0, 64, 16), (0, 0, 1), exact in fp32, so a vertex (px, py, 1) projects to exactly (64 px + 16, 64 py + 16)."""
    cam = L.Camera()
    cam.o[:], cam.d00[:], cam.du[:], cam.dv[:] = [0, 0, 0], [-0.25, -0.25, 1], [1 / 64, 0, 0], [0, 1 / 64, 0]
    cam.width, cam.height = w, h
    return cam


def special_vertices():
    """Vertices at the edges of the rule, for ``exact_camera``: name -> (x, y, z)."""
    nan, inf = np.nan, np.inf
    x_of = lambda pixel: (pixel - 16) / 64                      # the px that projects to that x at pz = 1
    return {
        "in the middle": (0.0, -0.125, 1.0),
        "behind the camera": (0.0, 0.0, -1.0), "behind, projecting into the image": (0.1, 0.05, -2.0),
        "on c == 0": (0.3, 0.1, 0.0), "on c == 0 at the origin": (0.0, 0.0, 0.0), "c == -0": (0.3, 0.1, -0.0),
        "a NaN x": (nan, 0.0, 1.0), "a NaN z": (0.0, 0.0, nan), "+inf x": (inf, 0.0, 1.0), "-inf y": (0.0, -inf, 1.0),
        "+inf z": (0.0, 0.0, inf), "all inf": (inf, inf, inf),
        "beyond +1e9 pixels": (1.0, 0.0, 2.0 ** -40), "beyond -1e9 pixels": (-1.0, -1.0, 2.0 ** -40),
        "beyond the float range": (3e38, 0.0, 1e-38),
        "exactly on x = -0.5": (x_of(-0.5), 0.0, 1.0), "just left of x = -0.5": (x_of(-0.5 - 2.0 ** -10), 0.0, 1.0),
        "exactly on x = w - 0.5": (x_of(W - 0.5), 0.0, 1.0), "just left of x = w - 0.5": (x_of(W - 0.5 - 2.0 ** -10), 0.0, 1.0),
        "exactly on y = -0.5": (0.0, x_of(-0.5), 1.0), "exactly on y = h - 0.5": (0.0, x_of(H - 0.5), 1.0),
        "exactly on x = 7.5": (x_of(7.5), 0.0, 1.0), "the last pixel": (x_of(W - 1), x_of(H - 1), 1.0), "the first pixel": (x_of(0), x_of(0), 8.0 / 8),
    }


@pytest.fixture(scope="module")
def select_case():
    """5000 vertices for ``exact_camera``: a cloud in front of it that overflows the image on every side, depths 0.5 .. 4, with
    the special vertices at rows 1 .. and again from row 4000 on; a mask (a polygon and a stroke), a t image that is +inf in
    a third of the pixels and otherwise lies among the vertices' depths, and sections of 0, 1 and 8 planes."""
    rng = np.random.default_rng(11)
    n = COUNTS[-1]
    z = rng.uniform(0.5, 4.0, n)
    xyz = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(-0.45, 0.3, n) * z, z], 1).astype(F32)
    special = np.array(list(special_vertices().values()), np.float64)
    with np.errstate(over="ignore"):
        xyz[1:1 + len(special)] = special.astype(F32)
        xyz[4000:4000 + len(special)] = special.astype(F32)
    cam = exact_camera()
    mask = R.region_mask(R.POLYGON, [(-2, -2), (20.5, 1), (34, 12), (12, 19), (3.25, 9)], W, H)
    mask = R.region_mask(R.STROKE, [(30, 2), (26, 14)], W, H, 2.5, R.ADD, mask)
    mask[16, 8] = 200                                           # (a byte that is neither 0 nor 1; the pixel of "exactly on x = 7.5")
    assert 0.3 < (mask != 0).mean() < 0.9
    t = rng.uniform(0.6, 4.2, (H, W)).astype(F32)
    t[rng.uniform(size=(H, W)) < 0.33] = np.inf
    s = np.sqrt(0.5)
    planes = {0: np.zeros((0, 4), F32), 1: np.array([[0.6, 0.0, 0.8, 1.4]], F32),
              8: np.array([[1, 0, 0, -1.2], [-1, 0, 0, -1.2], [0, 1, 0, -1.0], [0, -1, 0, -1.0], [0, 0, 1, 0.7], [0, 0, -1, -3.5],
                           [s, s, 0, -1.1], [0.6, 0.0, -0.8, -2.6]], F32)}
    return xyz, cam, V.camera_rows(cam), mask, t, planes


def _section(planes):
    if len(planes) == 0:
        return None
    s = L.Section()
    s.n_planes, s.cull = len(planes), 0
    for k, p in enumerate(planes):
        s.planes[k][:] = [float(x) for x in p]
    return s


def _select(xyz, cam, mask, t, slack, planes, rows=None):
    n = len(xyz)
    selected = torch.full((n,), 7, dtype=torch.uint8, device=DEV)            # a sentinel: every byte has to be written
    summary = torch.full((V.SELECT_SUMMARY.itemsize,), 0xAB, dtype=torch.uint8, device=DEV)
    got, s = V.select_vertices(_dev(xyz.reshape(-1, 3), F32), cam, _dev(mask, np.uint8), None if t is None else _dev(t, F32), slack,
                               _section(planes), rows, selected, summary)
    assert got is selected and s is summary
    return selected.cpu().numpy(), V.read_select_summary(summary.cpu().numpy())


def test_select_rule_on_the_special_vertices(select_case):
    """What the restatement itself says at the edges (so that the GPU comparison below is held to the issue's rule, not to a
    restatement that drifted): through an all-ones mask, without a section."""
    _, cam, rows, _, _, _ = select_case
    assert rows.tolist() == [64, 0, 16, 0, 64, 16, 0, 0, 1]
    names = list(special_vertices())
    with np.errstate(over="ignore"):
        xyz = np.array(list(special_vertices().values()), np.float64).astype(F32)
    want = R.select(xyz, cam, rows, np.ones((H, W), np.uint8))
    inside = {"in the middle": (16, 8), "exactly on x = -0.5": (0, 16), "just left of x = w - 0.5": (W - 1, 16), "exactly on x = 7.5": (8, 16),
              "exactly on y = -0.5": (16, 0),
              "the last pixel": (W - 1, H - 1), "the first pixel": (0, 0)}
    for k, name in enumerate(names):
        assert bool(want["selected"][k]) == (name in inside), name
        if name in inside:
            assert (want["u"][k], want["v"][k]) == inside[name], name
    assert want["flags"] == R.NOT_FINITE and want["n_selected"] == want["n_in_view"] == len(inside)


@pytest.mark.parametrize("n", COUNTS)
def test_select_against_the_rule(select_case, n):
    xyz, cam, rows, mask, t, planes = select_case
    xyz = xyz[:n]
    cases = [(None, 0.0, 0), (t, 0.0, 0), (t, 0.35, 0), (None, 0.0, 1), (t, 0.35, 1), (None, 0.0, 8), (t, 0.0, 8), (t, 0.35, 8)]
    seen = set()
    for tt, slack, k in cases:
        got, summary = _select(xyz, cam, mask, tt, slack, planes[k])
        want = R.select(xyz, cam, rows, mask, tt, slack, planes[k])
        assert np.array_equal(got, want["selected"]), (slack, k)
        assert summary == {"selected": want["n_selected"], "in_view": want["n_in_view"], "flags": want["flags"]}, (slack, k)
        seen.add((want["n_selected"], want["n_in_view"]))
    if n == COUNTS[-1]:
        assert len(seen) == len(cases)                          # every case selects another set: each input plays its part
        full = R.select(xyz, cam, rows, mask, t, 0.35, planes[0])
        assert 100 < full["n_selected"] < full["n_in_view"] < n - 500 and full["flags"] == R.NOT_FINITE
        # the rows argument is what the kernel projects with: other rows, another selection (and the rule's under them)
        other = rows.copy()
        other[:3] *= F32(1.25)                                  # (the first row alone: scaling all three changes no quotient)
        got, summary = _select(xyz, cam, mask, None, 0.0, planes[0], other)
        want = R.select(xyz, cam, other, mask)
        assert np.array_equal(got, want["selected"]) and want["n_selected"] != R.select(xyz, cam, rows, mask)["n_selected"]
    if n == 0:
        assert summary == {"selected": 0, "in_view": 0, "flags": 0}


def test_select_is_deterministic_and_checks_its_arguments(select_case):
    xyz, cam, rows, mask, t, planes = select_case
    a, b = _select(xyz, cam, mask, t, 0.1, planes[8]), _select(xyz, cam, mask, t, 0.1, planes[8])
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    x, m = _dev(xyz, F32), _dev(mask, np.uint8)
    for bad in (lambda: V.select_vertices(x, cam, m[:, :-1].contiguous()), lambda: V.select_vertices(x, cam, m, slack=-1.0),
                lambda: V.select_vertices(x, cam, m, slack=np.nan), lambda: V.select_vertices(x, cam, m.to(torch.int32)),
                lambda: V.select_vertices(x, cam, m, t=torch.zeros((H, W + 1), device=DEV)),
                lambda: V.select_vertices(x, cam, m, rows=np.zeros(8, F32)), lambda: V.select_vertices(x, cam, m, rows=np.full(9, np.inf, F32)),
                lambda: V.select_vertices(x, cam, m, section="none"), lambda: V.select_vertices(x.cpu(), cam, m),
                lambda: V.select_vertices(x, cam, m, selected=torch.zeros(3, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            bad()


def test_a_second_pass_of_the_grid(select_case):
    """More vertices than one pass of the grid holds (256 workgroups of 1024): a thread takes a second vertex, and the
    workgroups' sums are larger than a byte, a wave or a workgroup could hold."""
    xyz, cam, rows, mask, t, planes = select_case
    n = 256 * 1024 + 77
    big = np.ascontiguousarray(np.resize(xyz, (n, 3)))
    got, summary = _select(big, cam, mask, t, 0.35, planes[1])
    want = R.select(big, cam, rows, mask, t, 0.35, planes[1])
    assert np.array_equal(got, want["selected"]) and want["selected"][-77:].any()
    assert summary == {"selected": want["n_selected"], "in_view": want["n_in_view"], "flags": R.NOT_FINITE} and want["n_selected"] > 10000
    labels_in, on, obj, selected, colors, palette = _overlay_case(n)
    got = _overlay(labels_in, on, obj, selected, "paint", 7, colors, palette)
    want = R.overlay(labels_in, on, obj, selected, R.PAINT, 7, colors, palette)
    assert np.array_equal(got["on"], want["on"]) and np.array_equal(got["obj"], want["obj"]) and np.array_equal(got["labels"], want["labels"])
    assert np.array_equal(bits(got["colors"]), bits(want["colors"]))
    assert {k: got[k] for k in ("changed", "overridden", "differing", "err")} == {k: want[k] for k in ("changed", "overridden", "differing", "err")}
    assert want["changed"] > 100000


@pytest.mark.parametrize("name", ["sheet", "sheet at 50 m"])
def test_what_a_rendered_cloud_shows_is_selected(name):
    """On ``render_points``' image, an all-ones mask and slack 0: every vertex the id image shows AT THE PIXEL IT PROJECTS TO is
    selected, because its tt is the very t the image holds there (k_pick_ray's formula, the same pixel ray).  And the rule
    as a whole: bit for bit the restatement's, on a generic camera."""
    xyz, radius, eye, target, fov = cloud_scene(name)
    w, h = 37, 29
    cam = camera_of(eye, target, fov, (w, h))
    r = render(xyz, None, cam, radius)
    rows = V.camera_rows(cam)
    ones = np.ones((h, w), np.uint8)
    got, summary = _select(xyz, cam, ones, r["t"], 0.0, ())
    want = R.select(xyz, cam, rows, ones, r["t"], 0.0)
    assert np.array_equal(got, want["selected"]) and summary["selected"] == want["n_selected"] and summary["in_view"] == want["n_in_view"]
    v, u = np.nonzero(r["ids"] >= 0)
    shown = r["ids"][v, u]
    at_home = (want["u"][shown] == u) & (want["v"][shown] == v) & want["in_view"][shown]
    assert at_home.sum() > 50                                   # (discs span many pixels: most ids are shown away from home too)
    assert got[shown[at_home]].all()
    assert np.array_equal(bits(want["tt"][shown[at_home]]), bits(r["t"][v[at_home], u[at_home]]))     # why: the same bits
    # hidden vertices exist and slack 0 leaves them out; through mode takes everything in view
    through, s2 = _select(xyz, cam, ones, None, 0.0, ())
    assert s2["selected"] == s2["in_view"] == summary["in_view"] > summary["selected"]
    assert np.array_equal(through, want["in_view"].astype(np.uint8))


# ---------------------------------------------------------------------------------------------------- 3
def _overlay(labels_in, on, obj, selected, op, value, colors, palette, outputs=True):
    n = len(labels_in)
    on_d, obj_d = _dev(on, np.uint8), _dev(obj, np.int32)
    lab = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    col = torch.full((n, 3), -9.0, dtype=torch.float32, device=DEV)
    summary = torch.full((V.OVERLAY_SUMMARY.itemsize,), 0xAB, dtype=torch.uint8, device=DEV)
    sel = None if selected is None else _dev(selected, np.uint8)
    if outputs:
        out = V.session_overlay(_dev(labels_in, np.int32), on_d, obj_d, sel, op, value, _dev(colors, F32), _dev(palette, F32), lab, col, summary)
        assert out[0] is lab and out[1] is col
    else:
        out = V.session_overlay(_dev(labels_in, np.int32), on_d, obj_d, sel, op, value, summary=summary)
        assert out[0] is None and out[1] is None
    return dict(on=on_d.cpu().numpy(), obj=obj_d.cpu().numpy(), labels=lab.cpu().numpy(), colors=col.cpu().numpy(),
                **V.read_overlay_summary(summary.cpu().numpy()))


def _overlay_case(n, seed=0, bad=False):
    rng = np.random.default_rng(seed + n)
    palette = rng.uniform(0, 1, (6, 3)).astype(F32)             # entries 0..5: labels 6.. wrap over 1..5
    labels_in = rng.integers(0, 14, n).astype(np.int32)         # at and above n_palette
    on = (rng.uniform(size=n) < 0.3).astype(np.uint8) * rng.choice([1, 7, 255], n).astype(np.uint8)
    obj = np.where(on != 0, rng.integers(0, 12, n), 0).astype(np.int32)
    if bad and n > 70:
        labels_in[3], on[3] = 256, 0                            # the model's label is used: out of range
        labels_in[5], on[5], obj[5] = 256, 1, 2                 # ... is not used (only compared): fine
        obj[64], on[64] = 256, 1                                # the manual label is used: out of range
        obj[66], on[66] = 256, 0                                # ... is not used
        labels_in[67], on[67] = -1, 0
    selected = (rng.uniform(size=n) < 0.4).astype(np.uint8) * rng.choice([1, 3], n).astype(np.uint8)
    colors = rng.uniform(0, 1, (n, 3)).astype(F32)
    return labels_in, on, obj, selected, colors, palette


OPS = (("none", R.NONE), ("paint", R.PAINT), ("erase", R.ERASE))


@pytest.mark.parametrize("n", (0, 1, 64, 257, 3001))
def test_overlay_against_the_rule(n):
    labels_in, on, obj, selected, colors, palette = _overlay_case(n)
    for op, code in OPS:
        for sel in (selected, None):
            for value in (0, 4, 9, 255):
                got = _overlay(labels_in, on, obj, sel, op, value, colors, palette)
                want = R.overlay(labels_in, on, obj, sel, code, value, colors, palette)
                key = (op, sel is None, value)
                assert np.array_equal(got["on"], want["on"]) and np.array_equal(got["obj"], want["obj"]), key
                assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(bits(got["colors"]), bits(want["colors"])), key
                assert {k: got[k] for k in ("changed", "overridden", "differing", "err")} == \
                    {k: want[k] for k in ("changed", "overridden", "differing", "err")}, key
                if n == 3001 and sel is not None:
                    assert (want["changed"] > 100) == (op != "none") and want["err"] == 0
    if n == 3001:
        wrapped = R.overlay(labels_in, on, obj, selected, R.PAINT, 9, colors, palette)
        assert (wrapped["labels"] >= 6).sum() > 500             # the wrap is exercised: label 9 shows entry 1 + 8 % 5 = 4
        assert np.array_equal(wrapped["colors"][wrapped["labels"] == 9], np.broadcast_to(palette[4], ((wrapped["labels"] == 9).sum(), 3)))


def test_overlay_bad_labels_outputs_null_and_determinism():
    n = 300
    labels_in, on, obj, selected, colors, palette = _overlay_case(n, bad=True)
    selected[[3, 5, 64, 66, 67]] = 0
    for op, code in OPS:
        got = _overlay(labels_in, on, obj, selected, op, 2, colors, palette)
        want = R.overlay(labels_in, on, obj, selected, code, 2, colors, palette)
        assert want["err"] == 1 == got["err"] and (~want["written"]).nonzero()[0].tolist() == [3, 64, 67]
        w = want["written"]
        assert np.array_equal(got["labels"][w], want["labels"][w]) and np.array_equal(bits(got["colors"][w]), bits(want["colors"][w]))
        assert (got["labels"][~w] == -9).all() and (got["colors"][~w] == -9.0).all()       # left unwritten: the sentinels
        assert {k: got[k] for k in ("changed", "overridden", "differing")} == {k: want[k] for k in ("changed", "overridden", "differing")}
        # a pure layer update: the same layer and sums, nothing else written
        bare = _overlay(labels_in, on, obj, selected, op, 2, colors, palette, outputs=False)
        assert np.array_equal(bare["on"], want["on"]) and np.array_equal(bare["obj"], want["obj"])
        assert {k: bare[k] for k in ("changed", "overridden", "differing", "err")} == {k: got[k] for k in ("changed", "overridden", "differing", "err")}
        assert (bare["labels"] == -9).all()
        again = _overlay(labels_in, on, obj, selected, op, 2, colors, palette)
        for k in ("on", "obj", "labels", "colors"):
            assert got[k].tobytes() == again[k].tobytes(), (op, k)
    # painting 256 over a bad manual label heals it; the wrapper refuses what the library would
    healed = _overlay(labels_in, on, obj, np.ones(n, np.uint8), "paint", 1, colors, palette)
    assert healed["err"] == 0 and (healed["labels"] == 1).all() and healed["overridden"] == n
    x = _dev(labels_in, np.int32)
    o8, o32 = _dev(on, np.uint8), _dev(obj, np.int32)
    for bad in (lambda: V.session_overlay(x, o8, o32, op="fill"), lambda: V.session_overlay(x, o8, o32, op="paint", obj=256),
                lambda: V.session_overlay(x, o8[:-1], o32), lambda: V.session_overlay(x, o8, o32.to(torch.int64)),
                lambda: V.session_overlay(x, o8, o32, palette=_dev(palette, F32)),
                lambda: V.session_overlay(x, o8, o32, colors=_dev(colors, F32), palette=_dev(palette[:1], F32)),
                lambda: V.session_overlay(x, o8, o32, selected=o32)):
        with pytest.raises(ValueError):
            bad()
