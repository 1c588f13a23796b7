"""-m gpu: the annotation in the view (a3d_render_labels, a3d_render_annotate in csrc/session.hip; view.render_labels,
view.render_annotate, view.marker_table; InteractiveSession.label_image, object_at, annotate).

The rules are this library's and stated in include/agile3d_hip.h; the yardstick is their numpy float32 restatement in
``annotate_rule.py`` (which ``test_annotate_host.py`` checks on the CPU).  Every comparison is bit for bit.  The kernels are
per-pixel passes over images, so the images here are made up directly -- ids, weights, labels, depths -- at the three sizes
at which such a pass can go wrong: 1 x 1 (no neighbours), 16 x 16 (one workgroup), 37 x 29 (five workgroups of 256 pixels
whose rows are 37 wide: the up and down neighbours of a row's pixels lie in other workgroups).

1  the label image of a cloud and of a mesh: ids and face indices out of range, ties of the weights, NaN weights, m == 0
2  outlines: objects at the image's edge, side by side, background against nothing, outline = NULL
3  markers: 0, 1, 256 (257 is refused), d2 == radius^2, sub-pixel centres and centres outside the image, overlap, depth, NaN
4  in place; two calls, the same bytes; the library's refusals
5  the session on the committed mesh and on the small fixture cloud
"""
import os

import numpy as np
import pytest
import torch

import session_kit
from agile3d_amd import lib as L
from agile3d_amd import view as V
from annotate_rule import annotate_rule, labels_rule, marker_cover, outline_mask
from conftest import ROOT
from pick_rule import F32
from render_rule import quantise
from session_kit import CASES, DEV, _dev, f32_pointer, intrinsic, load_session_case, look_at, status

pytestmark = pytest.mark.gpu
SIZES = [(37, 29), (16, 16), (1, 1)]
NAN = np.nan


# ------------------------------------------------------------------------------------------- numpy in, numpy out
def labels_gpu(ids, u, v, faces, labels):
    """view.render_labels; the output starts as a sentinel."""
    mesh = faces is not None
    out = torch.full(ids.shape, -7, dtype=torch.int32, device=DEV)
    V.render_labels(_dev(ids, np.int32), _dev(u, F32) if mesh else None, _dev(v, F32) if mesh else None,
                    _dev(np.asarray(faces).reshape(-1, 3), np.int32) if mesh else None, _dev(labels, np.int32), out=out)
    return out.cpu().numpy()


def annotate_gpu(rgb, label, t, markers, radius, inner, slack, outline, border, in_place=False):
    """view.render_annotate; out of place the output starts as a sentinel, in place it is the input."""
    src = _dev(rgb, np.uint8)
    out = src if in_place else torch.full(rgb.shape, 77, dtype=torch.uint8, device=DEV)
    table = None if markers is None else _dev(np.asarray(markers, F32).reshape(-1, 6), F32)
    got = V.render_annotate(src, None if label is None else _dev(label, np.int32), _dev(t, F32), table, radius, inner, slack,
                            outline, border, out=out)
    assert got is out
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), rgb)                               # the input is left alone
    return out.cpu().numpy()


def _lead(image, values):
    """``image`` with its first pixels replaced by ``values`` (as many as fit)."""
    flat = image.reshape(-1)
    k = min(len(values), flat.size)
    flat[:k] = np.asarray(values, image.dtype)[:k]
    return image


# ------------------------------------------------------------------------------------------- 1: the label image
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_label_image_of_a_cloud(size):
    w, h = size
    rng = np.random.default_rng(w)
    n = 50
    labels = rng.integers(0, 6, n).astype(np.int32)
    labels[7] = -4                                                                   # (values pass through unchecked)
    ids = _lead(rng.integers(-3, n + 3, (h, w)).astype(np.int32), [7, -1, n, n - 1, 0, 1 << 30, -(1 << 31)])
    got = labels_gpu(ids, None, None, None, labels)
    assert np.array_equal(got, labels_rule(ids, None, None, None, labels))
    assert got.reshape(-1)[0] == -4 and (got[(ids < 0) | (ids >= n)] == -1).all()
    assert np.array_equal(labels_gpu(ids, None, None, None, labels), got)           # two calls, the same bytes


# (u, v) whose weights tie or are NaN: u == w -> corner 0, u == v above w -> corner 1, v == w above u -> corner 0, NaN -> 2
WEIGHTS = [(0.375, 0.25), (0.375, 0.375), (0.25, 0.375), (0.25, 0.25), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5),
           (NAN, 0.2), (0.2, NAN), (NAN, NAN), (np.inf, 0.1), (0.1, -np.inf)]
CORNERS = [0, 1, 0, 0, 0, 1, 2, 1, 2, 2, 2, 1, 0]


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_label_image_of_a_mesh(size):
    w, h = size
    rng = np.random.default_rng(10 + w)
    n, m = 40, 30
    labels = np.arange(100, 100 + n, dtype=np.int32)                                # every vertex its own label: the corner shows
    faces = np.stack([rng.permutation(n)[:3] for _ in range(m)]).astype(np.int32)
    faces[3], faces[4], faces[5], faces[6] = [-1, 2, 3], [1, n, 3], [1, 2, 1 << 30], [5, 5, 5]      # three bad faces, a repeated index
    ids = rng.integers(-2, m + 2, (h, w)).astype(np.int32)
    u = rng.uniform(0, 1, (h, w)).astype(F32)
    v = (rng.uniform(0, 1, (h, w)) * (1 - u)).astype(F32)
    k = len(WEIGHTS)
    if w * h > 1:                                                                    # the ties and NaNs on face 0, then the bad faces and ids
        _lead(ids, [0] * k + [3, 4, 5, 6, m, -1, m - 1])
        _lead(u, [a for a, _ in WEIGHTS])
        _lead(v, [b for _, b in WEIGHTS])
    got = labels_gpu(ids, u, v, faces, labels)
    assert np.array_equal(got, labels_rule(ids, u, v, faces, labels))
    if w * h > 1:
        flat = got.reshape(-1)
        assert flat[:k].tolist() == [100 + int(faces[0, c]) for c in CORNERS]
        assert flat[k:k + 6].tolist() == [-1, -1, -1, 105, -1, -1]
    assert np.array_equal(labels_gpu(ids, u, v, faces, labels), got)                # two calls, the same bytes
    # every tie and NaN on a single pixel as well: the 1 x 1 image
    for (a, b), c in zip(WEIGHTS, CORNERS):
        one = labels_gpu(np.zeros((1, 1), np.int32), F32([[a]]), F32([[b]]), faces, labels)
        assert one.tolist() == [[100 + int(faces[0, c])]], (a, b)
    # m == 0: no id is a face
    assert (labels_gpu(ids, u, v, np.zeros((0, 3), np.int32), labels) == -1).all()


# ------------------------------------------------------------------------------------------- 2, 3: outlines and markers
def _view(size, seed):
    """(rgb uint8 [h, w, 3], labels int32 [h, w] in patches of 4 x 4 with values -1 .. 2, t fp32 [h, w]: +inf where nothing)."""
    w, h = size
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    label = rng.integers(-1, 3, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w].astype(np.int32)
    t = np.where(label < 0, np.inf, rng.uniform(1.0, 5.0, (h, w))).astype(F32)
    return rgb, label, t


def _markers(size, k, seed):
    """k random rows: centres from 8 pixels outside the image to 8 outside, at sub-pixel positions; t around the surfaces'."""
    w, h = size
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-8, w + 8, (k, 1)), rng.uniform(-8, h + 8, (k, 1)), rng.uniform(0.5, 5.5, (k, 1)),
                           rng.uniform(-0.2, 1.2, (k, 3))], 1).astype(F32)


OUTLINE, BORDER = (0.1, 0.9, 0.3), (1.0, 0.5, 0.999)


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_outlines(size):
    w, h = size
    rgb, label, t = _view(size, 20 + w)
    if w >= 16:                                  # object 1 at the left and top edge beside object 2, background against nothing below
        label[:8, :8], label[:8, 8:16] = 1, 2
        label[8:12, :8], label[8:12, 8:16] = 0, -1
        t = np.where(label < 0, np.inf, np.where(np.isinf(t), 2.0, t)).astype(F32)
    else:
        label[...] = 2                           # 1 x 1: an object without a neighbour
    got = annotate_gpu(rgb, label, t, None, 5.0, 4.0, 0.1, OUTLINE, BORDER)
    assert np.array_equal(got, annotate_rule(rgb, label, t, None, 5.0, 4.0, 0.1, OUTLINE, BORDER))
    drawn = outline_mask(label)
    assert (got[drawn] == quantise(F32(OUTLINE))).all() and quantise(F32(OUTLINE)).tolist() == [26, 230, 77] and np.array_equal(got[~drawn], rgb[~drawn])
    if w >= 16:
        assert not drawn[0, :7].any() and not drawn[:7, 0].any()                    # the object ends at the image's edge: no outline there
        assert drawn[:8, 7].all() and drawn[:8, 8].all()                            # both sides of the border between two objects
        assert drawn[7, :8].all() and drawn[7, 8:16].all()                          # against the background, against nothing
        assert not drawn[8:12, :16].any()                                           # the background and nothing are never outlined
    else:
        assert not drawn.any()
    # outline = NULL: the image comes back, with and without a label image
    assert np.array_equal(annotate_gpu(rgb, label, t, None, 5.0, 4.0, 0.1, None, BORDER), rgb)
    assert np.array_equal(annotate_gpu(rgb, None, t, None, 5.0, 4.0, 0.1, None, BORDER), rgb)


@pytest.mark.parametrize("k", [0, 1, 256])
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_markers(size, k):
    """Random tables over random views, with and without outlines, out of place and in place, twice."""
    rgb, label, t = _view(size, 30 + size[0])
    markers = _markers(size, k, 40 + k)
    if k == 256:
        markers[5, 0], markers[17, 2], markers[200, 4] = NAN, NAN, NAN              # rows with a NaN cover nothing
    args = (5.5, 4.0, 0.25)
    want = annotate_rule(rgb, label, t, markers, *args, OUTLINE, BORDER)
    got = annotate_gpu(rgb, label, t, markers, *args, OUTLINE, BORDER)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:10]
    assert np.array_equal(annotate_gpu(rgb, label, t, markers, *args, OUTLINE, BORDER), got)              # two calls, the same bytes
    assert np.array_equal(annotate_gpu(rgb, label, t, markers, *args, OUTLINE, BORDER, in_place=True), got)
    plain = annotate_gpu(rgb, None, t, markers, *args, None, BORDER)
    assert np.array_equal(plain, annotate_rule(rgb, None, t, markers, *args, None, BORDER))
    if k == 0:
        assert np.array_equal(plain, rgb)
    if k == 256 and size[0] > 1:
        hit = marker_cover(t, markers, *args)[0]
        assert (hit >= 0).mean() > 0.5 and not np.isin(hit, [5, 17, 200]).any() and (plain != rgb).any()


def test_marker_edges():
    """One view of 37 x 29, depth 2 on the left, 3 in the middle, nothing on the right; markers placed by hand."""
    w, h = 37, 29
    rgb = np.full((h, w, 3), 128, np.uint8)
    t = np.full((h, w), 2.0, F32)
    t[:, 12:24], t[:, 24:] = 3.0, np.inf
    red, green, blue = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    white = np.array([255, 255, 255], np.uint8)

    def run(rows, radius=5.0, inner=3.0, slack=0.1):
        got = annotate_gpu(rgb, None, t, F32(rows), radius, inner, slack, None, (1.0, 1.0, 1.0))
        assert np.array_equal(got, annotate_rule(rgb, None, t, F32(rows), radius, inner, slack, None, (1.0, 1.0, 1.0)))
        return got

    # d2 == radius^2 exactly (3, 4, 5) and d2 == inner^2 exactly: both inside
    got = run([(10, 10, 2.0) + red])
    assert (got[14, 13] == white).all() and (got[15, 13] == 128).all() and (got[6, 7] == white).all()
    assert got[10, 13].tolist() == [255, 0, 0] and (got[10, 14] == white).all() and (got[10, 16] == 128).all()
    # the centre between pixels: (10.5, 10.5) is 0.5^2 + 0.5^2 from four pixels and reaches none with a radius of 0.7
    got = run([(10.5, 10.5, 2.0) + red], radius=0.75, inner=0.75)
    assert (got[10:12, 10:12] == np.array([255, 0, 0], np.uint8)).all() and ((got != 128).any(-1)).sum() == 4
    assert np.array_equal(run([(10.5, 10.5, 2.0) + red], radius=0.7, inner=0.0), rgb)
    # a radius and an inner radius of 0: the one pixel at the centre, in the marker's colour
    got = run([(4, 20, 2.0) + green], radius=0.0, inner=0.0)
    assert got[20, 4].tolist() == [0, 255, 0] and ((got != 128).any(-1)).sum() == 1
    # centres outside the image reach in
    got = run([(-3, 5, 2.0) + red, (40, 30, 9.0) + blue])
    assert (got[5, 2] == white).all() and (got[5, 3] == 128).all() and (got[28, 36] == white).all()
    # two overlapping markers: the later wins, also with its rim over the earlier one's core
    got = run([(6, 22, 2.0) + red, (10, 22, 2.0) + green])
    assert got[22, 10].tolist() == [0, 255, 0] and got[22, 4].tolist() == [255, 0, 0] and (got[22, 6] == white).all()
    got = run([(10, 22, 2.0) + green, (6, 22, 2.0) + red])
    assert got[22, 6].tolist() == [255, 0, 0] and (got[22, 10] == white).all() and got[22, 12].tolist() == [0, 255, 0]
    # hidden behind a nearer surface: at t = 3 it shows on the middle surface and over nothing, not on the left one at t = 2 ...
    got = run([(12, 8, 3.0) + blue])
    assert (got[:, :12] == 128).all() and got[8, 12].tolist() == [0, 0, 255] and (got[8, 16] == white).all()
    # ... just inside the slack it shows on both; just outside on neither side of it
    near = run([(12, 8, 2.0 + 0.0999) + blue])
    assert near[8, 11].tolist() == [0, 0, 255] and near[8, 12].tolist() == [0, 0, 255]
    assert (run([(12, 8, 2.0 + 0.1001) + blue])[:, :12] == 128).all()
    assert np.array_equal(run([(12, 8, 3.2) + blue])[:, :24], rgb[:, :24])
    # over pixels that show nothing every marker shows, however far away
    got = run([(30, 14, 1e30) + green])
    assert got[14, 30].tolist() == [0, 255, 0] and ((got != 128).any(-1)).sum() == 81                      # the disc of radius 5
    # a NaN anywhere in a row: nothing; an infinite position: nothing
    for at in range(6):
        row = [30.0, 14.0, 2.0, 0.0, 1.0, 0.0]
        row[at] = NAN
        assert np.array_equal(run([row, (-50, -50, 1.0) + red]), rgb), at
    assert np.array_equal(run([(np.inf, 14, 2.0) + red, (30, -np.inf, 2.0) + red]), rgb)
    # colours outside [0, 1] are clamped
    assert run([(30, 14, 2.0, -0.5, 1.5, 0.5)], inner=5.0)[14, 30].tolist() == [0, 255, 128]


def test_annotate_refusals():
    rgb, label, t = _view((16, 16), 3)
    with pytest.raises(L.A3DError):
        annotate_gpu(rgb, label, t, _markers((16, 16), 257, 1), 5.0, 4.0, 0.1, OUTLINE, BORDER)
    a, lab, tt, out = _dev(rgb, np.uint8), _dev(label, np.int32), _dev(t, F32), torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV)
    big = torch.zeros(3 * 16 * 16 + 30, dtype=torch.uint8, device=DEV)
    mk = _dev(_markers((16, 16), 257, 1), F32)
    col = f32_pointer([0.0, 0.0, 0.0])
    call = lambda *args: status("a3d_render_annotate", *args)                                   # the entry point as it is
    ok = [a.data_ptr(), lab.data_ptr(), tt.data_ptr(), mk.data_ptr(), 256, 5.0, 4.0, 0.1, col, col, out.data_ptr(), 16, 16, None]
    assert call(*ok) == 0
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (4, 257), (4, -1), (5, 3.0), (5, NAN), (5, np.inf), (6, -1.0),
                    (6, NAN), (7, -0.1), (7, NAN), (7, np.inf), (9, None), (10, None), (11, 0), (12, 0), (11, 4097)):
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)                                                     # A3D_ERR_INVALID
    # in place is allowed, a partial overlap is not
    assert call(*(ok[:10] + [a.data_ptr()] + ok[11:])) == 0
    assert call(*([big.data_ptr()] + ok[1:10] + [big.data_ptr() + 30] + ok[11:])) == -1
    # without outlines no label image is needed; without markers no table
    assert call(*(ok[:1] + [None, tt.data_ptr(), None, 0] + ok[5:8] + [None] + ok[9:])) == 0
    lcall = lambda *args: status("a3d_render_labels", *args)
    ids, labels = _dev(np.zeros((16, 16)), np.int32), _dev(np.zeros(5), np.int32)
    lok = [ids.data_ptr(), None, None, None, 0, labels.data_ptr(), 5, lab.data_ptr(), 16, 16, None]
    assert lcall(*lok) == 0
    for at, bad in ((0, None), (3, ids.data_ptr()), (4, -1), (5, None), (6, -1), (7, None), (8, 0), (9, 4097)):
        args = list(lok)
        args[at] = bad
        assert lcall(*args) == -1, (at, bad)
    with pytest.raises(ValueError):
        V.render_labels(ids, None, None, None, labels.to(torch.int64))
    with pytest.raises(ValueError):
        V.render_annotate(a, lab[:8], tt, None, 5.0, 4.0, 0.1, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        V.render_annotate(a, None, tt, None, 5.0, 4.0, 0.1, (0, 0, 0), (1, 1, 1))      # outlines need the label image


# ------------------------------------------------------------------------------------------- 5: the session
@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def _want_annotate(ses, res, labels_full, faces, **kw):
    """What ``ses.annotate(res, ...)`` must return, from the restatement fed with ``marker_table``."""
    ids = res.ids.cpu().numpy()
    u, v = (None, None) if faces is None else (res.u.cpu().numpy(), res.v.cpu().numpy())
    label = labels_rule(ids, u, v, faces, labels_full)
    cubes = ses._cubes[:ses.num_clicks]
    table = V.marker_table(res.camera, cubes[:, :3], cubes[:, 3:]) if kw.get("markers", True) else None
    px, rim = kw.get("marker_px", 6.0), kw.get("marker_border_px", 1.5)
    outline = kw.get("outline_color", (0.0, 0.0, 0.0)) if kw.get("outlines", True) else None
    return label, table, annotate_rule(res.rgb.cpu().numpy(), label, res.t.cpu().numpy(), table, px, px - rim,
                                       kw.get("depth_slack", ses.cube_size), outline, kw.get("marker_border_color", (1.0, 1.0, 1.0)))


def test_session_annotate_on_the_committed_mesh(model_005):
    """tests/golden/data/mesh_small.ply has 40 vertices and faces metres wide: a click in the middle of a face has no vertex in
    its cube, so ``preview`` paints nothing for it -- and ``annotate`` shows it."""
    from agile3d_amd.ply import read_ply
    from agile3d_amd.session import InteractiveSession
    vert, faces = read_ply(os.path.join(ROOT, "tests", "golden", "data", "mesh_small.ply"), triangular_mesh=True)
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(F32)
    col = np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(F32) / 255
    faces = np.asarray(faces, np.int32)
    ses = InteractiveSession(model_005, voxel_size=0.05)
    ses.load_scene(xyz, col, faces=faces)
    k, e = ses.default_view(64, 48)
    res = ses.render(k, e, 64, 48)
    ids, t = res.ids.cpu().numpy(), res.t.cpu().numpy()
    shows = ids >= 0
    assert shows.sum() >= 200 and (~shows).any()
    # before any inference: background where the mesh shows, nothing elsewhere; nothing to draw
    assert np.array_equal(ses.label_image(res).cpu().numpy(), np.where(shows, 0, -1))
    assert torch.equal(ses.annotate(res), res.rgb)
    # two pixels, 16 apart or more, whose surface points lie far (Chebyshev, as the cubes measure) from every vertex
    u, v = res.u.cpu().numpy(), res.v.cpu().numpy()
    f = faces[np.maximum(ids, 0)]
    uu, vv, ww = u[..., None], v[..., None], ((F32(1.0) - u) - v)[..., None]
    points = (ww * xyz[f[..., 0]] + uu * xyz[f[..., 1]]) + vv * xyz[f[..., 2]]                  # pick_from_render's arithmetic
    away = np.where(shows, np.abs(points[:, :, None, :] - xyz[None, None]).max(-1).min(-1), -1.0)
    clicks = []
    for _ in range(2):
        j, i = (int(a) for a in np.unravel_index(away.argmax(), away.shape))
        assert away[j, i] > 2 * ses.cube_size
        p = ses.pick_from_render(res, i, j)
        assert np.array_equal(F32(p), points[j, i])
        clicks.append((i, j, p))
        jj, ii = np.mgrid[:48, :64]
        away[np.hypot(ii - i, jj - j) < 16] = -1.0
    for obj, (i, j, p) in enumerate(clicks, 1):
        ses.click(p, obj)
    # THE case: the clicks steer the model, preview's colours show nothing of them, annotate does
    _, colours = ses.preview()
    assert torch.equal(colours, ses.colors_full) and torch.equal(ses.render(k, e, 64, 48).rgb, res.rgb)
    shown = ses.annotate(res)
    label, table, want = _want_annotate(ses, res, np.zeros(len(xyz), np.int32), faces)
    assert table.shape == (2, 6) and np.array_equal(shown.cpu().numpy(), want)
    assert shown.data_ptr() != res.rgb.data_ptr() and np.array_equal(res.rgb.cpu().numpy(), ses.render(k, e, 64, 48).rgb.cpu().numpy())
    changed = (shown != res.rgb).any(-1).cpu().numpy()
    for obj, (i, j, p) in enumerate(clicks, 1):
        assert changed[j, i] and np.array_equal(shown[j, i].cpu().numpy(), quantise(ses.palette[obj]))
        assert abs(table[obj - 1, 0] - i) < 1e-2 and abs(table[obj - 1, 1] - j) < 1e-2 and abs(table[obj - 1, 2] - t[j, i]) < 1e-3
    # an inference with made-up logits: object 1 left of the first click's x ... object 2 right of it, background high up
    qv = ses.raw_coords_qv.cpu().numpy()
    logits = np.zeros((len(qv), 3), F32)
    logits[:, 1], logits[:, 2] = qv[:, 0] < 0.0, qv[:, 0] >= 0.0
    logits[:, 0] = 2.0 * (qv[:, 2] > 1.0)
    out = ses.infer(logits=torch.from_numpy(logits).to(DEV))
    labels_full = out.labels_full.cpu().numpy()
    assert set(np.unique(labels_full)) == {0, 1, 2}
    after = ses.render(k, e, 64, 48, lit=True)
    label, table, want = _want_annotate(ses, after, labels_full, faces)
    assert np.array_equal(ses.label_image(after).cpu().numpy(), label) and set(np.unique(label)) == {-1, 0, 1, 2}
    assert np.array_equal(ses.annotate(after).cpu().numpy(), want) and outline_mask(label).sum() >= 20
    for i, j in [(0, 0), (63, 47), clicks[0][:2], clicks[1][:2]] + [(i, j) for i in range(16, 56, 6) for j in range(12, 44, 9)]:
        assert ses.object_at(after, i, j) == (None if label[j, i] < 0 else int(label[j, i])), (i, j)
    # labels of the caller's, other settings
    mine = np.where(np.arange(len(xyz)) % 2 == 0, 3, 0).astype(np.int32)
    kw = dict(outline_color=(1.0, 0.0, 0.5), marker_px=3.0, marker_border_px=0.0, marker_border_color=(0.0, 0.0, 0.0), depth_slack=0.0)
    label, table, want = _want_annotate(ses, after, mine, faces, **kw)
    assert np.array_equal(ses.annotate(after, labels=_dev(mine, np.int32), **kw).cpu().numpy(), want)
    assert np.array_equal(ses.label_image(after, labels=_dev(mine, np.int32)).cpu().numpy(), label)
    assert ses.object_at(after, clicks[0][0], clicks[0][1], labels=_dev(mine, np.int32)) == int(label[clicks[0][1], clicks[0][0]])
    assert np.array_equal(ses.annotate(after, outlines=False, markers=False).cpu().numpy(), after.rgb.cpu().numpy())
    assert np.array_equal(ses.annotate(after, markers=False).cpu().numpy(), _want_annotate(ses, after, labels_full, faces, markers=False)[2])
    # errors, as the session reports them
    for bad in (dict(marker_px=-1.0), dict(marker_px=2.0, marker_border_px=3.0), dict(marker_border_px=-0.5), dict(marker_px=NAN),
                dict(depth_slack=-1.0), dict(depth_slack=np.inf), dict(outline_color=(0.0, NAN, 0.0)), dict(marker_border_color=(1.0, 1.0)),
                dict(labels=_dev(mine[:-1], np.int32)), dict(labels=mine)):
        with pytest.raises(ValueError):
            ses.annotate(after, **bad)
    with pytest.raises(ValueError):
        ses.object_at(after, 64, 0)
    with pytest.raises(ValueError):
        ses.object_at(after, 0, -1)
    # reset(): the labels are background again and the markers gone
    ses.reset()
    assert np.array_equal(ses.label_image(after).cpu().numpy(), np.where(shows, 0, -1))
    assert torch.equal(ses.annotate(after), after.rgb) and ses.object_at(after, clicks[0][0], clicks[0][1]) == 0
    # a render of a mesh belongs to a mesh
    ses.load_scene(xyz, col)
    for call in (ses.label_image, ses.annotate, lambda r: ses.object_at(r, 0, 0)):
        with pytest.raises(ValueError):
            call(after)
    ses._drop_scene()
    with pytest.raises(RuntimeError):
        ses.label_image(after)


def test_session_annotate_on_the_fixture_cloud(model_005):
    """The small fixture scene, its scripted clicks and recorded logits: a pixel shows the label of its vertex."""
    from agile3d_amd.session import InteractiveSession
    c, meta = load_session_case(CASES[0])
    ses = InteractiveSession(model_005, voxel_size=meta["voxel_size"], palette=c["palette"],
                             background_click_color=c["background_click_color"])
    ses.load_scene(c["coords_full"], c["colors_full"], c["labels_full"], name=meta["name"])
    xyz = c["coords_full"].astype(F32)
    centre, extent = xyz.mean(0).astype(np.float64), float(np.ptp(xyz, axis=0).max())
    k, e, w, h = intrinsic(80, 60, 60.0), look_at(centre + [0.2 * extent, -1.1 * extent, 0.6 * extent], centre), 80, 60
    step = meta["steps"][1]
    for p, o in zip(c["click_points"][:step["num_clicks"]], c["click_objs"][:step["num_clicks"]]):
        ses.click(p, int(o))
    # between the clicks and the inference: preview's labels (background) and its cubes, the markers on top
    labels0, _ = ses.preview()
    res = ses.render(k, e, w, h, background=(0.0, 0.25, 1.0))
    ids = res.ids.cpu().numpy()
    assert (ids >= 0).sum() >= 300 and (ids < 0).any() and not labels0.any()
    label, table, want = _want_annotate(ses, res, np.zeros(len(xyz), np.int32), None)
    assert len(table) == step["num_clicks"] == 6 and np.array_equal(ses.annotate(res).cpu().numpy(), want)
    assert (want != res.rgb.cpu().numpy()).any()
    out = ses.infer(logits=torch.from_numpy(c["step1_logits"]).to(DEV))
    labels_full = out.labels_full.cpu().numpy()
    assert np.array_equal(labels_full, c["step1_mask"])
    res = ses.render(k, e, w, h, background=(0.0, 0.25, 1.0))
    label, table, want = _want_annotate(ses, res, labels_full, None)
    assert np.array_equal(label, np.where(ids >= 0, labels_full[np.maximum(ids, 0)], -1))
    assert np.array_equal(ses.label_image(res).cpu().numpy(), label) and len(np.unique(label)) >= 4
    assert np.array_equal(ses.annotate(res).cpu().numpy(), want) and outline_mask(label).sum() >= 20
    rng = np.random.default_rng(0)
    for i, j in zip(rng.integers(0, w, 12).tolist(), rng.integers(0, h, 12).tolist()):
        assert ses.object_at(res, i, j) == (None if ids[j, i] < 0 else int(labels_full[ids[j, i]])), (i, j)
    ses.reset()
    assert not ses.label_image(res).cpu().numpy()[ids >= 0].any() and torch.equal(ses.annotate(res), res.rgb)
