"""-m gpu: correcting a labelling by hand through the session (InteractiveSession.region_mask, select, paint, erase, corrected,
manual_labels, set_manual).  The rules are restated in ``region_rule.py``; logits are replayed through ``infer(logits=...)``.

1  select on a rendered view, a cloud and a mesh, against the rule; masks from region_mask and from label_image
2  paint, corrected, erase: the object's id and palette colour on exactly the selected vertices, the model's labels elsewhere
3  painting an object's ground-truth region does not lower the mean IoU
4  the layer follows the click list: remove_click, undo and redo renumber the paint; reset and load_scene clear it
5  set_manual(*manual_labels()) is the identity; an empty layer leaves preview()'s labels
"""
import numpy as np
import pytest
import torch

import region_rule as R
from agile3d_amd import view as V
from agile3d_amd.synthetic import make_scene
from session_kit import DEV, _model, bits, intrinsic, jittered_grid, look_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


def _session(model, xyz, col, lab=None, faces=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=0.02).load_scene(xyz, col, lab, faces=faces)


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene at full resolution: every voxel's point plus a second vertex 4 mm beside it, shuffled
    (as test_gpu_session_pieces.py builds its scene)."""
    sc = make_scene(5_000, seed=6, voxel_size=0.02)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def annotated(ses, scene, wrong=0.15):
    """Three objects and the background clicked, then logits replayed whose arg-max is the ground truth folded onto the objects
    0..3 with a share ``wrong`` of the voxels relabelled at random: a labelling that is nearly right.  Returns infer()'s result."""
    xyz, _, lab = scene
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:3]
    for k, i in enumerate(inst):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    ori = ses.labels_qv_ori.cpu().numpy()
    want = np.zeros(len(ori), np.int64)
    for k, i in enumerate(inst):
        want[ori == i] = k + 1
    rng = np.random.default_rng(1)
    flip = rng.uniform(size=len(ori)) < wrong
    want[flip] = rng.integers(0, 4, int(flip.sum()))
    logits = np.full((len(ori), 4), -2.0, np.float32)
    logits[np.arange(len(ori)), want] = 3.0
    return ses.infer(logits=torch.from_numpy(logits).to(DEV))


def planes_of(section):
    return np.zeros((0, 4), np.float32) if section is None else np.concatenate([section.normals, section.offsets[:, None]], 1)


def rule_select(ses, view, mask, through, slack, section):
    return R.select(ses.coords_full.cpu().numpy(), view.camera, V.camera_rows(view.camera), mask.cpu().numpy(),
                    None if through else view.t.cpu().numpy(), slack, planes_of(section))


def check_select(ses, view, mask, want_section, **kw):
    got = ses.select(view, mask, **kw)
    through, slack = bool(kw.get("through", False)), kw.get("slack", ses.voxel_size)
    want = rule_select(ses, view, mask, through, slack, want_section)
    assert got.selected.dtype == torch.uint8 and np.array_equal(got.selected.cpu().numpy(), want["selected"]), kw
    assert (got.count, got.in_view, got.through, got.slack) == (want["n_selected"], want["n_in_view"], through, slack), kw
    return got


# ---------------------------------------------------------------------------------------------------- 1
def test_select_on_a_cloud(model_002, scene):
    from agile3d_amd.session import Section
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    annotated(ses, scene)
    w, h = 96, 72
    k, e = ses.default_view(w, h)
    view = ses.render(k, e, w, h, radius=0.03)
    lasso = [(10.5, 8.0), (80.0, 5.5), (90.0, 60.0), (48.0, 30.0), (20.0, 66.0)]
    mask = ses.region_mask(view, polygon=lasso)
    assert np.array_equal(mask.cpu().numpy(), R.region_mask(R.POLYGON, lasso, w, h))
    brush = [(5.0, 70.0), (30.0, 40.0), (60.0, 50.0)]
    assert ses.region_mask(view, stroke=brush, radius=4.0, mask=mask, mode="add") is mask
    want_mask = R.region_mask(R.STROKE, brush, w, h, 4.0, R.ADD, R.region_mask(R.POLYGON, lasso, w, h))
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    before = (ses.clicks(), ses._labels_qv.clone(), ses._labels_last.clone())
    seen = check_select(ses, view, mask, None)                  # visible, slack = the voxel size
    front = check_select(ses, view, mask, None, slack=0.0)
    every = check_select(ses, view, mask, None, through=True)
    assert 0 < front.count <= seen.count <= every.count < every.in_view <= len(xyz)
    assert seen.count < every.count                             # the scan has a far side: through takes more than the eye sees
    # a section given, and the default: the one the view was rendered under
    centre = ses.coords_full.mean(0).cpu().numpy()
    cut = Section([((1.0, 0.2, 0.0), centre)])
    halved = check_select(ses, view, mask, cut, through=True, section=cut)
    assert 0 < halved.in_view < every.in_view
    cut_view = ses.render(k, e, w, h, radius=0.03, section=cut)
    assert check_select(ses, cut_view, mask, cut, through=True).in_view == halved.in_view
    assert check_select(ses, cut_view, mask, None, through=True, section=None).in_view == every.in_view
    # any image of that shape is a mask: what shows as object 2
    shows_2 = ses.label_image(view) == 2
    picked = check_select(ses, view, shows_2, None)
    assert shows_2.dtype == torch.bool and picked.count > 0
    # nothing of the session changed
    assert ses.clicks() == before[0] and torch.equal(ses._labels_qv, before[1]) and torch.equal(ses._labels_last, before[2])
    assert ses._manual is None
    for bad in (lambda: ses.region_mask(view), lambda: ses.region_mask(view, polygon=lasso, stroke=brush, radius=1.0),
                lambda: ses.select(view, mask[:-1]), lambda: ses.select(view, mask, slack=-1.0)):
        with pytest.raises(ValueError):
            bad()


def test_select_on_a_mesh(model_002):
    xyz, faces = jittered_grid(20, 20, seed=3)
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32), faces=faces)
    w, h = 64, 48
    view = ses.render(intrinsic(w, h), look_at([0.95, 0.95, 2.0], [0.95, 0.95, 0.0], up=(0.0, 1.0, 0.0)), w, h)     # from above
    mask = ses.region_mask(view, polygon=[(8, 6), (56, 4), (50, 44), (12, 40)])
    seen = check_select(ses, view, mask, None)
    every = check_select(ses, view, mask, None, through=True)
    assert 0 < seen.count <= every.count <= every.in_view <= len(xyz)
    other = _session(model_002, xyz[:100], np.full((100, 3), 0.5, np.float32))             # a cloud: another scene
    with pytest.raises(ValueError):
        other.select(view, mask)
    with pytest.raises(ValueError):
        other.paint(seen, 0)                                    # a selection of another scene's length


# ---------------------------------------------------------------------------------------------------- 2
def test_paint_corrected_erase(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    res = annotated(ses, scene)
    model = res.labels_full.cpu().numpy()
    w, h = 96, 72
    k, e = ses.default_view(w, h)
    view = ses.render(k, e, w, h, radius=0.03)
    sel = ses.select(view, ses.region_mask(view, polygon=[(20, 10), (70, 12), (75, 60), (30, 55)]), through=True)
    s = sel.selected.cpu().numpy() != 0
    assert 100 < s.sum() < len(xyz) and len(set(model[s])) > 1
    assert ses.paint(sel, 2) == s.sum()
    r = ses.corrected()
    want = np.where(s, 2, model)
    assert np.array_equal(r.labels_full.cpu().numpy(), want)
    colors = r.colors.cpu().numpy()
    assert np.array_equal(bits(colors[want > 0]), bits(ses.palette[want[want > 0]])) and np.array_equal(bits(colors[want == 0]), bits(col[want == 0]))
    assert (r.overridden, r.differing) == (s.sum(), (s & (model != 2)).sum())
    gt = ses.new_labels.cpu().numpy()
    ious = [((want == j) & (gt == j)).sum() / max(((want == j) | (gt == j)).sum(), 1) for j in (1, 2, 3)]
    assert abs(r.miou - np.mean(ious)) < 1e-6 and set(r.iou_per_object) == {1, 2, 3}
    assert ses.paint(sel, 2) == 0                               # already so: nothing changes
    assert ses.paint(sel.selected, 0) == s.sum()                # a plain tensor; the background is an object like any other
    assert np.array_equal(ses.corrected().labels_full.cpu().numpy(), np.where(s, 0, model))
    # the model's labels and the view's state are the session's own: paint touched neither
    assert torch.equal(ses._labels_last, res.labels_full) and np.array_equal(ses.preview(paint_cubes=False)[0].cpu().numpy(), model)
    # the result shows through the existing calls
    ses.paint(sel, 3)
    r = ses.corrected()
    shown = ses.render(k, e, w, h, colors=r.colors, radius=0.03)
    ses.annotate(shown, labels=r.labels_full)
    assert ses.measure(labels=r.labels_full, oriented=False).vertices[3] == (np.where(s, 3, model) == 3).sum()
    # erase: half of it, then all of it
    half = sel.selected.clone()
    half[len(half) // 2:] = 0
    n_half = int(half.sum().cpu())
    assert ses.erase(half) == n_half and ses.corrected().overridden == s.sum() - n_half
    assert ses.erase(sel) == s.sum() - n_half and ses.erase(sel) == 0
    r = ses.corrected()
    assert np.array_equal(r.labels_full.cpu().numpy(), model) and (r.overridden, r.differing) == (0, 0)
    assert abs(r.miou - res.miou) < 1e-6
    for bad in (lambda: ses.paint(sel, 4), lambda: ses.paint(sel, -1), lambda: ses.paint(sel.selected[:-1], 1),
                lambda: ses.paint(sel.selected.to(torch.int32), 1), lambda: ses.erase(sel.selected.cpu())):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------- 3
def test_painting_the_truth_does_not_lower_the_iou(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    res = annotated(ses, scene, wrong=0.3)
    assert res.miou < 0.9
    last = res.miou
    for obj in (2, 1, 3):
        region = ses.new_labels == obj                          # the ground-truth region of the object, as a bool tensor
        assert ses.paint(region, obj) > 0
        r = ses.corrected()
        assert r.miou >= last and r.iou_per_object[obj] > res.iou_per_object[obj]
        last = r.miou
    assert last > res.miou
    # without ground truth there is no IoU
    bare = _session(model_002, xyz, col)
    bare.click(xyz[0], 1)
    r = bare.corrected()
    assert r.miou is None and r.iou_per_object is None and (r.overridden, r.differing) == (0, 0)


# ---------------------------------------------------------------------------------------------------- 4
def test_the_layer_follows_the_click_list(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    annotated(ses, scene)                                       # clicks 0, 1, 2: objects 1, 2, 3; click 3: the background
    n = len(xyz)
    rng = np.random.default_rng(2)
    part = rng.integers(0, 5, n)                                # 0: not painted; 1..3: painted as that object; 4: painted background
    for obj, value in ((1, 1), (2, 2), (3, 3), (0, 4)):
        ses.paint(torch.from_numpy(part == value).to(DEV), obj)
    on, obj = (t.cpu().numpy() for t in ses.manual_labels())
    assert np.array_equal(on, (part > 0).astype(np.uint8)) and np.array_equal(obj, np.where(part == 4, 0, part))
    removed = ses.remove_click(1)                               # the only click of object 2: it is gone, object 3 becomes 2
    assert removed["id_map"] == {1: 1, 2: 0, 3: 2}
    lut = np.array([0, 1, 0, 2, 0])
    on2, obj2 = (t.cpu().numpy() for t in ses.manual_labels())
    assert np.array_equal(on2, on) and np.array_equal(obj2, lut[part])          # the paint of 2 is background now, still painted
    model = ses.preview(paint_cubes=False)[0].cpu().numpy()
    r = ses.corrected()
    assert np.array_equal(r.labels_full.cpu().numpy(), np.where(part > 0, lut[part], model)) and r.overridden == (part > 0).sum()
    with pytest.raises(ValueError):
        ses.paint(torch.from_numpy(part == 1).to(DEV), 3)       # there is no object 3 any more
    # undo takes the background click back (no renumbering), then the only click of the present object 2
    assert ses.undo()["obj"] == 0
    assert np.array_equal(ses.manual_labels()[1].cpu().numpy(), lut[part])
    assert ses.undo()["id_map"] == {1: 1, 2: 0}
    assert np.array_equal(ses.manual_labels()[1].cpu().numpy(), np.where(part == 1, 1, 0))
    ses.redo()                                                  # the object is back under its id; its paint is not, like its labels
    assert np.array_equal(ses.manual_labels()[1].cpu().numpy(), np.where(part == 1, 1, 0))
    assert len(ses.click_idx) - 1 == 2 and ses.paint(torch.from_numpy(part == 3).to(DEV), 2) == (part == 3).sum()
    # reset and a second load_scene clear the layer
    ses.reset()
    assert ses._manual is None and not ses.manual_labels()[0].any() and ses.corrected().overridden == 0
    ses.click(xyz[0], 1)
    ses.paint(torch.ones(n, dtype=torch.bool, device=DEV), 1)
    assert ses.corrected().overridden == n
    ses.load_scene(xyz[:500], col[:500], lab[:500])
    assert ses._manual is None and tuple(ses.manual_labels()[0].shape) == (500,) and ses.corrected().overridden == 0


# ---------------------------------------------------------------------------------------------------- 5
def test_set_manual_and_the_empty_layer(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    n = len(xyz)
    # an empty layer: corrected() is preview(), byte for byte -- before the first inference and after it
    assert np.array_equal(ses.corrected().labels_full.cpu().numpy(), ses.preview()[0].cpu().numpy())
    res = annotated(ses, scene)
    first = ses.corrected()
    assert first.labels_full.cpu().numpy().tobytes() == ses.preview()[0].cpu().numpy().tobytes() and first.overridden == 0
    assert abs(first.miou - res.miou) < 1e-6
    rng = np.random.default_rng(4)
    ses.paint(torch.from_numpy(rng.uniform(size=n) < 0.2).to(DEV), 1)
    ses.paint(torch.from_numpy(rng.uniform(size=n) < 0.1).to(DEV), 3)
    ses.erase(torch.from_numpy(rng.uniform(size=n) < 0.05).to(DEV))
    before = ses.corrected()
    saved = ses.manual_labels()
    assert saved[0].dtype == torch.uint8 and saved[1].dtype == torch.int32 and 0 < before.overridden < n
    saved[0][:] = 0                                             # copies: changing them changes nothing
    assert ses.corrected().overridden == before.overridden
    saved = ses.manual_labels()
    ses.set_manual(*saved)
    for a, b in zip(ses.manual_labels(), saved):
        assert torch.equal(a, b)
    after = ses.corrected()
    assert torch.equal(after.labels_full, before.labels_full) and torch.equal(after.colors, before.colors)
    assert (after.overridden, after.differing, after.miou) == (before.overridden, before.differing, before.miou)
    # carried over a reset, as a caller's own history would
    ses.reset()
    ses.set_manual(saved[0] != 0, saved[1])                     # (on as bool)
    assert ses.corrected().overridden == before.overridden
    # obj is looked at where on is set, and only there
    on, obj = saved[0].clone(), saved[1].clone()
    off = int((on == 0).nonzero()[0])
    obj[off] = 256
    ses.set_manual(on, obj)
    assert int(ses.manual_labels()[1][off]) == 0
    held = int((on != 0).nonzero()[0])
    obj[held] = 256
    with pytest.raises(ValueError):
        ses.set_manual(on, obj)
    assert torch.equal(ses.manual_labels()[0], saved[0]) and int(ses.manual_labels()[1][held]) == int(saved[1][held])
    for bad in (lambda: ses.set_manual(on[:-1], obj[:-1]), lambda: ses.set_manual(on, obj.to(torch.int64)), lambda: ses.set_manual(on.cpu(), obj.cpu())):
        with pytest.raises(ValueError):
            bad()
