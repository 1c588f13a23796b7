"""-m gpu: the objects of a labelling measured through the session (InteractiveSession.measure, MeasureResult.section, frame) on
session_kit's mesh and cloud scenes.  The integers are held to ``measure_rule.py`` exactly, on the session's labels copied to
the host; what ``object_table`` and ``principal_axes`` make of them is tested without a GPU in ``test_measure_host.py``.

1  from load_scene on: everything in object 0
2  after two clicks and infer(): every field against the rule; measure(labels=) on the ground truth and on despeckle()'s result;
   oriented=False; no session state changes
3  section(obj) isolates the object in render; frame(obj) shows it; refusals
"""
import numpy as np
import pytest
import torch

import session_kit
from agile3d_amd.session import InteractiveSession, object_table, principal_axes, ray_from_pixel
from measure_rule import extents_numpy, measure_numpy
from session_kit import DEV, PlanesScene, cloud_scene, rotation

pytestmark = pytest.mark.gpu
u32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
ROT = rotation(3)


@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def scene_of(kind):
    """(xyz, faces or None, ground truth: five stripes along y).  Both scenes are turned by a generic rotation: ``frame`` looks
    along +y, and a horizontal sheet would be seen edge-on, its near stripe hiding the others."""
    if kind == "mesh":
        sc = PlanesScene(8, rot=ROT)                                        # 177 vertices, 261 faces: two planes, five loose faces
        xyz, faces = sc.xyz, sc.faces
    else:
        xyz, faces = (cloud_scene("receding sheet")[0].astype(np.float64) @ ROT.T).astype(np.float32), None
    y = xyz[:, 1]
    lab = np.clip(np.floor((y - y.min()) / ((y.max() - y.min()) / 5)), 0, 4).astype(np.int32)
    return xyz, faces, lab


def session(model, kind):
    xyz, faces, lab = scene_of(kind)
    ses = InteractiveSession(model, voxel_size=0.05).load_scene(xyz, np.full(xyz.shape, 0.5, np.float32), lab, faces=faces)
    return ses, xyz, faces, lab


def against_the_rule(ses, got, labels_full, labels_qv, oriented=True):
    """Every field of a MeasureResult against the rule on host copies of the labels."""
    xyz = ses.coords_full.cpu().numpy()
    faces = None if ses.faces is None else ses.faces.cpu().numpy()
    origin, quantum, bits = ses._fixed_point_frame()
    half = np.abs(xyz.astype(np.float64) - origin).max()
    assert quantum * 2 ** bits >= half > quantum * 2 ** bits / 2 and bits == 20          # the frame fits the scene, and tightly
    aq = None if faces is None else quantum ** 2 * 256.0
    rec, err = measure_numpy(xyz, labels_full, origin, quantum, bits, 256, labels_qv, faces, aq)
    assert err == 0
    k = len(got.vertices)
    assert k >= len(ses.click_idx) and not rec["vertices"][k:].any() and not rec["voxels"][k:].any()
    for field in ("vertices", "voxels", "sum", "mom", "area_thirds"):
        assert np.array_equal(got.moments[field], rec[field][:k]), field
    assert np.array_equal(u32(got.lo), u32(rec["lo"][:k])) and np.array_equal(u32(got.hi), u32(rec["hi"][:k]))
    assert np.array_equal(got.vertices, np.bincount(labels_full, minlength=k)) and got.vertices.sum() == len(xyz)
    assert np.array_equal(got.voxels, np.bincount(labels_qv, minlength=k))
    t = object_table(rec[:k], origin, quantum, aq, ses.voxel_size)
    for field in ("centroid", "cov", "volume"):
        assert np.array_equal(getattr(got, field), t[field], equal_nan=True), field
    if faces is None:
        assert got.area is None
    else:
        a, b, c = (xyz[faces[:, j]].astype(np.float64) for j in range(3))
        total = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
        assert np.array_equal(got.area, t["area"]) and abs(got.area.sum() - total) <= len(faces) * aq / 4
    for obj in np.flatnonzero(got.vertices):
        p = xyz[labels_full == obj]
        assert np.array_equal(got.lo[obj], p.min(0)) and np.array_equal(got.hi[obj], p.max(0))
        assert np.abs(got.centroid[obj] - p.astype(np.float64).mean(0)).max() <= quantum / 2 + 1e-12
    if not oriented:
        assert got.axes is None and got.centre is None and got.extents is None
        return
    axes32 = np.tile(np.eye(3, dtype=np.float32), (256, 1, 1))
    axes32[:k] = principal_axes(t["cov"], t["vertices"])[0].astype(np.float32)
    span, err = extents_numpy(xyz, labels_full, axes32)
    assert err == 0 and np.array_equal(got.axes, axes32[:k].astype(np.float64))
    span = span[:k].astype(np.float64)
    live = got.vertices > 0
    assert np.array_equal(got.extents[live], (span[..., 1] - span[..., 0])[live]) and not got.extents[~live].any()
    centre = np.einsum("kj,kjc->kc", 0.5 * (span[..., 0] + span[..., 1])[live], axes32[:k][live].astype(np.float64))
    assert np.allclose(got.centre[live], centre, rtol=0, atol=1e-12) and np.isnan(got.centre[~live]).all()
    for obj in np.flatnonzero(live):                                      # the oriented box holds the object
        local = (xyz[labels_full == obj].astype(np.float64) - got.centre[obj]) @ got.axes[obj].T
        assert (np.abs(local) <= got.extents[obj] / 2 + 1e-5).all()


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", ["mesh", "cloud"])
def test_from_load_scene_on_everything_is_object_0(model_005, kind):
    ses, xyz, faces, lab = session(model_005, kind)
    got = ses.measure()
    n_qv = ses.raw_coords_qv.shape[0]
    assert got.vertices.tolist() == [len(xyz)] and got.voxels.tolist() == [n_qv] and got.volume.tolist() == [n_qv * 0.05 ** 3]
    assert (got.area is None) == (faces is None) and got.axes.shape == (1, 3, 3)
    against_the_rule(ses, got, np.zeros(len(xyz), np.int64), np.zeros(n_qv, np.int64))
    if kind == "cloud":                                                   # a sheet 6.6 m x 3 m x 0.1 m: its axes in that order
        assert got.extents[0, 0] > got.extents[0, 1] > got.extents[0, 2] > 0 and abs(abs(got.axes[0, 0] @ ROT[:, 1]) - 1) < 1e-2


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", ["mesh", "cloud"])
def test_after_clicks_and_infer_against_the_rule(model_005, kind):
    ses, xyz, faces, lab = session(model_005, kind)
    ses.click(xyz[np.flatnonzero(lab == 1)[0]], 1)
    ses.click(xyz[np.flatnonzero(lab == 3)[0]], 2)
    res = ses.infer()
    before = dict(clicks=ses.clicks(), labels_last=ses._labels_last, colors_last=ses._colors_last, logits=ses._guide_logits[0],
                  labels_qv=ses._labels_qv, qv_copy=ses._labels_qv.clone(), section=ses.section)
    got = ses.measure()
    labels_full, labels_qv = res.labels_full.cpu().numpy().astype(np.int64), ses._labels_qv.cpu().numpy().astype(np.int64)
    assert len(got.vertices) >= 3 and got.vertices[1] > 0 and got.vertices[2] > 0        # a clicked voxel keeps its object
    against_the_rule(ses, got, labels_full, labels_qv)
    flat = ses.measure(oriented=False)
    against_the_rule(ses, flat, labels_full, labels_qv, oriented=False)
    assert np.array_equal(flat.moments, got.moments)
    # another labelling: the ground truth (a voxel carries the label of the vertex it was made from), despeckle()'s result
    truth = ses.measure(labels=ses.labels_full_ori)
    against_the_rule(ses, truth, lab.astype(np.int64), ses.labels_qv_ori.cpu().numpy().astype(np.int64))
    assert len(truth.vertices) == 5 and (truth.vertices > 0).all()
    clean = ses.despeckle(min_voxels=4)
    against_the_rule(ses, ses.measure(labels=clean.labels_full), clean.labels_full.cpu().numpy().astype(np.int64),
                     clean.labels_qv.cpu().numpy().astype(np.int64))
    # no session state changed: the same objects, the same values
    assert ses.clicks() == before["clicks"] and ses._labels_last is before["labels_last"] and ses._colors_last is before["colors_last"]
    assert ses._guide_logits[0] is before["logits"] and ses._labels_qv is before["labels_qv"] and ses.section is before["section"]
    assert torch.equal(ses._labels_qv, before["qv_copy"])
    ses.guide()                                                           # still describes that inference
    for bad in (ses.labels_full_ori[:-1], ses.labels_full_ori.long(), ses.labels_full_ori.cpu(), lab):
        with pytest.raises(ValueError):
            ses.measure(labels=bad)
    out = ses.labels_full_ori.clone()
    out[0] = 256
    with pytest.raises(RuntimeError):
        ses.measure(labels=out)


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", ["mesh", "cloud"])
def test_section_and_frame_show_the_object(model_005, kind):
    ses, xyz, faces, lab = session(model_005, kind)
    ses.click(xyz[np.flatnonzero(lab == 1)[0]], 1)
    ses.click(xyz[np.flatnonzero(lab == 3)[0]], 2)
    ori = ses.labels_qv_ori.cpu().numpy()                                 # replayed logits: object 1 = stripe 1, object 2 = stripe 3
    logits = np.full((len(ori), 3), -2.0, np.float32)
    logits[np.arange(len(ori)), np.where(ori == 1, 1, np.where(ori == 3, 2, 0))] = 3.0
    ses.infer(logits=torch.from_numpy(logits).to(DEV))
    m = ses.measure(oriented=False)
    labels_full = ses._labels_last.cpu().numpy()
    assert m.vertices[1] > 20 and m.vertices[2] > 20
    w, h = 64, 48
    for obj in (1, 2):
        sec = m.section(obj, margin=0.02)
        assert sec.keeps(xyz[labels_full == obj]).all()
        k, e = ses.frame(obj, w, h, measure=m)
        k2, e2 = ses.frame(obj, w, h)                                     # measured on the spot: the same camera
        assert np.array_equal(k, k2) and np.array_equal(e, e2)
        # framed, without a section: the object is in the picture
        view = ses.render(k, e, w, h, radius=0.08)
        assert obj in np.unique(ses.label_image(view).cpu().numpy())
        # under the object's section every pixel shows something inside its box
        ses.set_section(sec)
        cut = ses.render(k, e, w, h, radius=0.08)
        ses.set_section(None)
        ids, t = cut.ids.cpu().numpy(), cut.t.cpu().numpy()
        shown = np.argwhere(ids >= 0)
        assert len(shown) > 0 and cut.section is sec
        lo, hi = m.lo[obj].astype(np.float64) - 0.02, m.hi[obj].astype(np.float64) + 0.02
        if faces is None:
            assert sec.keeps(xyz[ids[ids >= 0]]).all()                    # a cloud: the planes select vertices
        else:
            for v, u in shown[:: max(1, len(shown) // 40)]:               # a mesh: the planes cut the ray -- the point it meets
                o, d = ray_from_pixel(u, v, k, e)
                p = o + float(t[v, u]) * d
                assert (p >= lo - 1e-3).all() and (p <= hi + 1e-3).all()
        assert (ids >= 0).sum() <= (view.ids.cpu().numpy() >= 0).sum()
    with pytest.raises(ValueError):
        ses.frame(len(m.vertices), w, h, measure=m)
    with pytest.raises(ValueError):
        m.section(len(m.vertices))


def test_measure_before_load_scene_raises(model_005):
    ses = InteractiveSession(model_005, voxel_size=0.05)
    with pytest.raises(RuntimeError):
        ses.measure()
    with pytest.raises(RuntimeError):
        ses.frame(0, 64, 48)
