"""-m gpu: labels to and from another point set through the session (InteractiveSession.nearest_vertices, transfer,
import_labels).  The search is held to the brute-force rule of ``transfer_rule.py`` on the session's own vertices, bit for bit;
logits are replayed through ``infer(logits=...)``, so no result depends on the model's weights.

1  transfer(coords_full) returns the session's own labels; nearest is the vertex itself, the lowest id among exact duplicates
2  transfer to a jittered, permuted superset (numpy, a float64 host tensor, a device tensor) against the rule; points out of
   reach get ``fill`` and are counted
3  import_labels(into="manual"): corrected() shows the imported ids on the matched vertices and the model's elsewhere; a second
   import keeps the first; an id above 255 raises and leaves the layer
4  import_labels(into="truth") on a scene loaded without labels: infer() then reports the miou of the scene loaded with them;
   with clicks present it raises and changes nothing
5  the index over the vertices is reused, rebuilt for another max_distance, dropped by load_scene
6  every ValueError
"""
import numpy as np
import pytest
import torch

import transfer_rule as R
from agile3d_amd.synthetic import make_scene
from session_kit import DEV, _model

pytestmark = pytest.mark.gpu
VS = 0.02
F32 = np.float32


@pytest.fixture(scope="module")
def model_002():
    return _model(VS)


def _session(model, xyz, col, lab=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, lab)


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene: every voxel's point plus a second vertex 4 mm beside it, shuffled, and behind them exact
    copies of the first 50 vertices."""
    sc = make_scene(5_000, seed=6, voxel_size=VS)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(F32)]).astype(F32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(F32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    xyz, col, lab = xyz[p], col[p], lab[p]
    return np.concatenate([xyz, xyz[:50]]), np.concatenate([col, col[:50]]), np.concatenate([lab, lab[:50]])


def click_and_infer(ses, scene, seed=0):
    """Three objects and the background clicked, then random logits replayed: the same state for every session of the scene."""
    xyz, _, lab = scene
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:3]
    for k, i in enumerate(inst):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((ses.raw_coords_qv.shape[0], 4), generator=g).to(DEV)
    return ses.infer(logits=logits)


@pytest.fixture(scope="module")
def annotated(model_002, scene):
    ses = _session(model_002, *scene)
    return ses, click_and_infer(ses, scene)


@pytest.fixture(scope="module")
def other_set(scene):
    """Another point set of the same surface: the vertices jittered by up to a quarter voxel per axis plus 400 points a metre and
    more away, permuted; with labels of its own in 0..255."""
    xyz = scene[0]
    rng = np.random.default_rng(21)
    near = xyz.astype(np.float64) + rng.uniform(-VS / 4, VS / 4, xyz.shape)
    far = xyz[:400].astype(np.float64) + [0.0, 0.0, 50.0]
    pts = np.concatenate([near, far])[rng.permutation(len(xyz) + 400)]
    return pts, rng.integers(0, 256, len(pts)).astype(np.int32)


def same(result, want, labels=True):
    assert result.nearest.cpu().numpy().tolist() == want["nearest"].tolist()
    assert result.distance2.cpu().numpy().tobytes() == want["d2"].tobytes()
    assert (result.matched, result.unmatched, result.nonfinite) == (want["matched"], want["unmatched"], want["nonfinite"])
    if labels:
        assert result.labels.cpu().numpy().tolist() == want["labels"].tolist()


# ------------------------------------------------------------------------------------------- 1, 2
def test_transfer_to_the_scenes_own_vertices(annotated, scene):
    ses, res = annotated
    n = len(scene[0])
    r = ses.transfer(ses.coords_full)
    assert torch.equal(r.labels, res.labels_full) and r.matched == n and r.unmatched == 0 and r.nonfinite == 0
    assert not r.distance2.any()
    want = np.arange(n)
    want[n - 50:] = np.arange(50)                                    # the exact copies: the lowest id
    assert r.nearest.cpu().numpy().tolist() == want.tolist()
    lab = res.labels_full.cpu().numpy()
    assert r.colors.cpu().numpy().tobytes() == ses.palette[lab].tobytes() and r.max_distance == float(F32(VS))
    nv = ses.nearest_vertices(ses.coords_full)
    assert nv.labels is None and nv.colors is None and torch.equal(nv.nearest, r.nearest)


def test_transfer_to_a_jittered_permuted_superset(annotated, scene, other_set):
    ses, res = annotated
    pts, _ = other_set
    lab = res.labels_full.cpu().numpy()
    want = R.nearest(scene[0], pts.astype(F32), VS, labels=lab, fill=77)
    assert want["unmatched"] == 400 and want["matched"] == len(scene[0])
    r = ses.transfer(pts, fill=77)                                   # float64 numpy
    same(r, want)
    assert (r.labels[r.nearest < 0] == 77).all() and int((r.nearest < 0).sum()) == r.unmatched == 400
    same(ses.transfer(torch.from_numpy(pts)), dict(want, labels=np.where(want["nearest"] >= 0, want["labels"], 0)))   # a host tensor, fill 0
    part = pts[:3000].astype(F32)
    dev_pts = torch.from_numpy(part).to(DEV)
    same(ses.transfer(dev_pts, labels=ses.labels_full_ori, max_distance=VS / 2),
         R.nearest(scene[0], part, VS / 2, labels=scene[2], fill=0))                                             # labels of the caller's
    same(ses.nearest_vertices(dev_pts, max_distance=0.003), R.nearest(scene[0], part, 0.003), labels=False)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0]])
    r = ses.transfer(np.concatenate([odd, pts[:10]]))
    assert r.nonfinite == 2 and r.nearest[:2].cpu().tolist() == [-1, -1] and r.labels[:2].cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------- 3
def test_import_into_the_manual_layer(model_002, scene, other_set):
    ses = _session(model_002, *scene)
    res = click_and_infer(ses, scene)
    model = res.labels_full.cpu().numpy()
    pts, lab = other_set
    half = pts[::2], lab[::2]
    want = R.nearest(half[0].astype(F32), scene[0], VS, labels=half[1])
    r = ses.import_labels(*half)
    same(r, want)
    hit = want["nearest"] >= 0
    assert 0 < hit.sum() < len(hit)
    c = ses.corrected()
    assert c.labels_full.cpu().numpy().tolist() == np.where(hit, want["labels"], model).tolist() and c.overridden == hit.sum()
    # a second import, a short reach: what it matches is replaced, the rest of the layer stays
    want2 = R.nearest(pts[1::2].astype(F32), scene[0], 0.002, labels=lab[1::2])
    ses.import_labels(torch.from_numpy(pts[1::2]), torch.from_numpy(lab[1::2]).to(torch.int64), max_distance=0.002)
    hit2 = want2["nearest"] >= 0
    assert 0 < hit2.sum() < len(hit2)
    both = np.where(hit2, want2["labels"], np.where(hit, want["labels"], model))
    assert ses.corrected().labels_full.cpu().numpy().tolist() == both.tolist()
    with pytest.raises(ValueError, match="255"):
        ses.import_labels(pts[::2], lab[::2] + 300)
    assert ses.corrected().labels_full.cpu().numpy().tolist() == both.tolist()


# ------------------------------------------------------------------------------------------- 4
def test_import_as_ground_truth(model_002, scene, other_set):
    xyz, col, _ = scene
    pts, lab = other_set
    lab = (lab % 7).astype(np.int32)
    truth = R.nearest(pts.astype(F32), xyz, VS, labels=lab)["labels"]
    with_labels = _session(model_002, xyz, col, truth)
    want = click_and_infer(with_labels, (xyz, col, truth))
    ses = _session(model_002, xyz, col)
    assert ses.labels_full_ori is None
    r = ses.import_labels(pts, lab, into="truth")
    assert r.labels.cpu().numpy().tolist() == truth.tolist()
    assert torch.equal(ses.labels_full_ori, with_labels.labels_full_ori) and torch.equal(ses.labels_qv_ori, with_labels.labels_qv_ori)
    got = click_and_infer(ses, (xyz, col, truth))
    assert want.miou is not None and got.miou == want.miou and got.iou_per_object == want.iou_per_object
    # with clicks present: refused, nothing changed
    before = ses.labels_full_ori, ses.labels_qv_ori, ses.new_labels.clone()
    with pytest.raises(ValueError, match="click"):
        ses.import_labels(pts, lab + 1, into="truth")
    assert ses.labels_full_ori is before[0] and ses.labels_qv_ori is before[1] and torch.equal(ses.new_labels, before[2])
    ses.reset()
    ses.import_labels(pts, lab + 1, into="truth")                    # after reset() it is allowed again
    assert ses.labels_full_ori.cpu().numpy().tolist() == np.where(truth >= 0, truth + 1, 0).tolist()


# ------------------------------------------------------------------------------------------- 5
def test_the_index_is_kept_rebuilt_and_dropped(model_002, scene):
    ses = _session(model_002, *scene)
    assert ses._point_indices == {}
    pts = scene[0][:100]
    ses.nearest_vertices(pts)
    (cell, index), = ses._point_indices.items()
    assert cell == float(F32(2) * F32(VS)) and index.n == len(scene[0]) and index.handle is not None
    ses.preview()
    ses.transfer(pts)
    assert ses._point_indices[cell] is index and len(ses._point_indices) == 1           # reused
    ses.nearest_vertices(pts, max_distance=VS / 2)
    assert len(ses._point_indices) == 2 and ses._point_indices[cell] is index          # another reach: another index
    other = ses._point_indices[float(F32(2) * F32(VS / 2))]
    ses.import_labels(pts, np.ones(100, np.int32))                                     # an index of its own, gone after the call
    assert len(ses._point_indices) == 2
    ses.load_scene(scene[0][:500], scene[1][:500])
    assert ses._point_indices == {} and index.handle is None and other.handle is None
    r = ses.nearest_vertices(pts)
    assert ses._point_indices[cell].n == 500 and r.matched == int((r.nearest >= 0).sum()) > 0


# ------------------------------------------------------------------------------------------- 6
def test_value_errors(model_002, scene):
    ses = _session(model_002, *scene)
    n = len(scene[0])
    pts = scene[0][:20]
    with pytest.raises(ValueError, match="infer"):                   # no labels yet
        ses.transfer(pts)
    ses.preview()
    good = torch.zeros(n, dtype=torch.int32, device=DEV)
    for bad in (np.zeros((5, 2)), np.zeros(3), np.zeros((2, 3, 1)), np.zeros((5, 3), np.int64), torch.zeros((3, 5))):
        for call in (ses.nearest_vertices, ses.transfer, lambda p: ses.import_labels(p, np.zeros(len(p), np.int32))):
            with pytest.raises(ValueError, match="points"):
                call(bad)
    for bad in (good[:-1], good.cpu(), good.to(torch.int64), good.reshape(1, -1), np.zeros(n, np.int32)):
        with pytest.raises(ValueError, match="labels"):
            ses.transfer(pts, labels=bad)
    for bad in (0.0, -1.0, np.nan, np.inf, 1e39, 1e-50):
        for call in (ses.nearest_vertices, ses.transfer, lambda p, max_distance: ses.import_labels(p, np.zeros(len(p), np.int32), max_distance)):
            with pytest.raises(ValueError, match="max_distance"):
                call(pts, max_distance=bad)
    for bad in (np.zeros(19, np.int32), np.zeros(20, F32), np.zeros((20, 1), np.int32), np.zeros(20, bool)):
        with pytest.raises(ValueError, match="labels"):
            ses.import_labels(pts, bad)
    with pytest.raises(ValueError, match="into"):
        ses.import_labels(pts, np.zeros(20, np.int32), into="model")
    with pytest.raises(ValueError, match="fill"):
        ses.transfer(pts, fill=1 << 31)
    assert ses.manual_labels()[0].sum() == 0 and ses.labels_full_ori is not None
