"""-m gpu: the planes of a scan through the session (InteractiveSession.planes, plane_at; PlanesResult.selection, section,
upright; grow(within=planes.plane_qv)).  The scene is a closed box room of 1.6 x 1.2 x 1.0 m, tilted by 3 degrees and turned
by 10, points 1/32 m apart (about 3 800 voxels of 5 cm), loaded as a cloud and as a mesh.  The rule is restated in
``planes_rule.py`` and applied to the session's own voxel rows and normals: ids and records are compared by equality.

1  a cloud: planes() needs estimate_normals(); floor, ceiling and four walls with their kinds; against the rule; selection +
   paint + corrected() give the floor to object 0; a view under section(ceiling, "below") shows no ceiling vertex; plane_at
   agrees with plane_full; grow(within=plane_qv) stays on its plane; within= as a mask and "label"; no session state changes
2  a mesh needs normals=; the same planes; plane_at through a face
"""
import numpy as np
import pytest
import torch

import planes_cases as PC
import planes_rule as PR
from agile3d_amd import view as V
from session_kit import DEV, _grid_faces, _model, intrinsic, look_at

pytestmark = pytest.mark.gpu
VS = 0.05
F32 = np.float32
SIZE = (1.6, 1.2, 1.0)
TURN = PC.rotation(3.0, 10.0)


@pytest.fixture(scope="module")
def model_005():
    return _model(VS)


@pytest.fixture(scope="module")
def box_room():
    """``(xyz fp32, colours fp32, side int (0 floor, 1 ceiling, 2..5 walls) per vertex, faces int32)``: six lattices of vertices
    1/32 m apart, two triangles a cell."""
    h = 1.0 / 32
    verts, faces, side = [], [], []
    base = 0
    for s, (axis, value) in enumerate([(2, 0.0), (2, SIZE[2]), (0, 0.0), (0, SIZE[0]), (1, 0.0), (1, SIZE[1])]):
        b, c = (axis + 1) % 3, (axis + 2) % 3
        gu, gv = np.arange(0.0, SIZE[b] + h / 2, h), np.arange(0.0, SIZE[c] + h / 2, h)
        u, v = np.meshgrid(gu, gv, indexing="ij")
        p = np.zeros((*u.shape, 3))
        p[..., axis], p[..., b], p[..., c] = value, u, v
        faces.append(_grid_faces(base + np.arange(u.size).reshape(u.shape)))
        verts.append(p.reshape(-1, 3))
        side.append(np.full(u.size, s))
        base += u.size
    xyz = np.concatenate(verts) @ TURN.T
    col = np.random.default_rng(0).uniform(0.2, 0.8, (len(xyz), 3))
    return xyz.astype(F32), col.astype(F32), np.concatenate(side), np.concatenate(faces).astype(np.int32)


def _session(model, xyz, col, faces=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, None, faces=faces)


def state_of(ses):
    manual = None if ses._manual is None else tuple(t.clone() for t in ses._manual)
    return (ses.clicks(), ses._labels_qv.clone(), None if ses._labels_last is None else ses._labels_last.clone(), manual, ses.normals,
            ses.section, ses._normals_last)


def same_state(ses, before):
    clicks, labels_qv, labels_last, manual, normals, section, normals_last = state_of(ses)
    assert clicks == before[0] and torch.equal(labels_qv, before[1]) and normals is before[4] and section is before[5]
    assert normals_last is before[6]
    assert (labels_last is None) == (before[2] is None) and (labels_last is None or torch.equal(labels_last, before[2]))
    assert (manual is None) == (before[3] is None) and (manual is None or all(torch.equal(a, b) for a, b in zip(manual, before[3])))


def against_the_rule(ses, r, normals, candidate=None):
    """A PlanesResult against the restatement on the session's own rows."""
    origin, quantum, bits = ses._fixed_point_frame()
    w, tol, cos_min = PR.settings(quantum, VS, r.normal_deg, r.dist_tol)
    want = PR.find_planes(normals.normals_qv.cpu().numpy(), ses.raw_coords_qv.cpu().numpy(), origin, quantum, bits, w, tol, cos_min,
                          r.min_voxels, r.max_planes, candidate=candidate, inverse_map=ses.inverse_map.cpu().numpy())
    assert np.array_equal(r.plane_qv.cpu().numpy(), want["plane_qv"]) and np.array_equal(r.plane_full.cpu().numpy(), want["plane_full"])
    assert r.n_planes == len(r.records) == len(want["records"])
    for field in ("normal", "inliers", "score", "round", "bin", "count", "sum", "mom", "N", "off"):
        assert r.records[field].tobytes() == want["records"][field].tobytes(), field
    s = want["summary"]
    assert (r.rounds, r.spent, r.admitted, r.left_out) == (s["rounds"], s["spent"], s["admitted"], s["left_out"])
    return want


def room_planes(r, side, xyz):
    """The six planes with their kinds.  A voxel within a voxel of a crease blends two sides' normals and lies on no plane;
    a vertex 0.15 m (three voxels) or more from every other side has a neighbourhood of its own side alone, so ALL of those
    lie on their side's plane.  Returns side -> plane id."""
    assert r.n_planes == 6 and sorted(r.kinds) == ["ceiling", "floor", "wall", "wall", "wall", "wall"]
    assert r.kinds[r.floor] == "floor" and r.kinds[r.ceiling] == "ceiling" and sorted(r.walls) == sorted(
        k for k in range(6) if k not in (r.floor, r.ceiling))
    full = r.plane_full.cpu().numpy()
    local = xyz.astype(np.float64) @ TURN                                 # the room's own axes
    ids = {}
    for s in range(6):
        axis = (2, 2, 0, 0, 1, 1)[s]
        others = [a for a in range(3) if a != axis]
        inner = (side == s) & np.all([(local[:, a] >= 0.15) & (local[:, a] <= SIZE[a] - 0.15) for a in others], axis=0)
        assert inner.sum() > 300 and len(set(full[inner].tolist())) == 1 and full[inner][0] >= 0, (s, np.unique(full[inner]))
        ids[s] = int(full[inner][0])
    assert ids[0] == r.floor and ids[1] == r.ceiling and len(set(ids.values())) == 6
    planted = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], np.float64) @ TURN.T
    for s in range(6):
        assert np.degrees(PR.NR.angle(r.records["normal"][ids[s]], planted[s])) < 0.5
    return ids


def top_view(ses, w=96, h=72):
    """The room from above: without a section the ceiling hides everything."""
    centre = np.array([SIZE[0] / 2, SIZE[1] / 2, 0.0]) @ TURN.T
    eye = np.array([SIZE[0] / 2, SIZE[1] / 2, 4.0]) @ TURN.T
    return ses.render(intrinsic(w, h, 40.0), look_at(eye, centre, up=(0.0, 1.0, 0.0)), w, h, radius=0.03)


# ---------------------------------------------------------------------------------------------------- 1
def test_cloud(model_005, box_room):
    from agile3d_amd.session import PlanesResult
    xyz, col, side, _ = box_room
    ses = _session(model_005, xyz, col)
    with pytest.raises(ValueError, match="estimate_normals"):
        ses.planes()
    normals = ses.estimate_normals()
    before = state_of(ses)
    r = ses.planes()
    assert isinstance(r, PlanesResult) and (r.normal_deg, r.dist_tol, r.min_voxels, r.max_planes, r.within) == (20.0, 1.5 * VS, 200, 16, "all")
    room_planes(r, side, xyz)
    against_the_rule(ses, r, normals)
    print(f"cloud: {ses.raw_coords_qv.shape[0]} voxels, inliers {r.records['inliers'].tolist()}, kinds {r.kinds}, rms {r.records['rms'].tolist()}")
    assert np.allclose(r.upright() @ TURN[:, 2], [0, 0, 1], atol=5e-3) and torch.equal(ses.planes().plane_qv, r.plane_qv)
    # ---- within: a mask over the voxels, and "label" (everything is background here)
    mask = torch.from_numpy(ses.raw_coords_qv.cpu().numpy() @ TURN[:, 2] < 0.5).to(DEV)
    low = ses.planes(within=mask)
    against_the_rule(ses, low, normals, candidate=mask.cpu().numpy().astype(np.uint8))
    assert low.within == "keys" and low.left_out["candidate"] == int((~mask).sum()) and "ceiling" not in low.kinds
    assert torch.equal(ses.planes(within="label").plane_qv, r.plane_qv)
    for bad in (dict(within="floor"), dict(within=mask[:5]), dict(normals=r), dict(up=(0, 0, 0)), dict(max_planes=17),
                dict(min_voxels=0), dict(normal_deg=120.0), dict(dist_tol=-1.0)):
        with pytest.raises(ValueError):
            ses.planes(**bad)
    # ---- plane_at agrees with plane_full at the pixel's vertex; a view under the section shows no ceiling vertex
    view = top_view(ses)
    full, shown = r.plane_full.cpu().numpy(), view.ids.cpu().numpy()
    assert (shown >= 0).sum() > 500 and (full[shown[shown >= 0]] == r.ceiling).mean() > 0.5 and not (full[shown[shown >= 0]] == r.floor).any()
    rng = np.random.default_rng(4)
    for u, v in [(int(rng.integers(96)), int(rng.integers(72))) for _ in range(12)] + [(0, 0)]:
        want = None if shown[v, u] < 0 or full[shown[v, u]] < 0 else int(full[shown[v, u]])
        assert ses.plane_at(view, u, v, planes=r) == want
    with pytest.raises(ValueError):
        ses.plane_at(view, 0, 0, planes=normals)
    # ---- grow(within=plane_qv) stays on its plane
    row = int(np.flatnonzero(r.plane_qv.cpu().numpy() == r.floor)[0])
    on_floor = ses.grow([row], steps=100, within=r.plane_qv)
    whole = r.selection(r.floor)
    assert (on_floor.selected <= whole).all() and on_floor.count > 0.9 * int(whole.sum())      # (an inlier voxel beside a crease may lie apart)
    assert ses.grow([row], steps=100).count > int(whole.sum())
    same_state(ses, before)
    # ---- the section cuts the ceiling off
    ses.set_section(r.section(r.ceiling, "below", margin=0.05))
    cut = top_view(ses).ids.cpu().numpy()
    assert (cut >= 0).sum() > 500 and not (full[cut[cut >= 0]] == r.ceiling).any() and (full[cut[cut >= 0]] == r.floor).sum() > 500     # (the floor shows now)
    ses.set_section(None)
    # ---- selection, paint and corrected() give the floor to object 0
    ses.click(xyz[np.flatnonzero(side == 2)[0]], 1)
    everything = torch.ones(len(xyz), dtype=torch.uint8, device=DEV)
    assert ses.paint(everything, 1) == len(xyz)
    floor = r.selection(r.floor)
    assert ses.paint(floor, 0) == int(floor.sum()) > 1000
    labels = ses.corrected().labels_full
    assert (labels[floor != 0] == 0).all() and (labels[floor == 0] == 1).all()
    assert (side[floor.cpu().numpy() != 0] == 0).mean() > 0.9             # (a floor voxel along a crease holds wall vertices too)


# ---------------------------------------------------------------------------------------------------- 2
def test_mesh(model_005, box_room):
    xyz, col, side, faces = box_room
    ses = _session(model_005, xyz, col, faces=faces)
    normals = ses.estimate_normals()
    with pytest.raises(ValueError, match="normals="):
        ses.planes()
    before = state_of(ses)
    r = ses.planes(normals=normals, up=(0, 0, 2))
    room_planes(r, side, xyz)
    against_the_rule(ses, r, normals)
    ses.set_section(r.section(r.ceiling, "below", margin=0.05))
    view = top_view(ses)
    ses.set_section(None)
    full = r.plane_full.cpu().numpy()
    seen = 0
    for u, v in [(48, 36), (40, 30), (60, 40), (20, 20), (0, 0)]:
        vertex = ses._vertex_at(view, u, v)
        want = None if vertex < 0 or full[vertex] < 0 else int(full[vertex])
        assert ses.plane_at(view, u, v, planes=r) == want and want != r.ceiling
        seen += want is not None
    assert seen >= 3
    same_state(ses, before)
