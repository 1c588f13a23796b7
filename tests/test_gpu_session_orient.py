"""-m gpu: normals oriented by propagation through the session (InteractiveSession.orient_normals, orient_at).  The rule is
restated in ``orient_rule.py`` and applied to the session's own voxel rows and normals; the normals are compared by their bytes.

1  the room with the cabinet as a cloud: orient_normals() flips cabinet voxels only and matches the rule; a back-culled render
   from outside the cabinet shows its near face after the call and not before; few sweeps a call give the same bytes
2  orient_at on one of two plates changes that plate only; None on the background
3  on a mesh the result is returned and no state changes; load_scene drops the oriented normals, reset keeps them
4  the ValueErrors
"""
import numpy as np
import pytest
import torch

import orient_cases as K
import orient_rule as R
from pieces_rule import pieces_numpy
from session_kit import DEV, _model, intrinsic, jittered_grid, look_at

pytestmark = pytest.mark.gpu
VS = 0.05
F32 = np.float32


@pytest.fixture(scope="module")
def model_005():
    return _model(VS)


def _session(model, xyz, col=None, faces=None):
    from agile3d_amd.session import InteractiveSession
    col = np.full((len(xyz), 3), 0.5, F32) if col is None else col
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, None, faces=faces)


def cloud_of(coords4):
    """One vertex at the centre of every voxel."""
    return ((coords4[:, 1:].astype(np.float64) + 0.5) * VS).astype(F32)


def voxel_coords(ses):
    return ses._scene_handle().coords.cpu().numpy().astype(np.int64)


def raw(t):
    return t.cpu().numpy().tobytes()


def rule_of(ses, normals_qv, connectivity=26, **seeds):
    coords = voxel_coords(ses)
    nrm = normals_qv.cpu().numpy()
    if not seeds:
        comp = pieces_numpy(coords, R.admitted(nrm).astype(np.int64) - 1, connectivity)[0]
        seeds = dict(components=comp, positions=ses.raw_coords_qv.cpu().numpy(), viewpoint=ses._fixed_point_frame()[0])
    inv = ses.inverse_map.cpu().numpy()
    return R.orient_all(coords, nrm, n_full=len(inv), inverse_map=inv, connectivity=connectivity, **seeds)


def same_result(res, want):
    for name, key in (("normals_full", "normal_full"), ("normals_qv", "normal_out"), ("flipped_qv", "flipped"), ("dist_qv", "dist"),
                      ("owner_qv", "owner")):
        got = getattr(res, name).cpu().numpy()
        assert got.dtype == want[key].dtype and got.tobytes() == want[key].tobytes(), name
    for k, v in want["summary"].items():
        assert k == "converged" or getattr(res, k) == v, (k, getattr(res, k), v)


# ---------------------------------------------------------------------------------------------------- 1
def test_room_with_cabinet_cloud(model_005):
    from agile3d_amd.session import OrientResult, Section
    coords, _ = K.room_with_cabinet()
    ses = _session(model_005, cloud_of(coords))
    vox = voxel_coords(ses)[:, 1:]
    cab = torch.from_numpy(((vox >= K.CABINET_LO) & (vox <= K.CABINET_HI)).all(1)).to(DEV)
    assert len(vox) == 5308 and int(cab.sum()) == 260
    with pytest.raises(ValueError, match="estimate_normals"):
        ses.orient_normals()
    est = ses.estimate_normals()
    before = est.normals_qv.clone()
    # from inside the room, beyond the cabinet's side that faces away from the room's centre (x = 25), looking back at it
    eye = (np.array([28.5, 8.0, 5.0]) * VS, np.array([22.0, 8.0, 5.0]) * VS)
    view = (intrinsic(64, 48, 50.0), look_at(*eye), 64, 48)
    inner = (vox[:, 0] == 25) & (vox[:, 1] >= 6) & (vox[:, 1] <= 9) & (vox[:, 2] >= 3) & (vox[:, 2] <= 6)
    near = cab & torch.from_numpy(inner).to(DEV)                         # the planar middle of that side: normals along x
    shown = lambda r: int(near[ses.inverse_map[r.ids[r.ids >= 0].long()]].sum())
    culled_before = ses.render(*view, section=Section(cull="back"))
    assert shown(culled_before) == 0 and shown(ses.render(*view)) > 100    # turned into the cabinet: the near face is culled away
    assert ses._culled
    res = ses.orient_normals()
    assert isinstance(res, OrientResult) and res.launched == 512 and res.connectivity == 26
    same_result(res, rule_of(ses, before))
    assert res.seeds == 1 and res.reached == res.admitted == 5308 and res.unreached == 0 and res.err == 0
    assert int(res.flipped_qv[~cab].sum()) == 0 and int(res.flipped_qv[cab].sum()) == res.flipped > 50
    assert raw(res.normals_qv[~cab]) == raw(before[~cab])
    assert ses.normals is res.normals_full and ses._normals_last is res.result and ses._culled == {}
    assert ses._normals_last.variation_qv is est.variation_qv and raw(est.normals_qv) == raw(before)     # the estimate is not written over
    culled_after = ses.render(*view, section=Section(cull="back"))
    assert shown(culled_after) > 100 and not torch.equal(culled_after.ids, culled_before.ids)
    u, v = 32, 24
    assert ses.normal_at(culled_after, u, v)[0][0] > 0.9                # the near face now faces the camera (+x)
    # few sweeps a call: resumed until converged, the same bytes
    slow = ses.orient_normals(normals=est, sweeps=5)
    assert slow.launched > 5 and slow.launched % 5 == 0
    for name in ("normals_full", "normals_qv", "flipped_qv", "dist_qv", "owner_qv"):
        assert raw(getattr(slow, name)) == raw(getattr(res, name)), name
    # seeds that are trusted as they stand: a floor voxel, rows and a mask
    floor_row = int(np.flatnonzero((vox == (3, 3, 0)).all(1))[0])
    given = ses.orient_normals(seeds=[floor_row], normals=est, connectivity=18)
    same_result(given, rule_of(ses, before, 18, seed_qv=np.eye(1, 5308, floor_row, dtype=np.uint8)[0]))
    mask = torch.zeros(5308, dtype=torch.uint8, device=DEV)
    mask[floor_row] = 1
    assert raw(ses.orient_normals(seeds=mask, normals=est, connectivity=18).normals_qv) == raw(given.normals_qv)
    # load_scene drops the oriented normals, reset keeps them
    kept = ses.normals
    ses.reset()
    assert ses.normals is kept
    ses.load_scene(cloud_of(coords[:500]), np.full((500, 3), 0.5, F32), None)
    assert ses.normals is None and ses._normals_last is None
    with pytest.raises(ValueError, match="scene"):
        ses.orient_normals(normals=est)


# ---------------------------------------------------------------------------------------------------- 2
def test_orient_at_changes_one_component(model_005):
    coords = K.plates(7)
    ses = _session(model_005, cloud_of(coords))
    vox = voxel_coords(ses)[:, 1:]
    lower = torch.from_numpy(vox[:, 2] == 0).to(DEV)
    est = ses.estimate_normals(viewpoint=None)                          # the canonical sign: +z on both plates
    before = est.normals_qv.clone()
    assert float(before[:, 2].min()) > 0.9
    centre = np.array([3.5, 3.5, 0.5]) * VS
    below = ses.render(intrinsic(64, 48, 45.0), look_at(centre - [0.0, 0.0, 1.0], centre, up=(0.0, 1.0, 0.0)), 64, 48)
    assert int(below.ids[24, 32]) >= 0 and int(below.ids[0, 0]) < 0
    assert ses.orient_at(below, 0, 0) is None and ses.normals is est.normals_full
    res = ses.orient_at(below, 32, 24)
    same_result(res, rule_of(ses, before, seed_qv=np.eye(1, 98, int(ses.inverse_map[int(below.ids[24, 32])]), dtype=np.uint8)[0],
                             seed_flip=np.ones(98, np.uint8)))
    assert res.seeds == 1 and res.flipped == res.reached == 49 and res.unreached == 49
    assert raw(res.normals_qv[~lower]) == raw(before[~lower]) and raw(res.normals_qv[lower]) == raw(-before[lower])
    assert ses.normals is res.normals_full
    again = ses.orient_at(below, 32, 24)                                # it already faces the camera: nothing turns
    assert again.flipped == 0 and raw(again.normals_qv) == raw(res.normals_qv)


# ---------------------------------------------------------------------------------------------------- 3, 4
def test_on_a_mesh_no_state_changes_and_the_value_errors(model_005):
    xyz, faces = jittered_grid(12, 9, seed=3)
    xyz = (xyz * 0.5).astype(F32)                                       # vertices one voxel apart
    ses = _session(model_005, xyz, faces=faces)
    est = ses.estimate_normals()
    assert ses.normals is None and ses._normals_last is None
    with pytest.raises(ValueError, match="estimate_normals"):
        ses.orient_normals()
    res = ses.orient_normals(normals=est)
    same_result(res, rule_of(ses, est.normals_qv))
    assert ses.normals is None and ses._normals_last is None and ses._culled == {} and res.reached > 50
    n = ses.raw_coords_qv.shape[0]
    bad = [dict(seeds="farthest"), dict(viewpoint="origin"), dict(viewpoint=(0.0, np.nan, 0.0)), dict(viewpoint=(0.0, 1.0)),
           dict(connectivity=8), dict(sweeps=0), dict(sweeps=4097), dict(seeds=[n]), dict(seeds=[-1]), dict(seeds=3.5),
           dict(seeds=torch.zeros(n + 1, dtype=torch.uint8, device=DEV)), dict(seeds=torch.zeros(n, dtype=torch.int32, device=DEV)),
           dict(seeds=torch.zeros(n, dtype=torch.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            ses.orient_normals(normals=est, **kw)
    for normals in (est.normals_qv, "last"):
        with pytest.raises(ValueError, match="NormalsResult"):
            ses.orient_normals(normals=normals)
