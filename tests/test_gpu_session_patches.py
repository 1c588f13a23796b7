"""-m gpu: smooth patches, the magic wand and the snap through the session (InteractiveSession.patches, wand_at, snap;
grow(within=patches.piece_qv)).  The rules are restated in ``patches_rule.py`` and applied to the session's own voxel rows,
normals and colours; every comparison is by equality.

1  a room of three axis-aligned plates whose points lie at multiples of 1/32: every voxel whose 27-neighbourhood lies in one
   plate is in that plate's patch; patches() against the rule; wand_at in its three modes, by colour, on the background;
   paint / erase / grow / shrink take a wand; grow_at(within=patches.piece_qv) stays on the plate; no session state changes
2  patches() against the rule on the committed scan, with normals, colours and the labels together
3  snap() straightens a labelling whose boundary was pushed three voxels across a plate and leaves a patch that holds an
   opposing click alone; against the rule; the ValueErrors
4  a mesh needs normals=
"""
import os
import shutil

import numpy as np
import pytest
import torch

import patches_rule as P
from agile3d_amd import view as V
from conftest import GOLDEN
from session_kit import DEV, _model, intrinsic, look_at

pytestmark = pytest.mark.gpu
VS = 0.05
F32 = np.float32


@pytest.fixture(scope="module")
def model_005():
    return _model(VS)


def _session(model, xyz, col, lab=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, lab)


@pytest.fixture(scope="module")
def room():
    """A floor (z = 0, 1.5 m x 1.5 m) and two walls (x = 0 and y = 0, 1 m high) that meet in a corner, points 1/32 m apart:
    every coordinate is a multiple of 1/32 and so is the centre of the box, so the fixed-point frame of the normals holds them
    exactly.  Instances: floor 1, wall x = 0 is 2, wall y = 0 is 3.  The floor and the wall y = 0 share a colour."""
    g, up = np.arange(49) / 32, np.arange(1, 33) / 32
    a, b = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([a, b, np.zeros_like(a)], -1).reshape(-1, 3)
    y, z = np.meshgrid(g, up, indexing="ij")
    wall_x = np.stack([np.zeros_like(y), y, z], -1).reshape(-1, 3)
    wall_y = wall_x[:, [1, 0, 2]]
    xyz = np.concatenate([floor, wall_x, wall_y])
    lab = np.concatenate([np.full(len(floor), 1), np.full(len(wall_x), 2), np.full(len(wall_y), 3)])
    col = np.where((lab == 2).reshape(-1, 1), [0.9, 0.2, 0.2], [0.5, 0.5, 0.5])
    p = np.random.default_rng(7).permutation(len(xyz))
    return xyz[p].astype(F32), col[p].astype(F32), lab[p].astype(np.int32)


def voxel_coords(ses):
    return ses._scene_handle().coords.cpu().numpy().astype(np.int64)


def plates_of(coords):
    """Per plate the voxels whose 27-neighbourhood lies in that plate alone: two voxels or more from both other plates."""
    v = coords[:, 1:] - coords[:, 1:].min(0)
    return {"floor": (v[:, 2] == 0) & (v[:, 0] >= 2) & (v[:, 1] >= 2), "wall_x": (v[:, 0] == 0) & (v[:, 1] >= 2) & (v[:, 2] >= 2),
            "wall_y": (v[:, 1] == 0) & (v[:, 0] >= 2) & (v[:, 2] >= 2)}, v


def state_of(ses):
    manual = None if ses._manual is None else tuple(t.clone() for t in ses._manual)
    return ses.clicks(), ses._labels_qv.clone(), None if ses._labels_last is None else ses._labels_last.clone(), manual, ses.normals


def same_state(ses, before):
    clicks, labels_qv, labels_last, manual, normals = state_of(ses)
    assert clicks == before[0] and torch.equal(labels_qv, before[1]) and normals is before[4]
    assert (labels_last is None) == (before[2] is None) and (labels_last is None or torch.equal(labels_last, before[2]))
    assert (manual is None) == (before[3] is None) and (manual is None or all(torch.equal(a, b) for a, b in zip(manual, before[3])))


def same_patches(ses, got, keys=None, normals=None, feats=None, **settings):
    """A PatchesResult / WandResult's partition against the rule on the session's own rows."""
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    piece, rec = P.similar_numpy(coords, keys, normals, feats, got.connectivity, click_rows=ses._click_rows(), **settings)
    assert np.array_equal(got.piece_qv.cpu().numpy(), piece)
    if hasattr(got, "records"):
        assert got.n_pieces == len(rec) == len(got.records) and np.array_equal(got.piece_full.cpu().numpy(), piece[inv])
        for field in rec.dtype.names:                # root, key, voxels, clicked, lo, hi
            assert np.array_equal(got.records[field], rec[field]), field
    return piece, rec


def view_of(ses, w=96, h=72):
    """The room from above its open corner: the floor and both walls show."""
    return ses.render(intrinsic(w, h, 50.0), look_at([2.6, 2.2, 2.0], [0.5, 0.5, 0.2]), w, h, radius=0.03)


def pixel_showing(ses, view, voxels):
    """A pixel (u, v) of ``view`` whose vertex lies in one of ``voxels`` (a bool mask over the voxel rows), and that vertex."""
    ids, inv = view.ids.cpu().numpy(), ses.inverse_map.cpu().numpy()
    hit = np.argwhere((ids >= 0) & voxels[inv[np.maximum(ids, 0)]])
    assert len(hit)
    j, i = (int(a) for a in hit[len(hit) // 2])
    return i, j, int(ids[j, i])


def replay(ses, want):
    """infer() on logits whose arg-max is ``want`` (int [n_voxels], object ids that have a click)."""
    k = len(ses.click_idx)
    logits = np.full((len(want), k), -2.0, F32)
    logits[np.arange(len(want)), want] = 3.0
    return ses.infer(logits=torch.from_numpy(logits).to(DEV))


# ---------------------------------------------------------------------------------------------------- 1
def test_room(model_005, room):
    from agile3d_amd.session import PatchesResult, WandResult
    xyz, col, lab = room
    ses = _session(model_005, xyz, col, lab)
    view = view_of(ses)
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    inside, v = plates_of(coords)
    u0, v0, _ = pixel_showing(ses, view, inside["floor"])
    for call in (lambda: ses.patches(), lambda: ses.wand_at(view, u0, v0), lambda: ses.snap()):
        with pytest.raises(ValueError, match="estimate_normals"):
            call()
    feats = ses.colors_full[ses._unique_map].cpu().numpy()
    by_colour = ses.patches(normal_deg=None, color_tol=0.05)             # the colour test needs no normals
    same_patches(ses, by_colour, None, None, feats, tol2=F32(0.05) * F32(0.05))
    assert by_colour.cos_min is None and by_colour.tol2 == F32(0.05) * F32(0.05) and by_colour.n_pieces >= 2
    res = ses.estimate_normals()
    normals = res.normals_qv.cpu().numpy()
    before = state_of(ses)
    # ---- patches(): the rule; the plates
    r = ses.patches()
    assert isinstance(r, PatchesResult) and r.cos_min == F32(np.cos(np.radians(15.0))) and r.tol2 is None and r.within == "all"
    assert (r.normal_deg, r.color_tol, r.connectivity, r.oriented, r.object_pieces) == (15.0, None, 26, False, None)
    piece, rec = same_patches(ses, r, None, normals, None, cos_min=r.cos_min)
    roots = {}
    for name, mask in inside.items():
        assert mask.sum() > 300 and len(set(piece[mask].tolist())) == 1, name      # one patch holds the plate's inside
        roots[name] = int(piece[mask][0])
    assert len(set(roots.values())) == 3
    axis = {"floor": 2, "wall_x": 0, "wall_y": 1}
    for name, mask in inside.items():                                    # (the estimate is exact there: unit vectors along an axis)
        assert (np.abs(normals[mask][:, axis[name]]) == 1).all()
    print(f"room: {len(coords)} voxels, {r.n_pieces} patches, the plates' {[int(rec['voxels'][rec['root'] == x][0]) for x in roots.values()]}")
    same_patches(ses, ses.patches(normal_deg=40.0, color_tol=0.3, connectivity=6, oriented=True), None, normals, feats,
                 cos_min=F32(np.cos(np.radians(40.0))), tol2=F32(0.3) * F32(0.3), oriented=True)
    same_patches(ses, ses.patches(normals=res, within=(torch.from_numpy(v[:, 0] < 12).to(DEV))), np.where(v[:, 0] < 12, 0, -1), normals,
                 None, cos_min=r.cos_min)
    # ---- wand_at: the plate under the pixel
    wand = ses.wand_at(view, u0, v0)
    assert isinstance(wand, WandResult) and torch.equal(wand.piece_qv, r.piece_qv) and wand.mode == "chain"
    want = (r.piece_full == roots["floor"]).to(torch.uint8)
    assert torch.equal(wand.selected, want) and wand.count == int(want.sum()) > 1000
    assert wand.record.tobytes() == rec[rec["root"] == roots["floor"]][0].tobytes() and wand.record["voxels"] >= inside["floor"].sum()
    assert (lab[wand.selected.cpu().numpy() != 0] == 1).all()            # floor vertices only
    background = np.argwhere(view.ids.cpu().numpy() < 0)[0]
    assert ses.wand_at(view, int(background[1]), int(background[0])) is None
    row = int(inv[pixel_showing(ses, view, inside["floor"])[2]])
    seed = ses.wand_at(view, u0, v0, mode="seed")
    same_patches(ses, seed, None, normals, None, cos_min=F32(-1), ref_normal=normals[row], ref_cos_min=r.cos_min)
    assert seed.record["root"] == seed.piece_qv[row] and seed.count >= wand.count
    both = ses.wand_at(view, u0, v0, mode="both", color_tol=0.05, connectivity=6)
    same_patches(ses, both, None, normals, feats, cos_min=r.cos_min, tol2=F32(0.05) * F32(0.05), ref_normal=normals[row],
                 ref_cos_min=r.cos_min, ref_feat=feats[row], ref_tol2=F32(0.05) * F32(0.05))
    assert torch.equal(both.selected, wand.selected)
    grey = ses.wand_at(view, u0, v0, normal_deg=None, color_tol=0.05, mode="seed")        # everything of this colour around here
    same_patches(ses, grey, None, None, feats, tol2=np.finfo(F32).max, ref_feat=feats[row], ref_tol2=F32(0.05) * F32(0.05))
    picked = grey.selected.cpu().numpy() != 0                           # (a voxel on the crease has the colour of one of its vertices)
    assert picked[lab == 1].mean() > 0.9 and picked[lab == 3].mean() > 0.9 and picked[lab == 2].mean() < 0.1
    masked = ses.wand_at(view, u0, v0, within=torch.from_numpy(v[:, 0] >= 12).to(DEV)) if v[row, 0] < 12 else None
    assert masked is None or (masked.count == 0 and masked.record is None and not masked.selected.any())
    # ---- grow_at within the patches stays on the plate; walking anywhere leaves it
    on_plate = ses.grow_at(view, u0, v0, steps=60, within=r.piece_qv)
    anywhere = ses.grow_at(view, u0, v0, steps=60, within="all")
    assert torch.equal(on_plate.selected, wand.selected) and anywhere.count > on_plate.count
    same_state(ses, before)
    # ---- paint, erase, grow and shrink take the wand
    ses.click(xyz[np.flatnonzero(lab == 1)[0]], 1)
    assert ses.paint(wand, 1) == wand.count and ses.corrected().overridden == wand.count
    assert ses.erase(wand) == wand.count
    assert ses.grow(wand, steps=1).count > wand.count > ses.shrink(wand, steps=1).count > 0
    with pytest.raises(ValueError, match="mode"):
        ses.wand_at(view, u0, v0, mode="flood")
    for bad in (dict(normal_deg=-1.0), dict(normal_deg=float("nan")), dict(color_tol=-0.1), dict(connectivity=5), dict(within="object"),
                dict(normals="mine"), dict(normals=res.normals_qv), dict(oriented=2)):
        with pytest.raises(ValueError):
            ses.patches(**bad)
    other = _session(model_005, xyz[:2000], col[:2000])
    with pytest.raises(ValueError, match="NormalsResult of this scene"):
        other.patches(normals=res)


# ---------------------------------------------------------------------------------------------------- 2
def test_scan(model_005):
    from agile3d_amd.ply import read_ply
    p = read_ply(os.path.join(GOLDEN, "data", "scans", "scene0001_00.ply"))
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(F32)
    col = (np.stack([p["R"], p["G"], p["B"]], 1) / 255.0).astype(F32)
    ses = _session(model_005, xyz, col)
    res = ses.estimate_normals()
    normals, feats = res.normals_qv.cpu().numpy(), ses.colors_full[ses._unique_map].cpu().numpy()
    before = state_of(ses)
    r = ses.patches()
    piece, rec = same_patches(ses, r, None, normals, None, cos_min=r.cos_min)
    print(f"scan: {len(piece)} voxels, {r.n_pieces} patches at 15 degrees, largest {rec['voxels'].max()}, {(rec['voxels'] == 1).sum()} singletons")
    assert rec["voxels"].max() > 20
    half = torch.from_numpy(np.arange(len(piece)) % 3).to(torch.int32).to(DEV) - 1            # keys -1, 0, 1
    r = ses.patches(normal_deg=25.0, color_tol=0.2, connectivity=18, within=half)
    same_patches(ses, r, half.cpu().numpy(), normals, feats, cos_min=F32(np.cos(np.radians(25.0))), tol2=F32(0.2) * F32(0.2))
    assert r.within == "keys" and (r.piece_qv[half < 0] == -1).all()
    r = ses.patches(within="label")
    same_patches(ses, r, ses._labels_qv.cpu().numpy(), normals, None, cos_min=r.cos_min)
    assert r.object_pieces.tolist() == [r.n_pieces]
    same_state(ses, before)


# ---------------------------------------------------------------------------------------------------- 3
def test_snap(model_005, room):
    from agile3d_amd.session import SnapResult
    xyz, col, lab = room
    ses = _session(model_005, xyz, col, lab)
    coords = voxel_coords(ses)
    inside, v = plates_of(coords)
    res = ses.estimate_normals()
    ori = ses.labels_qv_ori.cpu().numpy()
    ses.click(xyz[np.flatnonzero((lab == 1) & (xyz[:, 0] > 1.0) & (xyz[:, 1] > 1.0))[0]], 1)
    ses.click(xyz[np.flatnonzero((lab == 2) & (xyz[:, 2] > 0.5) & (xyz[:, 1] > 0.5))[0]], 2)
    # the floor is object 1, the walls object 2 -- and the boundary pushed three voxels across the floor
    truth = np.where(ori == 1, 1, 2)
    pushed = (ori == 1) & (v[:, 0] >= 2) & (v[:, 0] <= 4)
    want = np.where(pushed, 2, truth)
    replay(ses, want)
    labels = ses._labels_qv.cpu().numpy()
    assert (labels[pushed] == 2).all() and pushed.sum() > 50
    before = state_of(ses)
    r = ses.patches()
    piece = r.piece_qv.cpu().numpy()
    s = ses.snap(r)
    assert isinstance(s, SnapResult) and (s.min_voxels, s.min_share) == (8, (2, 3))
    out, rule = P.vote_numpy(piece, labels, 8, (2, 3), ses._click_rows())
    assert np.array_equal(s.labels_qv.cpu().numpy(), out) and {k: getattr(s, k) for k in rule if k != "err"} == {k: rule[k] for k in rule if k != "err"}
    snapped = s.labels_qv.cpu().numpy()
    assert (snapped[inside["floor"]] == 1).all() and (snapped[inside["wall_x"]] == 2).all()        # straightened
    assert s.relabelled_pieces >= 1 and s.relabelled_voxels >= (pushed & inside["floor"]).sum() > 50 and s.blocked_pieces == 0
    assert torch.equal(s.labels_full, s.labels_qv[ses.inverse_map]) and tuple(s.colors.shape) == (len(xyz), 3)
    assert s.miou is not None and len(s.iou_per_object) >= 2
    default = ses.snap()                                                 # patches() computed here
    assert torch.equal(default.labels_qv, s.labels_qv) and default.relabelled_voxels == s.relabelled_voxels
    strict = ses.snap(r, min_share=(65536, 65536))
    assert np.array_equal(strict.labels_qv.cpu().numpy(), labels) and strict.below_share_pieces >= 1 and strict.relabelled_pieces == 0
    huge = ses.snap(r, min_voxels=10 ** 6)
    assert huge.eligible_pieces == 0 and np.array_equal(huge.labels_qv.cpu().numpy(), labels)
    same_state(ses, before)
    for bad in (dict(patches=ses.pieces()), dict(patches=r.piece_qv), dict(min_voxels=0), dict(min_share=(3, 2)), dict(min_share=0.66),
                dict(min_share=(1, 1 << 17))):
        with pytest.raises(ValueError):
            ses.snap(**bad)
    # ---- an opposing click: the user says the pushed band IS object 2 there; the floor's patch is left alone
    at = np.flatnonzero(pushed & inside["floor"])[0]
    ses.click(xyz[int(ses._unique_map[at])], 2)
    replay(ses, want)
    labels = ses._labels_qv.cpu().numpy()
    assert labels[at] == 2 and at in ses._click_rows()
    r = ses.patches()
    piece = r.piece_qv.cpu().numpy()
    s = ses.snap(r)
    out, rule = P.vote_numpy(piece, labels, 8, (2, 3), ses._click_rows())
    assert np.array_equal(s.labels_qv.cpu().numpy(), out) and s.blocked_pieces == rule["blocked_pieces"] >= 1
    assert np.array_equal(s.labels_qv.cpu().numpy()[piece == piece[at]], labels[piece == piece[at]]) and (labels[piece == piece[at]] == 1).sum() > 300


# ---------------------------------------------------------------------------------------------------- 4
def test_a_mesh_needs_normals(model_005, tmp_path):
    from agile3d_amd.session import InteractiveSession
    folder = tmp_path / "scene_small"
    os.makedirs(folder)
    shutil.copy(os.path.join(GOLDEN, "data", "mesh_small.ply"), folder / "scan.ply")
    ses = InteractiveSession(model_005, voxel_size=VS).load_scene_dir(str(folder))
    assert ses.faces is not None
    k, e = ses.default_view(64, 48)
    view = ses.render(k, e, 64, 48, lit=True)                            # (a mesh's own vertex normals are in ses.normals now)
    res = ses.estimate_normals()
    before = state_of(ses)
    hit = np.argwhere(view.ids.cpu().numpy() >= 0)[0]
    for call in (lambda: ses.patches(), lambda: ses.wand_at(view, int(hit[1]), int(hit[0])), lambda: ses.snap()):
        with pytest.raises(ValueError, match="normals="):
            call()
    r = ses.patches(normals=res)
    same_patches(ses, r, None, res.normals_qv.cpu().numpy(), None, cos_min=r.cos_min)
    wand = ses.wand_at(view, int(hit[1]), int(hit[0]), normals=res)
    vertex = ses._vertex_at(view, int(hit[1]), int(hit[0]))
    root = int(r.piece_full[vertex])
    assert torch.equal(wand.selected, ((r.piece_full == root) & (root >= 0)).to(torch.uint8)) and wand.count == int(wand.selected.sum())
    assert ses.snap(r).eligible_pieces >= 0
    same_state(ses, before)
