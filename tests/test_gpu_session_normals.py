"""-m gpu: normals for point clouds through the session (InteractiveSession.estimate_normals, normal_at; render(lit=True),
Section(cull=) on a cloud).  The rules are restated in ``normals_rule.py`` and ``shade_points_rule.py`` and applied to the
session's own voxel rows, inverse map and fixed-point frame; the normals are compared by their bytes.

1  before estimate_normals(): a cloud's lit=True is the depth shade, a culling section raises as it always did
2  after it, on a synthetic room (a closed box of points) and on the committed scan: the result against the rule; lit=True is
   the composition of the library calls and the rule's bytes; cloud_shade="depth" gives the old bytes; cull="back" is accepted
   by set_section, render, pick, click_ray and select; the culled render is the composition; pick_from_render == pick on 64
   sampled pixels; select sees only the shown vertices; normal_at on a hit and on the background
3  load_scene drops the normals, reset keeps them; viewpoints; on a mesh the result is returned and nothing changes
"""
import os
import shutil

import numpy as np
import pytest
import torch

import normals_rule as R
import shade_points_rule as SP
from agile3d_amd import view as V
from conftest import GOLDEN
from render_rule import camera_fields, pixel_rays
from session_kit import DEV, _model, intrinsic, look_at, sampled_pixels

pytestmark = pytest.mark.gpu
VS = 0.05
BG = (0.1, 0.2, 0.3)
F32 = np.float32


@pytest.fixture(scope="module")
def model_005():
    return _model(VS)


def _session(model, xyz, col, faces=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, None, faces=faces)


@pytest.fixture(scope="module")
def room():
    """A closed box of points, 1.2 m a side around (5, -3, 1): 24 x 24 jittered points a wall, about one a voxel."""
    k, half = 24, 0.6
    rng = np.random.default_rng(4)
    g = (np.arange(k) + 0.5) / k * 2 * half - half
    a, b = np.meshgrid(g, g, indexing="ij")
    pts = []
    for axis in range(3):
        for side in (-half, half):
            p = np.empty((k, k, 3))
            p[..., axis], p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = side, a, b
            pts.append(p.reshape(-1, 3))
    xyz = np.concatenate(pts) + rng.uniform(-0.004, 0.004, (6 * k * k, 3)) + (5.0, -3.0, 1.0)
    perm = rng.permutation(len(xyz))
    return xyz[perm].astype(F32), rng.uniform(0.2, 1.0, (len(xyz), 3)).astype(F32)


@pytest.fixture(scope="module")
def scan():
    """The committed scan tests/golden/data/scans/scene0001_00.ply: 4 416 points of a real scene."""
    from agile3d_amd.ply import read_ply
    v = read_ply(os.path.join(GOLDEN, "data", "scans", "scene0001_00.ply"))
    xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(F32)
    return xyz, (np.stack([v["R"], v["G"], v["B"]], 1) / 255.0).astype(F32)


def outside_view(xyz, w=64, h=48):
    centre = 0.5 * (xyz.min(0) + xyz.max(0)).astype(np.float64)
    reach = float(np.linalg.norm(xyz.max(0) - xyz.min(0)))
    return intrinsic(w, h, 45.0), look_at(centre + np.array([1.1, 0.8, 0.6]) * reach, centre), w, h


def voxel_coords(ses):
    return ses._scene_handle().coords.cpu().numpy().astype(np.int64)


def rule_of(ses, viewpoint):
    origin, quantum, bits = ses._fixed_point_frame()
    return R.estimate(voxel_coords(ses), ses.coords_full.cpu().numpy(), ses.inverse_map.cpu().numpy(), origin, quantum, bits, viewpoint)


def same_result(res, want):
    for name, key in (("normals_full", "normal_full"), ("normals_qv", "normal_qv"), ("variation_qv", "variation_qv"), ("count_qv", "count_qv")):
        got = getattr(res, name).cpu().numpy()
        assert got.dtype == want[key].dtype and got.tobytes() == want[key].tobytes(), name
    s = want["summary"]
    assert (res.counted, res.valid, res.invalid, res.err) == (s["counted"], s["valid"], s["invalid"], s["err"])


# ---------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("which", ["room", "scan"])
def test_a_cloud_before_and_after(model_005, room, scan, which):
    from agile3d_amd.session import Section
    xyz, col = room if which == "room" else scan
    ses = _session(model_005, xyz, col)
    k, e, w, h = outside_view(xyz)
    back = Section(cull="back")
    cut = Section([((0.0, 0.0, -1.0), -float(xyz[:, 2].max()) + 0.01)], cull="back")      # the top centimetre off, and culled
    # ---- before: today's code, error messages included
    assert ses.normals is None
    flat = ses.render(k, e, w, h, background=BG)
    depth = ses.render(k, e, w, h, background=BG, lit=True)
    assert torch.equal(depth.rgb, V.render_shade_depth(flat.ids, flat.t, None, None, None, ses.colors_full, 8.0, BG))
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True, cloud_shade="depth").rgb, depth.rgb)
    for call in (lambda: ses.render(k, e, w, h, section=back), lambda: ses.pick([0, 0, 0], [1, 0, 0], section=back),
                 lambda: ses.click_ray([0, 0, 0], [1, 0, 0], 1, section=back), lambda: ses.render(k, e, w, h, section=cut)):
        with pytest.raises(ValueError, match="only a mesh has faces to cull"):
            call()
    with pytest.raises(ValueError, match="estimate_normals"):
        ses.normal_at(flat, 0, 0)
    with pytest.raises(ValueError, match="cloud_shade"):
        ses.render(k, e, w, h, cloud_shade="flat")
    # ---- the estimate against the rule
    res = ses.estimate_normals()
    origin = ses._fixed_point_frame()[0]
    assert np.array_equal(res.viewpoint, origin) and ses.normals is res.normals_full and res.err == 0
    want = rule_of(ses, origin)
    same_result(res, want)
    n_full = len(xyz)
    assert res.counted == n_full and res.valid > 0.5 * (res.valid + res.invalid)
    if which == "room":                                                   # every wall looks at the centre of the room
        nf = res.normals_full.cpu().numpy().astype(np.float64)
        assert ((nf * (origin - xyz)).sum(1) > 0).mean() > 0.99
    # ---- lit: the composition of the library calls, the rule's bytes; the depth shade on request; flat unchanged
    lit = ses.render(k, e, w, h, background=BG, lit=True)
    assert lit.lit and torch.equal(lit.ids, flat.ids) and torch.equal(lit.t, flat.t)
    assert torch.equal(lit.rgb, V.render_shade_lit_points(flat.ids, ses.colors_full, ses.normals, lit.camera, 0.35, BG))
    ids = flat.ids.cpu().numpy()
    assert np.array_equal(lit.rgb.cpu().numpy(), SP.lit_points_rule(ids, col, want["normal_full"], lit.camera, 0.35, BG))
    assert not torch.equal(lit.rgb, depth.rgb) and not torch.equal(lit.rgb, flat.rgb) and (ids >= 0).sum() > 100
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True, cloud_shade="depth").rgb, depth.rgb)
    assert torch.equal(ses.render(k, e, w, h, background=BG).rgb, flat.rgb)
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True, ambient=1.0).rgb, flat.rgb)
    # ---- culling: accepted; the render is the library's composition for the camera's centre
    eye = np.array(lit.camera.o[:], F32)
    for sec in (back, cut, Section(cull="front")):
        got = ses.render(k, e, w, h, background=BG, section=sec)
        culled, hidden, _ = V.cull_points(ses.coords_full, ses.normals, eye, sec.cull)
        if sec.n_planes:
            ids_want, t_want, _ = V.render_points_section(culled, VS, got.camera, sec.with_cull("none").struct(), capacity=1 << 18)
        else:
            ids_want, t_want, _ = V.render_points(culled, VS, got.camera, capacity=1 << 18)
        assert torch.equal(got.ids, ids_want) and torch.equal(got.t, t_want) and got.section is sec
        shown = got.ids[got.ids >= 0].long()
        assert len(shown) > 50 and not hidden[shown].any() and 0 < int(hidden.sum()) < n_full
        assert sec.n_planes == 0 or sec.keeps(xyz[shown.cpu().numpy()]).all()
    assert len(ses._culled) == 2                                           # one copy per eye and mode: back (twice used) and front
    # ---- the image is what a click through the pixel picks, under the session's own section
    ses.set_section(back)
    view = ses.render(k, e, w, h, background=BG)
    assert view.section is back and not torch.equal(view.ids, flat.ids)
    o32, d = camera_fields(view.camera)[0], pixel_rays(view.camera)
    vids = view.ids.cpu().numpy()
    hits = 0
    for i, j in sampled_pixels(w, h, 64):
        got = ses.pick_from_render(view, i, j)
        assert (got is not None) == bool(vids[j, i] >= 0) and got == ses.pick(o32, d[j, i]), (i, j)
        hits += got is not None
    assert hits >= 5
    j, i = (int(a) for a in np.argwhere(vids >= 0)[len(np.argwhere(vids >= 0)) // 2])
    assert ses.click_ray(o32, d[j, i], 1) is not None and ses.num_clicks == 1
    # ---- select sees only the vertices the culled view shows
    mask = torch.ones((h, w), dtype=torch.uint8, device=DEV)
    everything = ses.select(view, mask, through=True, section=None)
    culled_sel = ses.select(view, mask, through=True)
    hidden = V.cull_points(ses.coords_full, ses.normals, eye, "back")[1]
    assert torch.equal(culled_sel.selected, everything.selected & (1 - hidden)) and 0 < culled_sel.count < everything.count
    visible = ses.select(view, mask)                                      # (a vertex's test looks at that vertex alone)
    assert torch.equal(visible.selected, ses.select(view, mask, section=None).selected & (1 - hidden))
    assert 0 < visible.count <= culled_sel.count and not (visible.selected & (1 - culled_sel.selected)).any()
    # ---- normal_at: a hit, the background
    normal, variation = ses.normal_at(view, i, j)
    vertex = int(vids[j, i])
    assert normal.tobytes() == want["normal_full"][vertex].tobytes() and variation == float(want["variation_qv"][int(ses.inverse_map[vertex])])
    jb, ib = (int(a) for a in np.argwhere(vids < 0)[0])
    assert ses.normal_at(view, ib, jb) is None and ses.normal_at(view, i, j, normals=res)[0].tobytes() == normal.tobytes()
    # ---- reset keeps the normals (and the section); load_scene drops them
    ses.reset()
    assert ses.normals is res.normals_full and ses.section is back and ses.num_clicks == 0
    assert torch.equal(ses.render(k, e, w, h, background=BG).ids, view.ids)
    ses.load_scene(xyz, col)
    assert ses.normals is None and ses._normals_last is None and ses._culled == {} and ses.section is None
    with pytest.raises(ValueError, match="only a mesh has faces to cull"):
        ses.render(k, e, w, h, section=back)
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True).rgb, depth.rgb)


# ---------------------------------------------------------------------------------------------------- 3
def test_viewpoints(model_005, room):
    xyz, col = room
    ses = _session(model_005, xyz, col)
    first = ses.estimate_normals(viewpoint=None)
    same_result(first, rule_of(ses, None))
    n = first.normals_qv.cpu().numpy()
    valid = np.abs(n).sum(1) > 0
    assert (n[valid][np.arange(valid.sum()), np.abs(n[valid]).argmax(1)] > 0).all() and first.viewpoint is None
    far = ses.estimate_normals(viewpoint=[50.0, -3.0, 1.0])
    same_result(far, rule_of(ses, (50.0, -3.0, 1.0)))
    assert ses.normals is far.normals_full and ses._normals_last is far and ses._culled == {}
    assert torch.equal(far.normals_qv.abs(), first.normals_qv.abs()) and not torch.equal(far.normals_qv, first.normals_qv)
    again = ses.estimate_normals(viewpoint=[50.0, -3.0, 1.0])
    assert torch.equal(again.normals_full, far.normals_full) and torch.equal(again.variation_qv, far.variation_qv)
    for bad in ("center", [0.0, 1.0], [0.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match="viewpoint"):
            ses.estimate_normals(viewpoint=bad)
    other = _session(model_005, xyz[:1000], col[:1000])
    k, e, w, h = outside_view(xyz)
    with pytest.raises(ValueError, match="another scene"):
        other.normal_at(other.render(k, e, w, h), 0, 0, normals=far)


def test_a_mesh_is_left_alone(model_005, tmp_path):
    """On a mesh the result is returned and no session state changes: a later render(lit=True) is byte-identical to one taken
    before the call, and culling stays that of the faces."""
    from agile3d_amd.session import InteractiveSession, Section
    folder = tmp_path / "scene_small"
    os.makedirs(folder)
    shutil.copy(os.path.join(GOLDEN, "data", "mesh_small.ply"), folder / "scan.ply")
    ses = InteractiveSession(model_005, voxel_size=VS).load_scene_dir(str(folder))
    assert ses.faces is not None
    k, e = ses.default_view(64, 48)
    before = ses.render(k, e, 64, 48, lit=True)
    culled = ses.render(k, e, 64, 48, section=Section(cull="back"))
    mesh_normals = ses.normals
    res = ses.estimate_normals()
    same_result(res, rule_of(ses, ses._fixed_point_frame()[0]))
    assert ses.normals is mesh_normals and ses._normals_last is None and ses._culled == {}
    after = ses.render(k, e, 64, 48, lit=True)
    assert torch.equal(after.rgb, before.rgb) and torch.equal(after.ids, before.ids)
    assert torch.equal(ses.render(k, e, 64, 48, section=Section(cull="back")).ids, culled.ids)
    with pytest.raises(ValueError, match="only a mesh has faces to cull"):
        ses.pick([0, 0, 0], [1, 0, 0], surface=False, section=Section(cull="back"))
    hit = np.argwhere(before.ids.cpu().numpy() >= 0)[0]
    with pytest.raises(ValueError, match="estimate_normals"):
        ses.normal_at(before, int(hit[1]), int(hit[0]))
    normal, variation = ses.normal_at(before, int(hit[1]), int(hit[0]), normals=res)
    vertex = ses._vertex_at(before, int(hit[1]), int(hit[0]))
    assert normal.tobytes() == res.normals_full[vertex].cpu().numpy().tobytes() and 0.0 <= variation <= 1 / 3 + 1e-6
