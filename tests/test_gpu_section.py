"""The section on the GPU: a3d_pick_ray_section, a3d_pick_mesh_section, a3d_render_mesh_section, a3d_render_points_section
(view.*_section) and InteractiveSession.set_section, held to the numpy restatement of ``section_rule.py`` bit for bit.

1  facing: one triangle, both windings, rays of every dominant axis and sign
2  the room: a closed box that faces inwards around a triangle, seen from outside -- culled, and cut by a plane
3  pick = render, pixel by pixel, on the room and on a lattice of points
4  boundaries: a plane through a layer of the lattice, a crossing exactly on both ends of an interval, a parallel ray
5  the camera inside the box (primitives every pixel tests)
6  no section = the calls without one, byte for byte
7  through the session
"""
import numpy as np
import pytest
import torch

import section_rule as R
import session_kit
from agile3d_amd import lib as L
from agile3d_amd import view as V
from pick_rule import F32
from session_kit import DEV, _dev, bits, camera_of

pytestmark = pytest.mark.gpu


def section(planes=(), cull=0):
    s = L.Section()
    s.n_planes, s.cull = len(planes), cull
    for k, p in enumerate(planes):
        s.planes[k][:] = [float(x) for x in p]
    return s


PLAIN = object()                               # "the call without a section", where a test compares the two


def pick_mesh(xyz, faces, rays, sec):
    """a3d_pick_mesh_section (``sec`` a lib.Section or None = NULL) or a3d_pick_mesh (``PLAIN``) for every ray: records."""
    xyz_dev, faces_dev = _dev(xyz, F32), _dev(np.asarray(faces).reshape(-1, 3), np.int32)
    out = torch.full((max(len(rays), 1) * 8,), -7, dtype=torch.int32, device=DEV)
    ws = V.session_workspace(DEV)
    for i, (o, d) in enumerate(rays):
        if sec is PLAIN:
            V.pick_mesh(xyz_dev, faces_dev, o, d, out=out[8 * i:8 * i + 8], workspace=ws)
        else:
            V.pick_mesh_section(xyz_dev, faces_dev, o, d, sec, out=out[8 * i:8 * i + 8], workspace=ws)
    return V.read_pick_mesh(out.cpu().numpy())[:len(rays)]


def pick_ray(xyz, rays, r, sec):
    """a3d_pick_ray_section / a3d_pick_ray for every ray: int32 [k, 4] result records as they are."""
    xyz_dev = _dev(xyz, F32)
    out = torch.full((max(len(rays), 1), 4), -7, dtype=torch.int32, device=DEV)
    ws = V.session_workspace(DEV)
    for i, (o, d) in enumerate(rays):
        if sec is PLAIN:
            V.pick_ray(xyz_dev, o, d, r, out=out[i], workspace=ws)
        else:
            V.pick_ray_section(xyz_dev, o, d, r, sec, out=out[i], workspace=ws)
    return out.cpu().numpy()[:len(rays)]


def render(xyz, faces, cam, sec, radius=None):
    """a3d_render_mesh_section / a3d_render_points_section (``faces`` None), or the calls without a section (``PLAIN``);
    the images start as sentinels."""
    h, w = cam.height, cam.width
    xyz_dev = _dev(np.asarray(xyz, F32).reshape(-1, 3), F32)
    ids = torch.full((h, w), -7, dtype=torch.int32, device=DEV)
    t, u, v = (torch.full((h, w), -7.0, dtype=torch.float32, device=DEV) for _ in range(3))
    header = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    if faces is not None:
        faces_dev = _dev(np.asarray(faces).reshape(-1, 3), np.int32)
        if sec is PLAIN:
            V.render_mesh(xyz_dev, faces_dev, cam, ids, t, u, v, header=header)
        else:
            V.render_mesh_section(xyz_dev, faces_dev, cam, sec, ids, t, u, v, header=header)
    elif sec is PLAIN:
        V.render_points(xyz_dev, float(radius), cam, ids, t, header)
    else:
        V.render_points_section(xyz_dev, float(radius), cam, sec, ids, t, header)
    flags, n_everywhere, pairs = V.read_render_header(header.cpu().numpy())
    return dict(ids=ids.cpu().numpy(), t=t.cpu().numpy(), u=u.cpu().numpy(), v=v.cpu().numpy(), flags=flags,
                n_everywhere=n_everywhere)


def same_mesh_images(got, want):
    face, t, u, v = want
    assert np.array_equal(got["ids"], face)
    assert np.array_equal(bits(got["t"]), bits(t)) and np.array_equal(bits(got["u"]), bits(u)) and np.array_equal(bits(got["v"]), bits(v))


def pixel_rays_of(cam):
    from render_rule import camera_fields, pixel_rays
    o, d = camera_fields(cam)[0], pixel_rays(cam)
    return [(o, d[j, i]) for j in range(cam.height) for i in range(cam.width)]


# ------------------------------------------------------------------------------------------- 1: facing
def test_facing():
    """Twelve picks: A3D_CULL_BACK keeps exactly the rays with g . d < 0 (float64), A3D_CULL_FRONT the rest."""
    fronts = 0
    for xyz, faces, o, d in R.facing_rays():
        a, b, c = xyz[faces[0]].astype(np.float64)
        front = float(np.cross(b - a, c - a) @ d.astype(np.float64)) < 0
        fronts += front
        plain = pick_mesh(xyz, faces, [(o, d)], PLAIN)[0]
        assert plain["face"] == 0
        for cull, shows in ((L.A3D_CULL_NONE, True), (L.A3D_CULL_BACK, front), (L.A3D_CULL_FRONT, not front)):
            got = pick_mesh(xyz, faces, [(o, d)], section(cull=cull))[0]
            if shows:
                assert got.tobytes() == plain.tobytes(), (cull, d)
            else:
                assert got["face"] == -1 and got["t"] == 0 and got["flags"] == 0, (cull, d)
    assert fronts == 6


# ------------------------------------------------------------------------------------------- 2: the room
OUTSIDE = ([0.3, -4.0, 0.6], [0.0, 0.0, 0.0], 50.0)       # eye, target, fov: looks at the wall y = -1 from outside


def test_the_room_from_outside():
    xyz, faces = R.room()
    cam = camera_of(*OUTSIDE, (40, 24))                    # 3 x 2 tiles, the last column 8 pixels wide
    plain = render(xyz, faces, cam, PLAIN)
    assert plain["flags"] == 0 and (plain["ids"] >= 0).sum() > 200 and (plain["ids"] < 0).any()
    assert not (plain["ids"] == R.INNER).any() and set(np.unique(plain["ids"])) <= {-1, *range(12)}
    cases = {"culled": ((), L.A3D_CULL_BACK), "cut": ([(0, 1, 0, -0.5)], L.A3D_CULL_NONE),
             "cut and culled": ([(0, 1, 0, -0.5), (0, 0, -1, -0.75)], L.A3D_CULL_BACK)}
    for name, (planes, cull) in cases.items():
        got = render(xyz, faces, cam, section(planes, cull))
        assert got["flags"] == 0 and (got["ids"] == R.INNER).sum() > 20, name
        same_mesh_images(got, R.render_mesh_section_rule(xyz, faces, cam, np.array(planes, F32).reshape(-1, 4), cull))
        assert not np.array_equal(got["ids"], plain["ids"])
    # front-face culling leaves the near wall and what else turns its back: the inner triangle is gone
    got = render(xyz, faces, cam, section(cull=L.A3D_CULL_FRONT))
    same_mesh_images(got, R.render_mesh_section_rule(xyz, faces, cam, np.zeros((0, 4), F32), L.A3D_CULL_FRONT))
    assert np.array_equal(got["ids"], plain["ids"])        # (from outside the first surface of every ray is a back face)


# ------------------------------------------------------------------------------------------- 3: pick = render
def test_pick_is_render_on_the_room():
    xyz, faces = R.room()
    cam = camera_of(*OUTSIDE, (12, 10))
    planes, cull = [(0, 1, 0, -0.5), (0.6, 0, -0.8, -0.5)], L.A3D_CULL_BACK
    sec = section(planes, cull)
    image = render(xyz, faces, cam, sec)
    same_mesh_images(image, R.render_mesh_section_rule(xyz, faces, cam, np.array(planes, F32), cull))
    assert (image["ids"] == R.INNER).any() and (image["ids"] < 0).any() and len(np.unique(image["ids"])) >= 4
    picks = pick_mesh(xyz, faces, pixel_rays_of(cam), sec).reshape(10, 12)
    hit = image["ids"] >= 0
    assert np.array_equal(picks["face"], image["ids"]) and not picks["flags"].any()
    for k in "tuv":
        assert np.array_equal(bits(picks[k])[hit], bits(image[k])[hit]), k
    assert not picks["t"][~hit].any() and np.isinf(image["t"][~hit]).all()


CLOUD_VIEW = ([0.2, -3.0, 0.4], [0.0, 0.0, 0.0], 28.0)


def test_pick_is_render_on_a_lattice_of_points():
    xyz = R.grid_cloud()
    cam = camera_of(*CLOUD_VIEW, (12, 10))
    planes = [(0, 1, 0, -0.25), (0, 0, -1, -0.25)]         # both through layers of the lattice
    sec = section(planes)
    image = render(xyz, None, cam, sec, radius=0.06)
    index, t = R.render_points_section_rule(xyz, 0.06, cam, np.array(planes, F32))
    assert np.array_equal(image["ids"], index) and np.array_equal(bits(image["t"]), bits(t))
    shown = index[index >= 0]
    assert len(np.unique(shown)) >= 6 and (index < 0).any()
    assert (xyz[shown, 1] >= -0.25).all() and (xyz[shown, 2] <= 0.25).all() and (xyz[shown, 1] == -0.25).any()
    assert not np.array_equal(render(xyz, None, cam, PLAIN, radius=0.06)["ids"], index)
    picks = pick_ray(xyz, pixel_rays_of(cam), 0.06, sec).reshape(10, 12, 4)
    assert np.array_equal(picks[..., 0], index)
    hit = index >= 0
    assert np.array_equal(picks[hit][:, 1:].view(F32), xyz[index[hit]]) and not picks[~hit][:, 1:].any()


# ------------------------------------------------------------------------------------------- 4: boundaries
def test_a_plane_through_a_layer_keeps_the_layer():
    """Seen from below, the lattice shows its layer z = -0.5 first (and higher layers through its gaps); the plane z >= 0
    passes exactly through the middle layer, which then shows first, with nothing from below it."""
    xyz = R.grid_cloud()
    cam = camera_of([0.05, -0.1, -4.0], [0.0, 0.0, 0.0], 20.0, (20, 18))
    plain = render(xyz, None, cam, PLAIN, radius=0.06)["ids"]
    assert (xyz[plain[plain >= 0], 2] == -0.5).sum() > 20
    planes = [(0, 0, 1, 0)]
    got = render(xyz, None, cam, section(planes), radius=0.06)
    index, t = R.render_points_section_rule(xyz, 0.06, cam, np.array(planes, F32))
    assert np.array_equal(got["ids"], index) and np.array_equal(bits(got["t"]), bits(t))
    assert (xyz[index[index >= 0], 2] >= 0.0).all() and (xyz[index[index >= 0], 2] == 0.0).sum() > 20


def test_a_crossing_on_the_ends_of_the_interval_counts():
    xyz, faces, o, d, t = R.exact_crossing()
    plain = pick_mesh(xyz, faces, [(o, d)], PLAIN)[0]
    assert plain["face"] == 0 and bits(plain["t"]) == bits(t)
    for planes in ([(0, 0, 1, 2)], [(0, 0, -1, -2)], [(0, 0, 1, 2), (0, 0, -1, -2)], [(1, 0, 0, 0.25)], [(-1, 0, 0, -0.25)]):
        lo, hi, empty = V.section_ray(section(planes), o, d)
        assert not empty and (bits(lo) == bits(t) or bits(hi) == bits(t) or planes[0][2] == 0)
        assert pick_mesh(xyz, faces, [(o, d)], section(planes))[0].tobytes() == plain.tobytes(), planes
    # cut away: in front of the interval, behind it, and by a plane the ray runs parallel to on its cut side
    for planes in ([(0, 0, 1, 2.5)], [(0, 0, -1, -1.5)], [(1, 0, 0, 1)], [(0, 0, 1, 2), (-1, 0, 0, 0)]):
        got = pick_mesh(xyz, faces, [(o, d)], section(planes))[0]
        assert got["face"] == -1 and got["t"] == 0 and not any(got[k] for k in "xyzuv"), planes
    # the same in the view: a camera whose pixel (0, 0) looks along +z from the ray's origin
    cam = L.Camera()
    cam.o[:], cam.d00[:], cam.du[:], cam.dv[:] = [float(x) for x in o], [0, 0, 1], [0.25, 0, 0], [0, 0.25, 0]
    cam.width, cam.height = 3, 2
    for planes, shows in (([(0, 0, 1, 2), (0, 0, -1, -2)], True), ([(0, 0, 1, 2.5)], False), ([(1, 0, 0, 1)], False)):
        got = render(xyz, faces, cam, section(planes))
        same_mesh_images(got, R.render_mesh_section_rule(xyz, faces, cam, np.array(planes, F32), 0))
        assert (got["ids"][0, 0] == 0) == shows and (not shows or bits(got["t"][0, 0]) == bits(t))


# ------------------------------------------------------------------------------------------- 5: the camera inside
def test_the_camera_inside_the_box():
    xyz, faces = R.room()
    # and a slanted face across the box whose bounding box holds the camera: no bound, every pixel tests it
    faces = np.concatenate([faces, [[len(xyz), len(xyz) + 1, len(xyz) + 2]]]).astype(np.int32)
    xyz = np.concatenate([xyz, np.array([[0.0, -1.0, -1.0], [0.0, 1.0, -1.0], [1.6, 0.0, 1.0]], F32)])
    cam = camera_of([0.3, -0.6, 0.1], [-0.2, 1.0, 0.2], 100.0, (24, 20))
    plain = render(xyz, faces, cam, PLAIN)
    assert plain["n_everywhere"] > 0 and (plain["ids"] == R.INNER).any()
    for planes, cull in (([(0, -1, 0, -0.5)], L.A3D_CULL_NONE), ((), L.A3D_CULL_FRONT), ([(0.8, 0, 0.6, -0.25)], L.A3D_CULL_BACK)):
        got = render(xyz, faces, cam, section(planes, cull))
        assert got["n_everywhere"] == plain["n_everywhere"] and got["flags"] == 0
        same_mesh_images(got, R.render_mesh_section_rule(xyz, faces, cam, np.array(planes, F32).reshape(-1, 4), cull))
        assert not np.array_equal(got["ids"], plain["ids"])


# ------------------------------------------------------------------------------------------- 6: no section
def test_no_section_is_the_call_without_one():
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-1, 1, (120, 3)).astype(F32)
    faces = rng.integers(0, 120, (200, 3)).astype(np.int32)
    cloud = rng.uniform(-1, 1, (500, 3)).astype(F32)
    cam = camera_of([0.2, -3.5, 0.5], [0.0, 0.0, 0.0], 45.0, (64, 48))
    rays = [pixel_rays_of(cam)[k] for k in rng.integers(0, 64 * 48, 12)]
    want_mesh, want_cloud = render(xyz, faces, cam, PLAIN), render(cloud, None, cam, PLAIN, radius=0.05)
    want_pm, want_pr = pick_mesh(xyz, faces, rays, PLAIN), pick_ray(cloud, rays, 0.05, PLAIN)
    assert (want_mesh["ids"] >= 0).sum() > 300 and (want_cloud["ids"] >= 0).sum() > 100
    assert (want_pm["face"] >= 0).sum() >= 3 and (want_pr[:, 0] >= 0).sum() >= 1
    junk = section()
    junk.planes[0][:] = [float("nan")] * 4                 # unused planes are not looked at
    for sec in (None, section(), junk):
        got = render(xyz, faces, cam, sec)
        for k in ("ids", "t", "u", "v"):
            assert got[k].tobytes() == want_mesh[k].tobytes(), k
        got = render(cloud, None, cam, sec, radius=0.05)
        assert got["ids"].tobytes() == want_cloud["ids"].tobytes() and got["t"].tobytes() == want_cloud["t"].tobytes()
        assert pick_mesh(xyz, faces, rays, sec).tobytes() == want_pm.tobytes()
        assert pick_ray(cloud, rays, 0.05, sec).tobytes() == want_pr.tobytes()


# ------------------------------------------------------------------------------------------- 7: the session
@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def _room_scene():
    """The room with loose vertices that no face uses: vertex 11 on the wall y = -1, where the rays of the test enter, and 40
    in a far corner (the voxelised scene has a few more rows)."""
    xyz, faces = R.room()
    rng = np.random.default_rng(2)
    loose = np.stack([rng.uniform(0.6, 0.9, 40), rng.uniform(0.6, 0.9, 40), rng.uniform(-0.9, -0.6, 40)], 1).astype(F32)
    xyz = np.concatenate([xyz, np.array([[0.0, -1.0, 0.5]], F32), loose])
    return xyz, faces, np.full((len(xyz), 3), 0.5, F32)


def test_through_the_session(model_005):
    from agile3d_amd.session import InteractiveSession, Section
    xyz, faces, col = _room_scene()
    ses = InteractiveSession(model_005, voxel_size=0.05)
    ses.load_scene(xyz, col, faces=faces)
    assert ses.section is None
    eye = np.array([0.0, -4.0, 0.25])
    ray = lambda target: (eye, np.asarray(target, np.float64) - eye)
    top, low = ray([0.0, 0.0, 0.45]), ray([0.0, 0.0, -0.45])   # at the inner triangle: near its apex (vertex 10), near its base
    # without a section the ray stops at the wall y = -1; under back-face culling it reaches the triangle
    wall = ses.pick(*top)
    assert abs(wall[1] + 1.0) < 1e-5 and ses.nearest(wall)[1] == 11
    assert ses.click_ray(*top, 1)[1] == 11 and ses.clicks()[0]["point"] == wall      # the click lands on the wall
    ses.reset()
    dollhouse = Section(cull="back")
    assert ses.set_section(dollhouse) is ses and ses.section is dollhouse
    inside = ses.pick(*top)
    assert abs(inside[1]) < 1e-6 and abs(inside[2] - 0.45) < 1e-3
    assert ses.pick(*top, section=Section()) == wall and ses.pick(*top, section=Section(cull="none")) == wall
    assert ses.click_ray(*top, 1)[1] == 10 and ses.clicks()[0]["point"] == inside
    assert ses.click_ray(*low, 2)[1] in (8, 9) and ses.num_clicks == 2
    # the view under the session's section, and under the caller's
    k, e = session_kit.intrinsic(48, 40, 40.0), session_kit.look_at(eye, [0.0, 0.0, 0.0])
    res = ses.render(k, e, 48, 40)
    assert res.section is dollhouse and (res.ids == R.INNER).any()
    want = R.render_mesh_section_rule(xyz, faces, res.camera, np.zeros((0, 4), F32), L.A3D_CULL_BACK)
    same_mesh_images(dict(ids=res.ids.cpu().numpy(), t=res.t.cpu().numpy(), u=res.u.cpu().numpy(), v=res.v.cpu().numpy()), want)
    plain = ses.render(k, e, 48, 40, section=Section())
    assert plain.section is None and not (plain.ids == R.INNER).any()
    # both clicks show their markers in the culled view; Section.below(0) cuts the upper one away
    pixel = lambda r, i: tuple(int(x) for x in np.rint(V.marker_table(r.camera, [ses.clicks()[i]["point"]], [[0, 0, 0]])[0, :2]))
    (u0, v0), (u1, v1) = pixel(res, 0), pixel(res, 1)
    assert ses.click_at(res, u0, v0) == 0 and ses.click_at(res, u1, v1) == 1
    shown = ses.annotate(res, outlines=False)
    assert not torch.equal(shown[v0, u0], res.rgb[v0, u0]) and not torch.equal(shown[v1, u1], res.rgb[v1, u1])
    cut = ses.render(k, e, 48, 40, section=Section.below(0.0, cull="back"))
    assert cut.section.n_planes == 1 and (cut.ids == R.INNER).any() and int(cut.ids[v0, u0]) != R.INNER
    assert ses.click_at(cut, u0, v0) is None and ses.click_at(cut, u1, v1) == 1
    shown = ses.annotate(cut, outlines=False)
    assert torch.equal(shown[v0 - 6:v0 + 7, u0 - 6:u0 + 7], cut.rgb[v0 - 6:v0 + 7, u0 - 6:u0 + 7])
    assert not torch.equal(shown[v1, u1], cut.rgb[v1, u1])
    # a cloud has no faces to cull
    with pytest.raises(ValueError):
        ses.pick(*top, surface=False)
    with pytest.raises(TypeError):
        ses.set_section("back")
    # reset keeps the section, load_scene drops it
    ses.reset()
    assert ses.section is dollhouse and ses.num_clicks == 0 and ses.pick(*top) == inside
    ses.load_scene(xyz, col)
    assert ses.section is None
    ses.set_section(dollhouse)
    with pytest.raises(ValueError):
        ses.render(k, e, 48, 40)
    with pytest.raises(ValueError):
        ses.click_ray(*top, 1)
    ses.set_section(Section.box([-2, -0.25, -2], [2, 2, 2]))
    got = ses.render(k, e, 48, 40, radius=0.1)
    index, t = R.render_points_section_rule(xyz, 0.1, got.camera, np.concatenate([ses.section.normals, ses.section.offsets[:, None]], 1))
    assert np.array_equal(got.ids.cpu().numpy(), index) and np.array_equal(bits(got.t.cpu().numpy()), bits(t))
    assert (index >= 8).any() and not np.isin(index, [0, 1, 4, 5, 11]).any()  # the vertices with y = -1 are cut away
