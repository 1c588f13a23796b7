"""-m gpu: the rendered view (a3d_render_mesh, a3d_render_points, a3d_render_shade in csrc/session.hip;
InteractiveSession.render / pick_from_render).

The specification is in the tree: the image is, pixel by pixel, what the picks return for the ray through the pixel's
centre.  The yardsticks are the numpy float32 restatements of ``render_rule.py`` (which ``test_render_host.py`` holds
against each other and against the bound on the CPU) and the existing picks themselves.  Scenes, cameras and the adaptors
that reach the library through ``agile3d_amd.view`` are in ``session_kit.py``.

1  images equal the per-pixel pick rule bit for bit (ids, t, u, v), and a3d_pick_mesh / a3d_pick_ray on 64 sampled pixels
2  no cracks: a jittered plane in front of a second one, near the origin and at 50 m
3  the capacity protocol, determinism
4  shading
5  the session: render, the hidden retry, pick_from_render
"""
import functools

import numpy as np
import pytest
import torch

import session_kit
from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.session import camera_from_matrices
from pick_rule import F32
from render_rule import camera_fields, pixel_rays, render_mesh_rule, render_points_rule, shade_rule
from session_kit import (CASES, DEV, FAR, PlanesScene, bits, camera_of, cloud_scene, intrinsic, load_session_case, look_at,
                         mesh_scene, pick_mesh, pick_ray, render, rotation, sampled_pixels, shade)

pytestmark = pytest.mark.gpu
SIZES = [(37, 29), (1, 1), (16, 16)]
MESH_SCENES = ["quad larger than the view", "receding plane", "receding plane at 50 m", "inside a box", "bad faces"]


# ------------------------------------------------------------------------------------------- 1, 4: meshes
@functools.lru_cache(maxsize=None)
def mesh_reference(name, size):
    xyz, faces, eye, target, fov, _ = mesh_scene(name)
    return render_mesh_rule(xyz, faces, camera_of(eye, target, fov, size))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", MESH_SCENES)
def test_mesh_images_equal_the_pick_rule(name, size):
    xyz, faces, eye, target, fov, want_flags = mesh_scene(name)
    cam = camera_of(eye, target, fov, size)
    got = render(xyz, faces, cam)
    face, t, u, v, flags = mesh_reference(name, size)
    assert got["flags"] == flags == want_flags
    assert np.array_equal(got["ids"], face)
    assert np.array_equal(bits(got["t"]), bits(t))
    assert np.array_equal(bits(got["u"]), bits(u)) and np.array_equal(bits(got["v"]), bits(v))
    w, h = size
    if size == (37, 29):
        assert (face >= 0).sum() >= 200, "an image that shows nothing proves nothing"
        if name == "inside a box":
            assert (face >= 0).all() and got["n_everywhere"] == 1 and (face == len(faces) - 1).sum() >= 50
        if name == "quad larger than the view":
            assert (face >= 0).all()
    # the existing pick on the restated rays of sampled pixels
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    px = sampled_pixels(w, h)
    picks = pick_mesh(xyz, faces, [(o, d[j, i]) for i, j in px])
    for (i, j), p in zip(px, picks):
        assert p["face"] == got["ids"][j, i] and p["flags"] == want_flags
        if p["face"] >= 0:
            assert bits(p["t"]) == bits(got["t"][j, i]) and bits(p["u"]) == bits(got["u"][j, i]) and bits(p["v"]) == bits(got["v"][j, i])
        else:
            assert got["t"][j, i] == np.inf and got["u"][j, i] == 0 and got["v"][j, i] == 0
    # shading: the fp32 restatement, exactly (colours beyond [0, 1] exercise the clamp)
    col = np.random.default_rng(1).uniform(-0.1, 1.1, (len(xyz), 3)).astype(F32)
    bg = (0.25, 0.5, 1.0)
    assert np.array_equal(shade(got, faces, col, bg, len(xyz)), shade_rule(face, u, v, faces, col, bg))
    # without u and v the ids and t are the same
    plain = render(xyz, faces, cam, uv=False)
    assert np.array_equal(plain["ids"], face) and np.array_equal(bits(plain["t"]), bits(t)) and (plain["u"] == -7).all()


def test_bad_faces_leave_the_image_unaffected():
    xyz, faces, eye, target, fov, _ = mesh_scene("bad faces")
    cam = camera_of(eye, target, fov, (37, 29))
    got, clean = render(xyz, faces, cam), render(xyz, faces[5:], cam)
    assert got["flags"] == 1 and clean["flags"] == 0
    assert np.array_equal(np.where(got["ids"] >= 0, got["ids"] - 5, -1), clean["ids"])
    assert np.array_equal(bits(got["t"]), bits(clean["t"])) and (clean["ids"] >= 0).sum() >= 100


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_faces_and_no_points(size):
    cam = camera_of([0.0, -1.0, 0.6], [0.0, 3.0, 0.0], 60.0, size)
    xyz = np.zeros((3, 3), F32)
    for got in (render(xyz, np.zeros((0, 3), np.int32), cam), render(np.zeros((0, 3), F32), None, cam, radius=0.05),
                render(np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), cam)):
        assert (got["ids"] == -1).all() and (got["t"] == np.inf).all() and got["flags"] == 0 and got["pairs"] == 0
    got = render(xyz, np.zeros((0, 3), np.int32), cam)
    rgb = shade(got, np.zeros((0, 3), np.int32), np.ones((3, 3), F32), (0.0, 0.5, 1.0), 3)
    assert (rgb == np.array([0, 128, 255], np.uint8)).all()


# ------------------------------------------------------------------------------------------- 1, 4: point clouds
@functools.lru_cache(maxsize=None)
def cloud_reference(name, size):
    xyz, r, eye, target, fov = cloud_scene(name)
    return render_points_rule(xyz, r, camera_of(eye, target, fov, size))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cloud", "cloud at 50 m"])
def test_point_images_equal_the_pick_rule(name, size):
    xyz, r, eye, target, fov = cloud_scene(name)
    cam = camera_of(eye, target, fov, size)
    got = render(xyz, None, cam, radius=r)
    index, t = cloud_reference(name, size)
    assert np.array_equal(got["ids"], index) and np.array_equal(bits(got["t"]), bits(t))
    assert got["n_everywhere"] >= 1                                   # the point within its radius of the camera
    assert not np.isin(index, np.arange(2000, 2020)).any()            # a duplicate never beats its lower row
    if size == (37, 29):
        assert (index >= 0).sum() >= 300 and (index == -1).any() and len(np.unique(index)) >= 50
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    dev = torch.from_numpy(xyz).to(DEV)
    for i, j in sampled_pixels(*size):
        idx, p = pick_ray(dev, o, d[j, i], r)
        assert idx == got["ids"][j, i]
        if idx >= 0:
            assert np.array_equal(p, xyz[idx])
    col = np.random.default_rng(2).uniform(-0.1, 1.1, (len(xyz), 3)).astype(F32)
    assert np.array_equal(shade(got, None, col, (1.0, 1.0, 1.0), len(xyz)), shade_rule(index, None, None, None, col, (1.0, 1.0, 1.0)))


def test_point_tie_order():
    """A 1 x 1 image whose ray is exactly +x (the principal point at the pixel's centre): t = 2 exactly for points that
    share x.  Equal t -> the smaller perpendicular distance although stored later; equal t and distance -> the lower row."""
    ext = np.eye(4)
    ext[:3, :3] = [[0, 1, 0], [0, 0, 1], [1, 0, 0]]                    # camera z = world x
    o = np.array([1.0, 1.0, 9.0])
    ext[:3, 3] = -ext[:3, :3] @ o
    cam = camera_from_matrices(np.array([[10.0, 0, 0.5], [0, 10.0, 0.5], [0, 0, 1.0]]), ext, 1, 1)
    assert np.array_equal(pixel_rays(cam)[0, 0], np.array([1, 0, 0], F32))
    xyz = (o + np.array([[2, 0.02, 0], [2, 0.01, 0], [2, 0.01, 0], [3, 0, 0]])).astype(F32)
    got = render(xyz, None, cam, radius=0.03)
    assert got["ids"][0, 0] == 1 and got["t"][0, 0] == 2.0
    assert render(xyz[[0, 3]], None, cam, radius=0.03)["ids"][0, 0] == 0
    assert np.array_equal(got["ids"], render_points_rule(xyz, 0.03, cam)[0])


# ------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("placement", ["near", "far"])
def test_no_cracks(placement):
    """A jittered plane of 2 x 30^2 faces that fills the view, a second plane half a metre behind it: no pixel is
    background and no pixel shows the rear plane."""
    shift = FAR if placement == "far" else np.zeros(3)
    rot = rotation(7)
    sc = PlanesScene(30, rot, shift, seed=2)
    cam = camera_of(rot @ [0.2, -0.1, 3.5] + shift, rot @ [0.0, 0.0, 0.0] + shift, 60.0, (96, 64))
    got = render(sc.xyz, sc.faces, cam)
    assert got["flags"] == 0 and (got["ids"] >= 0).all(), int((got["ids"] < 0).sum())
    kinds = sc.kind[got["ids"]]
    assert (kinds == "front").all(), {k: int((kinds == k).sum()) for k in np.unique(kinds)}
    assert len(np.unique(got["ids"])) >= 300


# ------------------------------------------------------------------------------------------- 3
def test_capacity_protocol_and_determinism():
    xyz, faces, eye, target, fov, _ = mesh_scene("receding plane")
    cam = camera_of(eye, target, fov, (37, 29))
    generous = render(xyz, faces, cam)
    assert generous["flags"] == 0 and generous["pairs"] > 392            # more pairs than faces: faces span tiles
    small = render(xyz, faces, cam, capacity=1)
    assert small["flags"] & L.A3D_RENDER_OVERFLOW and small["pairs"] == generous["pairs"]
    assert (small["ids"] == -7).all() and (small["t"] == -7).all() and (small["u"] == -7).all() and (small["v"] == -7).all()
    again = render(xyz, faces, cam, capacity=small["pairs"])
    twice = render(xyz, faces, cam, capacity=small["pairs"])
    for k in ("ids", "t", "u", "v"):
        assert np.array_equal(bits(again[k]) if k != "ids" else again[k], bits(generous[k]) if k != "ids" else generous[k])
        assert np.array_equal(bits(again[k]) if k != "ids" else again[k], bits(twice[k]) if k != "ids" else twice[k])
    assert again["flags"] == 0 and again["pairs"] == small["pairs"]
    # the same protocol on a cloud
    cxyz, r, ceye, ctarget, cfov = cloud_scene("cloud")
    ccam = camera_of(ceye, ctarget, cfov, (37, 29))
    big = render(cxyz, None, ccam, radius=r)
    tiny = render(cxyz, None, ccam, radius=r, capacity=1)
    assert tiny["flags"] & L.A3D_RENDER_OVERFLOW and (tiny["ids"] == -7).all() and tiny["pairs"] == big["pairs"]
    fit = render(cxyz, None, ccam, radius=r, capacity=tiny["pairs"])
    assert np.array_equal(fit["ids"], big["ids"]) and np.array_equal(bits(fit["t"]), bits(big["t"]))
    # argument checks
    assert V.render_workspace_bytes(10, 0, 5, 1) == 0 and V.render_workspace_bytes(10, 4097, 5, 1) == 0
    assert V.render_workspace_bytes(10, 16, 16, 1 << 20) >= 4 << 20


# ------------------------------------------------------------------------------------------- 5
@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def _ray_survives_pick(d32):
    """``pick`` renormalises a direction in float64 and rounds it to fp32: whether that returns these very bits."""
    d64 = d32.astype(np.float64)
    return np.array_equal((d64 / np.linalg.norm(d64)).astype(F32), d32)


def pixels_for_pick(ids, d, n_hit, n_miss):
    """``n_hit`` pixels that show something and ``n_miss`` that show nothing, drawn in a fixed shuffled order from the
    pixels whose restated ray ``pick`` takes bit for bit (``_ray_survives_pick``)."""
    h, w = ids.shape
    out, want = [], {True: n_hit, False: n_miss}
    for k in np.random.default_rng(w * h).permutation(w * h):
        i, j = int(k % w), int(k // w)
        shows = bool(ids[j, i] >= 0)
        if want[shows] and _ray_survives_pick(d[j, i]):
            want[shows] -= 1
            out.append((i, j))
    assert want == {True: 0, False: 0}, want
    return out


def check_pick_from_render(ses, res, n_hit, n_miss):
    """pick_from_render equals pick for the pixel's restated ray: a point where the image shows something, else None."""
    o32, d = camera_fields(res.camera)[0], pixel_rays(res.camera)
    ids = res.ids.cpu().numpy()
    for i, j in pixels_for_pick(ids, d, n_hit, n_miss):
        got = ses.pick_from_render(res, i, j)
        assert (got is not None) == bool(ids[j, i] >= 0), (i, j)
        assert got == ses.pick(o32, d[j, i]), (i, j)


def test_session_render_cloud(model_005):
    """The small fixture scene after its scripted clicks and infer: pixels that show a vertex carry that vertex's colour
    from infer's colours; before any inference the scan's own; pick_from_render equals pick."""
    from agile3d_amd.session import InteractiveSession
    c, meta = load_session_case(CASES[0])
    ses = InteractiveSession(model_005, voxel_size=meta["voxel_size"], palette=c["palette"],
                             background_click_color=c["background_click_color"])
    ses.load_scene(c["coords_full"], c["colors_full"], c["labels_full"], name=meta["name"])
    xyz = c["coords_full"].astype(F32)
    centre, extent = xyz.mean(0).astype(np.float64), float(np.ptp(xyz, axis=0).max())
    k, e, w, h = intrinsic(80, 60, 60.0), look_at(centre + [0.2 * extent, -1.1 * extent, 0.6 * extent], centre), 80, 60
    bg = (0.0, 0.25, 1.0)

    def check(res, colors):
        ids, rgb = res.ids.cpu().numpy(), res.rgb.cpu().numpy()
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and res.u is None and not res.mesh
        assert (ids >= 0).sum() >= 300 and (ids < 0).any()
        assert np.array_equal(rgb, shade_rule(ids, None, None, None, colors, bg))
        assert (rgb[ids < 0] == np.array([0, 64, 255], np.uint8)).all()
        return ids

    before = ses.render(k, e, w, h, background=bg)
    ids0 = check(before, ses.colors_full.cpu().numpy())
    assert np.array_equal(ids0, render(xyz, None, before.camera, radius=ses.voxel_size, capacity=1 << 22)["ids"])
    step = meta["steps"][0]
    for p, o in zip(c["click_points"][:step["num_clicks"]], c["click_objs"][:step["num_clicks"]]):
        ses.click(p, int(o))
    res = ses.infer(logits=torch.from_numpy(c["step0_logits"]).to(DEV))
    after = ses.render(k, e, w, h, background=bg)
    ids1 = check(after, res.colors.cpu().numpy())
    assert np.array_equal(ids1, ids0) and not np.array_equal(after.rgb.cpu().numpy(), before.rgb.cpu().numpy())
    assert torch.equal(ses.render(k, e, w, h, colors=ses.colors_full, background=bg).rgb, before.rgb)
    # pick_from_render: the vertex pick takes for the pixel's restated ray
    check_pick_from_render(ses, after, 20, 5)
    # errors, as the session reports them
    with pytest.raises(ValueError):
        ses.render(k, e, 0, h)
    with pytest.raises(ValueError):
        ses.render(np.eye(4), e, w, h)
    with pytest.raises(ValueError):
        ses.pick_from_render(after, w, 0)
    ses._drop_scene()
    assert ses._render_ws is None
    with pytest.raises(RuntimeError):
        ses.render(k, e, w, h)


def test_session_render_mesh_and_the_hidden_retry(model_005):
    from agile3d_amd.session import InteractiveSession
    xyz, faces, eye, target, fov, _ = mesh_scene("receding plane")
    # 6 000 vertices that no face uses, under the plane: they leave the mesh's image alone and fill the cloud's
    rng = np.random.default_rng(3)
    xyz = np.concatenate([xyz, rng.uniform([-1.0, 2.0, -0.35], [1.0, 8.0, -0.3], (6000, 3)).astype(F32)])
    col = rng.uniform(0, 1, xyz.shape).astype(F32)
    ses = InteractiveSession(model_005, voxel_size=0.05)
    ses.load_scene(xyz, col, faces=faces)
    k, e, w, h = intrinsic(37, 29, fov), look_at(eye, target), 37, 29
    res = ses.render(k, e, w, h)
    face, t, u, v, _ = mesh_reference("receding plane", (37, 29))
    assert res.mesh and np.array_equal(res.ids.cpu().numpy(), face) and np.array_equal(bits(res.t.cpu().numpy()), bits(t))
    assert np.array_equal(bits(res.u.cpu().numpy()), bits(u)) and np.array_equal(bits(res.v.cpu().numpy()), bits(v))
    assert np.array_equal(res.rgb.cpu().numpy(), shade_rule(face, u, v, faces, col, (1.0, 1.0, 1.0)))
    check_pick_from_render(ses, res, 20, 5)
    # a view that needs more pairs than the workspace holds: large discs of the vertices as a cloud, 640 x 480
    ses.load_scene(xyz, col)
    assert ses._render_ws is None
    k2, w2, h2 = intrinsic(640, 480, fov), 640, 480
    big = ses.render(k2, e, w2, h2, radius=0.3)
    assert big.pairs > max(4 * len(xyz), 1 << 16), big.pairs            # the first attempt's capacity did not suffice
    want = render(xyz, None, big.camera, radius=0.3, capacity=big.pairs)
    assert want["flags"] == 0 and np.array_equal(big.ids.cpu().numpy(), want["ids"])
    assert np.array_equal(bits(big.t.cpu().numpy()), bits(want["t"]))
    held = ses._render_ws
    assert torch.equal(ses.render(k2, e, w2, h2, radius=0.3).ids, big.ids) and ses._render_ws is held   # kept and reused
