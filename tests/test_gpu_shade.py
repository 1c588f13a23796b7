"""-m gpu: the lit view (a3d_vertex_normals, a3d_render_shade_lit, a3d_render_shade_depth in csrc/session.hip;
InteractiveSession.render(lit=True), default_view).

The rules are this library's and stated in include/agile3d_hip.h; the yardstick is their numpy float32 restatement in
``shade_rule.py`` (which ``test_shade_host.py`` holds to float64 on the CPU).  Every comparison is bit for bit.  Scenes,
cameras and the adaptors that reach the library through ``agile3d_amd.view`` are in ``session_kit.py``.

1  vertex normals on five meshes, twice
2  the lit colour image of three mesh views at three sizes; ambient = 1 is the flat image
3  the depth-shaded image of a cloud (and of a mesh's t image); strength = 0 is the flat image
4  the session: lit=False keeps today's bytes, lit=True on a mesh and on a cloud, default_view on the committed mesh
"""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

import session_kit
from agile3d_amd.session import vertex_corner_lists
from conftest import ROOT
from pick_rule import F32
from render_rule import shade_rule
from session_kit import (DEV, _dev, bits, byref, camera_of, cloud_scene, f32_pointer, intrinsic, jittered_grid, look_at,
                         mesh_scene, normals_gpu, render, shade, shade_depth, shade_lit, status)
from shade_rule import depth_factor, depth_rule, lit_factor, lit_rule, vertex_normals_rule

pytestmark = pytest.mark.gpu
SIZES = [(37, 29), (16, 16), (1, 1)]
BG = (0.25, 0.5, 1.0)


# ------------------------------------------------------------------------------------------- 1: normals
def _normal_mesh(name):
    rng = np.random.default_rng(9)
    if name == "tetrahedron":
        return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    if name == "fan of 300":
        a = np.linspace(0.0, 1.9 * np.pi, 301)
        rim = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.2, 0.2, 301)], 1) * rng.uniform(0.5, 1.5, (301, 1))
        xyz = np.concatenate([[[0.0, 0.0, 0.3]], rim]).astype(F32)
        return xyz, np.stack([np.zeros(300, np.int32), np.arange(1, 301), np.arange(2, 302)], 1).astype(np.int32)
    if name in ("grid of 257", "grid of 257 at 50 m"):
        shift = (50.3, -48.7, 1.2) if name.endswith("50 m") else (0.0, 0.0, 0.0)
        xyz, faces = jittered_grid(16, 16, seed=3, shift=shift)
        xyz = np.concatenate([xyz, (np.array([[1.7, 1.6, 0.2]]) + shift).astype(F32)])     # vertex 256: the second block's only one
        return xyz, np.concatenate([faces, [[255, 239, 256]]]).astype(np.int32)
    if name == "bad faces":
        xyz, faces = jittered_grid(6, 5, seed=5)
        n = len(xyz)
        xyz = np.concatenate([xyz, [[np.nan, 0.2, 0.1], [9.0, 9.0, 9.0]]]).astype(F32)       # a NaN vertex, an isolated one
        bad = [[0, 0, 7], [1, 2, 1], [3, 4, n], [5, 6, len(xyz)], [-1, 8, 9], [10, 11, 12]]  # repeated x 2, NaN, out of range x 2
        xyz[[10, 11, 12]] = [[0.0, 0.0, 0.0], [0.1, 0.1, 0.1], [0.2, 0.2, 0.2]]              # ... and three vertices on a line
        return xyz, np.concatenate([bad, faces]).astype(np.int32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["tetrahedron", "fan of 300", "grid of 257", "bad faces", "grid of 257 at 50 m"])
def test_vertex_normals_equal_the_rule(name):
    xyz, faces = _normal_mesh(name)
    offsets, corners = vertex_corner_lists(faces, len(xyz))
    got = normals_gpu(xyz, faces, offsets, corners)
    want = vertex_normals_rule(xyz, faces, offsets, corners)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero((bits(got) != bits(want)).any(1))[:10]
    assert np.array_equal(bits(normals_gpu(xyz, faces, offsets, corners)), bits(got))          # two calls, the same bytes
    length = np.linalg.norm(got.astype(np.float64), axis=1)
    if name == "fan of 300":
        assert offsets[1] - offsets[0] == 300 and length[0] == pytest.approx(1.0, abs=1e-6)
    if name.startswith("grid of 257"):
        assert len(xyz) == 257 and np.abs(length - 1).max() < 1e-6 and (got[:239, 2] > 0.5).all()   # (239, 255: the extra face)
    if name == "bad faces":
        n = len(xyz) - 2
        assert not got[n:].any() and np.abs(length[:n] - 1).max() < 1e-6                      # NaN and isolated vertex: zeros
        clean = normals_gpu(xyz, faces[6:], *vertex_corner_lists(faces[6:], len(xyz)))         # bad faces add nothing (or +0)
        assert np.array_equal(bits(got), bits(clean))
    if name == "tetrahedron":
        assert np.allclose(got[0], -np.ones(3) / np.sqrt(3), atol=1e-6)


def test_vertex_normals_arguments():
    call = lambda *args: status("a3d_vertex_normals", *args)                                   # the entry point as it is
    xyz, faces = _normal_mesh("tetrahedron")
    offsets, corners = vertex_corner_lists(faces, 4)
    x, f, o, c = _dev(xyz, F32), _dev(faces, np.int32), _dev(offsets, np.int64), _dev(corners, np.int32)
    out = torch.zeros((4, 3), dtype=torch.float32, device=DEV)
    ok = (x.data_ptr(), 4, f.data_ptr(), 4, o.data_ptr(), c.data_ptr(), out.data_ptr(), None)
    for at, bad in ((0, None), (1, -1), (2, None), (3, -1), (4, None), (5, None), (6, None), (3, 1 << 30)):
        args = list(ok)
        args[at] = bad
        assert call(*args) == -1, (at, bad)                                                    # A3D_ERR_INVALID
    assert call(None, 0, None, 0, None, None, None, None) == 0
    # lists that point outside themselves are skipped, not followed: the isolated vertex's zeros
    wild = _dev(np.array([-5, 1 << 40, 0, 3, 3], np.int64), np.int64)
    junk = _dev(np.full(12, 1 << 20, np.int32), np.int32)
    assert call(x.data_ptr(), 4, f.data_ptr(), 4, wild.data_ptr(), junk.data_ptr(), out.data_ptr(), None) == 0
    assert not out.cpu().numpy().any()
    # a mesh without faces: zeros
    out.fill_(5.0)
    zero = _dev(np.zeros(5, np.int64), np.int64)
    assert call(x.data_ptr(), 4, None, 0, zero.data_ptr(), None, out.data_ptr(), None) == 0
    assert not out.cpu().numpy().any()


# ------------------------------------------------------------------------------------------- 2: the lit image
LIT_VIEWS = ["quad larger than the view", "inside a box", "zero normals"]


@functools.lru_cache(maxsize=None)
def lit_scene(name):
    """(xyz, faces, eye, target, fov, normals): the scenes of ``test_gpu_render`` with the rule's normals; "zero normals" is
    its receding plane with the normals of the vertices left of x = 0 set to zero."""
    xyz, faces, eye, target, fov, _ = mesh_scene("receding plane" if name == "zero normals" else name)
    normals = vertex_normals_rule(xyz, faces, *vertex_corner_lists(faces, len(xyz)))
    if name == "zero normals":
        normals[xyz[:, 0] < 0] = 0
    return xyz, faces, eye, target, fov, normals


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", LIT_VIEWS)
def test_lit_image_equals_the_rule(name, size):
    xyz, faces, eye, target, fov, normals = lit_scene(name)
    cam = camera_of(eye, target, fov, size)
    r = render(xyz, faces, cam)
    ids, u, v = r["ids"], r["u"], r["v"]
    col = np.random.default_rng(1).uniform(-0.1, 1.1, (len(xyz), 3)).astype(F32)
    n = len(xyz)
    flat = shade(r, faces, col, BG, n)
    for ambient in (0.35, 0.0):
        got = shade_lit(r, faces, col, normals, cam, ambient, BG, n)
        assert np.array_equal(got, lit_rule(ids, u, v, faces, col, normals, cam, ambient, BG)), ambient
    assert np.array_equal(shade_lit(r, faces, col, normals, cam, 1.0, BG, n), flat)             # k == 1 exactly
    assert np.array_equal(flat, shade_rule(ids, u, v, faces, col, BG))
    # the ids and weights the shading read are untouched
    again = [x.cpu().numpy() for x in r["dev"][:3]]
    assert np.array_equal(again[0], ids) and np.array_equal(bits(again[1]), bits(u)) and np.array_equal(bits(again[2]), bits(v))
    if size == (37, 29):
        k, k0, dot = lit_factor(ids, u, v, faces, normals, cam, 0.35)
        assert (ids >= 0).sum() >= 200 and not np.array_equal(shade_lit(r, faces, col, normals, cam, 0.35, BG, n), flat)
        assert (k0[ids >= 0] <= 1).all() and (k[ids >= 0] >= F32(0.35)).all()
        if name == "inside a box":
            assert (dot > 0).sum() >= 200 and (k0[dot > 0] > 0).all()                            # normals that face away: the fabsf
        if name == "quad larger than the view":
            assert (dot < 0).all()                                                                # ... and one that faces the camera
        if name == "zero normals":
            dark = (ids >= 0) & (k0 == 1)
            assert dark.sum() >= 50 and ((ids >= 0) & (k0 < 1)).sum() >= 50
            white = shade_lit(r, faces, np.ones((n, 3), F32), normals, cam, 0.0, BG, n)
            zero = xyz[faces[np.where(ids >= 0, ids, 0)], 0].max(-1) < 0                          # all three normals zero
            assert (zero & (ids >= 0)).sum() >= 50 and (white[zero & (ids >= 0)] == 255).all()
    if size == (1, 1) and name == "quad larger than the view":
        assert ids[0, 0] >= 0


def test_lit_arguments():
    lit = lambda *args: status("a3d_render_shade_lit", *args)                                  # the entry points as they are
    depth = lambda *args: status("a3d_render_shade_depth", *args)
    xyz, faces, eye, target, fov, normals = lit_scene("quad larger than the view")
    cam = camera_of(eye, target, fov, (16, 16))
    r = render(xyz, faces, cam)
    ids, u, v, faces_dev = r["dev"]
    col, nrm = _dev(np.ones((4, 3)), F32), _dev(normals, F32)
    rgb = torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV)
    ok = [ids.data_ptr(), u.data_ptr(), v.data_ptr(), faces_dev.data_ptr(), 2, col.data_ptr(), 4, nrm.data_ptr(), byref(cam),
          0.35, f32_pointer(BG), rgb.data_ptr(), None]
    assert lit(*ok) == 0
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (4, -1), (5, None), (6, -1), (7, None), (8, None), (9, -0.01),
                    (9, 1.01), (9, float("nan")), (10, None), (11, None)):
        args = list(ok)
        args[at] = bad
        assert lit(*args) == -1, (at, bad)
    # no faces: every pixel the background, whatever the ids say
    args = list(ok)
    args[3], args[4] = None, 0
    assert lit(*args) == 0
    assert (rgb.cpu().numpy() == np.array([64, 128, 255], np.uint8)).all()
    # the depth pass
    t = torch.from_numpy(r["t"]).to(DEV)
    okd = [ids.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr(), faces_dev.data_ptr(), 2, col.data_ptr(), 4, 8.0,
           f32_pointer(BG), rgb.data_ptr(), 16, 16, None]
    assert depth(*okd) == 0
    for at, bad in ((0, None), (1, None), (2, None), (5, -1), (6, None), (7, -1), (8, -1.0), (8, float("inf")), (8, float("nan")),
                    (9, None), (10, None), (11, 0), (12, 4097)):
        args = list(okd)
        args[at] = bad
        assert depth(*args) == -1, (at, bad)


# ------------------------------------------------------------------------------------------- 3: the depth-shaded image
def test_depth_image_equals_the_rule():
    xyz, radius, eye, target, fov = cloud_scene("cloud")
    cam = camera_of(eye, target, fov, (37, 29))
    r = render(xyz, None, cam, radius=radius)
    ids, t = r["ids"], r["t"]
    shows = ids >= 0
    # what the view must hold for the test to mean anything: background, hits on all four borders, hits beside background
    assert shows.sum() >= 300 and (~shows).sum() >= 50
    assert shows[0].any() and shows[-1].any() and shows[:, 0].any() and shows[:, -1].any()
    assert (shows[:, 1:] & ~shows[:, :-1]).any() and (shows[1:] & ~shows[:-1]).any()
    col = np.random.default_rng(2).uniform(-0.1, 1.1, (len(xyz), 3)).astype(F32)
    n = len(xyz)
    flat = shade(r, None, col, BG, n)
    for strength in (8.0, 0.37):
        got = shade_depth(r, t, None, col, strength, BG, n)
        assert np.array_equal(got, depth_rule(ids, t, None, None, None, col, strength, BG)), strength
    assert np.array_equal(shade_depth(r, t, None, col, 0.0, BG, n), flat)
    assert not np.array_equal(shade_depth(r, t, None, col, 8.0, BG, n), flat)
    k = depth_factor(ids, t, 8.0)
    assert (k <= 1).all() and (k[shows] < 1).sum() >= 100 and (k[shows] > 0).all()
    assert (shade_depth(r, t, None, col, 8.0, BG, n)[~shows] == np.array([64, 128, 255], np.uint8)).all()


@pytest.mark.parametrize("size", [(16, 16), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_image_of_a_mesh(size):
    """The kernel takes a mesh's images too: the receding plane (a whole tile, and an image without neighbours)."""
    xyz, faces, eye, target, fov, _ = mesh_scene("receding plane")
    cam = camera_of(eye, target, fov, size)
    r = render(xyz, faces, cam)
    col = np.random.default_rng(3).uniform(0, 1, (len(xyz), 3)).astype(F32)
    got = shade_depth(r, r["t"], faces, col, 8.0, BG, len(xyz))
    assert np.array_equal(got, depth_rule(r["ids"], r["t"], r["u"], r["v"], faces, col, 8.0, BG))
    if size == (1, 1):
        assert np.array_equal(got, shade(r, faces, col, BG, len(xyz)))                           # no neighbour: k == 1


# ------------------------------------------------------------------------------------------- 4: the session
@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def test_session_lit_render(model_005):
    from agile3d_amd.session import InteractiveSession
    xyz, faces, eye, target, fov, _ = mesh_scene("receding plane")
    rng = np.random.default_rng(3)
    xyz = np.concatenate([xyz, rng.uniform([-1.0, 2.0, -0.35], [1.0, 8.0, -0.3], (6000, 3)).astype(F32)])   # vertices no face uses
    col = rng.uniform(0, 1, xyz.shape).astype(F32)
    ses = InteractiveSession(model_005, voxel_size=0.05)
    ses.load_scene(xyz, col, faces=faces)
    assert ses.normals is None
    offsets, corners = vertex_corner_lists(faces, len(xyz))
    assert np.array_equal(ses._corner_lists[0].cpu().numpy(), offsets) and np.array_equal(ses._corner_lists[1].cpu().numpy(), corners)
    k, e, w, h = intrinsic(37, 29, fov), look_at(eye, target), 37, 29
    flat = ses.render(k, e, w, h, background=BG)
    assert flat.lit is False and ses.normals is None
    ids, u, v = flat.ids.cpu().numpy(), flat.u.cpu().numpy(), flat.v.cpu().numpy()
    assert np.array_equal(flat.rgb.cpu().numpy(), shade_rule(ids, u, v, faces, col, BG))       # today's bytes
    direct = shade(dict(dev=(flat.ids, flat.u, flat.v, ses.faces)), faces, col, BG, len(xyz))
    assert np.array_equal(flat.rgb.cpu().numpy(), direct)
    lit = ses.render(k, e, w, h, background=BG, lit=True)
    normals = vertex_normals_rule(xyz, faces, offsets, corners)
    assert lit.lit is True and ses.normals is not None and tuple(ses.normals.shape) == (len(xyz), 3)
    assert np.array_equal(bits(ses.normals.cpu().numpy()), bits(normals)) and not normals[-6000:].any()
    assert torch.equal(lit.ids, flat.ids) and torch.equal(lit.t, flat.t) and torch.equal(lit.u, flat.u) and torch.equal(lit.v, flat.v)
    assert np.array_equal(lit.rgb.cpu().numpy(), lit_rule(ids, u, v, faces, col, normals, lit.camera, 0.35, BG))
    assert not torch.equal(lit.rgb, flat.rgb)
    held = ses.normals
    half = ses.render(k, e, w, h, background=BG, lit=True, ambient=0.5)
    assert ses.normals is held                                                                   # once per scene
    assert np.array_equal(half.rgb.cpu().numpy(), lit_rule(ids, u, v, faces, col, normals, lit.camera, 0.5, BG))
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True, ambient=1.0).rgb, flat.rgb)
    for bad in (dict(ambient=-0.1), dict(ambient=1.5), dict(ambient=float("nan")), dict(depth_strength=-1.0),
                dict(depth_strength=float("inf"))):
        with pytest.raises(ValueError):
            ses.render(k, e, w, h, lit=True, **bad)
    # the same vertices as a cloud: no normals, depth shading
    ses.load_scene(xyz, col)
    assert ses.normals is None and ses._corner_lists is None
    cflat = ses.render(k, e, w, h, background=BG)
    clit = ses.render(k, e, w, h, background=BG, lit=True)
    cids, ct = cflat.ids.cpu().numpy(), cflat.t.cpu().numpy()
    assert clit.lit and not clit.mesh and ses.normals is None and (cids >= 0).sum() >= 100
    assert torch.equal(clit.ids, cflat.ids) and torch.equal(clit.t, cflat.t)
    assert np.array_equal(cflat.rgb.cpu().numpy(), shade_rule(cids, None, None, None, col, BG))
    assert np.array_equal(clit.rgb.cpu().numpy(), depth_rule(cids, ct, None, None, None, col, 8.0, BG))
    assert torch.equal(ses.render(k, e, w, h, background=BG, lit=True, depth_strength=0.0).rgb, cflat.rgb)
    assert not torch.equal(clit.rgb, cflat.rgb)
    ses._drop_scene()
    with pytest.raises(RuntimeError):
        ses.default_view(8, 8)


def test_session_default_view_on_the_committed_mesh(model_005, tmp_path):
    """``render(*default_view(64, 48), 64, 48, lit=True)`` on tests/golden/data/mesh_small.ply shows the mesh; after
    ``infer()`` the colours a render takes by default are the painted ones."""
    from agile3d_amd.ply import read_ply
    from agile3d_amd.session import InteractiveSession
    src = os.path.join(ROOT, "tests", "golden", "data", "mesh_small.ply")
    folder = tmp_path / "scene_small"
    os.makedirs(folder)
    shutil.copy(src, folder / "scan.ply")
    vert, faces = read_ply(src, triangular_mesh=True)
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(F32)
    ses = InteractiveSession(model_005, voxel_size=0.05)
    ses.load_scene_dir(str(folder))
    assert ses.faces is not None and ses.faces.shape[0] == len(faces)
    k, e = ses.default_view(64, 48)
    res = ses.render(k, e, 64, 48, lit=True)
    ids, u, v = res.ids.cpu().numpy(), res.u.cpu().numpy(), res.v.cpu().numpy()
    assert res.lit and res.mesh and (ids >= 0).sum() >= 1
    offsets, corners = vertex_corner_lists(faces, len(xyz))
    normals = vertex_normals_rule(xyz, faces, offsets, corners)
    assert np.array_equal(bits(ses.normals.cpu().numpy()), bits(normals))
    own = ses.colors_full.cpu().numpy()
    assert np.array_equal(res.rgb.cpu().numpy(), lit_rule(ids, u, v, faces, own, normals, res.camera, 0.35, (1.0, 1.0, 1.0)))
    # one click, everything painted as object 1: the next render shows the painted colours
    row = ses.click(xyz[int(faces[ids[ids >= 0][0], 0])], 1)[0]
    n_qv = ses.raw_coords_qv.shape[0]
    logits = torch.zeros((n_qv, 2), dtype=torch.float32, device=DEV)
    logits[:, 1] = 1.0                                                                            # everything is object 1
    out = ses.infer(logits=logits)
    painted = out.colors.cpu().numpy()
    assert row >= 0 and np.array_equal(painted, np.tile(ses.palette[1], (len(xyz), 1)))
    after = ses.render(k, e, 64, 48, lit=True)
    assert torch.equal(after.ids, res.ids)
    assert np.array_equal(after.rgb.cpu().numpy(), lit_rule(ids, u, v, faces, painted, normals, res.camera, 0.35, (1.0, 1.0, 1.0)))
    assert not torch.equal(after.rgb, res.rgb)
    assert torch.equal(ses.render(k, e, 64, 48, lit=True, colors=ses.colors_full).rgb, res.rgb)
