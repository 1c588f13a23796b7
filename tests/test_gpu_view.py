"""-m gpu: the contract of ``agile3d_amd/view.py`` itself, at the smallest shapes where the layer can go wrong -- one face,
one point, images of 1 x 1 and 17 x 1 pixels (the second crosses a 16-pixel tile edge).  What the kernels compute is held
bit for bit by ``test_gpu_session*.py``, ``test_gpu_render.py`` and ``test_gpu_shade.py``, which run through this layer.

1  every wrapper refuses a wrong dtype, a host tensor, a non-contiguous tensor and a wrong trailing shape with ValueError,
   before the library is reached, and leaves the outputs it was given alone
2  n = 0 points and m = 0 faces reach the library as null pointers and give all-background, all -1 results
3  the outputs a caller passes are the ones written
4  the ``read_*`` decoders agree field by field with the ctypes structures of ``lib.py``
"""
import types

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.session import camera_from_matrices, vertex_corner_lists
from render_rule import camera_fields, pixel_rays
from session_kit import DEV

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (17, 1)]
BG = (0.25, 0.5, 1.0)
BG8 = np.array([64, 128, 255], np.uint8)


def _state(w, h):
    """Valid arguments of every wrapper, every output a sentinel.  The camera sits at the origin and pixel (0, 0) looks
    along +z, pixel (i, 0) along (i / 20, 0, 1); one face covers all 17 pixels at z = 2; the one point, radius 0.5, is met
    by the first pixels only."""
    s = types.SimpleNamespace(w=w, h=h)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    s.cam = camera_from_matrices(np.array([[20.0, 0, 0.5], [0, 20.0, 0.5], [0, 0, 1.0]]), np.eye(4), w, h)
    s.xyz = dev([[-1, -1, 2], [3, -1, 2], [-1, 3, 2]], np.float32)
    s.faces = dev([[0, 1, 2]], np.int32)
    s.point = dev([[0, 0, 2]], np.float32)
    s.offsets, s.corners = (dev(a, a.dtype) for a in vertex_corner_lists(s.faces.cpu().numpy(), 3))
    s.colors, s.normals = dev(np.full((3, 3), 0.5), np.float32), dev(np.tile([0, 0, -1.0], (3, 1)), np.float32)
    s.labels, s.inv, s.palette = dev([0, 1], np.int32), dev([1, 0, 1], np.int64), dev([[0, 0, 0], [1, 0, 0]], np.float32)
    s.o, s.q = np.zeros(3, np.float32), np.array([[0.1, 0.0, 2.0]], np.float32)
    s.ws = V.session_workspace(DEV)
    s.rws = torch.empty(V.render_workspace_bytes(3, w, h, 64), dtype=torch.uint8, device=DEV)
    full = lambda shape, value, dt: torch.full(shape, value, dtype=dt, device=DEV)
    s.out = dict(rows=full((2, 1), -7, torch.int32), rec4=full((4,), -7, torch.int32), rec8=full((8,), -7, torch.int32),
                 ids=full((h, w), -7, torch.int32), t=full((h, w), -7.0, torch.float32), u=full((h, w), -7.0, torch.float32),
                 v=full((h, w), -7.0, torch.float32), header=full((4,), -7, torch.int32), rgb=full((h, w, 3), 7, torch.uint8),
                 nrm=full((3, 3), -7.0, torch.float32), lab=full((3,), -7, torch.int32), col=full((3, 3), -7.0, torch.float32),
                 err=full((1,), -7, torch.int32))
    return s


# wrapper -> the call with valid arguments but for ``a``, which stands in for one fp32 [n, 3] argument
CALLS = {
    "nearest_rows": lambda s, o, a: V.nearest_rows([s.point, a], s.q, out=o["rows"], workspace=s.ws),
    "pick_ray": lambda s, o, a: V.pick_ray(a, s.o, pixel_rays(s.cam)[0, 0], 0.5, out=o["rec4"], workspace=s.ws),
    "pick_mesh": lambda s, o, a: V.pick_mesh(a, s.faces, s.o, pixel_rays(s.cam)[0, 0], out=o["rec8"], workspace=s.ws),
    "render_mesh": lambda s, o, a: V.render_mesh(a, s.faces, s.cam, o["ids"], o["t"], o["u"], o["v"], header=o["header"],
                                                 workspace=s.rws),
    "render_points": lambda s, o, a: V.render_points(a, 0.5, s.cam, o["ids"], o["t"], o["header"], workspace=s.rws),
    "render_shade": lambda s, o, a: V.render_shade(o["ids"], o["u"], o["v"], s.faces, a, BG, rgb=o["rgb"]),
    "render_shade_lit": lambda s, o, a: V.render_shade_lit(o["ids"], o["u"], o["v"], s.faces, a, s.normals, s.cam, 0.35, BG,
                                                           rgb=o["rgb"]),
    "render_shade_depth": lambda s, o, a: V.render_shade_depth(o["ids"], o["t"], o["u"], o["v"], s.faces, a, 8.0, BG,
                                                               rgb=o["rgb"]),
    "vertex_normals": lambda s, o, a: V.vertex_normals(a, s.faces, s.offsets, s.corners, out=o["nrm"]),
    "session_paint": lambda s, o, a: V.session_paint(s.labels, s.inv, s.xyz, a, s.palette, None, 0.1, o["lab"], o["col"],
                                                     o["err"]),
}
SPOILED = {
    "dtype": lambda a: a.double(),
    "host": lambda a: a.cpu(),
    "not contiguous": lambda a: torch.zeros((a.shape[0], 6), dtype=a.dtype, device=a.device)[:, ::2],
    "trailing shape": lambda a: a[:, :2].contiguous(),
}


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(CALLS))
def test_refusals_come_before_the_library(name, monkeypatch):
    s = _state(17, 1)
    before = {k: t.clone() for k, t in s.out.items()}

    def reached():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(L, "load", reached)
    for what, spoil in SPOILED.items():
        bad = spoil(s.xyz)
        assert tuple(bad.shape) == ((3, 2) if what == "trailing shape" else (3, 3))
        assert bad.is_contiguous() == (what != "not contiguous")
        with pytest.raises(ValueError):
            CALLS[name](s, s.out, bad)
    # an output of the wrong kind is refused like an input
    wrong = {k: t.to(torch.float64) for k, t in s.out.items()}
    with pytest.raises(ValueError):
        CALLS[name](s, wrong, s.xyz)
    monkeypatch.undo()
    torch.cuda.synchronize()
    for k, t in s.out.items():
        assert torch.equal(t, before[k]), k


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("size", SIZES, ids=lambda z: f"{z[0]}x{z[1]}")
def test_empty_tensors_travel_as_null_pointers(size, monkeypatch):
    s = _state(*size)
    lib = L.load()
    seen = {}
    for entry in ("a3d_render_mesh", "a3d_render_points", "a3d_pick_mesh", "a3d_pick_ray", "a3d_vertex_normals"):
        def spy(*args, _entry=entry, _fn=getattr(lib, entry)):
            seen[_entry] = args
            return _fn(*args)
        monkeypatch.setattr(lib, entry, spy)
    no_xyz, no_faces = s.xyz[:0], s.faces[:0]
    assert no_xyz.shape == (0, 3) and no_faces.shape == (0, 3)
    o = s.out
    for xyz, faces in ((s.xyz, no_faces), (no_xyz, None), (no_xyz, no_faces)):
        o["ids"].fill_(-7), o["t"].fill_(-7.0)
        if faces is None:
            V.render_points(xyz, 0.5, s.cam, o["ids"], o["t"], o["header"], workspace=s.rws)
            args = seen["a3d_render_points"]
            assert args[0] is None and args[1] == 0
        else:
            V.render_mesh(xyz, faces, s.cam, o["ids"], o["t"], o["u"], o["v"], header=o["header"], workspace=s.rws)
            args = seen["a3d_render_mesh"]
            assert (args[0] is None) == (len(xyz) == 0) and args[1] == len(xyz) and args[2] is None and args[3] == 0
        flags, n_everywhere, pairs = V.read_render_header(o["header"].cpu().numpy())
        assert (o["ids"] == -1).all() and (o["t"] == np.inf).all() and (flags, n_everywhere, pairs) == (0, 0, 0)
    rgb = V.render_shade(o["ids"], o["u"], o["v"], no_faces, s.colors, BG, rgb=o["rgb"]).cpu().numpy()
    assert (rgb == BG8).all()
    assert (V.render_shade(o["ids"], None, None, None, s.colors[:0], BG).cpu().numpy() == BG8).all()
    d = pixel_rays(s.cam)[0, 0]
    hit = V.read_pick_mesh(V.pick_mesh(s.xyz, no_faces, s.o, d, workspace=s.ws).cpu().numpy())[0]
    assert seen["a3d_pick_mesh"][2] is None and hit["face"] == -1 and hit["flags"] == 0
    assert V.read_pick(V.pick_ray(no_xyz, s.o, d, 0.5, workspace=s.ws).cpu().numpy())[0] == -1 and seen["a3d_pick_ray"][0] is None
    assert V.nearest_rows([no_xyz, s.point], s.q, workspace=s.ws).cpu().tolist() == [[-1], [0]]
    flat = V.vertex_normals(s.xyz, no_faces, s.offsets, s.corners[:0], out=o["nrm"])
    assert seen["a3d_vertex_normals"][2] is None and seen["a3d_vertex_normals"][5] is None and not flat.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------- 3, 4
@pytest.mark.parametrize("size", SIZES, ids=lambda z: f"{z[0]}x{z[1]}")
def test_outputs_are_the_callers_and_decoders_match_the_structures(size):
    s = _state(*size)
    o = s.out
    w, h = size
    ptr = {k: t.data_ptr() for k, t in o.items()}
    rays = pixel_rays(s.cam)[0]
    origin = camera_fields(s.cam)[0]
    # the mesh: images, header, shading, normals
    got = V.render_mesh(s.xyz, s.faces, s.cam, o["ids"], o["t"], o["u"], o["v"], header=o["header"], workspace=s.rws)
    assert all(a is b for a, b in zip(got, (o["ids"], o["t"], o["u"], o["v"], o["header"])))
    head = o["header"].cpu().numpy()
    want = L.RenderHeader.from_buffer_copy(head.tobytes())
    assert V.read_render_header(head) == (want.flags, want.n_everywhere, want.pairs_needed) == (0, 0, (w + 15) // 16)
    ids = o["ids"].cpu().numpy()
    assert (ids == 0).all() and (o["t"] > 0).all() and (o["u"] != -7).all() and (o["v"] != -7).all()
    for shade in (lambda: V.render_shade(o["ids"], o["u"], o["v"], s.faces, s.colors, BG, rgb=o["rgb"]),
                  lambda: V.render_shade_lit(o["ids"], o["u"], o["v"], s.faces, s.colors, s.normals, s.cam, 0.35, BG, rgb=o["rgb"]),
                  lambda: V.render_shade_depth(o["ids"], o["t"], o["u"], o["v"], s.faces, s.colors, 8.0, BG, rgb=o["rgb"])):
        o["rgb"].fill_(7)
        assert shade() is o["rgb"] and (o["rgb"] != 7).all()
    assert V.vertex_normals(s.xyz, s.faces, s.offsets, s.corners, out=o["nrm"]) is o["nrm"]
    assert np.array_equal(o["nrm"].cpu().numpy(), np.tile(np.float32([0, 0, 1]), (3, 1)))
    # the picks, pixel by pixel: the record as the structure reads it, and the image's id
    for i in range(w):
        rec = V.pick_mesh(s.xyz, s.faces, origin, rays[i], out=o["rec8"], workspace=s.ws)
        assert rec is o["rec8"]
        host = rec.cpu().numpy()
        c, r = L.PickMeshResult.from_buffer_copy(host.tobytes()), V.read_pick_mesh(host)[0]
        assert [r[k] for k in r.dtype.names] == [getattr(c, k) for k, _ in L.PickMeshResult._fields_]
        assert r["face"] == ids[0, i] == 0 and abs(r["z"] - 2.0) < 1e-5 and r["t"] == o["t"][0, i].item()
    # the cloud of one point: met by the first pixel, missed by the last of 17
    o["ids"].fill_(-7)
    got = V.render_points(s.point, 0.5, s.cam, o["ids"], o["t"], o["header"], workspace=s.rws)
    assert got[0] is o["ids"] and got[1] is o["t"] and got[2] is o["header"]
    ids = o["ids"].cpu().numpy()
    for i in (0, w - 1):
        rec = V.pick_ray(s.point, origin, rays[i], 0.5, out=o["rec4"], workspace=s.ws)
        host = rec.cpu().numpy()
        c, (index, xyz) = L.PickResult.from_buffer_copy(host.tobytes()), V.read_pick(host)
        assert rec is o["rec4"] and (index, *xyz) == (c.index, c.x, c.y, c.z) and index == ids[0, i]
        assert index == (0 if i == 0 else -1) and xyz.tolist() == ([0.0, 0.0, 2.0] if i == 0 else [0.0, 0.0, 0.0])
    rows = V.nearest_rows([s.point, s.xyz], s.q, out=o["rows"], workspace=s.ws)
    assert rows is o["rows"] and rows.cpu().tolist() == [[0], [0]]
    lab, col, err = V.session_paint(s.labels, s.inv, s.xyz, s.colors, s.palette, None, 0.1, o["lab"], o["col"], o["err"])
    assert lab is o["lab"] and col is o["col"] and err is o["err"]
    assert lab.cpu().tolist() == [1, 0, 1] and err.item() == 0 and col.cpu().tolist() == [[1, 0, 0], [0.5, 0.5, 0.5], [1, 0, 0]]
    assert {k: t.data_ptr() for k, t in o.items()} == ptr
