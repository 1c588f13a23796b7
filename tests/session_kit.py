"""What the session family's tests share (not collected, like ``backbone_fixture.py``): the fixture loader, scenes,
cameras, the model builder, and numpy-in / numpy-out adaptors over ``agile3d_amd.view`` -- the one way these tests reach the
session's entry points of the library.  An adaptor uploads its arrays, creates the outputs as sentinels (so that an
untouched output shows), calls the wrapper and copies back.  The rules the kernels are held to are in ``pick_rule.py``,
``render_rule.py`` and ``shade_rule.py``."""
import ctypes as C
import functools
import json
import os

import numpy as np
import torch

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.session import camera_from_matrices
from conftest import GOLDEN
from pick_rule import F32, U

DEV = "cuda"
CASES = ("near", "far")
FAR = np.array([50.3, -48.7, 1.2])
RESULT = V.PICK_MESH
bits = lambda x: np.ascontiguousarray(x, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------- fixtures, the model
def load_session_case(name):
    z = np.load(os.path.join(GOLDEN, f"session_case_{name}.npz"))
    with open(os.path.join(GOLDEN, f"session_case_{name}.json")) as f:
        return {k: z[k] for k in z.files}, json.load(f)


def f64_argmin(rows, p):
    return int(((rows.astype(np.float64) - p.astype(np.float64)) ** 2).sum(1).argmin())



def _model(voxel_size):
    from agile3d_amd import build_model, default_args, randomize_bn_stats
    torch.manual_seed(0)
    return randomize_bn_stats(build_model(default_args(voxel_size=voxel_size))).eval().to(DEV)


def model_005():
    return _model(0.05)


# ------------------------------------------------------------------------------------------- cameras
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4 x 4 world-to-camera, +z towards ``target``, +y down the image."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    ext = np.eye(4)
    ext[:3, :3] = np.stack([x, y, z])
    ext[:3, 3] = -ext[:3, :3] @ eye
    return ext


def intrinsic(w, h, fov_deg=60.0):
    f = 0.5 * w / np.tan(np.radians(fov_deg) / 2)
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])


def camera_of(eye, target, fov, size):
    w, h = size
    return camera_from_matrices(intrinsic(w, h, fov), look_at(eye, target), w, h)


def sampled_pixels(w, h, k=64):
    rng = np.random.default_rng(w * h)
    if w * h <= k:
        return [(i, j) for j in range(h) for i in range(w)]
    return [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(k)]



# ------------------------------------------------------------------------------------------- scenes
def rotation(seed):
    """A generic rotation (QR of a seeded Gaussian matrix, determinant +1)."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


class PlanesScene:
    """Two parallel jittered planes, each a ``grid`` x ``grid`` lattice of quads split into two triangles, the front one
    (6 m x 6 m at z = 0 in the scene's own frame) covering the back one (4 m x 4 m at z = -0.5) for every ray that starts
    in the origin box (|x|, |y| <= 1, 3 <= z <= 6), plus 5 free-standing triangles beside the planes (x > 3.5) that
    occlude nothing.  Faces are shuffled, so front, back and free faces interleave.  The whole scene -- vertices and ray
    origins -- is then rotated by ``rot`` and translated by ``shift``; vertices are fp32."""

    def __init__(self, grid, rot=None, shift=(0.0, 0.0, 0.0), seed=0):
        rng = np.random.default_rng(seed)
        self.rot = np.eye(3) if rot is None else np.asarray(rot, np.float64)
        self.shift = np.asarray(shift, np.float64)
        verts, faces, kind = [], [], []
        self.lattice = {}
        base = 0
        for name, half, z in (("front", 3.0, 0.0), ("back", 2.0, -0.5)):
            cell = 2 * half / grid
            g = np.linspace(-half, half, grid + 1)
            x, y = np.meshgrid(g, g, indexing="ij")
            p = np.stack([x, y, np.full_like(x, z)], -1)
            p[1:-1, 1:-1, :2] += rng.uniform(-0.25 * cell, 0.25 * cell, (grid - 1, grid - 1, 2))
            p[..., 2] += rng.uniform(-0.05 * cell, 0.05 * cell, p.shape[:2])
            idx = base + np.arange((grid + 1) ** 2).reshape(grid + 1, grid + 1)
            q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
            tri = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])
            verts.append(p.reshape(-1, 3))
            faces.append(tri)
            kind += [name] * len(tri)
            self.lattice[name] = idx
            base += (grid + 1) ** 2
        for k in range(5):
            c = np.array([4.0 + 0.3 * k, -2.0 + k, 1.0 + 0.2 * k])
            verts.append(c + rng.uniform(-0.3, 0.3, (3, 3)) * np.array([1.0, 1.0, 0.2]))
            faces.append(np.array([[base, base + 1, base + 2]]))
            kind.append("free")
            base += 3
        own = np.concatenate(verts)
        self.xyz = (own @ self.rot.T + self.shift).astype(F32)
        f = np.concatenate(faces).astype(np.int32)
        perm = rng.permutation(len(f))
        self.faces = np.ascontiguousarray(f[perm])
        self.kind = np.asarray(kind)[perm]

    def origins(self, rng, k):
        own = np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), rng.uniform(3, 6, k)], 1)
        return (own @ self.rot.T + self.shift).astype(F32)

    def ray_to(self, origin32, target64):
        """fp32 (origin, unit direction) of the ray from ``origin32`` to ``target64``, computed in float64."""
        d = np.asarray(target64, np.float64) - origin32.astype(np.float64)
        return origin32, (d / np.linalg.norm(d)).astype(F32)

    def interior_point(self, rng, face):
        """A uniformly random point of ``face`` (float64, from its fp32 vertices)."""
        a, b, c = self.xyz[self.faces[face]].astype(np.float64)
        r1, r2 = np.sqrt(rng.uniform()), rng.uniform()
        return (1 - r1) * a + r1 * (1 - r2) * b + r1 * r2 * c


def subset_with_target(scene, m, target, at_end):
    """``m`` faces of the scene -- its first m, shuffled as they are -- with face ``target`` moved to index 0 or m - 1
    (the displaced face takes the target's place when that lies inside the subset).  Returns (faces, kinds)."""
    order = np.arange(len(scene.faces))
    slot = m - 1 if at_end else 0
    where = int(np.flatnonzero(order == target)[0])
    order[where], order[slot] = order[slot], order[where]
    order = order[:m]
    return np.ascontiguousarray(scene.faces[order]), scene.kind[order]



def jittered_grid(nx, ny, seed=0, shift=(0.0, 0.0, 0.0)):
    """(xyz fp32 [nx * ny, 3], faces int32): a lattice 0.1 apart in the plane z = 0, jittered in all three directions, two
    triangles per cell."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx) * 0.1, np.arange(ny) * 0.1, indexing="ij")
    p = np.stack([x, y, np.zeros_like(x)], -1) + rng.uniform(-0.03, 0.03, (nx, ny, 3))
    idx = np.arange(nx * ny).reshape(nx, ny)
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])
    return (p.reshape(-1, 3) + np.asarray(shift)).astype(F32), faces.astype(np.int32)



def _grid_faces(idx):
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    return np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3)])


def _plane(grid, rng):
    """A jittered lattice of grid x grid quads in the plane z = 0, x in [-1, 1], y in [0, 12]: seen from (0, -1, 0.6) it
    recedes, its far faces smaller than a pixel of a 37-pixel image."""
    gx, gy = np.linspace(-1, 1, grid + 1), np.linspace(0, 12, grid + 1)
    x, y = np.meshgrid(gx, gy, indexing="ij")
    p = np.stack([x, y, np.zeros_like(x)], -1)
    p[1:-1, 1:-1, :2] += rng.uniform(-0.2, 0.2, (grid - 1, grid - 1, 2)) * [2 / grid, 12 / grid]
    p[..., 2] += rng.uniform(-0.01, 0.01, p.shape[:2])
    return p.reshape(-1, 3), _grid_faces(np.arange((grid + 1) ** 2).reshape(grid + 1, grid + 1))


def _box(k=3):
    """A closed box [-1, 1]^3, every side k x k quads: around a camera inside it faces lie ahead, cross the camera plane
    and lie wholly behind."""
    g = np.linspace(-1, 1, k + 1)
    a, b = np.meshgrid(g, g, indexing="ij")
    verts, faces = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = np.empty((k + 1, k + 1, 3))
            p[..., axis], p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = side, a, b
            faces.append(_grid_faces(len(verts) * (k + 1) ** 2 + np.arange((k + 1) ** 2).reshape(k + 1, k + 1)))
            verts.append(p.reshape(-1, 3))
    return np.concatenate(verts), np.concatenate(faces)



@functools.lru_cache(maxsize=None)
def mesh_scene(name):
    """(xyz fp32, faces int32, eye, target, fov, expected flags)."""
    rng = np.random.default_rng(5)
    if name == "quad larger than the view":
        xyz = np.array([[-50, 4, -50], [50, 4, -50], [50, 4, 50], [-50, 4, 50]], np.float64)
        return xyz.astype(F32), np.array([[0, 1, 2], [0, 2, 3]], np.int32), [0.2, 0.0, 0.1], [0.0, 4.0, 0.0], 70.0, 0
    if name in ("receding plane", "receding plane at 50 m"):
        xyz, faces = _plane(14, rng)                                   # 392 faces
        shift = FAR if name.endswith("50 m") else np.zeros(3)
        return (xyz + shift).astype(F32), faces.astype(np.int32), shift + [0.0, -1.0, 0.6], shift + [0.0, 3.0, 0.0], 60.0, 0
    if name == "inside a box":
        xyz, faces = _box()
        # and a slanted face across the box whose bounding box holds the camera: no bound, every pixel tests it
        faces = np.concatenate([faces, [[len(xyz), len(xyz) + 1, len(xyz) + 2]]])
        xyz = np.concatenate([xyz, [[0.0, -1.0, -1.0], [0.0, 1.0, -1.0], [1.6, 0.0, 1.0]]])
        return xyz.astype(F32), faces.astype(np.int32), [0.3, -0.2, 0.1], [1.0, 0.4, 0.3], 100.0, 0
    if name == "bad faces":
        xyz, faces = _plane(6, rng)
        nan_vertex = len(xyz)
        xyz = np.concatenate([xyz, [[np.nan, 1.0, 0.5]]])
        bad = [[0, 0, 5], [3, 9, nan_vertex], [1, 2, len(xyz)], [-1, 4, 7], [0, 7, 14]]   # repeated, NaN, out of range x 2, collinear
        xyz[[0, 7, 14]] = [[-1, 0, 0.5], [-0.5, 1, 0.5], [0, 2, 0.5]]                      # (three lattice vertices moved onto a line)
        return xyz.astype(F32), np.concatenate([bad, faces]).astype(np.int32), [0.0, -1.0, 0.6], [0.0, 3.0, 0.0], 60.0, 1
    raise KeyError(name)



@functools.lru_cache(maxsize=None)
def cloud_scene(name):
    """(xyz fp32, radius, eye, target, fov).  ~2 000 points on a receding sheet whose discs (radius 6 cm: 2 to 40 pixels of
    a 37-pixel image) straddle tile borders, exact duplicates of 20 of them at higher rows, and a point 3 cm from the eye,
    to its right: it is the first vertex of the rays that look far enough to the right, and of no others."""
    rng = np.random.default_rng(8)
    shift = FAR if name.endswith("50 m") else np.zeros(3)
    eye = shift + [0.0, -1.0, 0.6]
    p = np.stack([rng.uniform(-1.5, 1.5, 2000), rng.uniform(-0.6, 6.0, 2000), rng.uniform(-0.05, 0.05, 2000)], 1) + shift
    near = eye + [0.03, -0.012, 0.0]
    xyz = np.concatenate([p, p[:20], [near]]).astype(F32)
    return xyz, 0.06, eye, shift + [0.0, 3.0, 0.0], 60.0



# ------------------------------------------------------------------------------------------- the library, numpy in / numpy out
def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def nearest_rows(sources, queries):
    """a3d_nearest_rows: list of fp32 [n, 3] arrays x fp32 [m, 3] queries -> int32 [n_sources, m]."""
    out = torch.full((len(sources), len(queries)), -7, dtype=torch.int32, device=DEV)
    return V.nearest_rows([_dev(s, F32) for s in sources], queries, out=out).cpu().numpy()


def pick_ray(xyz_dev, o, d, r, workspace=None):
    """a3d_pick_ray on a device tensor: (index, the vertex fp32 [3])."""
    out = torch.zeros(4, dtype=torch.int32, device=DEV)
    return V.read_pick(V.pick_ray(xyz_dev, o, d, r, out=out, workspace=workspace).cpu().numpy())


def pick_mesh(xyz, faces, rays):
    """a3d_pick_mesh for every (origin, direction) of ``rays`` on one mesh: a RESULT record array, one copy at the end."""
    xyz_dev = _dev(xyz, F32)
    faces_dev = _dev(np.zeros((0, 3)) if faces is None else faces, np.int32)
    out = torch.full((max(len(rays), 1) * 8,), -7, dtype=torch.int32, device=DEV)
    ws = V.session_workspace(DEV)
    for i, (o, d) in enumerate(rays):
        V.pick_mesh(xyz_dev, faces_dev, o, d, out=out[8 * i:8 * i + 8], workspace=ws)
    return V.read_pick_mesh(out.cpu().numpy())[:len(rays)]


def session_paint(labels_qv, inverse_map, xyz32, colors32, palette, cubes, cube_size):
    n = len(inverse_map)
    lab = torch.full((n,), -9, dtype=torch.int32, device=DEV)
    out = torch.full((n, 3), -9.0, dtype=torch.float32, device=DEV)
    err = torch.ones(1, dtype=torch.int32, device=DEV)
    V.session_paint(_dev(labels_qv, np.int32), _dev(inverse_map, np.int64), _dev(xyz32, F32), _dev(colors32, F32),
                    _dev(palette, F32), _dev(cubes, F32) if len(cubes) else None, cube_size, lab, out, err)
    return lab.cpu().numpy(), out.cpu().numpy(), int(err.cpu()[0])


def render(xyz, faces, cam, radius=None, capacity=1 << 16, uv=True):
    """a3d_render_mesh (``faces`` an array, possibly empty) or a3d_render_points (``faces`` None), one attempt.  The images
    start as sentinels (-7 / -7.0) so that an untouched image shows."""
    h, w = cam.height, cam.width
    xyz_dev = _dev(np.asarray(xyz, F32).reshape(-1, 3), F32)
    mesh = faces is not None
    faces_dev = _dev(np.asarray(faces).reshape(-1, 3), np.int32) if mesh else None
    ids = torch.full((h, w), -7, dtype=torch.int32, device=DEV)
    t, u, v = (torch.full((h, w), -7.0, dtype=torch.float32, device=DEV) for _ in range(3))
    header = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    if mesh:
        V.render_mesh(xyz_dev, faces_dev, cam, ids, t, u if uv else None, v if uv else None, uv, header, capacity=capacity)
    else:
        V.render_points(xyz_dev, float(radius), cam, ids, t, header, capacity=capacity)
    flags, n_everywhere, pairs = V.read_render_header(header.cpu().numpy())
    return dict(ids=ids.cpu().numpy(), t=t.cpu().numpy(), u=u.cpu().numpy(), v=v.cpu().numpy(), flags=flags,
                n_everywhere=n_everywhere, pairs=pairs, dev=(ids, u, v, faces_dev))


def _shade_inputs(r, faces, colors, sentinel):
    """(ids, u, v, faces) on the device as the shading passes take them -- u, v, faces None on a cloud -- the colours and
    an rgb image filled with ``sentinel``."""
    ids, u, v, faces_dev = r["dev"]
    mesh = faces is not None
    rgb = torch.full((*ids.shape, 3), sentinel, dtype=torch.uint8, device=DEV)
    return (ids, u if mesh else None, v if mesh else None, faces_dev if mesh else None), _dev(colors, F32).reshape(-1, 3), rgb


def shade(r, faces, colors, background, n_vertices):
    """a3d_render_shade on the device images of ``render``."""
    images, col, rgb = _shade_inputs(r, faces, colors, 0)
    return V.render_shade(*images, col[:n_vertices], background, rgb=rgb).cpu().numpy()


def shade_lit(r, faces, colors, normals, cam, ambient, background, n_vertices):
    """a3d_render_shade_lit on the device images of ``render``."""
    images, col, rgb = _shade_inputs(r, faces, colors, 7)
    return V.render_shade_lit(*images, col[:n_vertices], _dev(normals, F32).reshape(-1, 3), cam, ambient, background,
                              rgb=rgb).cpu().numpy()


def shade_depth(r, t, faces, colors, strength, background, n_vertices):
    """a3d_render_shade_depth on the device images of ``render`` (``t``: the host copy of its t image)."""
    images, col, rgb = _shade_inputs(r, faces, colors, 7)
    return V.render_shade_depth(images[0], _dev(t, F32), *images[1:], col[:n_vertices], strength, background,
                                rgb=rgb).cpu().numpy()


def normals_gpu(xyz, faces, offsets, corners):
    """a3d_vertex_normals; the output starts as a sentinel."""
    out = torch.full((len(xyz), 3), -7.0, dtype=torch.float32, device=DEV)
    return V.vertex_normals(_dev(np.asarray(xyz, F32).reshape(-1, 3), F32), _dev(np.asarray(faces).reshape(-1, 3), np.int32),
                            _dev(offsets, np.int64), _dev(corners, np.int32), out=out).cpu().numpy()


# ------------------------------------------------------------------------------------------- the library's own refusals
# The wrappers refuse a malformed argument before the library sees it, so the tests of the C ABI's argument checks (null
# pointers, sizes no tensor can have) call the entry point as it is: ``status`` returns its code.
def status(entry, *args):
    return getattr(L.load(), entry)(*args)


def byref(structure):
    return C.byref(structure)


def f32_pointer(values):
    """A host fp32 array as the ``const float*`` of the C ABI (kept alive by the pointer object)."""
    return np.ascontiguousarray(values, F32).ctypes.data_as(C.POINTER(C.c_float))

