"""Host side of the mesh pick (no GPU): ``ray_from_pixel``, the faces of a mesh ``scan.ply`` on the path
``load_scene_dir`` takes, and the two statements of the mesh pick rule that ``test_gpu_session_mesh.py`` holds the kernel
to -- checked against each other here, so that the GPU test compares the kernel with yardsticks that agree.

The rule (include/agile3d_hip.h, a3d_pick_mesh): among the faces a ray crosses at a finite t > 0 the one with the smallest
t, ties -> the lower face index; double-sided, edges inclusive; faces with det == 0, a repeated index, a NaN coordinate or
an index outside [0, n) are skipped.

``mesh_rule_f64``  the rule in float64, Moeller-Trumbore form (NOT the kernel's arithmetic: an independent statement).
``mesh_rule_f32``  the kernel's arithmetic in numpy float32, one operation at a time, the double fallback included.
"""
import os

import numpy as np
import pytest

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of fp32


# ------------------------------------------------------------------------------------------- the rule, twice
def _valid_faces(faces, n):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < n)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return np.where(in_range[:, None], f, 0), in_range, in_range & distinct


def mesh_rule_f64(xyz, faces, o, d):
    """Per face, in float64: t (inf = no crossing), the weights u, v of the face's second and third vertex, and whether
    an index was out of range.  The fp32 inputs are exact in float64; its own rounding (1e-16) is nothing here."""
    f, in_range, ok = _valid_faces(faces, len(xyz))
    x = np.asarray(xyz, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        p = np.cross(d, e2)
        det = (e1 * p).sum(1)
        tv = o - a
        q = np.cross(tv, e1)
        u = (tv * p).sum(1) / det
        v = (q * d).sum(1) / det
        t = (e2 * q).sum(1) / det
        hit = ok & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0) & np.isfinite(t)
    return np.where(hit, t, np.inf), u, v, bool((~in_range).any())


def first_of(t):
    """(face or -1, t, gap to the next larger t) of a per-face t array under the order (t, face index)."""
    if len(t) == 0 or not np.isfinite(t).any():
        return -1, np.inf, np.inf
    best = int(np.argmin(t))                       # the first of equals: the lower index
    rest = np.delete(t, best)
    return best, float(t[best]), (float(rest.min()) - float(t[best]) if len(rest) else np.inf)


def shear_of(d32):
    """What a3d_pick_mesh derives from the unit direction on the host, in fp32: (kx, ky, kz, sx, sy, sz)."""
    d32 = np.asarray(d32, F32)
    kz = 0
    if abs(d32[1]) > abs(d32[kz]):
        kz = 1
    if abs(d32[2]) > abs(d32[kz]):
        kz = 2
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d32[kz] < 0:
        kx, ky = ky, kx
    return kx, ky, kz, F32(d32[kx] / d32[kz]), F32(d32[ky] / d32[kz]), F32(F32(1.0) / d32[kz])


def mesh_rule_f32(xyz32, faces, o32, d32):
    """The kernel's arithmetic, every fp32 operation rounded on its own, in the kernel's order.  Returns
    (face or -1, t as fp32, flags, (u, v, point) of the hit in fp32 or None)."""
    xyz32, o32 = np.asarray(xyz32, F32), np.asarray(o32, F32)
    f, in_range, ok = _valid_faces(faces, len(xyz32))
    flags = int((~in_range).any())
    if len(f) == 0:
        return -1, F32(0), flags, None
    kx, ky, kz, sx, sy, sz = shear_of(d32)
    with np.errstate(all="ignore"):
        a, b, c = xyz32[f[:, 0]] - o32, xyz32[f[:, 1]] - o32, xyz32[f[:, 2]] - o32      # translate (fp32 arrays: fp32 results)
        ax, ay = a[:, kx] - sx * a[:, kz], a[:, ky] - sy * a[:, kz]                      # permute and shear
        bx, by = b[:, kx] - sx * b[:, kz], b[:, ky] - sy * b[:, kz]
        cx, cy = c[:, kx] - sx * c[:, kz], c[:, ky] - sy * c[:, kz]
        uu = cx * by - cy * bx
        vv = ax * cy - ay * cx
        ww = bx * ay - by * ax
        assert uu.dtype == F32 and ax.dtype == F32
        z = (uu == 0) | (vv == 0) | (ww == 0)                                            # the double fallback
        if z.any():
            D = np.float64
            uu = np.where(z, (cx.astype(D) * by.astype(D) - cy.astype(D) * bx.astype(D)).astype(F32), uu)
            vv = np.where(z, (ax.astype(D) * cy.astype(D) - ay.astype(D) * cx.astype(D)).astype(F32), vv)
            ww = np.where(z, (bx.astype(D) * ay.astype(D) - by.astype(D) * ax.astype(D)).astype(F32), ww)
        mixed = ((uu < 0) | (vv < 0) | (ww < 0)) & ((uu > 0) | (vv > 0) | (ww > 0))
        det = (uu + vv) + ww
        az, bz, cz = sz * a[:, kz], sz * b[:, kz], sz * c[:, kz]
        tt = ((uu * az + vv * bz) + ww * cz) / det
        assert tt.dtype == F32
        hit = ok & ~mixed & (det != 0) & (tt > 0) & (tt < np.inf)
    if not hit.any():
        return -1, F32(0), flags, None
    key = np.where(hit, (tt.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(f), dtype=np.uint64),
                   np.uint64(0xffffffffffffffff))
    best = int(np.argmin(key))
    with np.errstate(all="ignore"):
        u, v = F32(vv[best] / det[best]), F32(ww[best] / det[best])
        w = F32(F32(F32(1.0) - u) - v)
        pa, pb, pc = xyz32[f[best, 0]], xyz32[f[best, 1]], xyz32[f[best, 2]]
        point = (w * pa + u * pb) + v * pc
    assert point.dtype == F32
    return best, tt[best], flags, (u, v, point)


# ------------------------------------------------------------------------------------------- the scene of tests 1-3
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


# ------------------------------------------------------------------------------------------- tests
def _camera(seed):
    rot = rotation(seed)
    centre = np.array([1.5, -2.0, 0.7])
    ext = np.eye(4)
    ext[:3, :3], ext[:3, 3] = rot, -rot @ centre
    intr = np.array([[520.0, 0.0, 319.5], [0.0, 515.0, 239.5], [0.0, 0.0, 1.0]])
    return intr, ext, centre


def test_ray_from_pixel_round_trip():
    """World points are projected through a rotated and translated camera to sub-pixel positions (px, py); the ray of
    the pixel that contains them, (floor px, floor py), must pass close to the point.

    The bound.  In camera coordinates the point is (xc, yc, z) with px = fx xc / z + cx.  The ray through the pixel's
    centre meets the plane of depth z at ((u + 0.5 - cx) z / fx, (v + 0.5 - cy) z / fy, z); |px - (u + 0.5)| <= 0.5, so
    that point is within 0.5 z / fx of the world point in x and 0.5 z / fy in y, and the distance of the world point to
    the ray is at most the distance to this one point of it: z hypot(0.5 / fx, 0.5 / fy).  Float64 evaluation of the chain
    (a 3 x 3 solve, a projection) adds ~1e-15 relative to coordinates of a few metres; 1e-9 m is allowed for it."""
    from agile3d_amd.session import ray_from_pixel
    intr, ext, centre = _camera(3)
    rng = np.random.default_rng(0)
    fx, fy, cx, cy = intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]
    done = 0
    while done < 200:
        cam = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(0.5, 8.0)])
        px, py = fx * cam[0] / cam[2] + cx, fy * cam[1] / cam[2] + cy
        if not (0 <= px < 640 and 0 <= py < 480):
            continue
        world = np.linalg.solve(ext[:3, :3], cam - ext[:3, 3])
        o, d = ray_from_pixel(int(np.floor(px)), int(np.floor(py)), intr, ext)
        w = world - o
        dist = np.linalg.norm(w - (w @ d) * d)
        assert dist <= cam[2] * np.hypot(0.5 / fx, 0.5 / fy) + 1e-9, (px, py, dist)
        assert w @ d > 0                                         # in front of the camera
        done += 1
    # a point exactly at a pixel centre lies on the ray
    cam = np.array([(100.5 - cx) / fx * 3.0, (50.5 - cy) / fy * 3.0, 3.0])
    world = np.linalg.solve(ext[:3, :3], cam - ext[:3, 3])
    o, d = ray_from_pixel(100, 50, intr, ext)
    assert np.linalg.norm((world - o) - ((world - o) @ d) * d) <= 1e-9


def test_ray_from_pixel_unit_direction_and_camera_centre():
    from agile3d_amd.session import ray_from_pixel
    intr, ext, centre = _camera(5)
    for u, v in ((0, 0), (639, 479), (320, 240), (17.25, 300.5)):
        o, d = ray_from_pixel(u, v, intr, ext)
        assert o.dtype == np.float64 and d.dtype == np.float64 and o.shape == d.shape == (3,)
        assert abs(np.linalg.norm(d) - 1.0) <= 4e-16
        assert np.allclose(o, centre, rtol=0, atol=1e-12)
    # the principal point looks along the camera's +z axis: the third row of the rotation
    o, d = ray_from_pixel(intr[0, 2] - 0.5, intr[1, 2] - 0.5, intr, ext)
    assert np.allclose(d, ext[2, :3], rtol=0, atol=1e-12)
    # identity camera: pixel (cx - 0.5 + fx, cy - 0.5) looks along (1, 0, 1) / sqrt 2
    o, d = ray_from_pixel(intr[0, 2] - 0.5 + intr[0, 0], intr[1, 2] - 0.5, intr, np.eye(4))
    assert np.allclose(o, 0) and np.allclose(d, np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        ray_from_pixel(0, 0, np.eye(4), np.eye(4))


def test_mesh_faces_survive_the_scene_dir_path(tmp_path):
    """What ``load_scene_dir`` does with a mesh ``scan.ply``: ``is_triangular_mesh`` then
    ``read_ply(..., triangular_mesh=True)`` -- the faces come back index for index, int32, degenerate ones included."""
    from agile3d_amd.ply import is_triangular_mesh, read_ply, write_ply
    rng = np.random.default_rng(1)
    xyz = rng.normal(size=(300, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (300, 3)).astype(np.uint8)
    faces = rng.integers(0, 300, (777, 3)).astype(np.int32)
    faces[5] = (7, 7, 9)                                          # a repeated index is data, not an error
    path = str(tmp_path / "scan.ply")
    assert write_ply(path, [xyz, rgb], ["x", "y", "z", "red", "green", "blue"], triangular_faces=faces)
    assert is_triangular_mesh(path)
    v, f = read_ply(path, triangular_mesh=True)
    assert f.dtype == np.int32 and f.shape == (777, 3) and np.array_equal(f, faces)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), xyz)
    cloud = str(tmp_path / "cloud.ply")
    assert write_ply(cloud, [xyz, rgb], ["x", "y", "z", "red", "green", "blue"])
    assert not is_triangular_mesh(cloud)


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (50.3, -48.7, 1.2)])
def test_the_two_statements_of_the_rule_agree(shift):
    """The fp32 restatement of the kernel and the float64 rule name the same face on rays aimed at interior points of
    random faces wherever the float64 margins are clear (smallest weight of the hit face > 1e-4, gap in t to the next
    surface > 1e-4 t), and few rays are left out by that condition: with a uniformly random point of a triangle the
    chance that one of its three weights is below 1e-4 is ~3e-4 x ... ~1e-3 with the gap condition; the cap is 5 %."""
    sc = PlanesScene(12, rotation(7), shift, seed=2)
    rng = np.random.default_rng(4)
    left_out = 0
    n_rays = 300
    for o in sc.origins(rng, n_rays):
        target = int(rng.integers(len(sc.faces)))
        o, d = sc.ray_to(o, sc.interior_point(rng, target))
        t, u, v, _ = mesh_rule_f64(sc.xyz, sc.faces, o, d)
        want, t0, gap = first_of(t)
        got, t32, flags, hit = mesh_rule_f32(sc.xyz, sc.faces, o, d)
        assert want >= 0 and got >= 0 and flags == 0
        if min(u[want], v[want], 1 - u[want] - v[want]) > 1e-4 and gap > 1e-4 * t0:
            assert got == want
            assert abs(float(t32) - t0) <= 1e-4 * t0
        else:
            left_out += 1
        assert sc.kind[got] != "back"
    assert left_out <= 0.05 * n_rays, left_out
