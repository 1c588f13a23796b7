"""-m gpu: the mesh pick (a3d_pick_mesh in csrc/session.hip; InteractiveSession.pick / click_ray on a triangle mesh).

No reference fixture exists for picking (the reference leaves it to Open3D's renderer): the yardsticks are the two
statements of the rule in ``pick_rule.py`` -- float64 (Moeller-Trumbore form) and the kernel's arithmetic in numpy
float32 -- which ``test_session_mesh_host.py`` holds against each other on the CPU.  The library is reached through
``session_kit.py``'s adaptors over ``agile3d_amd.view``.

1  bit identity with the fp32 restatement: face, t, u, v and hit point, at m = 0, 7, 256, 257 and 67 605 faces (the last
   is more than the first stage's 256 x 256 threads: the grid-stride loop takes a second trip), the aimed-at face at index
   0 and at m - 1, two placements, and all six (dominant axis, sign) cases of the permutation
2  the float64 rule's face wherever its margins are clear; the hit point against the float64 point
3  no leaks: rays at shared edges and vertices of the front plane never miss and never reach the back plane
4  occlusion through the session: a two-triangle wall in front of a tessellated object
5  the rule's details on hand-built faces
6  session plumbing
"""
import functools
import os

import numpy as np
import pytest
import torch

from agile3d_amd import view as V
from pick_rule import F32, U, first_of, mesh_rule_f32, mesh_rule_f64, shear_of
from session_kit import (DEV, PlanesScene, _model, f32_pointer, pick_mesh, pick_ray, rotation, status, subset_with_target)

pytestmark = pytest.mark.gpu
PLACEMENTS = {"near": (0.0, 0.0, 0.0), "far": (50.3, -48.7, 1.2)}
GRID = 130                                   # 2 x (2 x 130^2) + 5 = 67 605 faces > 65 536


@functools.lru_cache(maxsize=None)
def planes(placement, grid=GRID):
    return PlanesScene(grid, rotation(7), PLACEMENTS[placement], seed=2)


def aimed_rays(sc, rng, k, faces=None):
    """k rays from the origin box to uniformly random points of random faces (of ``faces``, indices into sc.faces)."""
    rays, targets = [], []
    for o in sc.origins(rng, k):
        f = int(rng.integers(len(sc.faces))) if faces is None else int(rng.choice(faces))
        rays.append(sc.ray_to(o, sc.interior_point(rng, f)))
        targets.append(f)
    return rays, targets


def same_bits(got, want):
    """One RESULT record against mesh_rule_f32's (face, t, flags, (u, v, point)): every field bit for bit."""
    face, t, flags, hit = want
    assert got["face"] == face and got["flags"] == flags, (got, want)
    if face < 0:
        assert got["t"] == 0 and got["u"] == 0 and got["v"] == 0 and got["x"] == 0 and got["y"] == 0 and got["z"] == 0
        return
    bits = lambda x: np.asarray(x, F32).view(np.uint32)
    assert bits(got["t"]) == bits(t), (got, want)
    assert bits(got["u"]) == bits(hit[0]) and bits(got["v"]) == bits(hit[1]), (got, want)
    assert np.array_equal(bits(np.array([got["x"], got["y"], got["z"]], F32)), bits(hit[2])), (got, want)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_bit_identity_with_the_fp32_restatement(placement):
    sc = planes(placement)
    assert len(sc.faces) == 2 * 2 * GRID * GRID + 5 > 256 * 256
    rng = np.random.default_rng(11)
    front = np.flatnonzero(sc.kind == "front")
    n_rays = hits = misses = 0
    for m, k in ((0, 6), (7, 30), (256, 30), (257, 30), (len(sc.faces), 40)):
        for at_end in (False, True):
            target = int(front[rng.integers(len(front))])
            faces, kinds = subset_with_target(sc, m, target, at_end) if m else (None, None)
            slot = (m - 1 if at_end else 0) if m else -1
            # the first ray: at the centroid of the face placed at index 0 / m - 1; then rays at random faces of the subset
            o0 = sc.origins(rng, 1)[0]
            rays = [sc.ray_to(o0, sc.xyz[sc.faces[target]].astype(np.float64).mean(0))]
            for o in sc.origins(rng, k - 1):
                f = sc.faces[target] if m == 0 else faces[rng.integers(m)]
                a, b, c = sc.xyz[f].astype(np.float64)
                r1, r2 = np.sqrt(rng.uniform()), rng.uniform()
                rays.append(sc.ray_to(o, (1 - r1) * a + r1 * (1 - r2) * b + r1 * r2 * c))
            got = pick_mesh(sc.xyz, faces, rays)
            for i, (o, d) in enumerate(rays):
                want = mesh_rule_f32(sc.xyz, np.zeros((0, 3), np.int32) if m == 0 else faces, o, d)
                same_bits(got[i], want)
                hits += want[0] >= 0
                misses += want[0] < 0
            if m:                                                  # the aimed-at face is a front face: nothing occludes it
                t64 = mesh_rule_f64(sc.xyz, faces, *rays[0])[0]
                assert first_of(t64)[0] == slot and got[0]["face"] == slot, (m, at_end, got[0])
            else:
                assert (got["face"] == -1).all() and (got["flags"] == 0).all()
            n_rays += len(rays)
    assert n_rays >= 270 and hits >= 230 and misses >= 12, (n_rays, hits, misses)


def test_bit_identity_on_every_axis_and_sign():
    """The permutation has six cases (dominant axis x, y, z; direction along it positive or negative, which swaps kx and
    ky): the scene turned so that the rays run mainly along each signed axis in turn."""
    seen = set()
    rng = np.random.default_rng(12)
    for axis in range(3):
        for sign in (1.0, -1.0):
            # the scene's own -z (the way its rays look) goes to sign * e_axis; a small generic turn on top
            rot = np.zeros((3, 3))
            rot[axis, 2] = -sign
            rot[(axis + 1) % 3, 0] = 1.0
            rot[(axis + 2) % 3, 1] = -sign
            assert abs(np.linalg.det(rot) - 1.0) < 1e-12
            tilt = rotation(3)
            tilt = np.eye(3) + 0.05 * (tilt - tilt.T)                     # near the identity
            tilt, r = np.linalg.qr(tilt)
            tilt = tilt * np.sign(np.diag(r))
            sc = PlanesScene(11, rot @ tilt, (1.0, -2.0, 0.5), seed=5)
            rays, _ = aimed_rays(sc, rng, 40)
            got = pick_mesh(sc.xyz, sc.faces, rays)
            for i, (o, d) in enumerate(rays):
                same_bits(got[i], mesh_rule_f32(sc.xyz, sc.faces, o, d))
                kx, ky, kz, sx, sy, sz = shear_of(d)
                seen.add((kz, bool(d[kz] < 0)))
            assert (got["face"] >= 0).all()
    assert len(seen) == 6, seen


# ---------------------------------------------------------------------------------------------------- 2
def point_bound(xyz, face, o, d):
    """Bound on |kernel hit point - float64 hit point| for a ray that crosses ``face``; u = 2^-24.

    Let M = the largest |coordinate| of the face's vertices, R = the largest |coordinate| of (vertex - origin), e = the
    longest edge, theta = the angle between the ray and the face's normal.

    (a) The sheared coordinates.  Ax = fl(akx - fl(sx akz)) with akx = fl(A[kx] - o[kx]): the two translations err by
    <= uR each (the second is multiplied by |sx| <= 1), sx = fl(d[kx] / d[kz]) by u relatively (<= uR in the product),
    the product's rounding <= uR, the subtraction's <= u |Ax| <= 2uR: <= 6uR per sheared coordinate, 6 sqrt2 uR per
    vertex in the sheared plane.  The kernel's weights are the exact weights of the ray in the triangle of the PERTURBED
    sheared vertices; applied to the true vertices they give a point of the face's plane whose image under the shear is
    within 6 sqrt2 uR of the ray.  The shear's projection shortens a vector of the face's plane by no more than a factor
    cos(theta) (the projection along d onto the plane perpendicular to d does exactly that in the worst in-plane
    direction; from there onto the plane perpendicular to the dominant axis lengths only grow), so the point is within
    6 sqrt2 uR / cos(theta) of the true crossing.
    (b) The edge functions.  The ray crosses the face, so every sheared coordinate is at most the sheared length of an
    edge, <= sqrt2 e (|sx|, |sy| <= 1).  U = fl(fl(Cx By) - fl(Cy Bx)): <= u (|Cx By| + |Cy Bx|) + u |U| <= 8u e^2.  A weight
    U / det, det = U + V + W = |n . d| / |d[kz]| (n = the face's unnormalised normal): its numerator errs by 8u e^2, its
    denominator by 3 x 8u e^2 + 2u det, the division by u: <= 32u e^2 / det + 3u per weight; two weights move the point
    along edges of length <= e: 2e (32u e^2 / det + 3u).
    (c) The combination.  w = fl(fl(1 - u) - v) errs by <= 2u, times |A| <= 2uM; the three products <= uM together (the
    weights sum to 1), the two additions <= 2uM, the roundings of u and v in the finish <= uM: 6uM per coordinate,
    6 sqrt3 uM in norm.
    For the scene of this test (M of 4 to 60 m, R up to 8 m, e = 0.25 m, cos(theta) >= 0.6) the sum is at most 7 (far
    placement) to 20 (near) times 2^-23 x the largest coordinate magnitude of vertices and origin -- a few ulps."""
    a, b, c = xyz[face].astype(np.float64)
    o, d = o.astype(np.float64), d.astype(np.float64)
    M = np.abs([a, b, c]).max()
    R = np.abs([a - o, b - o, c - o]).max()
    e = max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
    n = np.cross(b - a, c - a)
    cos = abs(n @ d) / np.linalg.norm(n)
    det = abs(n @ d) / np.abs(d).max()
    return 6 * np.sqrt(2) * U * R / cos + 2 * e * (32 * U * e * e / det + 3 * U) + 6 * np.sqrt(3) * U * M


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_against_the_float64_rule(placement):
    """300 rays aimed at uniformly random points of random faces (front, back -- occluded by the front plane -- and
    free).  Where the float64 margins are clear (smallest weight of the float64 hit face > 1e-4, gap in t to the next
    surface > 1e-4 t) the kernel names the float64 face.  A uniformly random point of a triangle has a weight below 1e-4
    with probability 3e-4, and the ray to an occluded back face crosses the front plane at an equally arbitrary point:
    ~1e-3 of the rays are expected to be left out (on the CPU, with the fp32 restatement: 1 of 300 in each placement);
    the test asserts the cap of 5 %.  A left-out ray still gets a face of the front plane (or, aimed at a free-standing
    triangle, that triangle or nothing: nothing else lies on such a ray)."""
    sc = planes(placement, 40)                                     # 6 405 faces: the float64 rule costs a millisecond per ray
    rng = np.random.default_rng(21)
    rays, targets = aimed_rays(sc, rng, 300)
    got = pick_mesh(sc.xyz, sc.faces, rays)
    left_out = 0
    worst = ulps = 0.0
    for i, (o, d) in enumerate(rays):
        t, u, v, bad = mesh_rule_f64(sc.xyz, sc.faces, o, d)
        want, t0, gap = first_of(t)
        g = got[i]
        assert want >= 0 and not bad and g["flags"] == 0
        clear = min(u[want], v[want], 1 - u[want] - v[want]) > 1e-4 and gap > 1e-4 * t0
        if not clear:
            left_out += 1
            if sc.kind[targets[i]] == "free":
                assert g["face"] in (targets[i], -1)
            else:
                assert g["face"] >= 0 and sc.kind[g["face"]] == "front"
            continue
        assert g["face"] == want, (i, g, want, t0, gap)
        assert sc.kind[want] == ("free" if sc.kind[targets[i]] == "free" else "front")
        a, b, c = sc.xyz[sc.faces[want]].astype(np.float64)
        p64 = (1 - u[want] - v[want]) * a + u[want] * b + v[want] * c
        p = np.array([g["x"], g["y"], g["z"]], np.float64)
        bound = point_bound(sc.xyz, sc.faces[want], o, d)
        err = np.linalg.norm(p - p64)
        worst = max(worst, err / bound)
        ulps = max(ulps, bound / (2 * U * max(np.abs([a, b, c]).max(), np.abs(o).max())))
        assert err <= bound, (i, err, bound)
        # the float64 point is on the ray: o + t d
        assert np.linalg.norm(p64 - (o.astype(np.float64) + t0 * d.astype(np.float64))) <= 1e-9
        # u, v and 1 - u - v reproduce the point: (c) of the bound alone
        gu, gv = float(g["u"]), float(g["v"])
        assert np.linalg.norm(p - ((1 - gu - gv) * a + gu * b + gv * c)) <= 6 * np.sqrt(3) * U * np.abs([a, b, c]).max()
    print(f"{placement}: left out {left_out} of {len(rays)}; worst point error / bound = {worst:.3f}; "
          f"largest bound = {ulps:.1f} x 2^-23 x the largest coordinate")
    assert left_out <= 0.05 * len(rays), left_out


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_no_ray_leaks_through_shared_edges_and_vertices(placement):
    """2 400 rays at points of interior edges of the front plane (lattice edges both ways and the quads' diagonals) and
    1 200 at its interior vertices, targets computed in float64, directions rounded to fp32: every ray gets a face of the
    front plane -- never nothing, never the back plane behind the crack."""
    sc = planes(placement)
    rng = np.random.default_rng(31)
    idx = sc.lattice["front"]
    x64 = sc.xyz.astype(np.float64)
    rays = []
    origins = sc.origins(rng, 3600)
    for k in range(2400):
        i, j = rng.integers(1, GRID - 1, 2)
        a = idx[i, j]
        b = (idx[i + 1, j], idx[i, j + 1], idx[i + 1, j + 1])[k % 3]
        s = rng.uniform()
        rays.append(sc.ray_to(origins[k], x64[a] + s * (x64[b] - x64[a])))
    for k in range(1200):
        i, j = rng.integers(1, GRID, 2)
        rays.append(sc.ray_to(origins[2400 + k], x64[idx[i, j]]))
    got = pick_mesh(sc.xyz, sc.faces, rays)
    assert (got["face"] >= 0).all(), int((got["face"] < 0).sum())
    kinds = sc.kind[got["face"]]
    assert (kinds == "front").all(), {k: int((kinds == k).sum()) for k in np.unique(kinds)}
    assert (got["flags"] == 0).all()


# ---------------------------------------------------------------------------------------------------- 4, 6
@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


def _wall_scene():
    """A 2 m x 2 m wall of two triangles at x = 0 and, 2 m behind it, a 1.4 m patch of 57 x 57 vertices 2.5 cm apart."""
    wall = np.array([[0, -1, -1], [0, 1, -1], [0, 1, 1], [0, -1, 1]], np.float64)
    g = np.arange(57) * 0.025 - 0.7
    y, z = np.meshgrid(g, g, indexing="ij")
    patch = np.stack([np.full_like(y, 2.0), y, z], -1).reshape(-1, 3)
    idx = 4 + np.arange(57 * 57).reshape(57, 57)
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.concatenate([[[0, 1, 2], [0, 2, 3]], np.stack([q00, q10, q11], -1).reshape(-1, 3),
                            np.stack([q00, q11, q01], -1).reshape(-1, 3)]).astype(np.int32)
    xyz = np.concatenate([wall, patch]).astype(np.float32)
    col = np.random.default_rng(0).uniform(0, 1, xyz.shape).astype(np.float32)
    return xyz, col, faces


def test_occlusion_wall_in_front_of_an_object(model_002):
    """The bug this fixes.  The ray starts 3 m in front of the wall, crosses it 10 and 15 cm off its middle -- 1.2 m from
    the nearest wall vertex -- and runs on exactly through a vertex of the object behind.  The vertex rule finds that
    vertex of the OBJECT (the wall has no vertex within a voxel of the ray); the surface rule finds the wall."""
    from agile3d_amd.session import InteractiveSession
    xyz, col, faces = _wall_scene()
    ses = InteractiveSession(model_002, voxel_size=0.02)
    ses.load_scene(xyz, col, faces=faces)
    target = xyz[4 + 34 * 57 + 36].astype(np.float64)               # a patch vertex: (2, 0.15, 0.2)
    origin = np.array([-3.0, 0.025, 0.075])
    direction = target - origin
    cross = origin + direction * (3.0 / 5.0)                        # where the ray meets x = 0: (0, 0.1, 0.15)
    assert np.allclose(cross, [0.0, 0.1, 0.15])
    behind = ses.pick(origin, direction, surface=False)
    assert behind is not None and np.array_equal(np.asarray(behind, np.float32), xyz[4 + 34 * 57 + 36])
    hit = ses.pick(origin, direction)
    assert hit is not None and np.abs(np.asarray(hit) - cross).max() <= 1e-5 and abs(hit[0]) <= 1e-6
    assert ses.pick(origin, direction, surface=True) == hit
    # click_ray books the voxel row nearest to the point on the wall: a corner of the wall, not the object
    rows = ses.click_ray(origin, direction, 1)
    qv = ses.raw_coords_qv.cpu().numpy().astype(np.float64)
    d2 = ((qv - np.asarray(hit, np.float64)) ** 2).sum(1)
    assert rows[0] == int(d2.argmin()) and np.sort(d2)[1] - d2.min() > 1e-3
    assert qv[rows[0]][0] == 0.0                                    # a wall vertex
    assert ses.click_idx == {"0": [], "1": [rows[0]]} and ses.num_clicks == 1
    assert rows == ses.nearest(hit)
    # a ray that meets nothing books nothing
    assert ses.click_ray([-3.0, 5.0, 5.0], [-1.0, 0.0, 0.0], 1) is None
    assert ses.click_idx == {"0": [], "1": [rows[0]]} and ses.num_clicks == 1


def test_session_plumbing(model_002, tmp_path):
    from agile3d_amd.ply import write_ply
    from agile3d_amd.session import InteractiveSession
    xyz, col, faces = _wall_scene()
    rgb = np.round(col * 255).astype(np.uint8)
    folder = tmp_path / "scene_wall"
    os.makedirs(folder)
    assert write_ply(str(folder / "scan.ply"), [xyz, rgb], ["x", "y", "z", "red", "green", "blue"], triangular_faces=faces)
    ses = InteractiveSession(model_002, voxel_size=0.02)
    ses.load_scene_dir(str(folder))
    assert ses.faces is not None and ses.faces.dtype == torch.int32 and ses.faces.is_cuda
    assert np.array_equal(ses.faces.cpu().numpy(), faces)
    origin, direction = np.array([-3.0, 0.025, 0.075]), np.array([5.0, 0.125, 0.125])
    script = [(origin, direction), (origin + [0, 0.3, 0], direction), ([-3.0, 0.0, 0.0], [1.0, 0.9, 0.0]),
              ([-3.0, 5.0, 5.0], [-1.0, 0.0, 0.0])]
    first = [ses.pick(o, d) for o, d in script]
    assert first[0] is not None and first[1] is not None and first[3] is None
    assert [ses.pick(o, d) for o, d in script] == first            # the same script twice
    vertex_rule = [ses.pick(o, d, surface=False) for o, d in script]
    # a point cloud after the mesh: no faces left behind, pick is the vertex pick of the same rays
    ses.load_scene(xyz, col)
    assert ses.faces is None
    assert [ses.pick(o, d) for o, d in script] == vertex_rule
    assert [ses.pick(o, d, surface=False) for o, d in script] == vertex_rule
    assert vertex_rule[0] != first[0]
    with pytest.raises(ValueError):
        ses.pick(origin, direction, surface=True)                   # no faces
    # and the vertex pick is a3d_pick_ray itself
    index, vertex = pick_ray(ses.coords_full, origin, (direction / np.linalg.norm(direction)).astype(F32), 0.02, workspace=ses._ws)
    assert index >= 0 and [float(x) for x in vertex] == vertex_rule[0]
    # faces out of range raise at load, and leave no scene behind
    for bad in (len(xyz), -1):
        f = faces.copy()
        f[7, 1] = bad
        with pytest.raises(ValueError):
            ses.load_scene(xyz, col, faces=f)
        assert ses.faces is None
    with pytest.raises(ValueError):
        ses.load_scene(xyz, col, faces=faces[:, :2])
    # a fresh session on the arrays gives the picks of the folder
    fresh = InteractiveSession(model_002, voxel_size=0.02)
    fresh.load_scene(xyz.astype(np.float64), rgb.astype(np.float64) / 255.0, faces=torch.from_numpy(faces).long())
    assert [fresh.pick(o, d) for o, d in script] == first


# ---------------------------------------------------------------------------------------------------- 5
def test_rule_details():
    nan = np.nan
    xyz = np.array([[0, 0, 2], [1, 0, 2], [0, 1, 2],                # 0-2   a triangle in the plane z = 2
                    [0, 0, 1], [1, 0, 1], [2, 0, 1],                # 3-5   collinear: zero area
                    [0, 0, 1.5], [1, 0, 1.5], [nan, 1, 1.5],        # 6-8   a NaN vertex
                    [0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], F32)    # 9-11  used by the faces with a repeated / bad index
    o = np.array([0.25, 0.25, 0.0], F32)
    up, down = np.array([0, 0, 1], F32), np.array([0, 0, -1], F32)
    one = lambda faces, o, d, pts=xyz: pick_mesh(pts, np.asarray(faces, np.int32).reshape(-1, 3), [(o, d)])[0]
    # both windings are hit, at t = 2 exactly, with weights u = v = 0.25 and the point on the triangle
    for f in ([0, 1, 2], [0, 2, 1]):
        g = one([f], o, up)
        assert g["face"] == 0 and g["flags"] == 0 and g["t"] == 2.0 and (g["x"], g["y"], g["z"]) == (0.25, 0.25, 2.0)
        assert g["u"] == 0.25 and g["v"] == 0.25
    # and from the other side (a back face for the first winding, a front face for the second)
    assert one([[0, 1, 2]], np.array([0.25, 0.25, 4.0], F32), down)["face"] == 0
    # behind the origin: not hit
    assert one([[0, 1, 2]], o, down)["face"] == -1
    assert one([[0, 1, 2]], np.array([0.25, 0.25, 2.0], F32), up)["face"] == -1          # t = 0 exactly: not > 0
    # parallel to the plane: beside it, and inside it (det == 0)
    x_dir = np.array([1, 0, 0], F32)
    assert one([[0, 1, 2]], np.array([-1, 0.25, 2.5], F32), x_dir)["face"] == -1
    assert one([[0, 1, 2]], np.array([-1, 0.25, 2.0], F32), x_dir)["face"] == -1
    # edges and vertices are inclusive
    assert one([[0, 1, 2]], np.array([0.5, 0.0, 0.0], F32), up)["face"] == 0               # on the edge y = 0
    assert one([[0, 1, 2]], np.array([0.5, 0.5, 0.0], F32), up)["face"] == 0               # on the hypotenuse
    assert one([[0, 1, 2]], np.array([0.0, 0.0, 0.0], F32), up)["face"] == 0               # at vertex 0
    assert one([[0, 1, 2]], np.array([0.5, 0.5 + 2.0 ** -20, 0.0], F32), up)["face"] == -1  # just outside
    # degenerate, NaN and repeated-index faces in front of the triangle are skipped, silently
    front = [[3, 4, 5], [6, 7, 8], [9, 9, 11], [9, 10, 10], [11, 10, 11]]
    g = one(front + [[0, 1, 2]], o, up)
    assert g["face"] == 5 and g["flags"] == 0 and g["t"] == 2.0
    assert one(front, o, up)["face"] == -1
    assert one([[3, 4, 5]], np.array([0.5, 0.0, 0.0], F32), up)["face"] == -1              # a ray THROUGH the zero-area face
    # out-of-range indices: skipped, and reported in flags
    for bad in (12, -1, 2 ** 31 - 1, -2 ** 31):
        g = one([[9, 10, bad], [0, 1, 2]], o, up)
        assert g["face"] == 1 and g["flags"] == 1 and g["t"] == 2.0, (bad, g)
        g = one([[0, 1, 2], [bad, 10, 11]], o, up)
        assert g["face"] == 0 and g["flags"] == 1
        g = one([[bad, bad, bad]], o, up)
        assert g["face"] == -1 and g["flags"] == 1
    assert one([[9, 10, 11], [0, 1, 2]], o, up)["flags"] == 0
    # coplanar duplicates: the lower index, wherever it sits among 300 faces (more than one workgroup)
    many = np.tile(np.array([[3, 4, 5]], np.int32), (300, 1))
    many[[40, 299]] = [0, 1, 2]
    assert one(many, o, up)["face"] == 40
    many[[40, 270]] = [[3, 4, 5], [0, 1, 2]]
    assert one(many, o, up)["face"] == 270
    # of two surfaces the nearer wins although it is stored later
    g = one([[0, 1, 2], [9, 10, 11]], o, up)
    assert g["face"] == 1 and g["t"] == 0.5
    # no faces at all
    g = pick_mesh(xyz, None, [(o, up)])[0]
    assert g["face"] == -1 and g["flags"] == 0
    # the argument checks of a3d_pick_mesh: the entry point as it is (sizes no tensor of this test has)
    ws = V.session_workspace(DEV)
    out = torch.zeros(8, dtype=torch.int32, device=DEV)
    dev = torch.from_numpy(xyz).to(DEV)
    fdev = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=DEV)
    call = lambda n, m, d, ws_bytes: status("a3d_pick_mesh", dev.data_ptr(), n, fdev.data_ptr(), m, f32_pointer(o),
                                            f32_pointer(d), out.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call(12, 1, up, ws.numel()) == 0
    assert call(12, 1, 2 * up, ws.numel()) != 0                     # not a unit vector
    assert call(12, 2 ** 31, up, ws.numel()) != 0 and call(2 ** 31, 1, up, ws.numel()) != 0
    assert call(12, 1, up, 64) != 0                                  # workspace too small
    torch.cuda.synchronize()
