"""Host side of the mesh pick (no GPU): ``ray_from_pixel``, the faces of a mesh ``scan.ply`` on the path
``load_scene_dir`` takes, and the two statements of the mesh pick rule that ``test_gpu_session_mesh.py`` holds the kernel
to (``pick_rule.py``: ``mesh_rule_f64`` and ``mesh_rule_f32``) -- checked against each other here, on the scene of
``session_kit.PlanesScene``, so that the GPU test compares the kernel with yardsticks that agree."""
import numpy as np
import pytest

from pick_rule import first_of, mesh_rule_f32, mesh_rule_f64
from session_kit import PlanesScene, rotation


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
