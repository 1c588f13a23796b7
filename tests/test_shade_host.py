"""Host side of the lit view (no GPU): the incidence lists ``load_scene`` builds for ``a3d_vertex_normals``, the camera
``default_view`` derives from a scene, and the numpy restatement of the normal rule (``shade_rule.py``) that
``test_gpu_shade.py`` holds the kernel to.  ``jittered_grid`` is in ``session_kit.py``."""
import numpy as np
import pytest

from agile3d_amd.session import camera_from_matrices, framing_view, vertex_corner_lists
from pick_rule import F32
from session_kit import jittered_grid
from shade_rule import vertex_normals_rule


def test_corner_lists_on_a_hand_made_mesh():
    # vertex 4 is isolated, face 2 lists vertex 0 twice, face 3 has an index outside [0, 6)
    faces = np.array([[0, 1, 2], [2, 1, 3], [0, 5, 0], [1, 6, 2]], np.int32)
    offsets, corners = vertex_corner_lists(faces, 6)
    assert offsets.dtype == np.int64 and corners.dtype == np.int32 and offsets.shape == (7,) and corners.shape == (12,)
    lists = [corners[offsets[v]:offsets[v + 1]].tolist() for v in range(6)]
    assert lists == [[0, 6, 8], [1, 4, 9], [2, 3, 11], [5], [], [7]]
    assert offsets[0] == 0 and offsets[6] == 11 and corners[11] == 10           # the corner that belongs to no vertex, behind
    for v, own in enumerate(lists):
        assert own == sorted(own) and all(faces.reshape(-1)[c] == v for c in own)
    assert sorted(corners.tolist()) == list(range(12))
    # no faces, and a grid: every corner once, in its vertex's list
    offsets, corners = vertex_corner_lists(np.zeros((0, 3), np.int32), 3)
    assert offsets.tolist() == [0, 0, 0, 0] and corners.shape == (0,)
    xyz, faces = jittered_grid(7, 5)
    offsets, corners = vertex_corner_lists(faces, len(xyz))
    assert np.array_equal(faces.reshape(-1)[corners], np.repeat(np.arange(len(xyz)), np.diff(offsets)))
    assert (np.diff(corners)[np.diff(faces.reshape(-1)[corners]) == 0] > 0).all()
    with pytest.raises(ValueError):
        vertex_corner_lists(np.zeros(4, np.int32), 3)


def _scene(name):
    rng = np.random.default_rng(11)
    if name == "random cloud":
        return rng.normal(0.0, [2.0, 0.5, 1.0], (500, 3))
    if name == "flat plane":
        x, y = np.meshgrid(np.linspace(-3, 3, 13), np.linspace(0, 8, 17), indexing="ij")
        return np.stack([x, y, np.full_like(x, 0.7)], -1).reshape(-1, 3)
    if name == "50 m from the origin":
        return rng.uniform(-1.5, 1.5, (400, 3)) * [1.0, 2.0, 0.3] + [50.3, -48.7, 1.2]
    raise KeyError(name)


@pytest.mark.parametrize("size", [(64, 48), (48, 64), (37, 29), (16, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["random cloud", "flat plane", "50 m from the origin"])
def test_default_view_frames_the_scene(name, size):
    xyz = _scene(name)
    w, h = size
    k, e = framing_view(xyz, w, h)
    assert k.shape == (3, 3) and e.shape == (4, 4) and k.dtype == np.float64 and e.dtype == np.float64
    rot, trans = e[:3, :3], e[:3, 3]
    assert np.array_equal(rot @ rot.T, np.eye(3)) and np.linalg.det(rot) == pytest.approx(1.0, abs=1e-12)
    assert np.array_equal(rot, [[1, 0, 0], [0, 0, -1], [0, 1, 0]]) and np.array_equal(e[3], [0, 0, 0, 1])
    assert k[0, 0] == k[1, 1] == pytest.approx(0.5 * h / np.tan(np.radians(17.5)), rel=1e-12)
    assert k[0, 2] == w / 2 and k[1, 2] == h / 2 and k[0, 1] == k[1, 0] == 0 and np.array_equal(k[2], [0, 0, 1])
    cam_space = xyz @ rot.T + trans
    assert (cam_space[:, 2] > 0).all()
    px = cam_space @ k.T
    px = px[:, :2] / px[:, 2:]
    assert (px[:, 0] >= 0).all() and (px[:, 0] <= w).all() and (px[:, 1] >= 0).all() and (px[:, 1] <= h).all()
    # the eye looks at the bounding box's centre along +y, and the frame is not loose: the farthest point of the bounding
    # sphere reaches at least a third of the way from the principal point to the nearer border
    centre = 0.5 * (xyz.min(0) + xyz.max(0))
    eye = -rot.T @ trans
    assert np.allclose(eye[[0, 2]], centre[[0, 2]], atol=1e-9) and eye[1] < xyz[:, 1].min()
    reach = np.abs(px - [w / 2, h / 2]).max()
    assert reach >= min(w, h) / 6
    cam = camera_from_matrices(k, e, w, h)
    assert cam.width == w and cam.height == h
    assert np.allclose(np.array(cam.o[:]), eye, rtol=1e-6)
    # a wider field of view moves the eye closer
    assert -np.linalg.solve(rot, framing_view(xyz, w, h, 70.0)[1][:3, 3])[1] > eye[1]


def test_default_view_edge_cases():
    k, e = framing_view([[1.0, 2.0, 3.0]], 8, 8)                        # one point: framed from 1 away
    assert np.allclose(-e[:3, :3].T @ e[:3, 3], [1.0, 1.0, 3.0])
    k, e = framing_view([[0.0, 0.0, 0.0], [np.nan, 1.0, 1.0], [2.0, 0.0, 0.0]], 8, 8)   # a NaN row is ignored
    assert np.isfinite(e).all() and np.allclose((-e[:3, :3].T @ e[:3, 3])[[0, 2]], [1.0, 0.0])
    for bad in (lambda: framing_view(np.full((3, 3), np.nan), 8, 8), lambda: framing_view(np.zeros((3, 3)), 0, 8),
                lambda: framing_view(np.zeros((3, 3)), 8, 8, 180.0), lambda: framing_view(np.zeros((3, 3)), 8, 8, float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_normal_rule_against_float64():
    """The restatement itself: on a jittered grid its normals are within 1e-5 (relative: they are unit vectors) of the
    area-weighted normals computed in float64 from the same fp32 vertices."""
    xyz, faces = jittered_grid(12, 9, seed=4)
    offsets, corners = vertex_corner_lists(faces, len(xyz))
    got = vertex_normals_rule(xyz, faces, offsets, corners)
    p = xyz.astype(np.float64)
    g = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
    s = np.zeros_like(p)
    for k in range(3):
        np.add.at(s, faces[:, k], g)
    want = s / np.linalg.norm(s, axis=1, keepdims=True)
    assert got.dtype == F32 and np.abs(got - want).max() < 1e-5
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6 and (got[:, 2] > 0.5).all()
    # degenerate input: the rule's zeros
    xyz2 = np.concatenate([xyz, [[np.nan, 0, 0], [5, 5, 5]]]).astype(F32)
    faces2 = np.concatenate([faces, [[0, 1, len(xyz)], [3, 3, 4], [2, 5, len(xyz2)]]]).astype(np.int32)
    offsets2, corners2 = vertex_corner_lists(faces2, len(xyz2))
    got2 = vertex_normals_rule(xyz2, faces2, offsets2, corners2)
    assert np.array_equal(got2[:len(xyz)], got) and not got2[len(xyz):].any()
