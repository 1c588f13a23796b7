"""Host side of the rendered view (no GPU): the camera, the fp32 pixel rays, and the conservative bound that bins
primitives to screen tiles -- restated in ``render_rule.py`` and held here against the exact per-pixel tests, so that
``test_gpu_render.py`` compares the kernels with yardsticks that agree.  The cameras' builders are in ``session_kit.py``."""
import ctypes as C

import numpy as np
import pytest

from pick_rule import F32, U
from render_rule import (camera_bounds, camera_fields, face_pass_f32, pixel_rays, point_pass_f32, rect_face, rect_point,
                         render_mesh_rule)
from session_kit import intrinsic, look_at


CAMERAS = [  # (intrinsic, extrinsic, width, height)
    (np.array([[520.0, 0.0, 319.5], [0.0, 515.0, 239.5], [0.0, 0.0, 1.0]]), look_at([1.5, -2.0, 0.7], [0.0, 0.3, 0.2]), 640, 480),
    (intrinsic(37, 29, 75.0), look_at([50.3, -48.7, 1.2], [53.0, -47.0, 0.9]), 37, 29),
    (intrinsic(4096, 4096, 20.0), look_at([-3.0, 0.1, 9.0], [0.0, 0.0, 0.0], up=(0.0, 1.0, 0.0)), 4096, 4096),
]


@pytest.mark.parametrize("case", range(len(CAMERAS)))
def test_pixel_rays_against_ray_from_pixel(case):
    """The fp32 restatement of a pixel's ray against float64 ``ray_from_pixel``.

    The tolerance.  u = 2^-24.  Per component k the exact direction is D_k = d00_k + i du_k + j dv_k.  Rounding the three
    camera vectors to fp32 moves it by <= u (|d00_k| + i |du_k| + j |dv_k|) =: u S_k.  The fp32 evaluation rounds two
    products (<= u i |du_k|, u j |dv_k|) and two sums (each <= u times a partial sum <= S_k (1 + 2u)): <= 3u S_k more.  So
    |dD| <= 4u |S| (+ O(u^2)), an angle of <= 4u |S| / |D|.  The normalisation divides every component by the same
    computed length -- an error of the length turns nothing -- and rounds each quotient once: <= u per component, an
    angle <= sqrt(3) u < 2u; the float64 side adds ~1e-16.  Allowed: (4 |S| / |D| + 2) u + 1e-12, compared as
    |d32 - d64| (a chord, <= the angle)."""
    from agile3d_amd.session import camera_from_matrices, ray_from_pixel
    k, e, w, h = CAMERAS[case]
    cam = camera_from_matrices(k, e, w, h)
    o, d00, du, dv, _, _ = camera_fields(cam)
    d = pixel_rays(cam)
    rng = np.random.default_rng(case)
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(60)]
    worst = 0.0
    for i, j in pixels:
        o64, d64 = ray_from_pixel(i, j, k, e)
        assert np.abs(o.astype(np.float64) - o64).max() <= U * np.abs(o64).max()
        S = np.abs(d00.astype(np.float64)) + i * np.abs(du.astype(np.float64)) + j * np.abs(dv.astype(np.float64))
        D = d00.astype(np.float64) + i * du.astype(np.float64) + j * dv.astype(np.float64)
        tol = (4 * np.linalg.norm(S) / np.linalg.norm(D) + 2) * U + 1e-12
        err = np.linalg.norm(d[j, i].astype(np.float64) - d64)
        worst = max(worst, err / tol)
        assert err <= tol, (i, j, err, tol)
    print(f"camera {case}: worst error / tolerance = {worst:.3f}")


def test_camera_from_matrices_fields_and_errors():
    from agile3d_amd.session import camera_from_matrices, ray_from_pixel
    k, e, w, h = CAMERAS[0]
    cam = camera_from_matrices(k, e, w, h)
    assert (cam.width, cam.height) == (640, 480)
    o64, d64 = ray_from_pixel(0, 0, k, e)
    d00 = np.array(cam.d00[:], np.float64)
    assert np.allclose(d00 / np.linalg.norm(d00), d64, rtol=0, atol=1e-6)
    assert np.allclose(e[:3, :3] @ d00, [(0.5 - k[0, 2]) / k[0, 0], (0.5 - k[1, 2]) / k[1, 1], 1.0], rtol=0, atol=1e-6)
    assert np.allclose(e[:3, :3] @ np.array(cam.du[:], np.float64), [1 / 520.0, 0, 0], rtol=0, atol=1e-9)
    assert np.allclose(e[:3, :3] @ np.array(cam.dv[:], np.float64), [0, 1 / 515.0, 0], rtol=0, atol=1e-9)
    for bad in ((np.eye(4), e, w, h), (k, np.eye(3), w, h), (k, e, 0, h), (k, e, w, 4097), (k, e, 2.5, h), (k, e, w, -1)):
        with pytest.raises(ValueError):
            camera_from_matrices(*bad)
    nan = k.copy()
    nan[0, 0] = np.nan
    with pytest.raises(ValueError):
        camera_from_matrices(nan, e, w, h)
    assert camera_from_matrices(k, e, 1, 1).width == 1 and camera_from_matrices(k, e, 4096, 4096).height == 4096


@pytest.mark.parametrize("case", range(len(CAMERAS)))
def test_camera_bounds_host_code(case):
    """``a3d_render_camera_bounds`` (host code of the library, no GPU) against numpy's inverse; dmax bounds every pixel."""
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib as L
    from agile3d_amd.session import camera_from_matrices
    lib = L.load()
    cam = camera_from_matrices(*CAMERAS[case])
    out = (C.c_double * 13)()
    assert lib.a3d_render_camera_bounds(C.byref(cam), out) == 0
    got = np.array(out[:])
    inv, norms, dmax = camera_bounds(cam)
    assert np.allclose(got[:9].reshape(3, 3), inv, rtol=1e-9, atol=0)
    assert np.allclose(got[9:12], norms, rtol=1e-9) and np.isclose(got[12], dmax, rtol=1e-12)
    o, d00, du, dv, w, h = camera_fields(cam)
    u, v = np.meshgrid(np.arange(0, w, max(1, w // 64), dtype=F32), np.arange(0, h, max(1, h // 64), dtype=F32))
    x = [(d00[k] + u * du[k]) + v * dv[k] for k in range(3)]
    assert np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]).max() <= got[12]
    # cameras the renders refuse: a size out of range, d00 parallel to du
    cam.width = 4097
    assert lib.a3d_render_camera_bounds(C.byref(cam), out) != 0
    cam.width = w
    cam.d00[:] = [2.0 * a for a in cam.du[:]]                      # (exact in fp32: the determinant is 0 but for float64 rounding)
    assert lib.a3d_render_camera_bounds(C.byref(cam), out) != 0


# ------------------------------------------------------------------------------------------- the bound never loses a hit
def _random_mesh(rng, m, centre, spread, edge):
    """m independent triangles: centres within ``spread`` of ``centre``, edges around ``edge``."""
    c = centre + rng.uniform(-spread, spread, (m, 1, 3))
    xyz = (c + rng.normal(0, edge, (m, 3, 3))).reshape(-1, 3).astype(F32)
    return xyz, np.arange(3 * m, dtype=np.int32).reshape(m, 3)


BOUND_CASES = {
    # name: (eye, target, fov, mesh centre, spread, edge)
    "outside": ([0.0, -4.0, 1.0], [0.0, 0.0, 0.0], 60.0, [0.0, 0.0, 0.0], 1.5, 0.15),
    "inside": ([0.1, 0.2, 0.0], [1.0, 0.3, 0.1], 90.0, [0.0, 0.0, 0.0], 1.5, 0.4),          # faces all around the camera
    "large near faces": ([0.0, 0.0, 0.0], [0.0, 1.0, 0.0], 70.0, [0.0, 0.3, 0.0], 0.5, 2.0),  # most straddle the camera plane
    "far from the origin": ([50.3, -52.0, 1.2], [50.3, -48.7, 1.2], 50.0, [50.3, -48.7, 1.2], 1.5, 0.2),
}


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_face_bound_contains_every_exact_hit(name):
    """Random triangles, a 40 x 30 image: every (pixel, face) pair whose exact fp32 test passes lies inside the face's
    restated bound -- in its rectangle of PIXELS, which is stricter than the tiles the kernel derives from it.  The cases
    include faces that straddle the camera plane, faces wholly behind it and faces that contain the camera's foot."""
    from agile3d_amd.session import camera_from_matrices
    eye, target, fov, centre, spread, edge = BOUND_CASES[name]
    w, h = 40, 30
    cam = camera_from_matrices(intrinsic(w, h, fov), look_at(eye, target), w, h)
    rng = np.random.default_rng(len(name))
    xyz, faces = _random_mesh(rng, 300, np.asarray(centre), spread, edge)
    bounds = camera_bounds(cam)
    o = camera_fields(cam)[0]
    verdicts = [rect_face(cam, bounds, *xyz[f]) for f in faces]
    inv = bounds[0]
    depth = ((xyz[faces].astype(np.float64) - o.astype(np.float64)) @ inv[2])          # camera-space c of every vertex
    straddle = (depth.min(1) < 0) & (depth.max(1) > 0)
    d = pixel_rays(cam)
    pairs = straddle_pairs = rect_pairs = 0
    for j in range(h):
        for i in range(w):
            hit = face_pass_f32(xyz, faces, o, d[j, i])[0]
            for f in np.flatnonzero(hit):
                kind, rect = verdicts[f]
                assert kind != "none", (name, i, j, f)
                if kind == "rect":
                    assert rect[0] <= i <= rect[2] and rect[1] <= j <= rect[3], (name, i, j, f, rect)
                    rect_pairs += 1
                pairs += 1
                straddle_pairs += bool(straddle[f])
    kinds = [k for k, _ in verdicts]
    print(f"{name}: {pairs} passing pairs ({rect_pairs} inside a rectangle, {straddle_pairs} on straddling faces); "
          f"verdicts: {kinds.count('rect')} rect, {kinds.count('every')} every, {kinds.count('none')} none")
    assert pairs >= 300 and rect_pairs >= 100
    if name in ("inside", "large near faces"):
        assert straddle.sum() >= 10 and straddle_pairs >= 50
        assert any(k == "rect" for k, s in zip(kinds, straddle) if s)      # a straddling face is clipped, not given up on
    if name == "outside":
        assert kinds.count("every") == 0


@pytest.mark.parametrize("name", ["outside", "inside", "far from the origin"])
def test_point_bound_contains_every_exact_pass(name):
    """Random points with a radius that makes discs of several pixels; some points nearer to the camera than the radius,
    some just beyond it, some beside and behind the camera."""
    from agile3d_amd.session import camera_from_matrices
    eye, target, fov, centre, spread, _ = BOUND_CASES[name]
    w, h = 40, 30
    cam = camera_from_matrices(intrinsic(w, h, fov), look_at(eye, target), w, h)
    rng = np.random.default_rng(7 + len(name))
    r = 0.08
    pts = np.asarray(centre) + rng.uniform(-spread, spread, (300, 3))
    eye = np.asarray(eye, np.float64)
    near = eye + rng.normal(0, 1, (40, 3)) * rng.uniform(0.02, 0.3, (40, 1))               # within and just beyond the radius
    xyz = np.concatenate([pts, near]).astype(F32)
    bounds = camera_bounds(cam)
    o = camera_fields(cam)[0]
    verdicts = [rect_point(cam, bounds, p, r) for p in xyz]
    d = pixel_rays(cam)
    pairs = rect_pairs = 0
    for j in range(h):
        for i in range(w):
            ok = point_pass_f32(xyz, o, d[j, i], r)[0]
            for p in np.flatnonzero(ok):
                kind, rect = verdicts[p]
                assert kind != "none", (name, i, j, p)
                if kind == "rect":
                    assert rect[0] <= i <= rect[2] and rect[1] <= j <= rect[3], (name, i, j, p, rect)
                    rect_pairs += 1
                pairs += 1
    kinds = [k for k, _ in verdicts]
    dist = np.linalg.norm(xyz.astype(np.float64) - o.astype(np.float64), axis=1)
    assert all(k == "every" for k, dd in zip(kinds, dist) if dd <= r)
    assert all(k != "every" for k, dd in zip(kinds, dist) if dd > 1.1 * r)
    print(f"{name}: {pairs} passing pairs, {rect_pairs} inside a rectangle; {kinds.count('every')} points everywhere")
    assert pairs >= 300 and rect_pairs >= 100 and kinds.count("every") >= 1


def test_per_face_restatement_equals_mesh_rule_f32():
    """``face_pass_f32`` keeps per face what ``mesh_rule_f32`` reduces: the same winner and the same bits."""
    from agile3d_amd.session import camera_from_matrices
    w, h = 12, 9
    cam = camera_from_matrices(intrinsic(w, h, 70.0), look_at([0.0, -3.0, 0.5], [0.0, 0.0, 0.0]), w, h)
    xyz, faces = _random_mesh(np.random.default_rng(3), 60, np.zeros(3), 1.0, 0.4)
    face, t, u, v, flags = render_mesh_rule(xyz, faces, cam)
    o = camera_fields(cam)[0]
    d = pixel_rays(cam)
    for j in range(h):
        for i in range(w):
            hit, tt, vv, ww, det = face_pass_f32(xyz, faces, o, d[j, i])
            if not hit.any():
                assert face[j, i] == -1 and t[j, i] == np.inf
                continue
            key = np.where(hit, tt.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.arange(len(faces), dtype=np.uint64),
                           np.uint64(2 ** 64 - 1))
            best = int(key.argmin())
            assert face[j, i] == best and t[j, i].view(np.uint32) == tt[best].view(np.uint32)
            assert u[j, i] == F32(vv[best] / det[best]) and v[j, i] == F32(ww[best] / det[best])
    assert (face >= 0).sum() >= 20 and flags == 0
