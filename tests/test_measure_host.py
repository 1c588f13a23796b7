"""No GPU: the host side of ``measure()``.  The rule (``measure_rule.py``: what the kernels are held to) and ``object_table``
against plain float64 numpy on a rotated cuboid; the conventions of ``principal_axes``; the guarantees of ``frame`` and of
``MeasureResult.section``."""
import types

import numpy as np
import pytest

from agile3d_amd.session import InteractiveSession, MeasureResult, object_table, principal_axes
from measure_rule import MOMENTS, face_quanta, fixed_point, measure_numpy, order_key, total_min_max
from session_kit import rotation

BITS = 20


def cuboid_scene():
    """A 21 x 9 x 5 lattice 0.1 apart, rotated and centred at (2.3, -1.7, 0.9): object 1.  Two vertices of object 0 at the
    corners of the 10 m scene [-5, 5]^3.  Faces: the lattice's 21 x 9 top sheet, two triangles per cell, and one face that
    joins the two objects.  Returns (xyz fp32, labels, faces, origin, quantum, area_quantum)."""
    g = np.stack(np.meshgrid(np.arange(21), np.arange(9), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    own = (g - g.mean(0)) * 0.1
    xyz = np.concatenate([own @ rotation(4).T + [2.3, -1.7, 0.9], [[-5.0, -5.0, -5.0], [5.0, 5.0, 5.0]]]).astype(np.float32)
    labels = np.concatenate([np.ones(len(g), np.int64), [0, 0]])
    idx = np.arange(21 * 9 * 5).reshape(21, 9, 5)[:, :, 4]
    q00, q10, q01, q11 = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    faces = np.concatenate([np.stack([q00, q10, q11], -1).reshape(-1, 3), np.stack([q00, q11, q01], -1).reshape(-1, 3),
                            [[0, len(g), len(g) + 1]]])
    quantum = 8.0 / 2 ** BITS                                   # 2^3 >= the half extent 5
    return xyz, labels, faces, np.zeros(3), quantum, quantum * quantum * 256.0


def test_rule_against_float64_on_a_rotated_cuboid():
    xyz, labels, faces, origin, q, aq = cuboid_scene()
    rec, err = measure_numpy(xyz, labels, origin, q, BITS, 2, labels_qv=[0, 1, 1, 1], faces=faces, area_quantum=aq)
    assert err == 0 and rec["vertices"].tolist() == [2, 945] and rec["voxels"].tolist() == [1, 3]
    t = object_table(rec, origin, q, aq, voxel_size=0.05)
    p = xyz[labels == 1].astype(np.float64)
    n = len(p)
    # the box is exact
    assert np.array_equal(rec["lo"][1], xyz[labels == 1].min(0)) and np.array_equal(rec["hi"][1], xyz[labels == 1].max(0))
    # centroid: X = u + d with u = (x - origin) / quantum and |d| <= 1/2, so the mean moves by at most quantum / 2 per axis
    mean = p.mean(0)
    d_centroid = np.abs(t["centroid"][1] - mean)
    print("centroid error / quantum:", d_centroid / q)
    assert (d_centroid <= q / 2 + 1e-15).all()
    # covariance: cov(X_a, X_b) - cov(u_a, u_b) = cov(u_a, d_b) + cov(d_a, u_b) + cov(d_a, d_b).  By Cauchy-Schwarz
    # |cov(u_a, d_b)| <= std(u_a) std(d_b), and std(d) <= 1/2 since |d| <= 1/2.  In world units, with s = the true standard
    # deviations: |delta cov_ab| <= (quantum / 2) (s_a + s_b) + quantum^2 / 4.  The float64 reference itself is good to a few
    # ulp of |x|^2 <= 75: 1e-13 covers it.
    c = p - mean
    cov = c.T @ c / n
    s = np.sqrt(np.diag(cov))
    bound = 0.5 * q * (s[:, None] + s[None, :]) + 0.25 * q * q + 1e-13
    d_cov = np.abs(t["cov"][1] - cov)
    print("covariance error / bound:", (d_cov / bound).max(), "largest error", d_cov.max())
    assert (d_cov <= bound).all()
    # eigenvalues (Weyl: they move by at most the 2-norm <= Frobenius norm of the perturbation) and axes (Davis-Kahan: sin of
    # the angle <= 2 |delta| / gap, and 1 - cos <= sin^2)
    axes, variances = principal_axes(t["cov"][1], n)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1], v[:, ::-1].T
    frob = float(np.sqrt((bound ** 2).sum()))
    gap = min(w[0] - w[1], w[1] - w[2])
    dots = np.abs((axes * v).sum(1))
    print("eigenvalues: relative error", np.abs(variances - w) / w, " 1 - |dot| of the axes", 1 - dots)
    assert (np.abs(variances - w) <= frob).all() and (1 - dots <= (2 * frob / gap) ** 2).all()
    assert np.allclose(variances, w, rtol=1e-6, atol=0) and (1 - dots <= 1e-12).all()      # what this case measures in fact
    assert np.allclose(w, [0.01 * (k * k - 1) / 12 for k in (21, 9, 5)], rtol=1e-5)       # the lattice's own variances
    # area: |Q - len / area_quantum| <= 1/2 per face, so the total is within faces * area_quantum / 2 in units of double area
    a, b, cc = (xyz[faces[:, k]].astype(np.float64) for k in range(3))
    twice = np.linalg.norm(np.cross(b - a, cc - a), axis=1)
    Q, ok = face_quanta(xyz, faces, aq)
    assert ok.all() and rec["area_thirds"].sum() == 3 * Q.sum()
    assert abs(rec["area_thirds"].sum() / 3 * aq - twice.sum()) <= len(faces) * aq / 2
    assert abs(t["area"].sum() - twice.sum() / 2) <= len(faces) * aq / 4
    sheet = twice[:-1].sum() / 2
    assert abs(sheet - 2.0 * 0.8) < 1e-5                          # the 20 x 8 cells of the top sheet
    assert abs(t["area"][1] - (sheet + twice[-1] / 6)) <= len(faces) * aq / 4 and abs(t["area"][0] - twice[-1] / 3) <= aq
    # volume: occupied voxels
    assert np.allclose(t["volume"], [0.05 ** 3, 3 * 0.05 ** 3])
    bare = object_table(rec, origin, q)
    assert bare["area"] is None and bare["volume"] is None and np.array_equal(bare["cov"], t["cov"])


def test_rule_edges():
    q = 2.0 ** -10
    lim = 2 ** 4 * q
    xyz = np.array([[lim, 0, 0], [lim + q, 0, 0], [-lim, -0.0, 0.0], [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.5, -0.125]], np.float32)
    X, ok = fixed_point(xyz, np.zeros(3), q, 4)
    assert ok.tolist() == [True, False, True, False, False, False] and X[0].tolist() == [16, 0, 0] and X[2].tolist() == [-16, 0, 0]
    rec, err = measure_numpy(xyz, [0, 0, 0, 0, 0, 7], np.zeros(3), q, 4, 2)
    assert err == 3 and rec["vertices"].tolist() == [2, 0] and rec["sum"][0].tolist() == [0, 0, 0] and rec["mom"][0].tolist() == [512, 0, 0, 0, 0, 0]
    assert np.isposinf(rec["lo"][1]).all() and np.isneginf(rec["hi"][1]).all()
    # the total order: -0 below +0, in the box as well
    assert order_key([-0.0])[0] < order_key([0.0])[0] and order_key([-1.0])[0] < order_key([-0.0])[0]
    lo, hi = total_min_max(np.array([[0.0], [-0.0]], np.float32))
    assert np.signbit(lo[0]) and not np.signbit(hi[0])
    assert np.signbit(rec["lo"][0][1]) and not np.signbit(rec["hi"][0][1]) and not np.signbit(rec["lo"][0][2])
    assert MOMENTS.itemsize == 128


def test_principal_axes_conventions():
    rng = np.random.default_rng(0)
    for seed in range(6):
        r = rotation(seed)
        lam = np.sort(rng.uniform(0.1, 2.0, 3))[::-1]
        cov = r.T @ np.diag(lam) @ r
        axes, variances = principal_axes(cov, 100)
        assert np.allclose(variances, lam) and (np.diff(variances) <= 0).all()
        assert np.allclose(axes @ axes.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(axes) - 1) < 1e-12     # right-handed
        assert np.allclose(np.cross(axes[0], axes[1]), axes[2])
        for j in (0, 1):
            assert axes[j, np.argmax(np.abs(axes[j]))] > 0
            assert np.allclose(np.abs(axes[j] @ r.T), np.eye(3)[j], atol=1e-9)                                 # the eigenvector
    # a tie of the largest magnitude goes to the lowest index: the axis (1, -1, 0) / sqrt 2 is signed by its x
    cov = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 0.5]])
    axes, variances = principal_axes(cov)
    assert np.allclose(variances, [3.0, 1.0, 0.5]) and axes[0, 0] > 0 and np.allclose(np.abs(axes[0]), [0.5 ** 0.5, 0.5 ** 0.5, 0])
    assert axes[1, 0] > 0
    # the degenerate cases: the identity
    eye = np.eye(3)
    assert np.array_equal(principal_axes(cov, 2)[0], eye) and np.array_equal(principal_axes(np.zeros((3, 3)), 50)[0], eye)
    bad = cov.copy()
    bad[0, 1] = np.nan
    assert np.array_equal(principal_axes(bad, 50)[0], eye) and np.array_equal(principal_axes(bad, 50)[1], np.zeros(3))
    batch, var = principal_axes(np.stack([cov, bad, np.zeros((3, 3)), cov]), [9, 9, 9, 1])
    assert np.array_equal(batch[0], axes) and all(np.array_equal(batch[k], eye) for k in (1, 2, 3)) and var.shape == (4, 3)


def _measured():
    xyz, labels, faces, origin, q, aq = cuboid_scene()
    rec, _ = measure_numpy(xyz, labels, origin, q, BITS, 3)
    t = object_table(rec, origin, q)
    return xyz, labels, MeasureResult(vertices=t["vertices"], voxels=t["voxels"], centroid=t["centroid"], lo=rec["lo"], hi=rec["hi"],
                                      cov=t["cov"])


def test_frame_shows_every_vertex_of_the_object():
    xyz, labels, m = _measured()
    ses = types.SimpleNamespace(_need_scene=lambda: None)
    for obj in (0, 1):
        for w, h, fov in ((64, 48, 35.0), (48, 64, 35.0), (33, 33, 100.0), (200, 20, 10.0)):
            k, e = InteractiveSession.frame(ses, obj, w, h, fov, measure=m)
            p = xyz[labels == obj].astype(np.float64) @ e[:3, :3].T + e[:3, 3]
            assert (p[:, 2] > 0).all()
            u, v = k[0, 0] * p[:, 0] / p[:, 2] + k[0, 2], k[1, 1] * p[:, 1] / p[:, 2] + k[1, 2]
            assert (u >= 0).all() and (u <= w).all() and (v >= 0).all() and (v <= h).all()
    for obj in (2, 3, -1):
        with pytest.raises(ValueError):
            InteractiveSession.frame(ses, obj, 64, 48, measure=m)


def test_section_keeps_every_vertex_of_the_object():
    xyz, labels, m = _measured()
    for obj in (0, 1):
        for margin in (0.0, 0.013):
            sec = m.section(obj, margin)
            assert sec.n_planes == 6 and sec.keeps(xyz[labels == obj]).all()
        assert m.section(obj, cull="back").cull == "back"
    inside = m.section(1).keeps(xyz)
    assert inside[labels == 1].all() and not inside[labels == 0].any()
    for bad in (dict(obj=2), dict(obj=1, margin=-1.0), dict(obj=1, margin=np.nan)):
        with pytest.raises(ValueError):
            m.section(**bad)
    # -0.0 and +0.0 on the box's faces: both are kept (the planes compare by value)
    rec, _ = measure_numpy(np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0]], np.float32), [0, 0], np.zeros(3), 2.0 ** -10, 12, 1)
    one = MeasureResult(vertices=rec["vertices"], lo=rec["lo"], hi=rec["hi"])
    assert one.section(0).keeps(np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0]], np.float32)).all()
