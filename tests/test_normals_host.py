"""Host side of the normals for point clouds (no GPU): the rule's restatement (``normals_rule.py``: Python integers, then
float64 scalars one operation at a time) against ``numpy.linalg.eigh`` on the same quantised integers; the cases whose answer
is exact; stage B as the library runs it (``a3d_normals_solve``, the function the kernel calls, compiled for the host) against
the restatement bit for bit; every ``ValueError`` the three ``view.py`` wrappers raise before the library is reached; the entry
points' refusals without a scene.  ``test_gpu_normals.py`` holds the kernels to the same restatement bit for bit.

THE ANGLE BOUND.  The rounding error of a double eigenvector is about 2^-52 |C| / gap; the test looks only at neighbourhoods
with (l_mid - l_min) / l_max >= 1e-3, where that is 2e-13, and asserts 1e-9: three orders of magnitude for the order of the
operations.  At most 2 % of the generator's cases may fall under the gap (0.15 % do)."""
import ctypes as C
import types

import numpy as np
import pytest

import normals_rule as R

ORIGIN, QUANTUM = (0.5, -1.0, 2.0), 0.25


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def sums_of(X):
    """(N, S, M) of integer points [k, 3] in Python integers."""
    X = [[int(v) for v in p] for p in np.asarray(X).tolist()]
    S = [sum(p[a] for p in X) for a in range(3)]
    M = [sum(p[a] * p[b] for p in X) for a, b in R.MOMENT_PAIRS]
    return len(X), S, M


def noisy_plane(rng):
    """3 to 199 quantised points of a noisy plane of random orientation, in-plane aspect >= 0.05, somewhere within +-1000."""
    k = int(rng.integers(3, 200))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    uv = rng.uniform(-1, 1, (k, 2)) * [1.0, rng.uniform(0.05, 1.0)] * 40.0
    noise = rng.normal(size=k) * rng.uniform(0.0, 1.0)
    return np.rint(np.c_[uv, noise] @ q.T + rng.uniform(-1000, 1000, 3)).astype(np.int64)


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(0)
    return [(noisy_plane(rng), rng.uniform(-2000, 2000, 3) if case % 2 else None) for case in range(2000)]


# ------------------------------------------------------------------------------------------- the rule against eigh
def test_restatement_against_eigh(planes):
    worst, under = 0.0, 0
    for X, vp in planes:
        N, S, M = sums_of(X)
        v, variation, valid = R.stage_b_double(N, S, M, ORIGIN, QUANTUM, vp)
        Xc = X - X.mean(0)
        w, vec = np.linalg.eigh(Xc.T @ Xc)
        if (w[1] - w[0]) / w[2] < 1e-3:
            under += 1
            continue
        assert valid and abs(float(np.linalg.norm(np.asarray(v, np.float64))) - 1.0) < 1e-12
        worst = max(worst, R.angle(v, vec[:, 0]))
        assert abs(float(variation) - w[0] / w.sum()) < 1e-9
    print(f"normals rule against eigh: worst angle {worst:.3g} rad over {len(planes) - under} cases, {under} under the gap")
    assert worst <= 1e-9
    assert under <= 0.02 * len(planes)


def test_library_stage_b_is_the_restatement(planes):
    """``a3d_normals_solve`` runs the kernel's own function on the host: the same bits as the restatement, with and without a
    viewpoint, on every generated neighbourhood and on the degenerate ones."""
    from agile3d_amd import view as V
    _lib()
    extra = [(np.array([[0, 0, 0]]), None), (np.array([[1, 2, 3], [4, 5, 6]]), None),
             (np.array([[k, 2 * k, -k] for k in range(9)]), None), (np.array([[5, 5, 5]] * 7), None),
             (np.array([[x, y, 7] for x in range(4) for y in range(4)]), (0.0, 0.0, -100.0)),
             (np.array([[(-1) ** k << 20, (k % 3 - 1) << 20, (k % 5 - 2) << 18] for k in range(40)]), (1e6, -1e6, 3.0))]
    for X, vp in list(planes[:600]) + extra:
        N, S, M = sums_of(X)
        want = R.stage_b(N, S, M, ORIGIN, QUANTUM, vp)
        got = V.normals_solve(N, S, M, ORIGIN, QUANTUM, vp)
        assert got[0].tobytes() == want[0].tobytes() and np.float32(got[1]).tobytes() == want[1].tobytes() and got[2] == want[2]
    for bad in (dict(quantum=0.3), dict(quantum=0.0), dict(origin=(0.0, np.nan, 0.0)), dict(viewpoint=(np.inf, 0, 0))):
        with pytest.raises(ValueError):
            V.normals_solve(**dict(dict(count=3, sums=[0, 0, 0], moments=[1] * 6, origin=ORIGIN, quantum=QUANTUM), **bad))


# ------------------------------------------------------------------------------------------- the exact cases
def test_plane_at_multiples_of_the_quantum_is_exact():
    for z, vp, want in ((7, None, 1.0), (-3, None, 1.0), (7, (0.0, 0.0, 100.0), 1.0), (7, (0.0, 0.0, -100.0), -1.0)):
        X = np.array([[x, y, z] for x in range(-2, 5) for y in range(3, 8)])
        normal, variation, valid = R.stage_b(*sums_of(X), ORIGIN, QUANTUM, vp)
        assert valid and normal.tolist() == [0.0, 0.0, want] and float(variation) == 0.0
    # the same plate along the other axes, without a viewpoint: the canonical sign is +
    for axis in (0, 1):
        X = np.array([[x, y, 7] for x in range(5) for y in range(4)])[:, np.roll(np.arange(3), axis + 1)]
        normal, variation, valid = R.stage_b(*sums_of(X), ORIGIN, QUANTUM)
        assert valid and np.abs(normal).tolist() == np.eye(3)[(2 + axis + 1) % 3].tolist() and normal.sum() == 1.0 and variation == 0.0


def test_too_few_points_and_lines_have_no_normal():
    zero = lambda r: r[0].tolist() == [0.0, 0.0, 0.0] and float(r[1]) == 0.0 and r[2] is False
    assert zero(R.stage_b(0, [0, 0, 0], [0] * 6, ORIGIN, QUANTUM))
    assert zero(R.stage_b(*sums_of([[4, 5, 6]]), ORIGIN, QUANTUM))
    assert zero(R.stage_b(*sums_of([[4, 5, 6], [9, -2, 1]]), ORIGIN, QUANTUM, (1.0, 2.0, 3.0)))
    assert zero(R.stage_b(*sums_of([[5, 5, 5]] * 7), ORIGIN, QUANTUM))                     # one point seven times
    for d in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 2, -1), (3, -7, 11)):                    # collinear, along any direction
        X = np.array([[1000, -2000, 500]]) + np.arange(40).reshape(-1, 1) * np.array(d)
        assert zero(R.stage_b(*sums_of(X), ORIGIN, QUANTUM)), d
    # a line 2000 long and 1 wide is narrower than 1/1024 of its length: still a line; 200 long and 1 wide is a surface
    thin = np.array([[x, x % 2, 0] for x in range(0, 4000, 2)])
    assert zero(R.stage_b(*sums_of(thin), ORIGIN, QUANTUM))
    assert R.stage_b(*sums_of(np.array([[x, x % 2, 0] for x in range(200)])), ORIGIN, QUANTUM)[2] is True


def test_viewpoint_flips_the_sign_and_zero_keeps_it():
    rng = np.random.default_rng(5)
    X = noisy_plane(rng)
    N, S, M = sums_of(X)
    free = R.stage_b(N, S, M, ORIGIN, QUANTUM)[0]
    mean = np.array(ORIGIN) + QUANTUM * X.mean(0)
    towards = R.stage_b(N, S, M, ORIGIN, QUANTUM, mean + 50.0 * free.astype(np.float64))[0]
    away = R.stage_b(N, S, M, ORIGIN, QUANTUM, mean - 50.0 * free.astype(np.float64))[0]
    assert towards.tobytes() == free.tobytes() and away.tobytes() == (-free).tobytes()
    # g == 0 keeps the vector the diagonalisation gave: a plate z = 0 about the origin of the frame, seen from inside its plane
    plate = np.array([[x, y, 0] for x in range(-2, 3) for y in range(-2, 3)])
    for vp in ((0.0, 0.0, 0.0), (5.0, -3.0, 0.0)):
        assert R.stage_b(*sums_of(plate), (0.0, 0.0, 0.0), 1.0, vp)[0].tolist() == [0.0, 0.0, 1.0]
    assert R.stage_b(*sums_of(plate), (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, -1e-300))[0].tolist() == [0.0, 0.0, -1.0]


def test_recentring_equals_big_integers_about_the_true_mean():
    """m_ab - s_a s_b / N, in exact rationals, is the scatter about the true mean, for coordinates at +-2^20; and the wrapping
    64-bit form gives the same integers as the Python one."""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    for case in range(50):
        k = int(rng.integers(3, 300))
        X = rng.integers(-3, 4, (k, 3)) + rng.choice([-(1 << 20) + 3, (1 << 20) - 3, 0], 3)
        X[rng.integers(k)] = rng.choice([-(1 << 20), 1 << 20], 3)
        N, S, M = sums_of(X)
        R_, s, m = R.recentre(N, S, M)
        assert all(0 <= v < N for v in s)
        pts = [[int(v) for v in p] for p in X.tolist()]
        mean = [Fraction(S[a], N) for a in range(3)]
        for i, (a, b) in enumerate(R.MOMENT_PAIRS):
            scatter = sum((p[a] - mean[a]) * (p[b] - mean[b]) for p in pts)
            assert Fraction(m[i]) - Fraction(s[a] * s[b], N) == scatter
            assert m[i] == sum((p[a] - R_[a]) * (p[b] - R_[b]) for p in pts)
            wrapped = (M[i] - R_[a] * S[b] - R_[b] * S[a] + ((N * R_[a]) % (1 << 64)) * R_[b]) % (1 << 64)
            assert (wrapped - (1 << 64) if wrapped >> 63 else wrapped) == m[i]


def test_stage_a_and_the_lift():
    """Vertices outside the rows or the range count nowhere and set their bits; the words are plain integer sums."""
    coords = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [0, 5, 5, 5]])
    xyz = np.array([[0.5, -1.0, 2.0], [0.75, -1.0, 2.25], [1.0, 0.0, 3.0], [np.nan, 0, 0], [1e9, 0, 0], [0.5, -1.0, 2.0], [3.0, 3.0, 3.0]], np.float32)
    inv = np.array([0, 0, 1, 1, 2, -1, 3])
    r = R.estimate(coords, xyz, inv, ORIGIN, QUANTUM, 20)
    assert r["moments_qv"][0].tolist() == [2, 1, 0, 1, 1, 0, 1, 0, 0, 1] and r["moments_qv"][1].tolist() == [1, 2, 4, 4, 4, 8, 8, 16, 16, 16]
    assert r["moments_qv"][2].tolist() == [0] * 10 and r["count_qv"].tolist() == [3, 3, 0]
    assert r["summary"] == dict(counted=3, valid=2, invalid=1, err=R.RANGE | R.BAD_INDEX)        # (three points span a plane)
    assert r["normal_qv"][0].tobytes() == r["normal_qv"][1].tobytes() and not r["normal_qv"][2].any()
    # the lift follows the map alone: a vertex that did not count still takes its voxel's normal; a row outside takes zeros
    assert r["normal_full"].shape == (7, 3) and (r["normal_full"][:4] == r["normal_qv"][0]).all() and not r["normal_full"][4:].any()
    plane = np.cross([1.0, 0.0, 1.0], [2.0, 4.0, 4.0])
    assert R.angle(r["normal_qv"][0], plane) < 1e-6
    assert R.estimate(coords, xyz[:3], None, ORIGIN, QUANTUM, 1)["summary"]["err"] == R.RANGE     # |X| = 4 > 2^1


def test_the_vectorised_restatement_is_the_restatement():
    """``estimate_large`` (numpy int64 sums; what the GPU test's large scene is held to) against ``estimate`` (Python integers) on
    a blob of two batch samples with vertices out of the rows and out of the range."""
    rng = np.random.default_rng(3)
    cells = np.unique(rng.integers(-3, 4, (260, 3)), axis=0)
    coords = np.concatenate([np.c_[np.zeros(len(cells), np.int64), cells], np.c_[np.ones(40, np.int64), cells[:40] + (1, 0, 0)]])
    coords = coords[rng.permutation(len(coords))]
    inv = rng.integers(-1, len(coords) + 1, 3000)
    xyz = (coords[np.clip(inv, 0, len(coords) - 1), 1:] + rng.uniform(0, 1, (3000, 3))).astype(np.float32)
    xyz[::97] = np.nan
    xyz[5] = 1e6
    for bits, vp in ((20, None), (12, (0.3, 0.2, 9.0)), (3, None)):
        a = R.estimate(coords, xyz, inv, (0.0, 0.5, 0.0), 2.0 ** (3 - bits), bits, vp)
        b = R.estimate_large(coords, xyz, inv, (0.0, 0.5, 0.0), 2.0 ** (3 - bits), bits, vp)
        assert a["summary"] == b["summary"] and a["summary"]["err"] == R.RANGE | R.BAD_INDEX
        assert bits == 3 or a["summary"]["valid"] > 100
        for k in ("moments_qv", "count_qv", "normal_qv", "variation_qv", "normal_full"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (bits, k)


def test_cull_rule():
    xyz = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0], [np.nan, 0, 1]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 0], [np.nan, 0, 1], [0, 0, 1], [0, 0, 1]], np.float32)
    out, hidden, count = R.cull(xyz, nrm, (0, 0, 0), R.CULL_BACK)
    assert hidden.tolist() == [1, 0, 0, 0, 0, 0] and count == 1 and np.isnan(out[0]).all() and out[1:5].tobytes() == xyz[1:5].tobytes()
    assert out.view(np.uint32)[0].tolist() == [0x7fc00000] * 3
    assert R.cull(xyz, nrm, (0, 0, 0), R.CULL_FRONT)[1].tolist() == [0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------- the wrappers' refusals
def test_wrappers_refuse_before_the_library():
    import torch
    from agile3d_amd import lib as L
    from agile3d_amd import view as V
    assert (V.NORMALS_RANGE, V.NORMALS_BAD_INDEX) == (R.RANGE, R.BAD_INDEX) and V.CULL_MODES == dict(back=R.CULL_BACK, front=R.CULL_FRONT)
    scene = types.SimpleNamespace(handle=C.c_void_p(0), n=[5])
    xyz = torch.zeros((4, 3), dtype=torch.float32)
    base = dict(scene=scene, xyz=xyz, origin=(0, 0, 0), quantum=0.5)
    for name, bad in (("scene", dict(scene=None)), ("scene", dict(scene=object())), ("GPU", dict()), ("GPU", dict(xyz=None)),
                      ("GPU", dict(xyz=np.zeros((4, 3), np.float32)))):
        with pytest.raises(ValueError, match=name):
            V.estimate_normals(**dict(base, **bad))
    # what is checked after the device: a stand-in for a device tensor lets the host checks be reached without a GPU
    class OnGpu(torch.Tensor):
        device = torch.device("cuda", 0)
    fake = lambda t: t.as_subclass(OnGpu)
    base["xyz"] = fake(xyz)
    for name, bad in (("xyz", dict(xyz=fake(torch.zeros((4, 2))))), ("xyz", dict(xyz=fake(torch.zeros((4, 3), dtype=torch.float64)))),
                      ("xyz", dict(xyz=fake(torch.zeros((3, 4)).t()))), ("inverse_map", dict(inverse_map=fake(torch.zeros(4, dtype=torch.int32)))),
                      ("inverse_map", dict(inverse_map=fake(torch.zeros(5, dtype=torch.int64)))), ("bits", dict(bits=21)),
                      ("bits", dict(bits=-1)), ("bits", dict(bits=2.5)), ("bits", dict(bits=True)), ("origin", dict(origin=(0, 0))),
                      ("origin", dict(origin=(0, np.inf, 0))), ("quantum", dict(quantum=0.3)), ("quantum", dict(quantum=-0.5)),
                      ("quantum", dict(quantum=np.nan)), ("viewpoint", dict(viewpoint=(0, np.nan, 0))),
                      ("viewpoint", dict(viewpoint=(1, 2, 3, 4))), ("normal_qv", dict(normal_qv=fake(torch.zeros((4, 3))))),
                      ("variation_qv", dict(variation_qv=fake(torch.zeros(5, dtype=torch.float64)))),
                      ("count_qv", dict(count_qv=fake(torch.zeros(5)))), ("moments_qv", dict(moments_qv=fake(torch.zeros((5, 9), dtype=torch.int64)))),
                      ("normal_full", dict(normal_full=fake(torch.zeros((5, 3))))), ("summary", dict(summary=fake(torch.zeros(31, dtype=torch.uint8))))):
        with pytest.raises(ValueError, match=name):
            V.estimate_normals(**dict(base, normal_qv=False, variation_qv=False, count_qv=False, moments_qv=False, normal_full=False) | bad)
    big = fake(torch.empty(((1 << 22) + 1, 3)))                          # 2^22 + 1 vertices overflow at bits = 20 (and fit at 19)
    with pytest.raises(ValueError, match="overflow"):
        V.estimate_normals(scene, big, (0, 0, 0), 0.5)
    with pytest.raises(ValueError, match="summary"):
        V.estimate_normals(scene, big, (0, 0, 0), 0.5, bits=19, normal_qv=False, variation_qv=False, count_qv=False, moments_qv=False,
                           normal_full=False, summary=fake(torch.zeros(3, dtype=torch.uint8)))
    # the lit pass and the cull
    cam = L.Camera()
    cam.width, cam.height = 4, 3
    ids, col, nrm = fake(torch.zeros((3, 4), dtype=torch.int32)), fake(torch.zeros((6, 3))), fake(torch.zeros((6, 3)))
    lit = dict(ids=ids, colors=col, normals=nrm, cam=cam, ambient=0.3, background=(1, 1, 1), rgb=fake(torch.zeros((3, 4, 3), dtype=torch.uint8)))
    for name, bad in (("GPU", dict(ids=torch.zeros((3, 4), dtype=torch.int32))), ("ids", dict(ids=fake(torch.zeros((3, 4))))),
                      ("camera", dict(ids=fake(torch.zeros((4, 3), dtype=torch.int32)), rgb=fake(torch.zeros((4, 3, 3), dtype=torch.uint8)))),
                      ("colors", dict(colors=fake(torch.zeros((6, 4))))),
                      ("normals", dict(normals=fake(torch.zeros((5, 3))))), ("normals", dict(normals=None)),
                      ("ambient", dict(ambient=1.5)), ("ambient", dict(ambient=-0.1)), ("ambient", dict(ambient=np.nan)),
                      ("background", dict(background=(1, 1))), ("rgb", dict(rgb=fake(torch.zeros((3, 4, 3)))))):
        with pytest.raises(ValueError, match=name):
            V.render_shade_lit_points(**dict(lit, **bad))
    cull = dict(xyz=fake(xyz), normals=fake(torch.zeros((4, 3))), eye=(0, 0, 0), mode="back", out=fake(torch.zeros((4, 3))), hidden=False,
                count=False)
    for name, bad in (("mode", dict(mode="none")), ("mode", dict(mode=1)), ("GPU", dict(xyz=xyz)), ("xyz", dict(xyz=fake(torch.zeros(4, 4)))),
                      ("normals", dict(normals=fake(torch.zeros((3, 3))))), ("eye", dict(eye=(0, 0))), ("eye", dict(eye=(0, np.nan, 0))),
                      ("eye", dict(eye=(1e39, 0, 0))), ("out", dict(out=fake(torch.zeros((4, 2))))),
                      ("hidden", dict(hidden=fake(torch.zeros(4)))), ("count", dict(count=fake(torch.zeros(1, dtype=torch.int32))))):
        with pytest.raises(ValueError, match=name):
            V.cull_points(**dict(cull, **bad))
    assert V.read_normals_summary(np.array([(7, 5, 2, 3, 0)], V.NORMALS_SUMMARY).view(np.uint8)) == dict(counted=7, valid=5, invalid=2, err=3)


def test_library_refuses_without_a_scene():
    lib, L = _lib()
    assert L.a3d_normals_workspace_bytes(-1) == 0 and L.a3d_normals_workspace_bytes(1 << 31) == 0
    for n in (0, 1, 1000):
        nbytes = L.a3d_normals_workspace_bytes(n)
        assert nbytes >= (4 + 72 + 12) * n and nbytes % 256 == 0
    assert C.sizeof(lib.EstimateNormalsArgs) == 168 and C.sizeof(lib.NormalsSummary) == 32
    assert L.a3d_estimate_normals(None, None) == lib.A3D_ERR_INVALID
    a = lib.EstimateNormalsArgs()
    a.n, a.bits, a.quantum = 0, 20, 0.5
    a.summary_dev = a.workspace_dev = 256                           # (never looked at: the scene is checked first)
    a.workspace_bytes = 1 << 20
    assert L.a3d_estimate_normals(C.byref(a), None) == lib.A3D_ERR_INVALID
    assert b"a3d_estimate_normals" in L.a3d_last_error()
    # the cull and the lit pass refuse on the host what no tensor can be: no GPU is needed to be refused
    eye = (C.c_float * 3)(0, 0, 0)
    for args in ((None, None, -1, eye, 1, None, None, None), (None, None, 1 << 31, eye, 1, None, None, None),
                 (None, None, 0, eye, 0, None, None, None), (None, None, 0, eye, 3, None, None, None),
                 (None, None, 0, None, 1, None, None, None), (None, None, 0, (C.c_float * 3)(0, float("nan"), 0), 1, None, None, None),
                 (None, None, 4, eye, 1, None, None, None), (None, None, 0, eye, 2, None, None, 4)):
        assert L.a3d_cull_points(*args, None) == lib.A3D_ERR_INVALID
    assert b"a3d_cull_points" in L.a3d_last_error()
    cam = lib.Camera()
    bg = (C.c_float * 3)(1, 1, 1)
    assert L.a3d_render_shade_lit_points(None, None, 0, None, C.byref(cam), 0.5, bg, None, None) == lib.A3D_ERR_INVALID
    assert L.a3d_render_shade_lit_points(256, None, 0, None, None, 0.5, bg, 256, None) == lib.A3D_ERR_INVALID    # no camera
    assert b"a3d_render_shade_lit_points" in L.a3d_last_error()
    assert L.a3d_normals_solve(3, None, None, None, 0.5, None, None) == lib.A3D_ERR_INVALID
