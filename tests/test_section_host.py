"""Host side of the section (no GPU): the layout of ``a3d_section``, what the four ``*_section`` calls refuse before they
touch a GPU, ``a3d_section_ray`` against the numpy restatement of the ray's interval bit for bit, the facing read off the
crossing test's det against g . d in float64, the ``Section`` class of ``agile3d_amd.session`` and the filtering of click
markers.  ``test_gpu_section.py`` holds the kernels to the same restatement (``section_rule.py``)."""
import ctypes as C

import numpy as np
import pytest

import section_rule as R
from pick_rule import F32
from render_rule import face_pass_f32

NAN, INF = float("nan"), float("inf")
bits = lambda x: np.ascontiguousarray(x, F32).view(np.uint32)


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def _section(lib, planes=(), cull=0, n_planes=None):
    s = lib.Section()
    s.n_planes, s.cull = len(planes) if n_planes is None else n_planes, cull
    for k, p in enumerate(planes):
        s.planes[k][:] = [float(x) for x in p]
    return s


def _f32p(values):
    return np.ascontiguousarray(values, F32).ctypes.data_as(C.POINTER(C.c_float))


def test_section_layout():
    lib, _ = _lib()
    assert C.sizeof(lib.Section) == 136
    assert lib.Section.n_planes.offset == 0 and lib.Section.cull.offset == 4 and lib.Section.planes.offset == 8
    assert (lib.A3D_SECTION_MAX_PLANES, lib.A3D_CULL_NONE, lib.A3D_CULL_BACK, lib.A3D_CULL_FRONT) == (8, 0, 1, 2)


# ------------------------------------------------------------------------------------------- refusals
def _calls(lib, L):
    """The four calls with null device pointers and no rows: name -> (mesh?, section -> status).  With a section the
    library accepts, each of them is refused for its missing result -- so nothing is ever launched."""
    cam = lib.Camera()
    cam.o[:], cam.d00[:], cam.du[:], cam.dv[:] = [0, 0, 0], [0, 0, 1], [0.01, 0, 0], [0, 0.01, 0]
    cam.width, cam.height = 4, 4
    o, d = _f32p([0, 0, 0]), _f32p([0, 0, 1])
    ref = lambda s: None if s is None else C.byref(s)
    return {
        "a3d_pick_ray_section": (False, lambda s: L.a3d_pick_ray_section(None, 0, o, d, 0.1, ref(s), None, None, 0, None)),
        "a3d_pick_mesh_section": (True, lambda s: L.a3d_pick_mesh_section(None, 0, None, 0, o, d, ref(s), None, None, 0, None)),
        "a3d_render_mesh_section": (True, lambda s: L.a3d_render_mesh_section(None, 0, None, 0, C.byref(cam), ref(s), None, None,
                                                                              0, None)),
        "a3d_render_points_section": (False, lambda s: L.a3d_render_points_section(None, 0, 0.1, C.byref(cam), ref(s), None, None,
                                                                                   0, None)),
    }


BAD = {
    "n_planes -1": dict(n_planes=-1),
    "n_planes 9": dict(n_planes=9),
    "cull -1": dict(cull=-1),
    "cull 3": dict(cull=3),
    "a NaN normal": dict(planes=[(NAN, 0, 1, 0)]),
    "an infinite normal": dict(planes=[(0, INF, 0, 0)]),
    "a NaN offset": dict(planes=[(0, 0, 1, NAN)]),
    "an infinite offset": dict(planes=[(0, 0, 1, -INF)]),
    "a zero normal": dict(planes=[(0, 0, 0, 0)]),
    "|n|^2 just below 0.5": dict(planes=[(0.7, 0, 0, 0)]),
    "|n|^2 just above 2": dict(planes=[(1.0, 1.0, 0.1, 0)]),
    "the last of 8 planes bad": dict(planes=[(0, 0, 1, 0)] * 7 + [(0, 0, 3, 0)]),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_calls_refuse_a_bad_section(name):
    lib, L = _lib()
    for entry, (mesh, call) in _calls(lib, L).items():
        assert call(_section(lib, **BAD[name])) == lib.A3D_ERR_INVALID, entry
        message = L.a3d_last_error().decode()
        assert entry in message and ": section:" in message, message


def test_cloud_calls_refuse_culling_and_good_sections_pass_the_check():
    lib, L = _lib()
    good = [None, _section(lib), _section(lib, [(0, 0, 1, 0.5)] * 8), _section(lib, [(0.8, 0, 0, 0)]),       # |n|^2 = 0.64
            _section(lib, [(1, 1, 0, -3)]),                                                                  # |n|^2 = 2
            _section(lib, [(NAN, NAN, NAN, NAN)], n_planes=0)]                                               # an unused plane
    for entry, (mesh, call) in _calls(lib, L).items():
        for s in good:
            # refused for the missing result, not for the section
            assert call(s) == lib.A3D_ERR_INVALID and ": section:" not in L.a3d_last_error().decode(), entry
        for cull in (lib.A3D_CULL_BACK, lib.A3D_CULL_FRONT):
            assert call(_section(lib, cull=cull)) == lib.A3D_ERR_INVALID
            assert (": section:" in L.a3d_last_error().decode()) == (not mesh), entry


# ------------------------------------------------------------------------------------------- the ray's interval
S2 = float(np.sqrt(0.5))
RAY_CASES = {
    # planes, origin, direction
    "den > 0": ([(0, 0, 1, 2)], [0.3, -0.2, -1.7], [0.1, 0.2, 0.97]),
    "den < 0": ([(0, 0, 1, -2)], [0.3, -0.2, 1.7], [0.1, 0.2, -0.97]),
    "den > 0 behind the origin": ([(0, 0, 1, -5)], [0, 0, 0], [0, 0, 1]),
    "den == 0 on the kept side": ([(1, 0, 0, 0.25)], [0.5, 0, 0], [0, 0, 1]),
    "den == 0 on the cut side": ([(1, 0, 0, 0.75)], [0.5, 0, 0], [0, 0, 1]),
    "den == 0 on the plane": ([(1, 0, 0, 0.5)], [0.5, 0, 0], [0, 0, 1]),
    "an empty interval": ([(0, 0, 1, 3), (0, 0, -1, -2)], [0, 0, 0], [0, 0, 1]),
    "a quotient of -0 against the bound +0": ([(0, 0, 1, -0.0)], [0, 0, 0], [0, 0, 1]),
    "a quotient of -0 after a bound of 0 from above": ([(0, 0, -1, 0.0), (0, 0, -1, 0.0)], [0, 0, 0.0], [0, 0, 1]),
    "a plane through the origin of the ray": ([(S2, S2, 0, F32(S2) * F32(0.5))], [0.25, 0.25, 7.0], [0.6, 0.0, 0.8]),
    "a plane through the origin, leaving": ([(0, 0, -1, -7)], [0.25, 0.25, 7.0], [0.6, 0.0, 0.8]),
    "a slab, oblique": ([(0.6, 0.8, 0, 1.1), (-0.6, -0.8, 0, -2.3)], [-1.3, 0.4, 0.2], [0.48, 0.64, 0.6]),
    "8 planes": ([(1, 0, 0, -1), (-1, 0, 0, -1), (0, 1, 0, -1), (0, -1, 0, -1), (0, 0, 1, -1), (0, 0, -1, -1),
                  (S2, S2, 0, -0.3), (0.6, 0, -0.8, -0.9)], [0.1, -3.0, 0.2], [0.05, 0.99, -0.13]),
    "8 planes, one of them parallel and cut": ([(1, 0, 0, -1), (-1, 0, 0, -1), (0, 1, 0, -1), (0, -1, 0, -1), (0, 0, 1, -1),
                                                (0, 0, -1, -1), (S2, S2, 0, -0.3), (1, 0, 0, 0.5)], [0.1, -3.0, 0.2], [0, 1, 0]),
}


def test_ray_cases_cover_what_they_name():
    """The restatement's own branches, so that the comparison below speaks about them."""
    got = {k: R.ray_interval(np.array(p, F32), o, d) for k, (p, o, d) in RAY_CASES.items()}
    assert got["den > 0"][0] > 0 and got["den > 0"][1] == np.inf
    assert got["den < 0"][0] == 0 and got["den < 0"][1] < np.inf
    assert got["den > 0 behind the origin"][:2] == (0, np.inf)
    assert [got[k][2] for k in ("den == 0 on the kept side", "den == 0 on the cut side", "den == 0 on the plane")] == [False, True, False]
    assert got["an empty interval"][0] > got["an empty interval"][1] and not got["an empty interval"][2]
    assert bits(got["a quotient of -0 against the bound +0"][0]) == 0                  # +0 stays: the sign of the zero is defined
    assert got["a quotient of -0 after a bound of 0 from above"][1] == 0
    assert got["a slab, oblique"][0] > 0 and got["a slab, oblique"][1] < np.inf
    assert 0 < got["8 planes"][0] < got["8 planes"][1] < np.inf and got["8 planes, one of them parallel and cut"][2]


@pytest.mark.parametrize("name", sorted(RAY_CASES))
def test_section_ray_equals_the_restatement(name):
    lib, L = _lib()
    from agile3d_amd import view as V
    planes, o, d = RAY_CASES[name]
    d = (np.asarray(d, np.float64) / np.linalg.norm(d)).astype(F32)
    want = R.ray_interval(np.array(planes, F32), np.array(o, F32), d)
    got = V.section_ray(_section(lib, planes, cull=lib.A3D_CULL_BACK), o, d)
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]) and got[2] == want[2], (got, want)


def test_section_ray_without_planes_and_refusals():
    lib, L = _lib()
    from agile3d_amd import view as V
    for s in (None, _section(lib)):
        assert V.section_ray(s, [1, 2, 3], [0, 1, 0]) == (0.0, np.inf, False)
    out = (C.c_float * 3)()
    assert L.a3d_section_ray(C.byref(_section(lib, n_planes=9)), _f32p([0, 0, 0]), _f32p([0, 0, 1]), out) == lib.A3D_ERR_INVALID
    assert L.a3d_section_ray(None, None, _f32p([0, 0, 1]), out) == lib.A3D_ERR_INVALID
    assert L.a3d_section_ray(None, _f32p([0, 0, 0]), _f32p([0, 0, 1]), None) == lib.A3D_ERR_INVALID


def test_a_crossing_exactly_on_the_interval_ends():
    """The scene of the GPU test's mesh boundary case: in the restatement the crossing's t and both planes' quotients are
    the same bits, and the crossing counts; half a unit further the plane cuts it away."""
    xyz, faces, o, d, t = R.exact_crossing()
    hit, tt, _, _, det = face_pass_f32(xyz, faces, o, d)
    assert hit[0] and bits(tt[0]) == bits(t)
    planes = np.array([(0, 0, 1, 2), (0, 0, -1, -2)], F32)
    t_lo, t_hi, empty = R.ray_interval(planes, o, d)
    assert bits(t_lo) == bits(t) and bits(t_hi) == bits(t) and not empty
    assert R.mesh_section_rule(xyz, faces, o, d, planes, 0)[0] == 0
    assert R.mesh_section_rule(xyz, faces, o, d, np.array([(0, 0, 1, 2.5)], F32), 0)[0] == -1
    assert R.mesh_section_rule(xyz, faces, o, d, np.array([(0, 0, -1, -1.5)], F32), 0)[0] == -1
    assert R.mesh_section_rule(xyz, faces, o, d, np.array([(1, 0, 0, 1)], F32), 0)[0] == -1      # parallel, on the cut side
    assert R.mesh_section_rule(xyz, faces, o, d, np.array([(1, 0, 0, 0.25)], F32), 0)[0] == 0    # parallel, on the plane


def test_the_sign_of_det_tells_the_facing():
    """FRONT is g . d < 0 in float64; the restatement reads it off det > 0.  All twelve rays cross the face, six see its
    front; culling keeps exactly those."""
    fronts = 0
    for xyz, faces, o, d in R.facing_rays():
        a, b, c = xyz[faces[0]].astype(np.float64)
        g = np.cross(b - a, c - a)
        gd = float(g @ d.astype(np.float64))
        assert abs(gd) > 0.3 * np.linalg.norm(g)
        hit, tt, _, _, det = face_pass_f32(xyz, faces, o, d)
        assert hit[0] and bool(R.front(det[0])) == (gd < 0)
        fronts += gd < 0
        none = np.zeros((0, 4), F32)
        assert R.mesh_section_rule(xyz, faces, o, d, none, R.CULL_NONE)[0] == 0
        assert (R.mesh_section_rule(xyz, faces, o, d, none, R.CULL_BACK)[0] == 0) == (gd < 0)
        assert (R.mesh_section_rule(xyz, faces, o, d, none, R.CULL_FRONT)[0] == 0) == (gd > 0)
    assert fronts == 6


def test_the_room_faces_inwards():
    xyz, faces = R.room()
    assert xyz.shape == (11, 3) and faces.shape == (13, 3)
    x = xyz.astype(np.float64)
    for a, b, c in x[faces[:12]]:
        g = np.cross(b - a, c - a)
        assert g @ -(a + b + c) > 0 and np.count_nonzero(g) == 1            # towards the centre, along one axis
    a, b, c = x[faces[R.INNER]]
    assert np.array_equal(np.cross(b - a, c - a), [0.0, -1.0, 0.0])
    # closed: every edge of the box is shared by two faces, in opposite directions
    edges = [(f[k], f[(k + 1) % 3]) for f in faces[:12].tolist() for k in range(3)]
    assert len(set(edges)) == 36 and all((q, p) in edges for p, q in edges)


# ------------------------------------------------------------------------------------------- the Section class
def test_section_class():
    from agile3d_amd.session import Section
    s = Section([((0, 0, 2), 3.0), ((0, 3, 4), (1.0, 1.0, 1.0))], cull="back")
    assert s.n_planes == 2 and s.cull == "back" and s.normals.dtype == F32 and s.offsets.dtype == F32
    assert np.array_equal(s.normals, np.array([[0, 0, 1], [0, 0.6, 0.8]], F32)) and np.array_equal(s.offsets, np.array([1.5, 1.4], F32))
    c = s.struct()
    assert (c.n_planes, c.cull) == (2, 1) and list(c.planes[1]) == [0.0, float(F32(0.6)), float(F32(0.8)), float(F32(1.4))]
    assert [Section(cull=k).struct().cull for k in ("none", "back", "front")] == [0, 1, 2]
    t = s.with_cull("front")
    assert t.cull == "front" and np.array_equal(t.normals, s.normals) and np.array_equal(t.offsets, s.offsets) and s.cull == "back"
    # with_cull shares the stored values: oblique planes come back bit for bit (normalising fp32 normals again would not)
    rng = np.random.default_rng(7)
    for _ in range(300):
        r = Section([(rng.normal(size=3), rng.normal()) for _ in range(4)], cull="front")
        for q in (r.with_cull("back"), r.with_cull("back").with_cull("none")):
            assert np.array_equal(bits(q.normals), bits(r.normals)) and np.array_equal(bits(q.offsets), bits(r.offsets))
            assert bytes(q.struct())[8:] == bytes(r.struct())[8:]
    with pytest.raises(ValueError):
        s.with_cull("both")
    with pytest.raises(AttributeError):
        t.cull = "none"
    assert Section().n_planes == 0 and Section().cull == "none" and Section().keeps(np.zeros((3, 3))).all()
    with pytest.raises(AttributeError):
        s.cull = "none"
    with pytest.raises(ValueError):
        s.normals[0, 0] = 1.0
    for bad in (dict(cull="both"), dict(planes=[((0, 0, 0), 1.0)]), dict(planes=[((0, NAN, 1), 1.0)]), dict(planes=[((0, 0, 1), INF)]),
                dict(planes=[((0, 0, 1), (0.0, NAN, 0.0))]), dict(planes=[((0, 1), 1.0)]), dict(planes=[((0, 0, 1), (1.0, 2.0))]),
                dict(planes=[(0, 0, 1, 1)]), dict(planes=[((0, 0, 1), 0.0)] * 9), dict(planes=[((0, 0, 1e-30), 1e30)])):
        with pytest.raises(ValueError):
            Section(**bad)
    # every Section passes the library's own check: |n|^2 of a normalised fp32 normal lies well inside [0.5, 2]
    rng = np.random.default_rng(0)
    for _ in range(50):
        n = rng.normal(size=3) * 10.0 ** rng.uniform(-6, 6)
        q = Section([(n, rng.normal())]).normals[0].astype(np.float64)
        assert abs(q @ q - 1.0) < 1e-6


def test_section_box_below_keeps():
    from agile3d_amd.session import Section
    box = Section.box([-1.0, -2.0, 0.0], [1.0, 2.0, 0.5])
    assert box.n_planes == 6 and box.cull == "none"
    pts = np.array([[0, 0, 0.25], [1, 2, 0.5], [-1, -2, 0], [1.0000001, 0, 0.25], [0, -2.0000002, 0.25], [0, 0, 0.50000006],
                    [0, 0, -1e-9], [NAN, 0, 0.25], [0, 0, NAN], [0.5, INF, 0.25]], np.float64)
    assert box.keeps(pts).tolist() == [True, True, True, False, False, False, False, False, False, False]
    below = Section.below(2.5, cull="back")
    assert below.n_planes == 1 and below.cull == "back"
    assert np.array_equal(below.normals, np.array([[0, 0, -1]], F32)) and np.array_equal(below.offsets, np.array([-2.5], F32))
    assert below.keeps([[9, 9, 2.5], [9, 9, 2.4999998], [9, 9, 2.5000002], [0, 0, -INF]]).tolist() == [True, True, False, True]
    # keeps IS the restatement the kernels are held to
    rng = np.random.default_rng(3)
    s = Section([(rng.normal(size=3), rng.normal()) for _ in range(8)])
    p = rng.normal(size=(500, 3)).astype(F32)
    planes = np.concatenate([s.normals, s.offsets[:, None]], 1)
    assert np.array_equal(s.keeps(p), R.keeps(planes, p))
    on = Section([((0.6, 0.0, 0.8), 0.0)])                       # a point exactly on an oblique plane: kept
    assert on.keeps([[0.8, 5.0, -0.6]]).tolist() == [bool((F32(0.6) * F32(0.8)) + F32(0.8) * F32(-0.6) >= 0)]
    assert Section([((0, 1, 0), 0.25)]).keeps([[3.0, 0.25, -7.0]]).tolist() == [True]


def test_marker_filtering_on_a_click_list():
    """``visible_clicks`` names the clicks whose marker a view under a section shows; ``click_at`` composes it with the
    rows ``marker_table`` keeps."""
    from agile3d_amd import view as V
    from agile3d_amd.session import Section, camera_from_matrices, visible_clicks
    points = np.array([[0.0, 0.0, 0.5], [0.2, 0.1, 1.5], [0.0, 0.0, -9.0], [0.1, -0.1, 1.0], [-0.3, 0.2, 0.99]], F32)
    assert visible_clicks(None, points).tolist() == [0, 1, 2, 3, 4]
    assert visible_clicks(Section(cull="back"), points).tolist() == [0, 1, 2, 3, 4]              # culling hides no click
    sec = Section.below(1.0)
    assert visible_clicks(sec, points).tolist() == [0, 2, 3, 4]
    assert visible_clicks(Section.box([-1, -1, 0], [1, 1, 2]), points).tolist() == [0, 1, 3, 4]
    assert visible_clicks(sec, np.zeros((0, 3), F32)).tolist() == []
    # the camera at the origin looks along +z: click 2 lies behind it, so marker_table leaves it out of the visible ones
    cam = camera_from_matrices(np.array([[50.0, 0, 32], [0, 50.0, 24], [0, 0, 1]]), np.eye(4), 64, 48)
    visible = visible_clicks(sec, points)
    rows, kept = V.marker_table(cam, points[visible], np.ones((len(visible), 3)), return_kept=True)
    assert kept.tolist() == [0, 2, 3] and visible[kept].tolist() == [0, 3, 4]
