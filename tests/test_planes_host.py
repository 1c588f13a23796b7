"""Host side of the planes of a scan (no GPU): the rule's restatement (``planes_rule.py``) on hand-made cases whose answer is
known, the admission of rows, the host's direction table, the naming of planes (``plane_kinds``), ``upright`` and ``section``,
every ``ValueError`` the ``view.py`` wrappers raise before the library is reached, the entry point's refusals, and the room of
DESIGN 4.9.  ``test_gpu_planes.py`` holds the kernels to the same restatement bit for bit.

THE HAND-MADE PLANES have the unit vector of a direction cell's centre as their normal and lie at the centre of an offset bin
of that cell, in the frame origin 0, quantum 2^-18, bits 20, with bins of 0.05: all their rows vote for ONE bin k, so scores are
row counts -- and the windows around k-1, k and k+1 tie, so a lone plane's peak is bin k-1, the lowest.  PARALLEL PLANES of one
cell, m bins apart, inlier distance 1.5 bins:
  m = 1  the window of three bins around either holds both: one peak, seeded by both; the fit lies between them, 0.5 bins from
         each: ONE plane.
  m = 2  the bin between them scores both (H[k-1] + H[k+1]) and is the peak -- equal to neither's own window only when one is
         empty; the fit lies 1 bin from each, inside 1.5: ONE plane.
  m = 3  no window of three bins holds both; the first is fitted alone and the other lies 3 bins off, beyond 1.5: TWO planes.

THE ROOM'S BOUNDS are the issue's: every planted plane holds >= 99 % of its rows under one id, its fit lies within 0.5 degrees,
no recorded plane is made of sphere rows.  The restatement's own numbers (printed): 100 %, 0.03 degrees (the table top 0.22)."""
import ctypes as C

import numpy as np
import pytest
import torch

import planes_cases as PC
import planes_rule as PR
from planes_cases import A, B, BIN, BITS, Cc, ORIGIN, QUANTUM, all_spent, cell_normal, cell_of, plate, seventeen, spent_then_found

G, D = PR.G, PR.D



def run(parts, min_voxels=200, max_planes=16, normal_deg=20.0, dist_tol=1.5 * BIN, offset_bin=BIN, candidate=None, frame=None,
        **kw):
    p = np.concatenate([x[0] for x in parts])
    v = np.concatenate([x[1] for x in parts])
    origin, quantum, bits = frame or (ORIGIN, QUANTUM, BITS)
    s = PC.settings(quantum, normal_deg, offset_bin, dist_tol, min_voxels, max_planes)
    out = PR.find_planes(v, p, origin, quantum, bits, candidate=candidate, **s, **kw)
    out["owner"] = np.concatenate([np.full(len(x[0]), i) for i, x in enumerate(parts)])
    return out


# ------------------------------------------------------------------------------------------- the rule on planes whose answer is known
def test_one_plane():
    part = plate(A, 530, 400)
    out = run([part])
    rec, s = out["records"], out["summary"]
    assert (s["n_planes"], s["rounds"], s["spent"], s["admitted"]) == (1, 1, 0, 400) and sum(s["left_out"].values()) == 0
    assert (out["plane_qv"] == 0).all() and rec["inliers"][0] == rec["count"][0] == rec["score"][0] == 400
    assert rec["bin"][0] == A * D + 529 and rec["round"][0] == 0     # windows 529, 530, 531 tie: the lowest
    assert PR.NR.angle(rec["normal"][0], cell_normal(A)) < 1e-5
    assert abs(float(rec["offset"][0]) - (530 - D // 2 + 0.5) * BIN) < 1e-5 and rec["rms"][0] < 1e-5
    X = PR.NR.fixed_point(part[0], ORIGIN, QUANTUM, BITS)[0]
    assert rec["sum"][0].tolist() == X.sum(0).tolist() and rec["mom"][0][0] == (X[:, 0] * X[:, 0]).sum()
    # the record's integer plane is the one the rows were tested against
    e = X @ rec["N"][0].astype(np.int64) - rec["off"][0]
    assert np.abs(e).max() <= PC.settings(QUANTUM)["dist_tol"]


@pytest.mark.parametrize("apart, planes", [(1, 1), (2, 1), (3, 2)])
def test_parallel_planes(apart, planes):
    out = run([plate(A, 500, 300), plate(A, 500 + apart, 260)])
    assert out["summary"]["n_planes"] == planes and out["summary"]["spent"] == 0
    if planes == 1:
        assert (out["plane_qv"] == 0).all() and out["records"]["inliers"][0] == 560
        assert out["records"]["bin"][0] == A * D + (501 if apart == 2 else 500)      # m = 2: the bin BETWEEN them is the peak
        assert abs(float(out["records"]["rms"][0]) - apart * BIN / 2) < 0.1 * BIN
    else:
        assert np.array_equal(out["plane_qv"], out["owner"]) and out["records"]["inliers"].tolist() == [300, 260]


def test_equal_planes_lower_bin_first():
    out = run([plate(Cc, 560, 250), plate(B, 470, 250), plate(A, 512, 250)])
    rec = out["records"]
    assert rec["score"].tolist() == [250, 250, 250] and rec["bin"].tolist() == sorted(rec["bin"].tolist())
    assert rec["bin"].tolist() == [B * D + 469, Cc * D + 559, A * D + 511]
    assert np.array_equal(out["plane_qv"], np.array([1, 0, 2])[out["owner"]])


def test_direction_cells():
    f = lambda *v: int(PR.direction_cell(np.array([v], np.float32))[0])
    # exactly on a boundary: n_b == t_j n_a counts (>=); just below it does not
    assert f(0.25, 0.0, 1.0) == cell_of(2, 10, 8)
    assert f(np.nextafter(np.float32(0.25), np.float32(0)), 0.0, 1.0) == cell_of(2, 9, 8)
    assert f(0.0, 0.0, 3.0) == cell_of(2, 8, 8) and f(1.0, 1.0, 1.0) == cell_of(0, 15, 15)
    # a face diagonal |n_x| == |n_y|: axis 0 wins; |n_y| == |n_z| > |n_x|: axis 1
    assert f(0.5, -0.5, 0.1) == cell_of(0, 0, 9) and f(-0.5, 0.5, 0.1) == cell_of(0, 0, 6)
    assert f(0.1, -0.5, 0.5) == cell_of(1, 0, 6)
    # opposite signs of one normal land in one cell
    v = np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32)
    assert np.array_equal(PR.direction_cell(v), PR.direction_cell(-v))
    assert len(np.unique(PR.direction_cell(v))) > 600 and PR.direction_cell(v).max() < 3 * G * G


def test_stop_score():
    """min_voxels = 200: the call ends at a peak under 50."""
    out = run([plate(A, 500, 49)])
    assert out["summary"] == dict(out["summary"], n_planes=0, rounds=0, spent=0, admitted=49) and (out["plane_qv"] == -1).all()
    out = run([plate(A, 500, 50)])
    assert out["summary"] == dict(out["summary"], n_planes=0, rounds=1, spent=1) and (out["plane_qv"] == -1).all()
    out = run([plate(A, 500, 2)], min_voxels=1)                                     # never under 3
    assert out["summary"]["rounds"] == 0
    out = run([plate(A, 500, 9, side=0.3)], min_voxels=1)
    assert out["summary"]["n_planes"] == 1


def test_spent_round_then_found():
    out = run(spent_then_found())
    s = out["summary"]
    assert (s["n_planes"], s["rounds"], s["spent"]) == (1, 2, 1)
    assert np.array_equal(out["plane_qv"], np.where(out["owner"] == 1, 0, -1))
    assert out["records"]["round"][0] == 1 and out["records"]["inliers"][0] == 300 and out["records"]["score"][0] < 199


def test_max_planes():
    parts = [plate(A, 500, 300), plate(B, 500, 260)]
    out = run(parts, max_planes=1)
    assert (out["summary"]["n_planes"], out["summary"]["rounds"]) == (1, 1)
    assert np.array_equal(out["plane_qv"], np.where(out["owner"] == 0, 0, -1))


def test_seventeen_planes_sixteen_found():
    out = run(seventeen(), min_voxels=40)
    assert (out["summary"]["n_planes"], out["summary"]["rounds"], out["summary"]["spent"]) == (16, 16, 0)
    assert out["records"]["inliers"].tolist() == list(range(76, 60, -1))             # the largest first; the smallest is left
    assert np.array_equal(out["plane_qv"], np.where(out["owner"] == 0, -1, 16 - out["owner"]))


def test_round_cap():
    """max_planes = 2: four rounds, all spent on planes too small to record; the fifth is never looked at."""
    out = run(all_spent(), min_voxels=40, max_planes=2)
    assert (out["summary"]["n_planes"], out["summary"]["rounds"], out["summary"]["spent"]) == (0, 4, 4)


# ------------------------------------------------------------------------------------------- admission
def test_admission():
    p, v = plate(A, 520, 300)
    p, v = p.copy(), v.copy()
    cand = np.ones(300, np.uint8)
    cand[:7] = 0
    v[3] = np.nan                                   # (not a candidate either: counted there)
    v[10:13, 1] = np.nan
    p[13, 2] = np.inf
    v[20:25] = 0.0
    v[25] = [0.0, -0.0, 0.0]
    p[30:34, 0] = 100.0                             # beyond 2^20 quanta of 2^-18
    v[30] = 0.0                                     # (a zero normal comes first)
    out = run([(p, v)], candidate=cand)
    assert out["summary"]["left_out"] == dict(candidate=7, nonfinite=4, zero_normal=7, frame=3, bins=0)
    assert out["summary"]["admitted"] == 300 - 21 and out["summary"]["n_planes"] == 1
    left = np.r_[0:7, 10:14, 20:26, 30:34]
    assert (out["plane_qv"][left] == -1).all() and (np.delete(out["plane_qv"], left) == 0).all()
    # offsets beyond D: bins of a quantum's width put everything but the rows next to the origin outside
    out = run([plate(A, 520, 300)], offset_bin=2.0 ** -18, dist_tol=2.0 ** -18)
    assert out["summary"]["left_out"]["bins"] == 300 and out["summary"]["admitted"] == 0 and out["summary"]["rounds"] == 0
    # no rows at all
    out = run([(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))])
    assert out["summary"]["n_planes"] == 0 and len(out["plane_qv"]) == 0


def test_inverse_map():
    parts = [plate(A, 500, 300)]
    inv = np.array([0, 299, 5, -1, 300, 7], np.int64)
    out = run(parts, inverse_map=inv)
    assert out["plane_full"].tolist() == [0, 0, 0, -2, -2, 0] and out["summary"]["err"] == PR.BAD_INDEX
    assert run(parts, inverse_map=inv[:3])["summary"]["err"] == 0


# ------------------------------------------------------------------------------------------- the host's table, the names, the cuts
def test_direction_table():
    from agile3d_amd import view as V
    t = V.direction_table()
    assert t.dtype == np.int32 and t.shape == (3 * G * G, 3) and np.array_equal(t, PR.direction_table())
    length = np.sqrt((t.astype(np.float64) ** 2).sum(1)) / PR.SCALE
    assert np.abs(length - 1.0).max() <= 2.0 ** -20
    t4 = t.reshape(3, G, G, 3)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        assert (t4[a, :, :, a] > 0).all()
        flipped = t4[a, ::-1].copy()
        flipped[..., b] *= -1
        assert np.array_equal(flipped, t4[a])                                        # u -> -u
        assert np.array_equal(t4[a].transpose(1, 0, 2)[..., [a, c, b]], t4[a][..., [a, b, c]])   # u <-> v
        assert np.array_equal(t4[a][..., [a, b, c]], t4[0][..., [0, 1, 2]])          # the three faces alike
    # a cell's own centre lands in that cell
    assert np.array_equal(PR.direction_cell(t.astype(np.float32)), np.arange(3 * G * G))


def test_plane_kinds_and_upright():
    from agile3d_amd.session import plane_kinds, upright_rotation
    tilt = PC.rotation(3.0, 20.0)
    normals = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1]], np.float64)
    normals[5] /= np.sqrt(2.0)
    offsets = np.array([0.0, -2.5, 0.0, 3.0, 0.75, 1.0])
    kinds = plane_kinds(normals @ tilt.T, offsets, up=(0, 0, 1))
    assert kinds == ["floor", "ceiling", "wall", "wall", "horizontal", "other"]       # (a ceiling's normal may point down)
    assert plane_kinds(normals[:1], offsets[:1]) == ["floor"] and plane_kinds(normals[2:4], offsets[2:4]) == ["wall", "wall"]
    assert plane_kinds(normals[:0], offsets[:0]) == []
    assert plane_kinds(normals, offsets, up=(2, 0, 0))[:4] == ["wall", "wall", "floor", "wall"]
    assert plane_kinds(normals[[0, 4]], [1.0, 1.0]) == ["floor", "horizontal"]        # equal heights: the earlier is the floor
    for bad in (dict(up=(0, 0, 0)), dict(up=(1, np.nan, 0)), dict(normal_deg=46.0), dict(normal_deg=-1.0)):
        with pytest.raises(ValueError):
            plane_kinds(normals, offsets, **bad)
    for n in (tilt[:, 2], -tilt[:, 2], np.array([0.0, 0.0, 1.0])):
        R = upright_rotation(n)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1.0) < 1e-14
        assert np.allclose(R @ (n if n[2] > 0 else -n), [0, 0, 1], atol=1e-14)
    assert np.array_equal(upright_rotation((0, 0, 1)), np.eye(3))


def hand_result(normals, offsets, up=(0.0, 0.0, 1.0)):
    from agile3d_amd import view as V
    from agile3d_amd.session import PlanesResult, plane_kinds
    rec = np.zeros(len(offsets), V.PLANE)
    rec["normal"], rec["offset"] = normals, offsets
    kinds = plane_kinds(rec["normal"], rec["offset"], up)
    first = lambda kind: kinds.index(kind) if kind in kinds else None
    return PlanesResult(records=rec, n_planes=len(rec), kinds=kinds, floor=first("floor"), ceiling=first("ceiling"),
                        walls=[k for k, x in enumerate(kinds) if x == "wall"], up=np.asarray(up, np.float64),
                        plane_full=torch.tensor([0, 1, -1, 2, 1], dtype=torch.int32))


def test_section_and_selection():
    r = hand_result([[0, 0, 1], [0, 0, -1], [1, 0, 0]], [0.0, -2.5, 4.0])
    assert (r.floor, r.ceiling, r.walls) == (0, 1, [2])
    pts = np.array([[0, 0, -0.1], [0, 0, 0.02], [0, 0, 1.0], [0, 0, 2.47], [0, 0, 2.5], [0, 0, 2.6], [5, 0, 1.0]], np.float32)
    assert r.section(r.ceiling, "below", margin=0.05).keeps(pts).tolist() == [True, True, True, False, False, False, True]
    assert r.section(r.ceiling, "below").keeps(pts).tolist() == [True, True, True, True, True, False, True]
    assert r.section(r.floor, "above", margin=0.05).keeps(pts).tolist() == [False, False, True, True, True, True, True]
    assert r.section(r.floor, "below").keeps(pts).tolist() == [True, False, False, False, False, False, False]
    assert r.section(2, "above").keeps(pts).tolist() == [False] * 6 + [True]           # a wall: the side its normal points to
    assert r.section(2, "below", cull="back").cull == "back"
    assert r.selection(1).tolist() == [0, 1, 0, 0, 1] and r.selection(1).dtype == torch.uint8
    for bad in (lambda: r.section(3), lambda: r.section(-1), lambda: r.section(0, "left"), lambda: r.section(0, margin=np.inf),
                lambda: r.selection(3), lambda: r.selection(None), lambda: r.section(True)):
        with pytest.raises(ValueError):
            bad()
    tilted = hand_result([PC.rotation(3.0, 0.0)[:, 2]], [0.0])
    assert np.allclose(tilted.upright() @ PC.rotation(3.0, 0.0)[:, 2], [0, 0, 1], atol=1e-6)
    assert np.array_equal(hand_result([[1, 0, 0]], [0.0]).upright(), np.eye(3))          # no floor


# ------------------------------------------------------------------------------------------- refusals
def test_wrapper_value_errors():
    from agile3d_amd import view as V
    assert V.planes_settings(QUANTUM, BIN, 20.0, 1.5 * BIN, 200, 16) == (*PR.settings(QUANTUM, BIN, 20.0, 1.5 * BIN), 200, 16)
    for bad in (dict(quantum=0.3), dict(offset_bin=0.0), dict(offset_bin=np.nan), dict(offset_bin="wide"), dict(offset_bin=1e9),
                dict(dist_tol=-1e-3), dict(dist_tol=np.inf), dict(normal_deg=91.0), dict(normal_deg=-1.0), dict(normal_deg=np.nan),
                dict(normal_deg=None), dict(min_voxels=0), dict(min_voxels=2.5), dict(max_planes=0), dict(max_planes=17),
                dict(max_planes=True)):
        kw = dict(quantum=QUANTUM, offset_bin=BIN, normal_deg=20.0, dist_tol=1.5 * BIN, min_voxels=200, max_planes=16)
        with pytest.raises(ValueError):
            V.planes_settings(**dict(kw, **bad))
    with pytest.raises(ValueError, match="GPU"):                                       # there is no CPU path
        V.find_planes(torch.zeros(4, 3), torch.zeros(4, 3), ORIGIN, QUANTUM, offset_bin=BIN, dist_tol=BIN)
    rec, s = V.read_planes(np.zeros(V.PLANES_OUT_BYTES, np.uint8))
    assert len(rec) == 0 and s["n_planes"] == 0 and set(s["left_out"]) == set(V.PLANES_LEFT_OUT) == set(PR.LEFT_OUT)
    assert V.PLANE == PR.PLANE


def test_entry_point_refusals():
    """Every refusal comes before the first launch, so none needs a GPU; the pointers are never followed."""
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib as L
    lib = L.load()
    assert lib.a3d_planes_workspace_bytes(-1) == 0 and lib.a3d_planes_workspace_bytes(1 << 31) == 0
    need = lib.a3d_planes_workspace_bytes(1000)
    assert need > 3 * G * G * D * 4 and need % 256 == 0 and lib.a3d_planes_workspace_bytes(0) > 0

    def args(**kw):
        a = L.FindPlanesArgs()
        a.normal_dev = a.pos_dev = a.table_dev = a.plane_qv_dev = a.out_dev = a.workspace_dev = 4096
        a.n, a.workspace_bytes, a.quantum, a.bits, a.cos_min = 1000, need, QUANTUM, BITS, 0.9
        a.bin_width, a.dist_tol, a.min_voxels, a.max_planes = 1 << 30, 1 << 30, 200, 16
        for k, v in kw.items():
            if k == "origin":
                a.origin[:] = v
            else:
                setattr(a, k, v)
        return a

    assert lib.a3d_find_planes(None, None) == L.A3D_ERR_INVALID
    for bad in (dict(n=-1), dict(n=1 << 31), dict(n=1 << 23), dict(bits=21), dict(bits=-1), dict(quantum=0.3), dict(quantum=0.0),
                dict(origin=[0.0, np.nan, 0.0]), dict(bin_width=0), dict(bin_width=(1 << 44) + 1), dict(dist_tol=-1),
                dict(dist_tol=(1 << 44) + 1), dict(cos_min=1.5), dict(cos_min=-0.1), dict(cos_min=float("nan")), dict(min_voxels=0),
                dict(max_planes=0), dict(max_planes=17), dict(normal_dev=None), dict(pos_dev=None), dict(plane_qv_dev=None),
                dict(table_dev=None), dict(out_dev=None), dict(out_dev=4100), dict(workspace_dev=None), dict(workspace_dev=4224),
                dict(workspace_bytes=need - 1), dict(n_full=5), dict(plane_full_dev=4096), dict(n_full=-1, inverse_map_dev=4096),
                dict(n_full=5, inverse_map_dev=4096), dict(n_full=1 << 31, inverse_map_dev=4096, plane_full_dev=4096)):
        assert lib.a3d_find_planes(C.byref(args(**bad)), None) == L.A3D_ERR_INVALID, bad
        assert b"a3d_find_planes" in lib.a3d_last_error()


# ------------------------------------------------------------------------------------------- the room
@pytest.mark.parametrize("yaw", [0, 20, 45])
def test_room(yaw):
    p, v, surface, planted, _ = PC.room(yaw, sigma_deg=3.0)
    origin, quantum, bits = PC.frame(p)
    out = PR.find_planes(v, p, origin, quantum, bits, **PC.settings(quantum))
    rows, sphere = PC.room_report(out, surface, planted)
    print(f"room yaw {yaw}: {len(p)} rows, {out['summary']}")
    for name, (k, share, deg) in zip(PC.ROOM_SURFACES, rows):
        print(f"  {name:8s} id {k} share {share:.4f} fit {deg:.3f} deg")
    print("  sphere rows per plane", [round(x, 3) for x in sphere], "rms", out["records"]["rms"].round(4).tolist())
    assert out["summary"]["n_planes"] == 7 and len({k for k, _, _ in rows}) == 7
    assert all(share >= 0.99 and deg <= 0.5 for _, share, deg in rows)
    assert max(sphere) < 0.5 and (out["plane_qv"][surface == PC.SPHERE] == -1).mean() > 0.9
