"""-m gpu: the planes of a scan -- a3d_find_planes (csrc/session_planes.hip) -- against the rule restated in ``planes_rule.py``.
plane_qv, plane_full, every integer of the records (inliers, score, round, bin, count, sum, mom, N, off), the normals, the
summary's counters and the error word are compared BIT FOR BIT.  offset and rms are compared within 1 fp32 ulp and the measured
ulps are printed: both are a double rounded once to fp32; the offset's double is built from + and x alone and is expected to
agree exactly, the rms' goes through a division and a square root, whose last bit may differ from numpy's and move the rounded
fp32 value by at most one step.

Row counts: 1, 63, 64, 65, 257 (a wave is 64 rows, a workgroup 256) and ROW_PASS + 1, at which a workgroup of every row kernel
(vote, sums, assign, lift) walks its grid a second time; the peak kernel's grid always walks the 786432 bins three times.  Plane
counts 0, 1, 2 of one direction cell 1, 2 and 3 bins apart, 16 of 17; a spent round followed by a found plane; the cap of
2 max_planes rounds.  The outputs start as sentinels, so that an untouched entry shows."""
import numpy as np
import pytest
import torch

import planes_cases as PC
import planes_rule as PR
from agile3d_amd import view as V
from planes_cases import A, B, BIN, BITS, ORIGIN, QUANTUM, all_spent, plate, seventeen, spent_then_found
from session_kit import DEV, _dev

pytestmark = pytest.mark.gpu
F32 = np.float32
ROW_PASS = 256 * 256           # rows one pass of a row kernel's grid covers (kPlB x kPlRowBlocks)
PEAK_PASS = 256 * 1024         # bins one pass of the peak kernel's grid covers (kPlB x kPlPeakBlocks)
assert 3 * PR.G * PR.G * PR.D == 3 * PEAK_PASS
INTEGERS = ("inliers", "score", "round", "bin", "count", "sum", "mom", "N", "off")


def ulps(a, b):
    """The distance of fp32 arrays in units in the last place (finite values of one sign, or zeros)."""
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-(2 ** 31)) - x.view(np.int32), x.view(np.int32)).astype(np.int64)
    return np.abs(key(np.ascontiguousarray(a, F32)) - key(np.ascontiguousarray(b, F32)))


def run_gpu(v, p, frame, settings, candidate=None, inverse_map=None):
    n = len(v)
    origin, quantum, bits = frame
    plane_qv = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    plane_full = None if inverse_map is None else torch.full((len(inverse_map),), -2, dtype=torch.int32, device=DEV)
    out = torch.full((V.PLANES_OUT_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
    got = V.find_planes(_dev(v, F32).reshape(-1, 3), _dev(p, F32).reshape(-1, 3), origin, quantum, bits,
                        candidate=None if candidate is None else _dev(candidate, np.uint8),
                        inverse_map=None if inverse_map is None else _dev(inverse_map, np.int64), plane_qv=plane_qv,
                        plane_full=plane_full, out=out, **settings)
    assert got[0] is plane_qv and got[1] is plane_full and got[2] is out
    raw = out.cpu().numpy()
    records, summary = V.read_planes(raw)
    return dict(plane_qv=plane_qv.cpu().numpy(), plane_full=None if plane_full is None else plane_full.cpu().numpy(),
                records=records, summary=summary, raw=raw)


def check(v, p, frame=(ORIGIN, QUANTUM, BITS), candidate=None, inverse_map=None, what="", **kw):
    settings = dict(offset_bin=BIN, normal_deg=20.0, dist_tol=1.5 * BIN, min_voxels=200, max_planes=16)
    settings.update(kw)
    got = run_gpu(v, p, frame, settings, candidate, inverse_map)
    w, tol, cos_min = PR.settings(frame[1], settings["offset_bin"], settings["normal_deg"], settings["dist_tol"])
    want = PR.find_planes(v, p, *frame, w, tol, cos_min, settings["min_voxels"], settings["max_planes"], candidate=candidate,
                          inverse_map=inverse_map)
    assert got["summary"] == want["summary"], (got["summary"], want["summary"])
    assert got["plane_qv"].tobytes() == want["plane_qv"].tobytes(), np.flatnonzero(got["plane_qv"] != want["plane_qv"])[:8]
    if inverse_map is not None:
        assert got["plane_full"].tobytes() == want["plane_full"].tobytes()
    g, r = got["records"], want["records"]
    assert len(g) == len(r)
    for field in INTEGERS + ("normal",):
        assert g[field].tobytes() == r[field].tobytes(), (field, g[field], r[field])
    u_off, u_rms = ulps(g["offset"], r["offset"]), ulps(g["rms"], r["rms"])
    print(f"{what}: n={len(v)} planes={len(g)} rounds={got['summary']['rounds']} spent={got['summary']['spent']} max ulps: offset "
          f"{u_off.max() if len(g) else 0} rms {u_rms.max() if len(g) else 0}")
    assert np.isfinite(g["offset"]).all() and np.isfinite(g["rms"]).all() and (u_off <= 1).all() and (u_rms <= 1).all()
    # what lies behind the records is as it was cleared
    assert not got["raw"][len(g) * V.PLANE.itemsize:V.PLANES_MAX * V.PLANE.itemsize].any()
    return got


def join(parts):
    return np.concatenate([x[1] for x in parts]), np.concatenate([x[0] for x in parts])


@pytest.fixture(scope="module")
def scan():
    """A shuffled room of 65 k rows and more (scale 1.45), with its frame."""
    p, v, surface, _, _ = PC.room(33.0, sigma_deg=3.0, seed=3, scale=1.45)
    assert len(p) > ROW_PASS
    order = np.random.default_rng(1).permutation(len(p))
    return v[order], p[order], PC.frame(p)


# ------------------------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_few_rows(n):
    p, v, _, _, _ = PC.room(20.0, seed=n, scale=0.3)
    order = np.random.default_rng(n).permutation(len(p))[:n]
    got = check(v[order], p[order], PC.frame(p), min_voxels=12, what="few rows")
    assert n < 63 or got["summary"]["rounds"] >= 1


def test_second_grid_pass(scan):
    v, p, frame = scan
    n = ROW_PASS + 1
    inverse_map = np.random.default_rng(2).integers(0, n, n + 5)
    got = check(v[:n], p[:n], frame, inverse_map=inverse_map, what="second pass")
    assert got["summary"]["n_planes"] >= 7 and (got["plane_qv"][ROW_PASS:] >= -1).all() and got["plane_qv"][ROW_PASS - 300:].max() >= 0


# ------------------------------------------------------------------------------------------- plane counts
def test_no_plane():
    v, p = join([plate(A, 520, 300)])
    got = check(np.zeros_like(v), p, what="zero normals")
    assert got["summary"]["left_out"]["zero_normal"] == 300 and (got["plane_qv"] == -1).all()
    got = check(*join([plate(A, 520, 49), plate(B, 500, 40)]), what="peaks below the stop")
    assert got["summary"]["rounds"] == 0 and got["summary"]["admitted"] == 89 and (got["plane_qv"] == -1).all()


def test_one_plane():
    got = check(*join([plate(A, 530, 400)]), what="one plane")
    assert got["summary"]["n_planes"] == 1 and (got["plane_qv"] == 0).all()


@pytest.mark.parametrize("apart, planes", [(1, 1), (2, 1), (3, 2)])
def test_two_planes_of_one_cell(apart, planes):
    got = check(*join([plate(A, 500, 300), plate(A, 500 + apart, 260)]), what=f"{apart} bins apart")
    assert got["summary"]["n_planes"] == planes


def test_sixteen_of_seventeen():
    got = check(*join(seventeen()), min_voxels=40, what="16 of 17")
    assert got["summary"]["n_planes"] == 16 and got["summary"]["rounds"] == 16 and (got["plane_qv"][:60] == -1).all()


def test_normals_on_cell_boundaries():
    """Normals exactly on a boundary (n_b == t_j n_a), on a face diagonal, on the cube's diagonal, and their opposites: each
    group is a small plane of its own cell, so the records' bins show the cells the kernel chose."""
    special = [(0.25, 0.0, 1.0), (0.5, -0.5, 0.1), (-0.5, 0.5, 0.1), (1.0, 1.0, 1.0), (0.0, 0.0, -3.0), (0.1, -0.5, 0.5),
               (-0.75, 0.0, -1.0), (0.0, 1.0, 0.0)]
    parts = []
    for i, n in enumerate(special):
        p, _ = PC.rectangle(n, 0.3 + 0.2 * i, 0.5, 40 + i)
        parts.append((p, np.tile(np.float32(n), (len(p), 1))))
    got = check(*join(parts), min_voxels=20, what="normals on cell boundaries")
    cells = sorted(set((got["records"]["bin"] // PR.D).tolist()))
    want = sorted(set(PR.direction_cell(np.float32(special)).tolist()))
    assert got["summary"]["rounds"] == len(special) and set(cells) <= set(want) and len(cells) >= 5, (cells, want)   # (every group was a peak)


# ------------------------------------------------------------------------------------------- rounds
def test_spent_round_then_found():
    got = check(*join(spent_then_found()), what="spent, then found")
    assert (got["summary"]["n_planes"], got["summary"]["rounds"], got["summary"]["spent"]) == (1, 2, 1)
    assert (got["plane_qv"][:199] == -1).all() and (got["plane_qv"][199:] == 0).all()


def test_round_cap():
    got = check(*join(all_spent()), min_voxels=40, max_planes=2, what="the cap of rounds")
    assert (got["summary"]["n_planes"], got["summary"]["rounds"], got["summary"]["spent"]) == (0, 4, 4)
    got = check(*join([plate(A, 500, 300), plate(B, 500, 260)]), max_planes=1, what="max_planes = 1")
    assert got["summary"]["n_planes"] == 1 and (got["plane_qv"][300:] == -1).all()


# ------------------------------------------------------------------------------------------- inputs
def test_admission_candidate_and_lift():
    p, v = plate(A, 520, 300)
    p, v = p.copy(), v.copy()
    cand = np.ones(300, np.uint8)
    cand[:7] = 0
    v[3], v[10:13, 1], p[13, 2], v[20:25], v[25] = np.nan, np.nan, np.inf, 0.0, [0.0, -0.0, 0.0]
    p[30:34, 0], v[30] = 100.0, 0.0
    inverse_map = np.array([0, 299, 40, -1, 300, 41, 1 << 40, 7], np.int64)
    got = check(v, p, candidate=cand, inverse_map=inverse_map, what="admission")
    assert got["summary"]["left_out"] == dict(candidate=7, nonfinite=4, zero_normal=7, frame=3, bins=0)
    assert got["summary"]["err"] == V.PLANES_BAD_INDEX and got["plane_full"].tolist() == [-1, 0, 0, -2, -2, 0, -2, 0]
    got = check(v, p, inverse_map=inverse_map[:3], what="no candidate mask")
    assert got["summary"]["left_out"]["candidate"] == 0 and got["summary"]["err"] == 0
    got = check(*join([plate(A, 520, 300)]), offset_bin=2.0 ** -18, dist_tol=2.0 ** -18, what="beyond the bins")
    assert got["summary"]["left_out"]["bins"] == 300
    check(np.zeros((0, 3), F32), np.zeros((0, 3), F32), what="no rows")
    check(np.zeros((0, 3), F32), np.zeros((0, 3), F32), inverse_map=np.zeros(3, np.int64), what="no rows, a map")


def test_permutation_and_repeat(scan):
    v, p, frame = scan
    n = 20000
    v, p = v[:n], p[:n]
    settings = dict(offset_bin=BIN, normal_deg=20.0, dist_tol=1.5 * BIN, min_voxels=200, max_planes=16)
    first = run_gpu(v, p, frame, settings)
    again = run_gpu(v, p, frame, settings)
    assert first["raw"].tobytes() == again["raw"].tobytes() and first["plane_qv"].tobytes() == again["plane_qv"].tobytes()
    order = np.random.default_rng(5).permutation(n)
    moved = run_gpu(v[order], p[order], frame, settings)
    assert moved["raw"].tobytes() == first["raw"].tobytes() and np.array_equal(moved["plane_qv"], first["plane_qv"][order])
    assert first["summary"]["n_planes"] >= 5


def test_wrapper_refusals():
    v, p = (_dev(x, F32) for x in join([plate(A, 520, 300)]))
    ok = dict(offset_bin=BIN, dist_tol=1.5 * BIN)
    for bad in (dict(positions=p[:5]), dict(normals=v.double()), dict(candidate=torch.ones(300, dtype=torch.int32, device=DEV)),
                dict(candidate=torch.ones(5, dtype=torch.uint8, device=DEV)), dict(bits=21), dict(origin=(0, np.nan, 0)),
                dict(quantum=0.3), dict(offset_bin=None), dict(dist_tol=None), dict(plane_qv=torch.zeros(5, dtype=torch.int32, device=DEV)),
                dict(plane_full=torch.zeros(5, dtype=torch.int32, device=DEV)), dict(out=torch.zeros(8, dtype=torch.uint8, device=DEV)),
                dict(table=torch.zeros((5, 3), dtype=torch.int32, device=DEV)), dict(workspace=torch.zeros(256, dtype=torch.uint8, device=DEV)),
                dict(inverse_map=torch.zeros(5, dtype=torch.int32, device=DEV)), dict(max_planes=17), dict(min_voxels=0)):
        kw = dict(dict(normals=v, positions=p, origin=ORIGIN, quantum=QUANTUM, **ok), **bad)
        with pytest.raises(ValueError):
            V.find_planes(**kw)
    # plane_full=False: the lift is not wanted although there is a map
    got = V.find_planes(v, p, ORIGIN, QUANTUM, inverse_map=torch.zeros(4, dtype=torch.int64, device=DEV), plane_full=False, **ok)
    assert got[1] is None and V.read_planes(got[2].cpu().numpy())[1]["n_planes"] == 1
