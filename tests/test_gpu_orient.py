"""-m gpu: normals oriented by propagation (a3d_orient_normals in csrc/session_orient.hip; view.orient_normals) against its
restatement ``orient_rule.py``, bit for bit, on normal_out_qv, flipped_qv, dist_qv, owner_qv, normal_full and the summary.

1  sizes at their edges (1, 2, 255, 256, 257 voxels; one full pass of the grid + 77 rows)
2  the line of 600: 64 sweeps are not enough, resumed until converged, the same bytes as one call of 1024 sweeps; seeded at one
   end it is a chain of 599 parents for the pointer jumping
3  the ring that cannot be oriented, the plates apart and joined, two batch samples that touch
4  connectivity 6 / 18 / 26, both seed modes, 0 / 1 / 40 seeds, seed flips; rows with zero, NaN and infinite normals; map
   entries out of range; components out of range
5  outputs omitted; two calls give the same bytes; the library's refusals leave every output untouched
6  with normals from a3d_estimate_normals: every voxel with an exactly planar neighbourhood points outward on the shells and on
   the cabinet, and into the room on the room
"""
import numpy as np
import pytest
import torch

import orient_cases as K
import orient_rule as R
from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.engine import Scene
from session_kit import DEV, _dev, byref, status

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -77
FILL = 0x5a
OUTPUTS = ("normal_out_qv", "flipped_qv", "dist_qv", "owner_qv", "normal_full")
RULE = dict(normal_out_qv="normal_out", flipped_qv="flipped", dist_qv="dist", owner_qv="owner", normal_full="normal_full")
INVALID, OK = -1, 0


def scene_of(coords4):
    return Scene(torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(DEV))


def orient_gpu(scene, normals, n_full=0, inverse_map=None, omit=(), workspace=None, sweeps=1024, resume=False, connectivity=26,
               **seeds):
    """view.orient_normals, numpy in / numpy out; every output starts as a sentinel."""
    n = scene.n[0]
    outs = dict(normal_out_qv=torch.full((n, 3), float(SENTINEL), dtype=torch.float32, device=DEV),
                flipped_qv=torch.full((n,), FILL, dtype=torch.uint8, device=DEV),
                dist_qv=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                owner_qv=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                normal_full=torch.full((n_full, 3), float(SENTINEL), dtype=torch.float32, device=DEV))
    given = {k: (False if k in omit else t) for k, t in outs.items()}
    summary = torch.full((V.ORIENT_SUMMARY.itemsize,), FILL, dtype=torch.uint8, device=DEV)
    kinds = dict(seed_qv=np.uint8, seed_flip=np.uint8, components=np.int32, positions=F32)
    dev = {k: (_dev(v, kinds[k]) if k in kinds else v) for k, v in seeds.items() if v is not None}
    got = V.orient_normals(scene, _dev(normals, F32), connectivity=connectivity, sweeps=sweeps, resume=resume,
                           inverse_map=None if inverse_map is None else _dev(inverse_map, np.int64), n_full=n_full, summary=summary,
                           workspace=workspace, **dev, **given)
    for k, t in zip(OUTPUTS, got[:5]):
        assert t is (None if k in omit else outs[k])
    raw = summary.cpu().numpy()
    res = {k: t.cpu().numpy() for k, t in outs.items()}
    res.update(summary=V.read_orient_summary(raw), raw=raw, workspace=got[6])
    return res


def same(got, want, what=None, omit=()):
    for k in OUTPUTS:
        if k in omit:
            assert (got[k] == (FILL if k == "flipped_qv" else SENTINEL)).all(), (what, k)
        else:
            w = want[RULE[k]]
            assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k)
            a, b = (got[k].view(np.uint32), w.view(np.uint32)) if w.dtype == F32 else (got[k], w)
            assert np.array_equal(a, b), (what, k, int((a != b).sum()))
    assert got["summary"] == want["summary"], (what, got["summary"], want["summary"])


def check(coords4, scene, normals, what=None, **kw):
    """One call against the rule; returns (got, want)."""
    got = orient_gpu(scene, normals, **kw)
    rule = {k: v for k, v in kw.items() if k not in ("omit", "workspace", "sweeps", "resume")}
    want = R.orient_all(coords4, normals, **rule)
    same(got, want, what, kw.get("omit", ()))
    return got, want


def marks(n, rows):
    m = np.zeros(n, np.uint8)
    m[list(rows)] = 1
    return m


def blob(m, seed):
    """m random voxels of a small box, about half of it: loops, corners, dead ends, a few pieces."""
    rng = np.random.default_rng(seed)
    side = max(2, int(round((2.0 * m) ** (1 / 3))))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    keep = cells[rng.permutation(len(cells))[:m]]
    return np.concatenate([np.zeros((m, 1), np.int64), keep], 1).astype(np.int32)


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_sizes_at_their_edges(m):
    coords = blob(m, seed=m)
    assert len(coords) == m
    sc = scene_of(coords)
    nrm = unit_normals(m, m + 1)
    seeds = marks(m, {0, m - 1, m // 2})
    for c in (6, 26):
        check(coords, sc, nrm, (m, c), seed_qv=seeds, n_full=m, connectivity=c)
    got, _ = check(coords, sc, nrm, seed_qv=seeds, n_full=m + 1)       # one vertex more than there are rows
    assert got["summary"]["err"] == R.BAD_INDEX and not got["normal_full"][m].any()
    check(coords, sc, nrm, components=np.zeros(m, np.int32), positions=K.centres(coords), viewpoint=(0.3, -5.0, 9.0))


def lines_of_five(coords4, normals, seed_qv, seed_flip):
    """The rule in CLOSED FORM for voxels (x in 0..4, y, z) whose lines along x never touch: dict as ``orient_rule.orient_all``
    without the lift.  Along a line the only neighbours are slots 12 (x - 1) and 14 (x + 1): the distance to a seed at q is
    the sum of w between, the parent lies towards the owner, the parity is the XOR of the flips between and the seed's.
    Vectorised over the lines (fp32 numpy arithmetic rounds every operation on its own)."""
    n = len(coords4)
    _, lid = np.unique(coords4[:, 2:4], axis=0, return_inverse=True)
    lid = lid.reshape(-1)
    row = np.full((lid.max() + 1, 5), -1, np.int64)
    row[lid, coords4[:, 1]] = np.arange(n)
    there = row >= 0
    nrm = np.asarray(normals, F32)[np.where(there, row, 0)]
    ok = there & np.isfinite(nrm).all(2) & (nrm != 0).any(2)
    a, b = nrm[:, :-1], nrm[:, 1:]
    dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    w = 1 + np.floor(F32(1023.0) * np.maximum(F32(1.0) - np.abs(dot), F32(0.0))).astype(np.int64)
    link = ok[:, :-1] & ok[:, 1:]
    flip = (dot < 0) & link
    cw = np.concatenate([np.zeros((len(w), 1), np.int64), np.cumsum(w, 1)], 1)
    cf = np.concatenate([np.zeros((len(w), 1), np.int64), np.cumsum(flip, 1)], 1)
    seed = ok & (np.asarray(seed_qv)[np.where(there, row, 0)] != 0)
    sflip = seed & (np.asarray(seed_flip)[np.where(there, row, 0)] != 0)
    none = 1 << 40
    best_d, best_s, best_p = np.full(row.shape, none), np.full(row.shape, none), np.zeros(row.shape, np.int64)
    for p in range(5):
        for q in range(5):
            lo, hi = min(p, q), max(p, q)
            open_way = seed[:, q] & ok[:, p] & (link[:, lo:hi].all(1) if hi > lo else True)
            d = cw[:, hi] - cw[:, lo]
            better = open_way & ((d < best_d[:, p]) | ((d == best_d[:, p]) & (row[:, q] < best_s[:, p])))
            best_d[better, p], best_s[better, p] = d[better], row[better, q]
            best_p[better, p] = ((cf[:, hi] - cf[:, lo]) & 1)[better] ^ sflip[better, q]
    dist, owner, parity = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    hit = best_d < none
    dist[row[hit]], owner[row[hit]], parity[row[hit]] = best_d[hit], best_s[hit], best_p[hit]
    bits = np.ascontiguousarray(normals, F32).view(np.uint32).copy()
    bits[parity == 1] ^= np.uint32(0x80000000)
    par_line = np.zeros(row.shape, np.int64)
    par_line[there] = parity[row[there]]
    conflicts = int((link & (np.where(par_line[:, :-1] ^ par_line[:, 1:], -dot, dot) < 0)).sum())
    okr = np.zeros(n, bool)
    okr[row[there]] = ok[there]
    summary = dict(admitted=int(okr.sum()), seeds=int(seed.sum()), reached=int(hit.sum()), unreached=int(okr.sum() - hit.sum()),
                   flipped=int(parity.sum()), conflicts=conflicts, max_dist=int(dist.max(initial=0)), converged=1, err=0)
    return dict(normal_out=bits.view(F32), flipped=parity, dist=dist, owner=owner, summary=summary)


def test_one_full_grid_pass_and_77_rows():
    """2048 workgroups x 256 rows is one pass of the grid: 524 365 voxels take a second pass of 77 rows.  Lines of five voxels,
    two apart in y and z (never neighbours), the last one cut short.  The rule is evaluated in closed form here
    (``lines_of_five``), which is first held to ``orient_rule.py`` on the first 3 000 voxels."""
    m = 2048 * 256 + 77
    side = 324
    yz = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 1, 2) * 2
    pts = np.concatenate([np.broadcast_to(np.arange(5).reshape(1, 5, 1), (side * side, 5, 1)), np.broadcast_to(yz, (side * side, 5, 2))], 2)
    rng = np.random.default_rng(3)
    ordered = np.concatenate([np.zeros((m, 1), np.int64), pts.reshape(-1, 3)[:m]], 1).astype(np.int32)
    nrm = K.random_signs(m, seed=5, tilt=0.4)
    nrm[rng.random(m) < 0.05] = 0
    seeds = (rng.random(m) < 0.15).astype(np.uint8)
    flips = (rng.random(m) < 0.5).astype(np.uint8)
    few = np.random.default_rng(4).permutation(3000)
    closed = lines_of_five(ordered[:3000][few], nrm[:3000][few], seeds[:3000][few], flips[:3000][few])
    rule = R.orient_numpy(ordered[:3000][few], nrm[:3000][few], 6, seed_qv=seeds[:3000][few], seed_flip=flips[:3000][few])
    for k in ("normal_out", "flipped", "dist", "owner"):
        assert np.array_equal(closed[k].view(np.uint32) if k == "normal_out" else closed[k],
                              rule[k].view(np.uint32) if k == "normal_out" else rule[k]), k
    assert closed["summary"] == rule["summary"] and rule["summary"]["flipped"] > 300 and rule["summary"]["unreached"] > 100
    perm = rng.permutation(m)
    coords, nrm, seeds, flips = ordered[perm], nrm[perm], seeds[perm], flips[perm]
    sc = scene_of(coords)
    assert sc.n[0] == m
    inv = rng.integers(0, m, 300_000)                                  # more vertices than one pass of the finish's grid
    want = lines_of_five(coords, nrm, seeds, flips)
    want["normal_full"], _ = R.lift_numpy(want["normal_out"], len(inv), inv)
    assert want["summary"]["flipped"] > 100_000 and want["summary"]["conflicts"] > 1000
    for c in (6, 26):                                                  # under 26 the lines are still apart
        same(orient_gpu(sc, nrm, seed_qv=seeds, seed_flip=flips, inverse_map=inv, n_full=len(inv), sweeps=8, connectivity=c), want, c)


# ---------------------------------------------------------------------------------------------------- 2
def test_line_of_600_resumed_and_the_chain_of_599_parents():
    coords, at = K.line(600, seed=9)
    sc = scene_of(coords)
    nrm = K.random_signs(600, seed=10)
    seeds = marks(600, {at[0]})
    whole, want = check(coords, sc, nrm, seed_qv=seeds, n_full=600, connectivity=6, sweeps=1024)
    assert whole["summary"]["reached"] == 600 and whole["summary"]["conflicts"] == 0 and 200 < whole["summary"]["flipped"] < 400
    assert (np.sign(whole["normal_out_qv"][:, 2]) == np.sign(nrm[at[0], 2])).all()
    assert np.array_equal(np.argsort(whole["dist_qv"][at]), np.arange(600))     # 599 parents in a row
    part = orient_gpu(sc, nrm, seed_qv=seeds, n_full=600, connectivity=6, sweeps=64)
    assert part["summary"]["converged"] == 0 and part["summary"]["reached"] < 600
    calls = 1
    while part["summary"]["converged"] == 0:
        part = orient_gpu(sc, nrm, seed_qv=seeds, n_full=600, connectivity=6, sweeps=64, resume=True, workspace=part["workspace"])
        calls += 1
        assert calls <= 12
    assert calls >= 9                                                   # 599 edges at 64 sweeps a call
    same(part, want, "resumed")
    again = orient_gpu(sc, nrm, seed_qv=seeds, n_full=600, connectivity=6, sweeps=7, resume=True, workspace=part["workspace"])
    same(again, want, "resumed at the fixed point")


# ---------------------------------------------------------------------------------------------------- 3
def test_ring():
    coords, nrm, at = K.ring()
    sc = scene_of(coords)
    for c in (6, 18, 26):
        got, want = check(coords, sc, nrm, c, seed_qv=marks(40, {at[0]}), n_full=40, connectivity=c)
        assert got["summary"]["conflicts"] >= 1 and got["summary"]["reached"] == 40
    got, _ = check(coords, sc, nrm, seed_qv=marks(40, {at[0], at[20]}), connectivity=6)   # two seeds: their regions meet
    assert set(got["owner_qv"].tolist()) == {at[0], at[20]}


@pytest.mark.parametrize("joined", [False, True])
def test_plates(joined):
    coords = K.plates(7, joined)
    n = len(coords)
    sc = scene_of(coords)
    nrm = K.random_signs(n, seed=6)
    low = int(np.flatnonzero((coords[:, 1:] == (3, 3, 0)).all(1))[0])
    for c in (6, 18, 26):
        got, _ = check(coords, sc, nrm, (joined, c), seed_qv=marks(n, {low}), n_full=n, connectivity=c)
        upper = coords[:, 3] == 2
        assert (got["dist_qv"][upper] >= 0).all() == joined and got["summary"]["unreached"] == (0 if joined else 49)
        assert np.array_equal(got["normal_out_qv"][upper & (got["dist_qv"] < 0)], nrm[upper & (got["dist_qv"] < 0)])


def test_touching_batch_samples():
    coords = K.touching_samples()
    n = len(coords)
    sc = scene_of(coords)
    nrm = K.random_signs(n, seed=7)
    first = int(np.flatnonzero(coords[:, 0] == 0)[0])
    got, _ = check(coords, sc, nrm, seed_qv=marks(n, {first}), n_full=n)
    assert np.array_equal(got["dist_qv"] >= 0, coords[:, 0] == 0)      # never across batch samples
    comp = coords[:, 0].astype(np.int32) * 3                            # components named 0 and 3
    got, _ = check(coords, sc, nrm, components=comp, positions=K.centres(coords), viewpoint=(5.0, 2.0, 4.0))
    assert got["summary"]["seeds"] == 2 and got["summary"]["reached"] == n


# ---------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("conn", [6, 18, 26])
def test_connectivities_seed_counts_and_bad_rows(conn):
    coords = K.shell(7, seed=conn)
    n = len(coords)
    sc = scene_of(coords)
    rng = np.random.default_rng(conn)
    nrm = unit_normals(n, conn)
    bad = rng.permutation(n)[:30]
    nrm[bad[:10]] = 0
    nrm[bad[10:14]] = [0, -0.0, 0]
    nrm[bad[14:22], rng.integers(0, 3, 8)] = np.nan
    nrm[bad[22:30], rng.integers(0, 3, 8)] = [np.inf, -np.inf] * 4
    for k in (0, 1, 40):
        rows = rng.permutation(n)[:k]
        flips = (rng.random(n) < 0.5).astype(np.uint8)
        got, want = check(coords, sc, nrm, (conn, k), seed_qv=marks(n, rows), seed_flip=flips, n_full=n, connectivity=conn)
        assert got["summary"]["admitted"] == n - 30 and (got["dist_qv"][bad] == -1).all()
        assert got["summary"]["seeds"] == int(R.admitted(nrm)[rows].sum()) and (k == 0) == (got["summary"]["reached"] == 0)
    comp = rng.integers(-1, 4, n).astype(np.int32)
    comp[rng.permutation(n)[:5]] = n + 3                                # components no row can name
    inv = rng.integers(-2, n + 2, 500)                                  # map entries out of range
    got, _ = check(coords, sc, nrm, components=comp, positions=K.centres(coords) * F32(0.5), viewpoint=(9.0, 1.5, -2.0),
                   inverse_map=inv, n_full=500, connectivity=conn)
    assert got["summary"]["err"] == R.BAD_INDEX | R.BAD_COMPONENT and got["summary"]["seeds"] == 4


# ---------------------------------------------------------------------------------------------------- 5
def test_outputs_omitted_and_twice_the_same_bytes():
    coords = K.shell(6)
    n = len(coords)
    sc = scene_of(coords)
    nrm = unit_normals(n, 8)
    kw = dict(seed_qv=marks(n, {3, 70}), n_full=n + 2, inverse_map=np.arange(n + 2) % (n + 1))
    first, want = check(coords, sc, nrm, **kw)
    second = orient_gpu(sc, nrm, workspace=first["workspace"], **kw)    # the used workspace, not cleared by the caller
    for k in OUTPUTS + ("raw",):
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k
    for k in OUTPUTS:
        same(orient_gpu(sc, nrm, omit=(k,), **kw), want, k, omit=(k,))
    same(orient_gpu(sc, nrm, omit=OUTPUTS, **kw), want, "all", omit=OUTPUTS)


def test_refusals_leave_the_outputs_untouched():
    coords = K.shell(5)
    n = len(coords)
    sc = scene_of(coords)
    ws = V.orient_workspace(n, DEV)
    nrm, seeds = _dev(unit_normals(n, 1), F32), _dev(marks(n, {0}), np.uint8)
    pos, comp = _dev(K.centres(coords), F32), torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.full((n, 3), float(SENTINEL), dtype=torch.float32, device=DEV)
    summary = torch.full((64,), FILL, dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = L.OrientNormalsArgs()
        a.scene, a.n = getattr(sc.handle, "value", sc.handle), n
        a.normal_qv_dev, a.seed_qv_dev, a.normal_out_qv_dev = nrm.data_ptr(), seeds.data_ptr(), out.data_ptr()
        a.summary_dev, a.workspace_dev, a.workspace_bytes = summary.data_ptr(), ws.data_ptr(), ws.shape[0]
        a.connectivity, a.sweeps, a.mode = 26, 16, L.A3D_ORIENT_GIVEN
        for k, v in kw.items():
            if k == "viewpoint":
                a.viewpoint[:] = v
            else:
                setattr(a, k, v)
        return a

    nearest = dict(mode=L.A3D_ORIENT_NEAREST, component_qv_dev=comp.data_ptr(), position_qv_dev=pos.data_ptr())
    assert status("a3d_orient_normals", None, None) == INVALID
    bad = [dict(scene=None), dict(n=n + 1), dict(connectivity=7), dict(sweeps=0), dict(sweeps=4097), dict(seed_qv_dev=None),
           dict(mode=2), dict(resume=2), dict(normal_qv_dev=None), dict(summary_dev=None), dict(normal_out_qv_dev=nrm.data_ptr()),
           dict(workspace_dev=None), dict(workspace_bytes=ws.shape[0] - 1), dict(workspace_dev=ws.data_ptr() + 128),
           dict(n_full=-1), dict(nearest, component_qv_dev=None), dict(nearest, position_qv_dev=None),
           dict(nearest, viewpoint=[0.0, float("nan"), 0.0]), dict(nearest, viewpoint=[float("inf"), 0.0, 0.0])]
    for kw in bad:
        assert status("a3d_orient_normals", byref(args(**kw)), L.stream(torch.device(DEV))) == INVALID, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all() and (summary.cpu().numpy() == FILL).all()
    assert status("a3d_orient_normals", byref(args(**nearest)), L.stream(torch.device(DEV))) == OK
    assert status("a3d_orient_normals", byref(args()), L.stream(torch.device(DEV))) == OK
    assert V.read_orient_summary(summary.cpu().numpy())["reached"] == n
    with pytest.raises(ValueError):
        V.orient_normals(sc, nrm, seed_qv=seeds, normal_out_qv=nrm)
    with pytest.raises(ValueError):
        V.orient_normals(sc, nrm, seed_qv=seeds, resume=True)
    with pytest.raises(ValueError):
        V.orient_normals(sc, nrm, seed_qv=seeds, workspace=ws[:-256])


# ---------------------------------------------------------------------------------------------------- 6
def estimated(coords, viewpoint):
    """(scene, normals fp32 [n, 3] of a3d_estimate_normals with one vertex per voxel centre, turned towards ``viewpoint``)."""
    sc = scene_of(coords)
    xyz = _dev(K.centres(coords), F32)
    origin = K.centres(coords).astype(np.float64).mean(0).round()
    nrm = V.estimate_normals(sc, xyz, origin, 2.0 ** -10, 20, viewpoint=viewpoint, variation_qv=False, count_qv=False,
                             moments_qv=False, normal_full=False)[0]
    return sc, nrm.cpu().numpy()


def wrong(coords, normals, planar, centre, outward):
    side = ((K.centres(coords).astype(np.float64) - centre) * normals).sum(1)
    return int((planar & ((side < 0) if outward else (side > 0))).sum())


@pytest.fixture(scope="module")
def planar_of():
    memo = {}

    def get(name, coords):
        if name not in memo:
            memo[name] = R.pca_normals(coords)[1]
        return memo[name]
    return get


def test_estimated_normals_on_the_shell_point_outward(planar_of):
    coords = K.shell(12, seed=12)
    vp = np.array([40.0, 3.0, 5.0])
    sc, nrm = estimated(coords, vp)
    planar = planar_of("shell", coords)
    centre = np.full(3, 5.5)
    assert planar.sum() == 384 and wrong(coords, nrm, planar, centre, True) > 100           # the viewpoint sign alone
    got, _ = check(coords, sc, nrm, components=np.zeros(len(coords), np.int32), positions=K.centres(coords), viewpoint=vp)
    assert got["summary"]["reached"] == got["summary"]["admitted"] and got["summary"]["seeds"] == 1
    assert wrong(coords, got["normal_out_qv"], planar, centre, True) == 0


def test_estimated_normals_on_the_room_with_the_cabinet(planar_of):
    coords, cab = K.room_with_cabinet()
    centre = np.full(3, 14.5)
    sc, nrm = estimated(coords, centre)
    planar = planar_of("room", coords)
    cab_centre = (K.CABINET_LO + K.CABINET_HI) / 2
    assert wrong(coords[cab], nrm[cab], planar[cab], cab_centre, True) > 10                  # the viewpoint sign alone
    got, _ = check(coords, sc, nrm, components=np.zeros(len(coords), np.int32), positions=K.centres(coords), viewpoint=centre)
    out = got["normal_out_qv"]
    assert wrong(coords[cab], out[cab], planar[cab], cab_centre, True) == 0
    assert wrong(coords[~cab], out[~cab], planar[~cab], centre, False) == 0
