"""-m gpu: normals for point clouds -- a3d_estimate_normals and a3d_cull_points (csrc/session_normals.hip) and
a3d_render_shade_lit_points (csrc/session.hip), through view.py, against their restatements ``normals_rule.py`` and
``shade_points_rule.py``, bit for bit: the integer outputs (moments_qv, count_qv, the summary) by equality, the fp32 normals
and the variation by their bytes.

1  sizes at their edges (1, 2, 255, 256, 257 voxels; the identity map); one full pass of both grids + 77 (262 221 voxels,
   266 000 vertices: mostly lone vertices, 400 voxels with a surface of their own, the last 77 rows among them)
2  geometry: voxels holding 1 and 300 vertices; an 8 x 8 x 1 plate at multiples of the quantum (exactly (0, 0, +-1)); two
   plates meeting in a crease; the shell of a 6^3 cube with the viewpoint inside, outside and absent; a 40-voxel line (no
   normal anywhere); two batch samples whose coordinates touch
3  input edges: inverse-map entries out of range, NaN / infinite / out-of-range coordinates
4  every output omitted in turn; two calls give the same bytes, and so does a permutation of the vertices; the refusals
5  the lit pass at 37 x 29, 16 x 16 and 1 x 1, zero and NaN normals, ambient = 1, ids out of range
6  the cull bit for bit, its always-shown cases, and a closed box seen from outside: the culled render is the render of the
   cloud with the culled vertices deleted
"""
import numpy as np
import pytest
import torch

import normals_rule as R
import shade_points_rule as SP
from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.engine import Scene
from render_rule import render_points_rule
from session_kit import DEV, _dev, byref, camera_of, f32_pointer, status

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL, FILL = -77, 0x5a
OUTPUTS = ("normal_qv", "variation_qv", "count_qv", "moments_qv", "normal_full")
INVALID, OK = -1, 0


# ---------------------------------------------------------------------------------------------------- the adaptors
def scene_of(coords4):
    return Scene(torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(DEV))


def frame_of(xyz, bits=20):
    """(origin, quantum, bits) as the session derives them: the centre of the finite box, 2^e >= the half extent."""
    p = np.asarray(xyz, np.float64)
    p = p[np.isfinite(p).all(1)]
    lo, hi = p.min(0), p.max(0)
    origin = 0.5 * (lo + hi)
    half = float(np.maximum(hi - origin, origin - lo).max())
    e = int(np.ceil(np.log2(half))) if half > 0 else 0
    while 2.0 ** e < half:
        e += 1
    return origin, 2.0 ** (e - bits), bits


def normals_gpu(scene, xyz, inverse_map, origin, quantum, bits, viewpoint=None, omit=(), workspace=None):
    """view.estimate_normals, numpy in / numpy out; every output starts as a sentinel."""
    n, n_full = scene.n[0], len(xyz)
    outs = dict(normal_qv=torch.full((n, 3), float(SENTINEL), dtype=torch.float32, device=DEV),
                variation_qv=torch.full((n,), float(SENTINEL), dtype=torch.float32, device=DEV),
                count_qv=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                moments_qv=torch.full((n, 10), SENTINEL, dtype=torch.int64, device=DEV),
                normal_full=torch.full((n_full, 3), float(SENTINEL), dtype=torch.float32, device=DEV))
    given = {k: (False if k in omit else t) for k, t in outs.items()}
    summary = torch.full((V.NORMALS_SUMMARY.itemsize,), FILL, dtype=torch.uint8, device=DEV)
    got = V.estimate_normals(scene, _dev(np.asarray(xyz, F32).reshape(-1, 3), F32), origin, quantum, bits,
                             None if inverse_map is None else _dev(inverse_map, np.int64), viewpoint, summary=summary,
                             workspace=workspace, **given)
    for k, t in zip(OUTPUTS, got[:5]):
        assert t is (None if k in omit else outs[k])
    assert got[5] is summary
    res = {k: t.cpu().numpy() for k, t in outs.items()}
    res.update(summary=V.read_normals_summary(summary.cpu().numpy()), workspace=got[6])
    return res


def same(got, want, what=None, omit=()):
    for k in OUTPUTS:
        if k in omit:
            assert (got[k] == SENTINEL).all(), (what, k)
        else:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            if got[k].tobytes() != want[k].tobytes():
                bad = np.flatnonzero((got[k].reshape(len(got[k]), -1).view(np.uint8) != want[k].reshape(len(want[k]), -1).view(np.uint8)).any(1))
                raise AssertionError((what, k, len(bad), bad[:5], got[k][bad[:3]], want[k][bad[:3]]))
    assert got["summary"] == want["summary"], (what, got["summary"], want["summary"])


def check(coords4, scene, xyz, inverse_map, frame=None, viewpoint=None, what=None, rule=R.estimate, **kw):
    origin, quantum, bits = frame_of(xyz) if frame is None else frame
    got = normals_gpu(scene, xyz, inverse_map, origin, quantum, bits, viewpoint, **kw)
    want = rule(coords4, xyz, inverse_map, origin, quantum, bits, viewpoint)
    same(got, want, what, kw.get("omit", ()))
    return got, want


def cloud(coords4, per_voxel, seed=0, lo=0.0, hi=1.0):
    """(xyz fp32, inverse_map): ``per_voxel`` (an int or one per row) random vertices inside each unit voxel, shuffled."""
    rng = np.random.default_rng(seed)
    c = np.asarray(coords4, np.int64)
    inv = np.repeat(np.arange(len(c)), per_voxel)
    inv = inv[rng.permutation(len(inv))]
    return (c[inv, 1:] + rng.uniform(lo, hi, (len(inv), 3))).astype(F32), inv


def render_ids(xyz, radius, cam):
    """The id image of a3d_render_points on the device (the pair capacity sufficed)."""
    ids, _, header = V.render_points(_dev(xyz, F32), radius, cam)
    assert V.read_render_header(header.cpu().numpy())[0] == 0
    return ids


def cells(points, batch=0, seed=0):
    c = np.unique(np.asarray(points, np.int64).reshape(-1, 3), axis=0)
    coords = np.concatenate([np.full((len(c), 1), batch, np.int64), c], 1).astype(np.int32)
    return coords[np.random.default_rng(seed).permutation(len(coords))]


def plate(nx, ny, z=0):
    return cells([[x, y, z] for x in range(nx) for y in range(ny)])


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_sizes_at_their_edges(m):
    coords = cells([[x, x // 7, 3] for x in range(m)], seed=m)
    sc = scene_of(coords)
    xyz, inv = cloud(coords, 4, seed=m)
    got, _ = check(coords, sc, xyz, inv, what=m)
    assert got["summary"]["counted"] == 4 * m and got["summary"]["err"] == 0
    assert got["summary"]["valid"] == m                                 # 4 random vertices: never a line
    for vp in (None, (3.0, -2.0, 50.0)):                                # the identity map: one vertex per voxel, n_full = n
        check(coords, sc, xyz[np.argsort(inv, kind="stable")][::4], None, viewpoint=vp, what=(m, "identity"))


def test_one_full_pass_of_both_grids_and_77():
    """1024 workgroups x 256 voxels is one pass of stage B's grid, 256 x 1024 vertices one pass of stage A's and the lift's:
    262 221 voxels and 266 000 vertices take a second pass.  Voxels two apart (never neighbours), a lone vertex in most --
    no normal -- and five more in 400 of them, the last 77 rows included."""
    m = 1024 * 256 + 77
    side = 64
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side + 1), indexing="ij"), -1).reshape(-1, 3)[:m] * 2
    rng = np.random.default_rng(11)
    coords = np.concatenate([np.zeros((m, 1), np.int64), g], 1).astype(np.int32)[rng.permutation(m)]
    rich = np.unique(np.concatenate([rng.integers(0, m, 323), np.arange(m - 77, m)]))
    per = np.ones(m, np.int64)
    per[rich] = 6
    xyz, inv = cloud(coords, per, seed=12)
    extra = 266_000 - len(xyz)
    assert extra > 0
    inv = np.concatenate([inv, rng.integers(0, m, extra)])               # (and second lone-ish vertices elsewhere)
    xyz = np.concatenate([xyz, (coords[inv[-extra:], 1:] + rng.uniform(0, 1, (extra, 3))).astype(F32)])
    sc = scene_of(coords)
    assert sc.n[0] == m
    got, want = check(coords, sc, xyz, inv, viewpoint=(64.0, 64.0, 300.0), rule=R.estimate_large)
    assert want["summary"]["counted"] == 266_000 and want["summary"]["valid"] >= len(rich) and want["summary"]["invalid"] > 250_000
    assert (np.abs(got["normal_qv"][rich]).sum(1) > 0.9).all() and (got["count_qv"][rich] >= 6).all()


# ---------------------------------------------------------------------------------------------------- 2
def test_voxels_holding_1_and_300_vertices():
    coords = plate(3, 3)
    per = np.ones(9, np.int64)
    per[(coords[:, 1:] == (1, 1, 0)).all(1)] = 300                    # the centre: in every voxel's neighbourhood
    xyz, inv = cloud(coords, per, seed=2)
    got, _ = check(coords, scene_of(coords), xyz, inv)
    assert sorted(got["moments_qv"][:, 0].tolist()) == [1] * 8 + [300] and (got["count_qv"] >= 302).all()


def test_plate_at_multiples_of_the_quantum_is_exact():
    coords = plate(8, 8)
    rng = np.random.default_rng(4)
    inv = rng.permutation(np.repeat(np.arange(64), 5))
    frame = (np.array([4.0, 4.0, 0.0]), 2.0 ** -17, 20)
    xy = coords[inv, 1:3] + np.rint(rng.uniform(0, 1, (len(inv), 2)) * 2.0 ** 17) / 2.0 ** 17
    for z, vp, sign in ((0.25, None, 1.0), (0.25, (4.0, 4.0, 9.0), 1.0), (0.25, (4.0, 4.0, -9.0), -1.0), (-0.5, None, 1.0)):
        xyz = np.c_[xy, np.full(len(inv), z)].astype(F32)
        got, _ = check(coords, scene_of(coords), xyz, inv, frame=frame, viewpoint=vp, what=(z, vp))
        assert (got["normal_qv"] == np.array([0.0, 0.0, sign], F32)).all() and (got["variation_qv"] == 0).all()
        assert (got["normal_full"] == np.array([0.0, 0.0, sign], F32)).all() and got["summary"]["valid"] == 64


def test_two_plates_meeting_in_a_crease():
    coords = cells([[x, y, 0] for x in range(8) for y in range(8)] + [[0, y, z] for y in range(8) for z in range(8)])
    xyz, inv = cloud(coords, 6, seed=5)
    # the floor's vertices lie in the plane z = 0.5, the wall's in x = 0.5; those of the crease's voxels alternate
    on_wall = (coords[inv, 3] > 0) | ((coords[inv, 1] == 0) & (np.arange(len(inv)) % 2 == 1))
    xyz[on_wall, 0], xyz[~on_wall, 2] = 0.5, 0.5
    got, _ = check(coords, scene_of(coords), xyz, inv, viewpoint=(4.0, 4.0, 4.0))
    far_floor = (coords[:, 3] == 0) & (coords[:, 1] >= 3)
    far_wall = (coords[:, 1] == 0) & (coords[:, 3] >= 3)
    assert np.abs(got["normal_qv"][far_floor] - [0, 0, 1]).max() < 1e-6 and np.abs(got["normal_qv"][far_wall] - [1, 0, 0]).max() < 1e-6
    crease = (coords[:, 1] == 0) & (coords[:, 3] == 0)
    assert (np.abs(got["normal_qv"][crease][:, [0, 2]]).min(1) > 0.2).all() and (got["variation_qv"][crease] > 0.01).all()


@pytest.fixture(scope="module")
def shell():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    coords = cells(g[((g == 0) | (g == 5)).any(1)], seed=6)
    assert len(coords) == 152
    xyz, inv = cloud(coords, 5, seed=6, lo=0.3, hi=0.7)
    return coords, scene_of(coords), xyz, inv


@pytest.mark.parametrize("viewpoint", ["inside", "outside", None])
def test_shell_of_a_cube(shell, viewpoint):
    coords, sc, xyz, inv = shell
    vp = {"inside": (3.0, 3.0, 3.0), "outside": (40.0, 3.0, 3.0), None: None}[viewpoint]
    got, _ = check(coords, sc, xyz, inv, viewpoint=vp, what=viewpoint)
    n = got["normal_qv"]
    assert got["summary"]["valid"] == 152 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    centre = coords[:, 1:] + 0.5
    if viewpoint == "inside":
        assert ((n * (3.0 - centre)).sum(1) > 0).all()                  # every normal looks into the room
    elif viewpoint == "outside":
        face = (coords[:, 1:] == 5).sum(1) + (coords[:, 1:] == 0).sum(1) == 1
        assert (n[face & (coords[:, 1] == 5)][:, 0] > 0.9).all() and (n[face & (coords[:, 1] == 0)][:, 0] > 0.9).all()
    else:
        assert (n[np.arange(152), np.abs(n).argmax(1)] > 0).all()        # the canonical sign


def test_a_line_has_no_normal():
    coords = cells([[x, 2, -1] for x in range(40)])
    xyz = (coords[:, 1:] + 0.5).astype(F32)                               # one vertex at every voxel's centre: the identity map
    got, _ = check(coords, scene_of(coords), xyz, None, viewpoint=(0.0, 0.0, 9.0))
    assert got["summary"] == dict(counted=40, valid=0, invalid=40, err=0) and not got["normal_qv"].any() and not got["variation_qv"].any()
    assert sorted(got["count_qv"].tolist()) == [2, 2] + [3] * 38


def test_two_batch_samples_that_touch_do_not_bleed():
    a, b = plate(5, 5, z=0), plate(5, 5, z=1)
    b[:, 0] = 1
    coords = np.concatenate([a, b])                                      # (a sample's rows are contiguous; each is shuffled within)
    xyz, inv = cloud(coords, 4, seed=8)
    got, want = check(coords, scene_of(coords), xyz, inv)
    # 4 vertices a voxel: a corner voxel of a 5 x 5 plate sees 4 voxels of ITS sample, an inner one 9; never 18
    assert set(got["count_qv"].tolist()) == {16, 24, 36}
    alone = R.estimate(coords[coords[:, 0] == 0], xyz[coords[inv, 0] == 0], np.cumsum(coords[:, 0] == 0)[inv[coords[inv, 0] == 0]] - 1,
                       *frame_of(xyz))
    assert alone["normal_qv"].tobytes() == got["normal_qv"][coords[:, 0] == 0].tobytes()


# ---------------------------------------------------------------------------------------------------- 3
def test_input_edges():
    coords = plate(6, 5)
    n = len(coords)
    xyz, inv = cloud(coords, 5, seed=9)
    sc = scene_of(coords)
    inv2 = inv.copy()
    inv2[[0, 7, 20, 33]] = [-1, n, 1 << 40, -(1 << 40)]
    got, _ = check(coords, sc, xyz, inv2, frame=frame_of(xyz))
    assert got["summary"]["err"] == R.BAD_INDEX and got["summary"]["counted"] == len(xyz) - 4 and not got["normal_full"][[0, 7, 20, 33]].any()
    xyz2 = xyz.copy()
    xyz2[3, 0], xyz2[11, 1], xyz2[12, 2], xyz2[40] = np.nan, np.inf, -np.inf, (1e30, 0, 0)
    got, _ = check(coords, sc, xyz2, inv, frame=frame_of(xyz))
    assert got["summary"]["err"] == R.RANGE and got["summary"]["counted"] == len(xyz) - 4
    got, _ = check(coords, sc, xyz2, inv2, frame=frame_of(xyz))
    assert got["summary"]["err"] == R.RANGE | R.BAD_INDEX
    # a frame too narrow for the scene: |X| <= 2^bits cuts vertices away, exactly as the rule says
    origin, quantum, _ = frame_of(xyz)
    for bits in (0, 3, 9):
        got, _ = check(coords, sc, xyz, inv, frame=(origin, quantum * 2.0 ** 11, bits), what=bits)
        assert got["summary"]["err"] == (R.RANGE if bits < 9 else 0)


# ---------------------------------------------------------------------------------------------------- 4
def test_outputs_omitted_same_bytes_and_permutations(shell):
    coords, sc, xyz, inv = shell
    frame = frame_of(xyz)
    full, want = check(coords, sc, xyz, inv, frame=frame, viewpoint=(3.0, 3.0, 3.0))
    for k in OUTPUTS:
        got = normals_gpu(sc, xyz, inv, *frame, (3.0, 3.0, 3.0), omit=(k,), workspace=full["workspace"])
        same(got, want, k, omit=(k,))
    same(normals_gpu(sc, xyz, inv, *frame, (3.0, 3.0, 3.0), omit=OUTPUTS), want, "all", omit=OUTPUTS)
    again = normals_gpu(sc, xyz, inv, *frame, (3.0, 3.0, 3.0), workspace=full["workspace"])
    for k in OUTPUTS:
        assert again[k].tobytes() == full[k].tobytes()
    perm = np.random.default_rng(1).permutation(len(xyz))
    shuffled = normals_gpu(sc, xyz[perm], inv[perm], *frame, (3.0, 3.0, 3.0))
    for k in OUTPUTS[:4]:
        assert shuffled[k].tobytes() == full[k].tobytes()
    assert shuffled["normal_full"].tobytes() == full["normal_full"][perm].tobytes()


def test_refusals(shell):
    coords, sc, xyz, inv = shell
    n, n_full = len(coords), len(xyz)
    x, iv = _dev(xyz, F32), _dev(inv, np.int64)
    origin, quantum, bits = frame_of(xyz)
    ws = V.normals_workspace(n, DEV)
    good = dict(scene=sc, xyz=x, origin=origin, quantum=quantum, bits=bits, inverse_map=iv)
    assert len(V.estimate_normals(**good)) == 7
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
    for bad in (dict(xyz=x[:, :2]), dict(xyz=x.double()), dict(xyz=x.cpu()), dict(inverse_map=iv[:9]), dict(inverse_map=iv.int()),
                dict(normal_qv=z(n, 2)), dict(variation_qv=z(n + 1)), dict(count_qv=z(n)), dict(moments_qv=z(n, 10)),
                dict(normal_full=z(n, 3)), dict(workspace=ws[:512]), dict(workspace=ws[8:]), dict(summary=z(8, dtype=torch.uint8)),
                dict(bits=21), dict(quantum=0.3), dict(origin=(0, 0, np.nan)), dict(viewpoint=(np.inf, 0, 0)), dict(scene=None)):
        with pytest.raises(ValueError):
            V.estimate_normals(**dict(good, **bad))
    # the library's own checks: nothing is launched, nothing is written
    outs = dict(normal_qv_dev=torch.full((n, 3), float(SENTINEL), device=DEV), variation_qv_dev=torch.full((n,), float(SENTINEL), device=DEV),
                count_qv_dev=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                moments_qv_dev=torch.full((n, 10), SENTINEL, dtype=torch.int64, device=DEV),
                normal_full_dev=torch.full((n_full, 3), float(SENTINEL), device=DEV),
                summary_dev=torch.full((32,), FILL, dtype=torch.uint8, device=DEV))

    def estimate(**kw):
        a = L.EstimateNormalsArgs()
        base = dict(scene=sc.handle.value, n=n, xyz_dev=x, inverse_map_dev=iv, n_full=n_full, workspace_dev=ws, workspace_bytes=ws.numel(),
                    origin=tuple(origin), quantum=quantum, viewpoint=(0.0, 0.0, 0.0), bits=bits, has_viewpoint=0, **outs)
        for k, v in dict(base, **kw).items():
            if k in ("origin", "viewpoint"):
                getattr(a, k)[:] = v
            else:
                setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_estimate_normals", byref(a), None)

    assert status("a3d_estimate_normals", None, None) == INVALID
    nan, inf = float("nan"), float("inf")
    for bad in (dict(scene=None), dict(n=n - 1), dict(n=n + 1), dict(xyz_dev=None), dict(n_full=-1), dict(n_full=1 << 31),
                dict(n_full=(1 << 22) + 1), dict(bits=-1), dict(bits=21), dict(quantum=0.0), dict(quantum=-0.5), dict(quantum=0.3),
                dict(quantum=nan), dict(quantum=inf), dict(origin=(0.0, nan, 0.0)), dict(origin=(inf, 0.0, 0.0)),
                dict(has_viewpoint=1, viewpoint=(0.0, 0.0, nan)), dict(has_viewpoint=1, viewpoint=(-inf, 0.0, 0.0)),
                dict(summary_dev=None), dict(workspace_dev=None), dict(workspace_bytes=ws.numel() - 1),
                dict(workspace_dev=ws.data_ptr() + 8)):
        assert estimate(**bad) == INVALID, bad
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert (t.cpu().numpy() == (FILL if t.dtype == torch.uint8 else SENTINEL)).all(), k
    assert estimate() == OK and estimate(has_viewpoint=0, viewpoint=(nan, 0.0, 0.0)) == OK       # (not looked at without the flag)
    assert estimate(n_full=0, xyz_dev=None, inverse_map_dev=None, normal_full_dev=None) == OK
    torch.cuda.synchronize()
    assert V.read_normals_summary(outs["summary_dev"].cpu().numpy()) == dict(counted=0, valid=0, invalid=n, err=0)


# ---------------------------------------------------------------------------------------------------- 5
def sheet(seed=3):
    """A receding sheet of 2 000 points with a normal each: unit, scaled, zero, NaN and infinite ones among them."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-1.5, 1.5, 2000), rng.uniform(-0.6, 6.0, 2000), rng.uniform(-0.05, 0.05, 2000)], 1).astype(F32)
    nrm = rng.normal(size=(2000, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(F32)
    nrm[::7] *= F32(3.5)                                                 # (the rule divides by the length: not unit on purpose)
    nrm[::11] = 0.0
    nrm[5::53] = np.nan
    nrm[9::61, 1] = np.inf
    nrm[13::67] = F32(3e19)                                              # l2 overflows to +inf: k0 = 1
    return xyz, nrm, rng.uniform(0, 1, (2000, 3)).astype(F32)


@pytest.mark.parametrize("size", [(37, 29), (16, 16), (1, 1)])
def test_lit_points(size):
    xyz, nrm, col = sheet()
    cam = camera_of([0.0, -1.0, 0.6], [0.0, 3.0, 0.0], 60.0, size)
    ids = render_ids(xyz, 0.06, cam)
    ids_host = ids.cpu().numpy()
    assert size == (1, 1) or ((ids_host >= 0).sum() > 40 and (ids_host < 0).any())
    bg = (0.2, 0.4, 0.9)
    for ambient in (0.0, 0.35, 1.0):
        rgb = torch.full((*ids.shape, 3), 7, dtype=torch.uint8, device=DEV)
        got = V.render_shade_lit_points(ids, _dev(col, F32), _dev(nrm, F32), cam, ambient, bg, rgb=rgb).cpu().numpy()
        assert got.tobytes() == SP.lit_points_rule(ids_host, col, nrm, cam, ambient, bg).tobytes(), (size, ambient)
    flat = V.render_shade(ids, None, None, None, _dev(col, F32), bg).cpu().numpy()
    assert got.tobytes() == flat.tobytes()                              # ambient = 1: the flat pass, byte for byte
    # zero normals everywhere: unshaded whatever the ambient; ids beyond a shorter table: the background
    got = V.render_shade_lit_points(ids, _dev(col, F32), _dev(np.zeros_like(nrm), F32), cam, 0.1, bg).cpu().numpy()
    assert got.tobytes() == flat.tobytes()
    short = 1200
    got = V.render_shade_lit_points(ids, _dev(col[:short], F32), _dev(nrm[:short], F32), cam, 0.35, bg).cpu().numpy()
    assert got.tobytes() == SP.lit_points_rule(ids_host, col[:short], nrm[:short], cam, 0.35, bg).tobytes()
    assert size == (1, 1) or (ids_host >= short).any()
    assert V.render_shade(ids, None, None, None, _dev(col[:short], F32), bg).cpu().numpy().tobytes() == SP.flat_points_rule(ids_host, col[:short], bg).tobytes()


def test_lit_points_refusals():
    cam = camera_of([0.0, -1.0, 0.6], [0.0, 3.0, 0.0], 60.0, (8, 8))
    ids = torch.full((8, 8), -1, dtype=torch.int32, device=DEV)
    col = torch.zeros((5, 3), device=DEV)
    rgb = torch.full((8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    bg = f32_pointer((1, 1, 1))
    call = lambda **kw: status("a3d_render_shade_lit_points", *[kw.get(k, v) for k, v in dict(
        ids=ids.data_ptr(), col=col.data_ptr(), n=5, nrm=col.data_ptr(), cam=byref(cam), ambient=0.5, bg=bg, rgb=rgb.data_ptr(), stream=None).items()])
    bad_cam = L.Camera()
    for bad in (dict(ids=None), dict(col=None), dict(nrm=None), dict(n=-1), dict(cam=None), dict(cam=byref(bad_cam)), dict(ambient=-0.1),
                dict(ambient=1.1), dict(ambient=float("nan")), dict(bg=None), dict(rgb=None)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == 9).all()
    assert call() == OK and call(n=0, col=None, nrm=None) == OK
    torch.cuda.synchronize()
    assert (rgb.cpu().numpy() == 255).all()


# ---------------------------------------------------------------------------------------------------- 6
def cull_gpu(xyz, nrm, eye, mode, hidden=True, count=True):
    out = torch.full((len(xyz), 3), float(SENTINEL), device=DEV)
    hid = torch.full((len(xyz),), FILL, dtype=torch.uint8, device=DEV) if hidden else False
    cnt = torch.full((1,), SENTINEL, dtype=torch.int64, device=DEV) if count else False
    got = V.cull_points(_dev(xyz, F32), _dev(nrm, F32), eye, mode, out=out, hidden=hid, count=cnt)
    assert got[0] is out
    return out.cpu().numpy(), hid.cpu().numpy() if hidden else None, int(cnt.cpu()[0]) if count else None


@pytest.mark.parametrize("n", [1, 63, 1025, 300_000])
def test_cull_bit_for_bit(n):
    rng = np.random.default_rng(n)
    xyz = rng.uniform(-3, 3, (n, 3)).astype(F32)
    nrm = rng.normal(size=(n, 3)).astype(F32)
    nrm[::5] = 0.0
    nrm[3::17, 2] = np.nan
    xyz[4::19, 0] = np.nan
    # g == 0 exactly: a normal at right angles to the offset from the eye, in numbers fp32 holds
    eye = np.array([0.5, -0.25, 2.0], F32)
    xyz[1::23] = eye + np.array([1.0, 2.0, 0.0], F32)
    nrm[1::23] = np.array([2.0, -1.0, 0.0], F32)
    for mode in ("back", "front"):
        out, hidden, count = cull_gpu(xyz, nrm, eye, mode)
        want = R.cull(xyz, nrm, eye, V.CULL_MODES[mode])
        assert out.tobytes() == want[0].tobytes() and hidden.tobytes() == want[1].tobytes() and count == want[2]
        shown = hidden == 0
        assert shown[::5].all() and shown[3::17].all() and shown[4::19].all() and shown[1::23].all() and (n < 63 or not shown.all())
        assert out[shown].tobytes() == xyz[shown].tobytes()
        out2, _, _ = cull_gpu(xyz, nrm, eye, mode, hidden=False, count=False)
        assert out2.tobytes() == out.tobytes()
    x = _dev(xyz, F32)
    V.cull_points(x, _dev(nrm, F32), eye, "back", out=x, hidden=False, count=False)         # in place
    assert x.cpu().numpy().tobytes() == R.cull(xyz, nrm, eye, R.CULL_BACK)[0].tobytes()


def test_cull_refusals():
    x = torch.zeros((4, 3), device=DEV)
    out = torch.full((4, 3), 9.0, device=DEV)
    eye = f32_pointer((0, 0, 0))
    call = lambda **kw: status("a3d_cull_points", *[kw.get(k, v) for k, v in dict(
        xyz=x.data_ptr(), nrm=x.data_ptr(), n=4, eye=eye, mode=1, out=out.data_ptr(), hidden=None, count=None, stream=None).items()])
    for bad in (dict(xyz=None), dict(nrm=None), dict(out=None), dict(n=-1), dict(n=1 << 31), dict(eye=None),
                dict(eye=f32_pointer((0, np.inf, 0))), dict(mode=0), dict(mode=3), dict(count=out.data_ptr() + 4)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 9).all()
    assert call() == OK and call(mode=2) == OK and call(n=0, xyz=None, nrm=None, out=None) == OK


def test_closed_box_seen_from_outside():
    """A closed box of points whose normals look inward, rendered from outside with the back-facing vertices culled: the id
    image is the render of the cloud with the culled vertices DELETED, the ids mapped back -- and it shows the far walls'
    inside through the near walls."""
    k = 14
    g = (np.arange(k) + 0.5) / k * 2 - 1
    a, b = np.meshgrid(g, g, indexing="ij")
    pts, nrm = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = np.empty((k, k, 3))
            p[..., axis], p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = side, a, b
            pts.append(p.reshape(-1, 3))
            nrm.append(np.tile(-side * np.eye(3)[axis], (k * k, 1)))
    perm = np.random.default_rng(2).permutation(6 * k * k)
    xyz, nrm = np.concatenate(pts)[perm].astype(F32), np.concatenate(nrm)[perm].astype(F32)
    cam = camera_of([4.0, 2.5, 1.5], [0.0, 0.0, 0.0], 40.0, (40, 31))
    eye = np.array(cam.o[:], F32)
    out, hidden, count = cull_gpu(xyz, nrm, eye, "back")
    assert 0 < count < len(xyz) and count == 3 * k * k                   # three walls face away from a corner view
    ids_culled = render_ids(out, 0.09, cam).cpu().numpy()
    kept = np.flatnonzero(hidden == 0)
    ids_deleted = render_ids(xyz[kept], 0.09, cam).cpu().numpy()
    mapped = np.where(ids_deleted >= 0, kept[np.maximum(ids_deleted, 0)], -1)
    assert np.array_equal(ids_culled, mapped) and (ids_culled >= 0).sum() > 200
    assert np.array_equal(ids_deleted, render_points_rule(xyz[kept], 0.09, cam)[0])
    plain = render_ids(xyz, 0.09, cam).cpu().numpy()
    seen = plain[plain >= 0]
    assert (hidden[seen] == 1).mean() > 0.6 and (hidden[ids_culled[ids_culled >= 0]] == 0).all()
