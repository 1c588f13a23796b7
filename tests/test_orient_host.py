"""Host side of orienting normals by propagation (no GPU): ``a3d_orient_edge`` -- the function the kernel calls -- against the
restatement bit for bit; the restatement (``orient_rule.py``, Dijkstra) against a brute-force relaxation; the parity tie on the
ring, seed flips, the nearest-seed rule; every ``ValueError`` ``view.orient_normals`` raises before the library is reached and
``a3d_orient_normals``' refusal of a call without a scene; and the property the feature exists for: on the cube shells and on
the room with a cabinet, with PCA normals signed by a viewpoint, every voxel whose neighbourhood is exactly planar ends up
pointing outward (into the room, for the room).  ``test_gpu_orient.py`` holds the kernels to the same restatement."""
import ctypes as C
import types

import numpy as np
import pytest

import orient_cases as K
import orient_rule as R

F32 = np.float32


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def _view():
    _lib()
    from agile3d_amd import view
    return view


# ------------------------------------------------------------------------------------------- the edge function
def test_edge_function_bit_for_bit_and_symmetric():
    V = _view()
    rng = np.random.default_rng(5)
    a = rng.normal(size=(10000, 3))
    b = rng.normal(size=(10000, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    b[:3000] = (a[:3000] + rng.normal(0, 0.02, (3000, 3))) * rng.choice([-1.0, 1.0], (3000, 1))    # nearly parallel pairs
    a, b = a.astype(F32), b.astype(F32)
    costs = set()
    for x, y in zip(a, b):
        w, flip, _ = R.edge(x, y)
        assert V.orient_edge(x, y) == (w, flip) == V.orient_edge(y, x) and 1 <= w <= 1024
        costs.add(w)
    assert len(costs) > 500 and {1, 2} <= costs
    up = F32(np.nextafter(F32(1), F32(2)))
    one, z = F32(1), F32(0)
    edge_values = [((one, z, z), (z, one, z), 1024, False),             # dot exactly 0
                   ((one, z, z), (one, z, z), 1, False),                # +1
                   ((one, z, z), (-one, z, z), 1, True),                # -1
                   ((up, z, z), (up, z, z), 1, False),                  # slightly beyond +1: 1 - |dot| < 0 is clamped
                   ((up, z, z), (-up, z, z), 1, True),                  # slightly beyond -1
                   ((one, one, one), (-z, -z, -z), 1024, False),        # dot = -0.0 is not < 0
                   ((F32(3e38), F32(3e38), z), (F32(3e38), -F32(3e38), z), 1, False)]   # inf - inf: a NaN dot
    for x, y, w, flip in edge_values:
        x, y = np.array(x, F32), np.array(y, F32)
        assert V.orient_edge(x, y) == V.orient_edge(y, x) == (w, flip) == R.edge(x, y)[:2], (x, y)
    assert R.edge(edge_values[5][0], edge_values[5][1])[2].view(np.uint32) == 0x80000000


def test_edge_entry_point_refuses_null():
    lib, L = _lib()
    a = (C.c_float * 3)(1, 0, 0)
    w, f = C.c_int32(7), C.c_int32(7)
    assert L.a3d_orient_edge(None, a, C.byref(w), C.byref(f)) == lib.A3D_ERR_INVALID
    assert L.a3d_orient_edge(a, a, None, C.byref(f)) == lib.A3D_ERR_INVALID and (w.value, f.value) == (7, 7)


# ------------------------------------------------------------------------------------------- the rule against a brute force
def _random_case(rng):
    box = rng.integers(1, 6, 3)
    cells = np.stack(np.meshgrid(*[np.arange(s) for s in box], indexing="ij"), -1).reshape(-1, 3)
    keep = cells[rng.random(len(cells)) < rng.uniform(0.4, 1.0)]
    if len(keep) == 0:
        keep = cells[:1]
    batch = rng.integers(0, 2, (len(keep), 1)) if rng.random() < 0.3 else np.zeros((len(keep), 1), np.int64)
    coords = np.concatenate([batch, keep - rng.integers(0, 3)], 1)[rng.permutation(len(keep))]
    n = len(coords)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    nrm[rng.random(n) < 0.1] = 0
    seeds = np.zeros(n, np.uint8)
    seeds[rng.choice(n, rng.integers(0, min(n, 4) + 1), replace=False)] = 1
    return coords, nrm, seeds, int(rng.choice([6, 18, 26]))


def test_rule_against_brute_force_on_random_graphs():
    rng = np.random.default_rng(12)
    reached = flipped = 0
    for _ in range(200):
        coords, nrm, seeds, conn = _random_case(rng)
        adj = R.edges(coords, nrm, conn)
        got = R.orient_numpy(coords, nrm, conn, seed_qv=seeds, adj=adj)
        ok = R.admitted(nrm)
        dist, owner = R.brute_force(adj, ok & (seeds != 0), len(coords))
        assert np.array_equal(got["dist"], dist) and np.array_equal(got["owner"], owner)
        for v in np.flatnonzero(dist > 0):                              # the parent explains the dist and is the lowest such slot
            u = got["parent"][v]
            hits = [(k, j) for k, j, w, _, _ in adj[v] if owner[j] == owner[v] and dist[j] + w == dist[v]]
            assert hits and hits[0][1] == u
        out = got["normal_out"]
        for v in np.flatnonzero(dist > 0):                              # along every tree edge the OUTPUT normals agree
            assert not R.edge(out[v], out[got["parent"][v]])[2] < 0
        assert np.array_equal(out.view(np.uint32)[~ok], nrm.view(np.uint32)[~ok]) and not got["flipped"][dist < 0].any()
        reached += int((dist > 0).sum())
        flipped += int(got["flipped"].sum())
    assert reached > 500 and flipped > 100


# ------------------------------------------------------------------------------------------- the ring, flips, nearest seeds
def test_ring_parity_tie_goes_to_the_lowest_slot():
    coords, nrm, at = K.ring()
    seeds = np.zeros(40, np.uint8)
    seeds[at[0]] = 1
    for conn in (6, 26):
        adj = R.edges(coords, nrm, conn)
        got = R.orient_numpy(coords, nrm, conn, seed_qv=seeds, adj=adj)
        d = got["dist"][at]
        assert d[20] == d[19] + (d[1] - d[0]) == d[21] + (d[1] - d[0]) and got["summary"]["reached"] == 40   # two equal routes
        anti = at[20]
        both = sorted((k, j) for k, j, w, _, _ in adj[anti] if got["dist"][j] + w == got["dist"][anti])
        assert len(both) == 2 and got["parent"][anti] == both[0][1]
        f = got["flipped"][at]
        via = int(np.flatnonzero(at == both[0][1])[0])                  # 19 or 21: the side the antipode hangs on
        assert f[:20].sum() == 0 and f[21:].all() and f[20] == (via == 21)
        assert got["summary"]["conflicts"] >= 1 and got["summary"]["flipped"] == 19 + int(via == 21)


def test_seed_flips():
    coords, at = K.line(30, seed=2)
    nrm = K.random_signs(30, seed=3, tilt=0.05)
    seeds = np.zeros(30, np.uint8)
    seeds[at[0]] = 1
    plain = R.orient_numpy(coords, nrm, 6, seed_qv=seeds)
    sign = np.sign(plain["normal_out"][:, 2])
    assert (sign == np.sign(nrm[at[0], 2])).all() and plain["summary"]["conflicts"] == 0
    flips = np.zeros(30, np.uint8)
    flips[at[0]] = 1
    flips[at[7]] = 1                                                    # a flip on a row that is no seed says nothing
    turned = R.orient_numpy(coords, nrm, 6, seed_qv=seeds, seed_flip=flips)
    assert np.array_equal(turned["flipped"], 1 - plain["flipped"]) and np.array_equal(turned["dist"], plain["dist"])
    assert np.array_equal(turned["normal_out"], -plain["normal_out"])


def test_nearest_seed_rule_with_equal_d2():
    coords, at = K.line(9, seed=4)
    nrm = np.tile(np.array([0, 0, 1], F32), (9, 1))
    pos = K.centres(coords)
    comp = np.zeros(9, np.int32)
    vp = np.array([4.0, 3.0, 10.0])                                     # above the middle voxel x = 4: 3 and 5 are equally far
    seed, flip, err = R.nearest_seeds(nrm, comp, pos, vp)
    assert seed.sum() == 1 and seed[at[4]] and not flip.any() and err == 0
    nrm[at[4]] = 0                                                      # the middle is not admitted: the lower ROW of 3 and 5 wins
    seed, flip, _ = R.nearest_seeds(nrm, comp, pos, vp)
    assert seed.sum() == 1 and seed[min(at[3], at[5])]
    seed, flip, _ = R.nearest_seeds(nrm, comp, pos, vp * [1, 1, -1])    # seen from below: the seed is turned
    assert seed[min(at[3], at[5])] and flip[min(at[3], at[5])]
    comp[at[:3]] = 5
    comp[at[8]] = -1
    comp[at[7]] = 9                                                     # a component no row can name
    seed, _, err = R.nearest_seeds(nrm, comp, pos, vp)
    assert seed.sum() == 2 and seed[at[2]] and err == R.BAD_COMPONENT and not seed[at[7]] and not seed[at[8]]


# ------------------------------------------------------------------------------------------- refusals
def test_wrapper_refusals():
    import torch
    V = _view()
    scene = types.SimpleNamespace(handle=C.c_void_p(1), n=[4])
    nrm = torch.zeros(4, 3)
    seeds = torch.zeros(4, dtype=torch.uint8)
    comp = torch.zeros(4, dtype=torch.int32)
    refuse = lambda *a, **kw: pytest.raises(ValueError, V.orient_normals, *a, **kw)
    for conn in (0, 7, 27, None):
        refuse(scene, nrm, seed_qv=seeds, connectivity=conn)
    for sweeps in (0, -1, 4097, 1.5, True):
        refuse(scene, nrm, seed_qv=seeds, sweeps=sweeps)
    refuse(types.SimpleNamespace(handle=None, n=[4]), nrm, seed_qv=seeds)
    refuse(types.SimpleNamespace(handle=C.c_void_p(1), n=[(1 << 21) + 1]), nrm, seed_qv=seeds)
    refuse(scene, nrm)                                                  # no seeds of either mode
    refuse(scene, nrm, seed_flip=seeds)                                 # flips without marks
    refuse(scene, nrm, seed_qv=seeds, components=comp, positions=nrm, viewpoint=(0, 0, 0))     # both modes
    refuse(scene, nrm, components=comp, positions=nrm)                  # no viewpoint
    refuse(scene, nrm, components=comp, viewpoint=(0, 0, 0))            # no positions
    refuse(scene, nrm, positions=nrm, viewpoint=(0, 0, 0))              # no components
    refuse(scene, nrm, seed_qv=seeds)                                   # tensors that are not on the GPU: there is no CPU path
    for n in (-1, (1 << 21) + 1):                                        # sizes the library has no workspace for
        with pytest.raises(ValueError):
            V.orient_workspace(n, "cpu")


def test_entry_point_without_a_scene():
    lib, L = _lib()
    assert L.a3d_orient_normals(None, None) == lib.A3D_ERR_INVALID
    a = lib.OrientNormalsArgs()
    a.n, a.connectivity, a.sweeps, a.mode = 4, 26, 8, lib.A3D_ORIENT_GIVEN
    assert L.a3d_orient_normals(C.byref(a), None) == lib.A3D_ERR_INVALID
    assert b"a3d_orient_normals" in L.a3d_last_error()
    assert L.a3d_orient_workspace_bytes(-1) == 0 == L.a3d_orient_workspace_bytes((1 << 21) + 1)
    small, large = L.a3d_orient_workspace_bytes(1), L.a3d_orient_workspace_bytes(1 << 21)
    assert 0 < small and small % 256 == 0 and large >= (1 << 21) * (8 + 4 + 1 + 1 + 8 + 4 + 54)


def test_summary_record():
    V = _view()
    raw = np.zeros(1, V.ORIENT_SUMMARY)
    raw["admitted"], raw["conflicts"], raw["converged"], raw["err"] = 5, 1 << 40, 1, 3
    s = V.read_orient_summary(raw.view(np.uint8))
    assert s == dict(admitted=5, seeds=0, reached=0, unreached=0, flipped=0, conflicts=1 << 40, max_dist=0, converged=1, err=3)


# ------------------------------------------------------------------------------------------- what the feature is for
def _wrong(coords, normals, planar, centre, outward):
    side = ((K.centres(coords).astype(np.float64) - centre) * normals).sum(1)
    return int((planar & ((side < 0) if outward else (side > 0))).sum())


@pytest.mark.parametrize("k,before", [(12, 547), (24, None)])
def test_cube_shells_point_outward(k, before):
    coords = K.shell(k, seed=k)
    vp = np.array([40.0, 3.0, 5.0])
    nrm, planar = R.pca_normals(coords, viewpoint=vp)
    centre = np.full(3, (k - 1) / 2)
    inward = ((K.centres(coords) - centre) * nrm).sum(1) < 0
    assert inward.sum() == (before or inward.sum()) > 0 and planar.sum() == 6 * (k - 4) ** 2     # the viewpoint sign alone
    assert _wrong(coords, nrm, planar, centre, True) > 0
    comp = np.zeros(len(coords), np.int32)
    got = R.orient_numpy(coords, nrm, 26, components=comp, positions=K.centres(coords), viewpoint=vp)
    out = got["normal_out"]
    assert got["summary"]["seeds"] == 1 and got["summary"]["reached"] == len(coords) and got["summary"]["conflicts"] == 0
    assert _wrong(coords, out, planar, centre, True) == 0
    assert (((K.centres(coords) - centre) * out).sum(1) < 0).sum() == 0          # the prototype's figure: no voxel at all


def test_room_with_cabinet():
    coords, cab = K.room_with_cabinet()
    centre = np.full(3, 14.5)
    nrm, planar = R.pca_normals(coords, viewpoint=centre)
    cab_centre = (K.CABINET_LO + K.CABINET_HI) / 2
    away = ((K.centres(coords) - cab_centre) * nrm).sum(1)
    assert (cab & (away < 0)).sum() == 116                              # the viewpoint sign turns these into the cabinet
    assert _wrong(coords[cab], nrm[cab], planar[cab], cab_centre, True) > 0
    comp = np.zeros(len(coords), np.int32)                              # one component: the cabinet stands on the floor
    got = R.orient_numpy(coords, nrm, 26, components=comp, positions=K.centres(coords), viewpoint=centre)
    out = got["normal_out"]
    assert got["summary"]["reached"] == len(coords) == 5308
    assert _wrong(coords[cab], out[cab], planar[cab], cab_centre, True) == 0
    assert _wrong(coords[~cab], out[~cab], planar[~cab], centre, False) == 0
    assert not got["flipped"][~cab].any() and got["flipped"][cab].sum() == 116  # no room voxel changes
