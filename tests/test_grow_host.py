"""Host side of growing a selection along the surface (no GPU): the rule's restatement (``grow_rule.py``, Dijkstra) against an
independent brute force (repeated full relaxation to a fixed point), the metric costs, ``session.grow_limit``, every
``ValueError`` the ``view.py`` wrapper raises before the library is reached, and ``a3d_grow_voxels``' refusal of a call
without a scene.  ``test_gpu_grow.py`` holds the kernels to the same restatement bit for bit."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import grow_rule as G


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


# ------------------------------------------------------------------------------------------- the rule against a brute force
def brute_force(coords4, keys, cost, limit, connectivity, seeds):
    """Jacobi sweeps over ALL voxels until nothing changes: value[v] = min(own, min over walkable neighbours u of
    (dist[u] + step, owner[u]) within the limit), pairs compared lexicographically.  Shares no code with ``grow_numpy`` but the
    coordinates' dictionary."""
    c = np.asarray(coords4, np.int64).tolist()
    n = len(c)
    where = {tuple(p): i for i, p in enumerate(c)}
    none = (1 << 40, 1 << 40)
    value = [(0, i) if i in seeds and keys[i] >= 0 else none for i in range(n)]
    admitted = {6: 1, 18: 2, 26: 3}[connectivity]
    while True:
        new = list(value)
        for i, (b, x, y, z) in enumerate(c):
            if keys[i] < 0:
                continue
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dz in (-1, 0, 1):
                        l1 = abs(dx) + abs(dy) + abs(dz)
                        j = where.get((b, x + dx, y + dy, z + dz))
                        if not 1 <= l1 <= admitted or j is None or keys[j] != keys[i] or value[j] == none:
                            continue
                        cand = (value[j][0] + cost[l1 - 1], value[j][1])
                        if cand[0] <= limit and cand < new[i]:
                            new[i] = cand
        if new == value:
            break
        value = new
    dist = np.array([-1 if v == none else v[0] for v in value], np.int32).reshape(n)
    owner = np.array([-1 if v == none else v[1] for v in value], np.int32).reshape(n)
    return dist, owner


def _random_case(rng):
    box = rng.integers(1, 6, 3)
    cells = np.stack(np.meshgrid(*[np.arange(s) for s in box], indexing="ij"), -1).reshape(-1, 3)
    keep = cells[rng.random(len(cells)) < rng.uniform(0.4, 1.0)]
    if len(keep) == 0:
        keep = cells[:1]
    batch = rng.integers(0, 2, (len(keep), 1)) if rng.random() < 0.3 else np.zeros((len(keep), 1), np.int64)
    coords = np.concatenate([batch, keep - rng.integers(0, 3)], 1)[rng.permutation(len(keep))]
    n = len(coords)
    keys = [np.zeros(n, np.int64), rng.integers(-1, 3, n), rng.integers(-1, 1, n)][rng.integers(3)]
    cost = G.METRIC_COST if rng.random() < 0.4 else tuple(int(x) for x in rng.integers(1, 6, 3))
    limit = int(rng.integers(0, 6 * max(cost)))
    seeds = set(rng.choice(n, rng.integers(0, min(n, 4) + 1), replace=False).tolist())
    return coords, keys, cost, limit, int(rng.choice([6, 18, 26])), seeds


def test_rule_against_brute_force_on_random_graphs():
    rng = np.random.default_rng(11)
    reached = ties = 0
    for _ in range(200):
        coords, keys, cost, limit, conn, seeds = _random_case(rng)
        seed_qv = np.zeros(len(coords), np.uint8)
        seed_qv[sorted(seeds)] = 1
        dist, owner = G.grow_numpy(coords, keys, cost, limit, conn, seed_qv=seed_qv)
        want_dist, want_owner = brute_force(coords, keys, cost, limit, conn, seeds)
        assert np.array_equal(dist, want_dist) and np.array_equal(owner, want_owner), (coords, keys, cost, limit, conn, seeds)
        assert ((dist >= 0) == (owner >= 0)).all() and (dist <= limit).all()
        assert all(dist[s] == 0 and owner[s] == s for s in seeds if keys[s] >= 0)
        reached += int((dist > 0).sum())
        ties += len(seeds) > 1
    assert reached > 500 and ties > 50


def test_cube_and_symmetric_seeds():
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    cube = np.concatenate([np.zeros((125, 1), np.int64), g], 1)[np.random.default_rng(0).permutation(125)]
    keys = np.zeros(125, np.int64)
    centre = int(np.flatnonzero((cube[:, 1:] == 2).all(1))[0])
    for conn in (6, 18, 26):
        for cost, limit in ((G.METRIC_COST, 4000), ((1, 1, 1), 3), ((2, 3, 4), 7)):
            seed_qv = np.zeros(125, np.uint8)
            seed_qv[centre] = 1
            dist, owner = G.grow_numpy(cube, keys, cost, limit, conn, seed_qv=seed_qv)
            want = brute_force(cube, keys, cost, limit, conn, {centre})
            assert np.array_equal(dist, want[0]) and np.array_equal(owner, want[1])
            assert set(owner[dist >= 0].tolist()) == {centre}
    # the metric costs in the open cube: a face, an edge and a corner neighbour, and two faces in a row
    dist, _ = G.grow_numpy(cube, keys, G.METRIC_COST, 4000, 26, seed_qv=seed_qv)
    d = lambda *o: int(dist[np.flatnonzero((cube[:, 1:] == np.array([2, 2, 2]) + o).all(1))[0]])
    assert (d(1, 0, 0), d(1, 1, 0), d(1, 1, 1), d(2, 0, 0), d(2, 1, 0)) == (1024, 1448, 1774, 2048, 1024 + 1448)
    # two seeds symmetric about a voxel: the smaller ROW owns it, wherever the rows lie
    line = np.array([[0, x, 0, 0] for x in range(5)], np.int64)
    for perm in ([0, 1, 2, 3, 4], [4, 1, 2, 3, 0], [3, 0, 4, 2, 1]):
        coords = line[np.argsort(perm)]                              # row perm[x] holds the voxel at x
        a, b, mid = perm[0], perm[4], perm[2]
        seed_qv = np.zeros(5, np.uint8)
        seed_qv[[a, b]] = 1
        dist, owner = G.grow_numpy(coords, None, (1, 1, 1), 2, 6, seed_qv=seed_qv)
        assert dist[mid] == 2 and owner[mid] == min(a, b)
        assert (owner[perm[1]], owner[perm[3]]) == (a, b)
        assert np.array_equal(owner, brute_force(coords, np.zeros(5), (1, 1, 1), 2, 6, {a, b})[1])


def test_lift_summary_and_shrink_rules():
    coords = np.array([[0, x, 0, 0] for x in range(7)], np.int64)
    inv = np.array([0, 0, 1, 2, 2, 3, 5, 6, 6, -1, 7])
    seed_full = np.zeros(len(inv), np.uint8)
    seed_full[[3, 9, 10]] = 1                                        # voxel 2, and two vertices outside the rows (ignored)
    r = G.grow_all(coords, None, (1, 1, 1), 2, 6, seed_full=seed_full, inverse_map=inv, n_full=len(inv))
    assert r["dist_qv"].tolist() == [2, 1, 0, 1, 2, -1, -1]
    assert r["dist_full"].tolist() == [2, 2, 1, 0, 0, 1, -1, -1, -1, -1, -1] and r["selected_full"].tolist() == [1] * 6 + [0] * 5
    assert r["summary"] == dict(seeds=1, reached=5, selected=6, max_dist=2, err=G.BAD_INDEX)
    # shrink: vertices in voxels 1..5 selected; the outside is {0, 6}; one step takes voxels 1 and 5 away
    inv = np.array([0, 1, 1, 2, 3, 4, 5, 6])
    sel = np.array([0, 1, 0, 1, 1, 1, 1, 0], np.uint8)               # (voxel 1 holds a selected and an unselected vertex)
    assert G.shrink_numpy(coords, inv, sel, (1, 1, 1), 0, 6).tolist() == sel.tolist()
    assert G.shrink_numpy(coords, inv, sel, (1, 1, 1), 1, 6).tolist() == [0, 0, 0, 1, 1, 1, 0, 0]
    assert G.shrink_numpy(coords, inv, sel, (1, 1, 1), 3, 6).tolist() == [0] * 8


def test_metric_costs_are_the_roundings_claimed():
    from agile3d_amd import view as V
    want = tuple(int(round(1024 * math.sqrt(k))) for k in (1, 2, 3))
    assert want == (1024, 1448, 1774) == G.METRIC_COST == V.GROW_METRIC_COST
    assert all(abs(c - 1024 * math.sqrt(k)) <= 0.5 for c, k in zip(want, (1, 2, 3)))
    assert G.MAX_STEPS == V.GROW_MAX_STEPS == 1024 and G.BAD_INDEX == V.GROW_BAD_INDEX


# ------------------------------------------------------------------------------------------- session.grow_limit
def test_grow_limit():
    from agile3d_amd.session import grow_limit
    assert grow_limit(None, 0, 0.05) == ((1, 1, 1), 0) and grow_limit(None, 1024, 0.05) == ((1, 1, 1), 1024)
    assert grow_limit(None, np.int64(7), 0.02) == ((1, 1, 1), 7)
    assert grow_limit(0.0, None, 0.05) == (G.METRIC_COST, 0)
    # a voxel size that is a power of two: every multiple is exact, the limit is k * 1024
    for vs in (0.0625, 0.5, 2.0):
        for k in (0, 1, 3, 17, 1024):
            assert grow_limit(k * vs, None, vs) == (G.METRIC_COST, k * 1024)
    # any other voxel size: the float64 formula as stated, floor(radius / voxel_size * 1024) -- the quotient of an exact
    # multiple k * vs may round to just below k, so the limit is k * 1024 or one unit (1/1024 voxel) less
    below = 0
    for vs in (0.05, 0.02, 0.03, 0.1):
        for k in range(0, 1025):
            radius = k * vs
            cost, limit = grow_limit(radius, None, vs)
            assert limit == int(np.floor(np.float64(radius) / np.float64(vs) * 1024.0)) and cost == G.METRIC_COST
            assert limit in (k * 1024, k * 1024 - 1), (vs, k, limit)
            below += limit != k * 1024
    print(f"grow_limit: {below} of {4 * 1025} exact multiples land one unit below k * 1024")
    assert grow_limit(0.15, None, 0.05)[1] == int(np.floor(np.float64(0.15) / np.float64(0.05) * 1024.0))
    assert grow_limit(1024.999 * 0.0625, None, 0.0625)[1] // 1024 == 1024        # the last radius that is taken
    for bad in (dict(radius=None, steps=None), dict(radius=1.0, steps=1), dict(radius=-0.1, steps=None),
                dict(radius=float("nan"), steps=None), dict(radius=float("inf"), steps=None), dict(radius=None, steps=-1),
                dict(radius=None, steps=1.5), dict(radius=None, steps=True), dict(radius=None, steps=1025),
                dict(radius=1025 * 0.0625, steps=None), dict(radius=1e30, steps=None)):
        with pytest.raises(ValueError):
            grow_limit(voxel_size=0.0625, **bad)
    with pytest.raises(ValueError, match="pieces"):
        grow_limit(None, 5000, 0.05)


# ------------------------------------------------------------------------------------------- the wrapper's refusals
def test_wrapper_refuses_before_the_library():
    import torch
    from agile3d_amd import view as V
    assert V.grow_settings((1, 1, 1), 1024, 6) == ((1, 1, 1), 1024, 6)
    assert V.grow_settings([1024, 1448, 1774], 1024 * 1024 + 1023, 26) == (G.METRIC_COST, 1024 * 1024 + 1023, 26)
    assert V.grow_settings((65536, 65536, 65536), 1 << 26, 18)[1] == 1 << 26
    for name, bad in (("connectivity", dict(connectivity=8)), ("connectivity", dict(connectivity=None)),
                      ("cost", dict(cost=(1, 1))), ("cost", dict(cost=(0, 1, 1))), ("cost", dict(cost=(1, 65537, 1))),
                      ("cost", dict(cost=(1.5, 2, 3))), ("cost", dict(cost=7)), ("limit", dict(limit=-1)),
                      ("limit", dict(limit=(1 << 30) + 1)), ("limit", dict(limit=0.5)), ("limit", dict(limit=1025)),
                      ("limit", dict(cost=G.METRIC_COST, limit=1025 * 1024)),
                      ("limit", dict(cost=(4, 2, 9), limit=2050))):
        with pytest.raises(ValueError, match=name):
            V.grow_settings(**dict(dict(cost=(1, 1, 1), limit=3, connectivity=26), **bad))
    scene = types.SimpleNamespace(handle=C.c_void_p(0), n=[5])
    seed = torch.zeros(5, dtype=torch.uint8)
    for name, bad in (("n_full", dict(n_full=-1)), ("n_full", dict(n_full=1.5)), ("n_full", dict(n_full=1 << 31)),
                      ("seed", dict(seed_qv=None)), ("n_full", dict(seed_full=seed)), ("n_full", dict(inverse_map=seed)),
                      ("scene", dict(scene=None)), ("scene", dict(scene=object())), ("limit", dict(limit=-3)),
                      ("cost", dict(cost=(1, 2))), ("connectivity", dict(connectivity=7)),
                      ("GPU", dict()), ("GPU", dict(seed_qv=None, seed_full=seed, n_full=5))):
        with pytest.raises(ValueError, match=name):
            V.grow_voxels(**dict(dict(scene=scene, n_full=0, seed_qv=seed), **bad))
    assert V.read_grow_summary(np.array([(3, 9, 20, 4096, 1)], V.GROW_SUMMARY).view(np.uint8)) == dict(
        seeds=3, reached=9, selected=20, max_dist=4096, err=1)


def test_library_refuses_without_a_scene():
    lib, L = _lib()
    assert L.a3d_grow_workspace_bytes(-1) == 0 and L.a3d_grow_workspace_bytes(1 << 31) == 0
    for n in (0, 1, 1000):
        nbytes = L.a3d_grow_workspace_bytes(n)
        assert nbytes >= 9 * n + 4 * (lib.A3D_GROW_MAX_STEPS + 1) and nbytes % 256 == 0
    assert C.sizeof(lib.GrowVoxelsArgs) == 136 and C.sizeof(lib.GrowSummary) == 32
    assert L.a3d_grow_voxels(None, None) == lib.A3D_ERR_INVALID
    a = lib.GrowVoxelsArgs()
    a.n, a.connectivity, a.limit = 0, 26, 0
    a.cost[:] = (1, 1, 1)
    a.seed_qv_dev = a.summary_dev = 256                             # (never looked at: the scene is checked first)
    assert L.a3d_grow_voxels(C.byref(a), None) == lib.A3D_ERR_INVALID
    assert b"a3d_grow_voxels" in L.a3d_last_error()
