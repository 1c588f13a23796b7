"""-m gpu: the bounded shortest-path distance from a set of seed voxels (a3d_grow_voxels in csrc/session_grow.hip;
view.grow_voxels) against its restatement ``grow_rule.py``, bit for bit, on dist_qv, owner_qv, selected_full, dist_full and
the summary.  Everything is integer: every comparison is exact.

1  sizes at their edges (1, 2, 255, 256, 257 voxels; one full pass of the grid + 77 rows); a line of 600 voxels seeded at one
   end (hundreds of sweeps, several workgroups); the serpentine cut mid-line by the step bound
2  a solid cube with 1, 2 and 40 seeds under each connectivity (equal-cost paths, owner ties); two plates an empty layer
   apart, and joined by one voxel; the limit at an exact distance
3  keys: NULL against zeros, a mask, labels, a seed on a voxel without a key; seeds per voxel, per vertex through a
   many-to-one inverse map, both, none; inverse-map entries out of range
4  random blobs with random keys, seeds, costs and limits
5  outputs omitted one at a time; two calls give the same bytes; the library's refusals leave every output untouched
"""
import numpy as np
import pytest
import torch

import grow_rule as G
from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from session_kit import DEV, _dev, byref, status

pytestmark = pytest.mark.gpu

SENTINEL = -77
FILL = 0x5a
CONN = (6, 18, 26)
HOPS = (1, 1, 1)
OUTPUTS = ("dist_qv", "owner_qv", "selected_full", "dist_full")
INVALID, OK = -1, 0


# ---------------------------------------------------------------------------------------------------- the adaptors
def scene_of(coords4):
    return Scene(torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(DEV))


def grow_gpu(scene, keys=None, seed_qv=None, seed_full=None, inverse_map=None, n_full=0, cost=HOPS, limit=0, connectivity=26,
             omit=(), workspace=None):
    """view.grow_voxels, numpy in / numpy out; every output starts as a sentinel."""
    n = scene.n[0]
    outs = dict(dist_qv=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                owner_qv=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                selected_full=torch.full((n_full,), FILL, dtype=torch.uint8, device=DEV),
                dist_full=torch.full((n_full,), SENTINEL, dtype=torch.int32, device=DEV))
    given = {k: (False if k in omit else t) for k, t in outs.items()}
    summary = torch.full((V.GROW_SUMMARY.itemsize,), FILL, dtype=torch.uint8, device=DEV)
    dev = lambda a, dtype: None if a is None else _dev(a, dtype)
    got = V.grow_voxels(scene, n_full, dev(keys, np.int32), dev(seed_qv, np.uint8), dev(seed_full, np.uint8),
                        dev(inverse_map, np.int64), cost, limit, connectivity, summary=summary, workspace=workspace, **given)
    for k, t in zip(OUTPUTS, got[:4]):
        assert t is (None if k in omit else outs[k])
    assert got[4] is summary
    raw = summary.cpu().numpy()
    res = {k: t.cpu().numpy() for k, t in outs.items()}
    res.update(summary=V.read_grow_summary(raw), raw=raw, workspace=got[5])
    return res


def same(got, want, what=None, omit=()):
    for k in OUTPUTS:
        if k in omit:
            assert (got[k] == (FILL if k == "selected_full" else SENTINEL)).all(), (what, k)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert got["summary"] == want["summary"], (what, got["summary"], want["summary"])


def check(coords4, scene, what=None, **kw):
    """One call against the rule; returns (got, want)."""
    got = grow_gpu(scene, **kw)
    rule = {k: v for k, v in kw.items() if k not in ("omit", "workspace")}
    want = G.grow_all(coords4, rule.pop("keys", None), rule.pop("cost", HOPS), rule.pop("limit", 0), rule.pop("connectivity", 26),
                      **rule)
    same(got, want, what, kw.get("omit", ()))
    return got, want


def marks(n, rows):
    m = np.zeros(n, np.uint8)
    m[list(rows)] = 1
    return m


def line(m, seed=0):
    """m voxels along x, rows shuffled: row ``at[x]`` holds the voxel at x."""
    perm = np.random.default_rng(seed).permutation(m)
    coords = np.stack([np.zeros(m), np.arange(m), np.full(m, 3), np.full(m, -2)], 1).astype(np.int32)[perm]
    at = np.empty(m, np.int64)
    at[perm] = np.arange(m)
    return coords, at


def cube(k, seed=0):
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 3)
    coords = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)
    return coords[np.random.default_rng(seed).permutation(len(coords))]


def row_at(coords4, x, y, z):
    return int(np.flatnonzero((coords4[:, 1:] == (x, y, z)).all(1))[0])


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_sizes_at_their_edges(m):
    coords, at = line(m, seed=m)
    sc = scene_of(coords)
    seeds = marks(m, {at[0], at[m - 1], at[m // 2]})
    for c in (6, 26):
        for limit in (0, 1, 40, 300):
            # the lift through the identity: no inverse_map, n_full = n; and one vertex more than there are rows
            check(coords, sc, (m, c, limit), seed_qv=seeds, n_full=m, limit=limit, connectivity=c)
    got, _ = check(coords, sc, seed_qv=seeds, n_full=m + 1, limit=5)
    assert got["summary"]["err"] == G.BAD_INDEX and got["dist_full"][m] == -1 and got["selected_full"][m] == 0
    got, _ = check(coords, sc, seed_full=marks(m, {at[0]}), n_full=m, limit=21, cost=(7, 9, 11))
    assert got["summary"]["seeds"] == 1 and got["summary"]["max_dist"] == (0 if m == 1 else 7 if m == 2 else 21)


def lines_of_five(coords4, keys, seed_qv, limit):
    """``(dist, owner)`` of the rule in CLOSED FORM for voxels (x in 0..4, y, z) whose lines along x never touch, walked with hop
    costs: a seed at position q reaches position p when every voxel between them is there and holds a key >= 0, at cost
    |p - q|.  Vectorised over the lines, so that half a million voxels take a second (Dijkstra in Python takes twenty)."""
    n = len(coords4)
    _, lid = np.unique(coords4[:, 2:4], axis=0, return_inverse=True)
    lid = lid.reshape(-1)
    row = np.full((lid.max() + 1, 5), -1, np.int64)
    row[lid, coords4[:, 1]] = np.arange(n)
    ok = (row >= 0) & (np.asarray(keys)[row] >= 0)
    seed = ok & (np.asarray(seed_qv)[row] != 0)
    none = 1 << 40
    best_d, best_s = np.full(row.shape, none), np.full(row.shape, none)
    for p in range(5):
        for q in range(5):
            d = abs(p - q)
            open_way = seed[:, q] & ok[:, min(p, q):max(p, q) + 1].all(1) & (d <= limit)
            better = open_way & ((d < best_d[:, p]) | ((d == best_d[:, p]) & (row[:, q] < best_s[:, p])))
            best_d[better, p], best_s[better, p] = d, row[better, q]
    dist, owner = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    hit = best_d < none
    dist[row[hit]], owner[row[hit]] = best_d[hit], best_s[hit]
    return dist, owner


def test_one_full_grid_pass_and_77_rows():
    """2048 workgroups x 256 rows is one pass of the sweep's grid: 524 365 voxels take a second pass of 77 rows.  Lines of five
    voxels, two apart in y and z (never neighbours, under any connectivity), the last one cut short; hop costs.  The rule is
    evaluated in closed form here (``lines_of_five``), which is first held to ``grow_rule.py`` on the first 3 000 voxels."""
    m = 2048 * 256 + 77
    side = 324
    assert side * side * 5 >= m
    yz = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 1, 2) * 2
    pts = np.concatenate([np.broadcast_to(np.arange(5).reshape(1, 5, 1), (side * side, 5, 1)), np.broadcast_to(yz, (side * side, 5, 2))], 2)
    rng = np.random.default_rng(3)
    ordered = np.concatenate([np.zeros((m, 1), np.int64), pts.reshape(-1, 3)[:m]], 1).astype(np.int32)
    seeds = (rng.random(m) < 0.15).astype(np.uint8)
    keys = np.where(rng.random(m) < 0.05, -1, 0)
    few = np.random.default_rng(4).permutation(3000)
    for limit in (0, 2, 3, 9):
        dist, owner = lines_of_five(ordered[:3000][few], keys[:3000], seeds[:3000], limit)
        rule = G.grow_numpy(ordered[:3000][few], keys[:3000], HOPS, limit, 6, seed_qv=seeds[:3000])
        assert np.array_equal(dist, rule[0]) and np.array_equal(owner, rule[1]) and (limit == 0 or (dist > 0).sum() > 500)
    coords = ordered[rng.permutation(m)]
    sc = scene_of(coords)
    assert sc.n[0] == m
    inv = rng.integers(0, m, 300_000)                                  # more vertices than one pass of the lift's grid
    dist, owner = lines_of_five(coords, keys, seeds, 3)
    selected, dist_full, err = G.lift_numpy(dist, len(inv), inv)
    want = dict(dist_qv=dist, owner_qv=owner, selected_full=selected, dist_full=dist_full, summary=G.summary_numpy(dist, selected, err))
    assert want["summary"]["max_dist"] == 3 and (dist < 0).sum() > 1000 and (dist > 0).sum() > 100_000
    for c in (6, 26):                                                  # under 26 the lines are still apart: the same distances
        same(grow_gpu(sc, keys=keys, seed_qv=seeds, inverse_map=inv, n_full=len(inv), limit=3, connectivity=c), want, c)


def test_line_of_600():
    coords, at = line(600, seed=9)
    sc = scene_of(coords)
    seeds = marks(600, {at[0]})
    for limit in (0, 1, 599, 1024):
        got, want = check(coords, sc, limit, seed_qv=seeds, n_full=600, limit=limit, connectivity=6)
        reach = min(limit, 599)
        assert np.array_equal(got["dist_qv"][at], np.where(np.arange(600) <= reach, np.arange(600), -1))
        assert got["summary"] == dict(seeds=1, reached=reach + 1, selected=reach + 1, max_dist=reach, err=0)
        assert set(got["owner_qv"][got["dist_qv"] >= 0].tolist()) == {at[0]}
    check(coords, sc, seed_qv=seeds, limit=599 * 1024, cost=G.METRIC_COST, connectivity=26)     # the same walk in metric units


def test_serpentine_cut_by_the_step_bound():
    coords = G.serpentine(40, 64)
    n = len(coords)
    assert n == 2599
    sc = scene_of(coords)
    start = row_at(coords, 0, 0, 0)
    seeds = marks(n, {start})
    got, want = check(coords, sc, seed_qv=seeds, limit=1024, connectivity=6)
    assert got["summary"]["reached"] == 1025 and got["summary"]["max_dist"] == 1024          # hops 0 .. 1024 and no further
    hops = G.grow_numpy(coords, None, HOPS, 1 << 20, 6, seed_qv=seeds)[0]                    # (the rule alone, without the bound)
    assert hops.max() == 2598 and np.array_equal(got["dist_qv"], np.where(hops <= 1024, hops, -1))
    assert (got["dist_qv"][hops == 1024] == 1024).all() and (got["dist_qv"][hops == 1025] == -1).all() and (hops == 1025).any()
    # the metric walk under 26 cuts the corners at the joints: two diagonal steps instead of two faces and a joint voxel
    got, want = check(coords, sc, seed_qv=seeds, limit=1024 * 1024, cost=G.METRIC_COST, connectivity=26)
    straight = check(coords, sc, seed_qv=seeds, limit=1024 * 1024, cost=G.METRIC_COST, connectivity=6)[0]
    both = (got["dist_qv"] >= 0) & (straight["dist_qv"] >= 0)
    far = both & (coords[:, 2] >= 2) & ~((coords[:, 1] == 63) & (coords[:, 2] == 2))      # (63, 2) lies straight above (63, 0)
    assert (got["dist_qv"][both] <= straight["dist_qv"][both]).all()
    assert far.sum() > 900 and (got["dist_qv"][far] < straight["dist_qv"][far]).all()
    assert got["summary"]["reached"] > straight["summary"]["reached"]


# ---------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("c", CONN)
def test_solid_cube(c):
    coords = cube(12)
    n = len(coords)
    sc = scene_of(coords)
    rng = np.random.default_rng(c)
    for k in (1, 2, 40):
        seeds = marks(n, rng.choice(n, k, replace=False))
        got, _ = check(coords, sc, (c, k), seed_qv=seeds, n_full=n, limit=7 * 1024, cost=G.METRIC_COST, connectivity=c)
        assert got["summary"]["seeds"] == k and len(set(got["owner_qv"][got["dist_qv"] >= 0].tolist())) == k
        got, _ = check(coords, sc, (c, k, "hops"), seed_qv=seeds, limit=5, connectivity=c)
    # hop costs and 40 seeds: many voxels are equally near to two seeds, and the smaller row owns them
    d = [G.grow_numpy(coords, None, HOPS, 5, c, seed_qv=marks(n, [s]))[0] for s in np.flatnonzero(seeds)]
    d = np.where(np.stack(d) < 0, 99, np.stack(d))
    assert ((d == d.min(0)).sum(0)[d.min(0) < 99] > 1).sum() > 100


def test_plates_apart_and_joined():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2)
    plate = lambda z: np.concatenate([np.zeros((36, 1), np.int64), g, np.full((36, 1), z)], 1)
    apart = np.concatenate([plate(0), plate(2)]).astype(np.int32)[np.random.default_rng(2).permutation(72)]
    seeds = marks(72, {row_at(apart, 0, 0, 0)})
    sc = scene_of(apart)
    for c in CONN:
        got, _ = check(apart, sc, seed_qv=seeds, limit=100, connectivity=c)
        assert (got["dist_qv"][apart[:, 3] == 0] >= 0).all() and (got["dist_qv"][apart[:, 3] == 2] == -1).all()     # nothing leaks
    joined = np.concatenate([apart, [[0, 5, 5, 1]]]).astype(np.int32)
    seeds = marks(73, {row_at(joined, 0, 0, 0)})
    sc = scene_of(joined)
    for c in CONN:
        got, _ = check(joined, sc, seed_qv=seeds, limit=100, connectivity=c)
        assert (got["dist_qv"] >= 0).all()
        bridge, far = got["dist_qv"][72], got["dist_qv"][joined[:, 3] == 2]
        assert (far > bridge).all()                                     # the far plate is reached only through the one voxel
        if c == 6:
            assert bridge == 11 and far.min() == 12 and far.max() == 22
        # a limit that ends on the bridge: the far plate stays out
        got, _ = check(joined, sc, seed_qv=seeds, limit=int(bridge), connectivity=c)
        assert got["dist_qv"][72] == bridge and (got["dist_qv"][joined[:, 3] == 2] == -1).all()


def test_the_limit_is_exact():
    coords = cube(5)
    sc = scene_of(coords)
    seeds = marks(125, {row_at(coords, 2, 2, 2)})
    edge = row_at(coords, 3, 3, 2)
    for limit, inside in ((1448, True), (1447, False)):
        got, _ = check(coords, sc, seed_qv=seeds, limit=limit, cost=G.METRIC_COST, connectivity=26)
        assert (got["dist_qv"][edge] == 1448) == inside and (got["dist_qv"][edge] == -1) != inside
        assert got["summary"]["reached"] == (1 + 6 + 12 if inside else 1 + 6)
    # under 6 the same voxel is two faces away
    assert check(coords, sc, seed_qv=seeds, limit=2048, cost=G.METRIC_COST, connectivity=6)[0]["dist_qv"][edge] == 2048


# ---------------------------------------------------------------------------------------------------- 3
def test_keys():
    coords = cube(8, seed=4)
    n = len(coords)
    sc = scene_of(coords)
    a, b = row_at(coords, 1, 1, 1), row_at(coords, 6, 6, 6)
    seeds = marks(n, {a, b})
    kw = dict(seed_qv=seeds, n_full=n, limit=12 * 1024, cost=G.METRIC_COST)
    # NULL against all zeros: the same bytes
    null, _ = check(coords, sc, **kw)
    zeros, _ = check(coords, sc, keys=np.zeros(n), **kw)
    for k in OUTPUTS + ("raw",):
        assert null[k].tobytes() == zeros[k].tobytes(), k
    # a mask that cuts the cube in two: the wall x = 4 cannot be walked on, each half is reached from its own seed only
    mask = np.where(coords[:, 1] == 4, -1, 0)
    got, _ = check(coords, sc, keys=mask, **kw)
    assert (got["dist_qv"][mask < 0] == -1).all() and (got["owner_qv"][coords[:, 1] < 4] == a).all() and (got["owner_qv"][coords[:, 1] > 4] == b).all()
    got, _ = check(coords, sc, keys=mask, **dict(kw, seed_qv=marks(n, {a})))
    assert (got["dist_qv"][coords[:, 1] > 4] == -1).all() and got["summary"]["reached"] == 4 * 64
    # labels of two objects: a walk stops at the border, whatever the labels' values are
    for labels in (np.where(coords[:, 3] < 3, 7, 2), np.where(coords[:, 3] < 3, 2 ** 31 - 1, 0)):
        got, _ = check(coords, sc, keys=labels, **dict(kw, seed_qv=marks(n, {a})))
        assert ((got["dist_qv"] >= 0) == (coords[:, 3] < 3)).all()
    # a seed on a voxel without a key is no seed and is not counted
    got, _ = check(coords, sc, keys=np.where(np.arange(n) == a, -1, 0), **kw)
    assert got["summary"]["seeds"] == 1 and got["dist_qv"][a] == -1 and got["owner_qv"][a] == -1
    got, _ = check(coords, sc, keys=np.full(n, -1), **kw)
    assert got["summary"] == dict(seeds=0, reached=0, selected=0, max_dist=0, err=0)


def test_seeds():
    coords = cube(9, seed=5)
    n = len(coords)
    sc = scene_of(coords)
    rng = np.random.default_rng(5)
    # several vertices share a voxel, and the voxels of the upper third have no vertex
    below = np.flatnonzero(coords[:, 3] < 6)
    inv = rng.choice(below, 3 * n)
    seed_full = marks(len(inv), rng.choice(len(inv), 8, replace=False))
    seed_qv = marks(n, rng.choice(n, 3, replace=False))
    kw = dict(n_full=len(inv), inverse_map=inv, limit=3 * 1024, cost=G.METRIC_COST)
    only_qv, _ = check(coords, sc, seed_qv=seed_qv, **kw)
    only_full, _ = check(coords, sc, seed_full=seed_full, **kw)
    both, _ = check(coords, sc, seed_qv=seed_qv, seed_full=seed_full, **kw)
    assert only_full["summary"]["seeds"] == len(set(inv[seed_full != 0].tolist())) > 3
    assert both["summary"]["seeds"] == len(set(inv[seed_full != 0].tolist()) | set(np.flatnonzero(seed_qv).tolist()))
    assert both["summary"]["reached"] > max(only_qv["summary"]["reached"], only_full["summary"]["reached"])
    # no seed at all: everything is -1 / 0 and the counts are 0
    for empty in (dict(seed_qv=np.zeros(n, np.uint8)), dict(seed_full=np.zeros(len(inv), np.uint8)),
                  dict(seed_qv=np.zeros(n, np.uint8), seed_full=np.zeros(len(inv), np.uint8))):
        got, _ = check(coords, sc, **empty, **kw)
        assert got["summary"] == dict(seeds=0, reached=0, selected=0, max_dist=0, err=0)
        assert (got["dist_qv"] == -1).all() and (got["owner_qv"] == -1).all() and not got["selected_full"].any() and (got["dist_full"] == -1).all()
    # inverse-map entries of -1 and n: the error bit; those vertices are 0 / -1, and as seeds they are ignored
    bad = inv.copy()
    bad[[0, 7]] = [-1, n]
    seed_full[[0, 7, 9]] = 1
    got, _ = check(coords, sc, seed_full=seed_full, **dict(kw, inverse_map=bad))
    assert got["summary"]["err"] == G.BAD_INDEX and (got["dist_full"][[0, 7]] == -1).all() and not got["selected_full"][[0, 7]].any()
    assert got["dist_full"][9] == 0
    only_bad = marks(len(inv), {0, 7})
    got, _ = check(coords, sc, seed_full=only_bad, **dict(kw, inverse_map=bad))
    assert got["summary"] == dict(seeds=0, reached=0, selected=0, max_dist=0, err=G.BAD_INDEX)


# ---------------------------------------------------------------------------------------------------- 4
def _random_walk(rng, m):
    """At most m distinct voxels of a random walk with 26-steps, cut into one to three blobs 40 voxels apart."""
    pts = rng.integers(-1, 2, (m, 3)).cumsum(0)
    pts[:, 0] += np.arange(m) * int(rng.integers(1, 4)) // m * 40
    pts = np.unique(pts, axis=0)
    return np.concatenate([np.zeros((len(pts), 1), np.int64), pts], 1).astype(np.int32)[rng.permutation(len(pts))]


@pytest.mark.parametrize("seed", range(20))
def test_random_blobs(seed):
    rng = np.random.default_rng(100 + seed)
    size = int(rng.integers(1, 5001)) if seed else 1
    if seed % 2:
        sc0 = make_scene(max(size, 200), seed=seed)
        coords = sc0["coords"][rng.permutation(len(sc0["coords"]))][:size]
        coords = np.ascontiguousarray(coords, np.int32)
    else:
        coords = _random_walk(rng, size)
    n = len(coords)
    sc = scene_of(coords)
    keys = [None, rng.integers(-1, 3, n), np.where(rng.random(n) < 0.1, -1, 0)][seed % 3]
    cost = G.METRIC_COST if seed % 4 < 2 else tuple(int(x) for x in rng.integers(1, 9, 3))
    limit = int(rng.integers(0, 30 * min(cost)))
    inv = rng.integers(0, n, int(rng.integers(0, 2 * n + 2)))
    kw = dict(keys=keys, cost=cost, limit=limit, connectivity=int(rng.choice(CONN)), n_full=len(inv),
              inverse_map=inv if len(inv) else None)
    if len(inv) and seed % 2:
        kw["seed_full"] = (rng.random(len(inv)) < 4.0 / len(inv)).astype(np.uint8)
    if "seed_full" not in kw or seed % 3 == 0:
        kw["seed_qv"] = (rng.random(n) < min(1.0, 5.0 / n)).astype(np.uint8)
    got, want = check(coords, sc, (seed, n), **kw)
    print(f"seed {seed}: n={n} n_full={len(inv)} limit={limit} cost={cost} connectivity={kw['connectivity']} {got['summary']}")


# ---------------------------------------------------------------------------------------------------- 5
def test_outputs_omitted_and_twice_the_same_bytes():
    sc0 = make_scene(3000, seed=5)
    coords = np.ascontiguousarray(sc0["coords"], np.int32)
    n = len(coords)
    sc = scene_of(coords)
    rng = np.random.default_rng(8)
    inv = rng.integers(0, n, 2 * n + 3)
    kw = dict(keys=sc0["labels"].astype(np.int64), seed_qv=marks(n, rng.choice(n, 12, replace=False)), n_full=len(inv),
              inverse_map=inv, limit=12 * 1024, cost=G.METRIC_COST, connectivity=26)
    first, want = check(coords, sc, **kw)
    assert want["summary"]["reached"] > 200 and want["summary"]["selected"] > 400
    ws = first["workspace"]
    for name in OUTPUTS:
        check(coords, sc, name, omit=(name,), workspace=ws, **kw)       # (the workspace of the call before, as it was left)
    check(coords, sc, omit=OUTPUTS, workspace=ws, **kw)                 # the summary alone
    second = grow_gpu(sc, workspace=ws, **kw)
    for k in OUTPUTS + ("raw",):
        assert first[k].tobytes() == second[k].tobytes(), k


def test_refusals():
    coords = cube(3)
    n = 27
    sc = scene_of(coords)
    seed = _dev(marks(n, {0}), np.uint8)
    keys = _dev(np.zeros(n), np.int32)
    inv = _dev(np.arange(n), np.int64)
    ws = V.grow_workspace(n, DEV)
    # the wrapper's operand checks
    good = dict(scene=sc, n_full=n, seed_qv=seed, inverse_map=inv, limit=2)
    assert len(V.grow_voxels(**good)) == 6
    for bad in (dict(keys=keys[:5]), dict(keys=keys.long()), dict(keys=keys.cpu()), dict(seed_qv=seed[:3]), dict(seed_qv=seed.int()),
                dict(seed_full=seed[:3]), dict(inverse_map=inv[:9]), dict(inverse_map=inv.int()), dict(dist_qv=keys[:3]),
                dict(owner_qv=keys.long()), dict(selected_full=keys), dict(dist_full=seed), dict(workspace=ws[:512]),
                dict(workspace=ws[8:]), dict(summary=torch.zeros(8, dtype=torch.uint8, device=DEV)), dict(connectivity=8),
                dict(limit=1025, cost=HOPS), dict(limit=1025 * 1024), dict(cost=(0, 1, 1)), dict(n_full=-1), dict(scene=None), dict(seed_qv=None)):
        with pytest.raises(ValueError):
            V.grow_voxels(**dict(good, **bad))
    # the library's own checks: nothing is launched, nothing is written
    outs = dict(dist_qv_dev=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                owner_qv_dev=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                selected_full_dev=torch.full((n,), FILL, dtype=torch.uint8, device=DEV),
                dist_full_dev=torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV),
                summary_dev=torch.full((32,), FILL, dtype=torch.uint8, device=DEV))

    def grow(**kw):
        a = L.GrowVoxelsArgs()
        base = dict(scene=sc.handle.value, n=n, keys_dev=keys, seed_qv_dev=seed, inverse_map_dev=inv, n_full=n, workspace_dev=ws,
                    workspace_bytes=ws.numel(), connectivity=26, limit=2, cost=(1, 1, 1), **outs)
        for k, v in dict(base, **kw).items():
            if k == "cost":
                a.cost[:] = v
            else:
                setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_grow_voxels", byref(a), None)

    assert status("a3d_grow_voxels", None, None) == INVALID
    for bad in (dict(scene=None), dict(n=26), dict(n=28), dict(connectivity=7), dict(connectivity=0), dict(cost=(0, 1, 1)),
                dict(cost=(1, 65537, 1)), dict(cost=(1, 1, -1)), dict(limit=-1), dict(limit=(1 << 30) + 1), dict(limit=1025),
                dict(limit=1025 * 1024, cost=G.METRIC_COST), dict(seed_qv_dev=None), dict(summary_dev=None), dict(n_full=-1),
                dict(workspace_dev=None), dict(workspace_bytes=ws.numel() - 1), dict(workspace_dev=ws.data_ptr() + 8)):
        assert grow(**bad) == INVALID, bad
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert (t.cpu().numpy() == (SENTINEL if t.dtype == torch.int32 else FILL)).all(), k
    assert grow() == OK and grow(limit=1024) == OK and grow(seed_qv_dev=None, seed_full_dev=seed) == OK
    assert grow(limit=1024 * 1024 + 1023, cost=G.METRIC_COST, keys_dev=None) == OK
    torch.cuda.synchronize()
    want = G.grow_all(coords, None, G.METRIC_COST, 1024 * 1024 + 1023, 26, seed_qv=marks(n, {0}), n_full=n)
    assert np.array_equal(outs["dist_qv_dev"].cpu().numpy(), want["dist_qv"])
    assert V.read_grow_summary(outs["summary_dev"].cpu().numpy()) == want["summary"]
