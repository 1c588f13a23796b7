"""-m gpu: connected components under a similarity of normals and colours, and the vote that snaps a labelling to a
partition (a3d_similar_pieces, a3d_vote_pieces in csrc/session_pieces.hip; view.similar_pieces, view.vote_pieces).  The rules
are restated in ``patches_rule.py``: the predicates round every fp32 operation on its own and the rest is integer, so every
comparison is by equality.

1  sizes at their edges (1, 2, 255, 256, 257 voxels; one full pass of the grid + 77 rows); which offsets each connectivity
   joins; batch samples that touch; the serpentine (deep trees)
2  the predicates: two plates at a right angle, a quarter cylinder (chain against the reference test), colour alone on a
   checkerboard and a ramp, zero and NaN normals, `oriented`
3  synthetic scenes, permuted: keys and similarity together, clicks, every record field, max_out below the count, the lift
   and an inverse-map entry out of range, two calls bit-identical; with neither array the bytes of a3d_label_pieces
4  the vote: the known answers, a noisy labelling at capacities that do and do not fit, a label out of range -- fed once by
   a3d_similar_pieces and once by a3d_label_pieces
5  the wrappers' and the library's refusals
"""
import numpy as np
import pytest
import torch

import patches_rule as P
from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from pieces_rule import BAD_INDEX, PIECE, lift_numpy, noisy, offsets, serpentine
from session_kit import DEV, _dev, byref, status

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -77
CONN = (6, 18, 26)
INVALID, OK = -1, 0
cosd = lambda deg: F(np.cos(np.radians(deg)))


# ---------------------------------------------------------------------------------------------------- the adaptors
def scene_of(coords4):
    return Scene(torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(DEV))


def similar_gpu(scene, keys=None, normals=None, feats=None, connectivity=26, click_rows=(), inverse_map=None, max_out=1024,
                workspace=None, **settings):
    """view.similar_pieces, numpy in / numpy out; every output starts as a sentinel."""
    n = scene.n[0]
    piece = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    records = torch.full((max_out * PIECE.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    kw = {}
    if inverse_map is not None:
        kw = dict(inverse_map=_dev(inverse_map, np.int64),
                  piece_full=torch.full((len(inverse_map),), SENTINEL, dtype=torch.int32, device=DEV))
    got = V.similar_pieces(scene, None if keys is None else _dev(keys, np.int32), None if normals is None else _dev(normals, F),
                           None if feats is None else _dev(feats, F), connectivity=connectivity, click_rows=click_rows,
                           piece_qv=piece, records=records, count=count, workspace=workspace, **settings, **kw)
    assert got[0] is piece and got[2] is records and got[3] is count
    raw = records.cpu().numpy()
    rec, n_pieces, err = V.read_pieces(raw, count.cpu().numpy())
    return dict(piece=piece.cpu().numpy(), full=None if got[1] is None else got[1].cpu().numpy(), records=rec, n=n_pieces,
                err=err, raw=raw, piece_dev=piece, workspace=got[4])


def same_as_rule(got, coords4, keys=None, normals=None, feats=None, connectivity=26, click_rows=(), what=None, **settings):
    piece, rec = P.similar_numpy(coords4, keys, normals, feats, connectivity, click_rows=click_rows, **settings)
    assert got["piece"].dtype == np.int32 and np.array_equal(got["piece"], piece), what
    assert got["n"] == len(rec) and got["err"] == 0, (what, got["n"], len(rec))
    kept = rec[:len(got["records"])]
    for field in PIECE.names:                    # root, key, voxels, clicked, lo, hi
        assert np.array_equal(got["records"][field], kept[field]), (what, field)
    return piece, rec


def check(coords4, scene, keys=None, normals=None, feats=None, connectivity=26, click_rows=(), what=None, **settings):
    got = similar_gpu(scene, keys, normals, feats, connectivity, click_rows, **settings)
    return got, same_as_rule(got, coords4, keys, normals, feats, connectivity, click_rows, what, **settings)


def line(m, seed):
    """A shuffled line of m voxels along x; ``at[x]`` = the row at position x."""
    rng = np.random.default_rng(seed)
    coords = np.stack([np.zeros(m), np.arange(m), np.full(m, 2), np.full(m, -1)], 1).astype(np.int32)[rng.permutation(m)]
    at = np.empty(m, np.int64)
    at[coords[:, 1]] = np.arange(m)
    return coords, at


def turning(angles_deg):
    """Unit normals (sin t, 0, cos t), fp32."""
    t = np.radians(np.asarray(angles_deg, np.float64))
    return np.stack([np.sin(t), np.zeros_like(t), np.cos(t)], 1).astype(F)


def plate(nx, ny, z=0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g, np.full((len(g), 1), z)], 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_sizes_at_their_edges(m):
    coords, at = line(m, seed=m)
    sc = scene_of(coords)
    rng = np.random.default_rng(m)
    # normals turn 5 degrees a voxel with a jump of 40 every 50 voxels; colours in four levels
    normals = turning(5.0 * coords[:, 1] + 40.0 * (coords[:, 1] // 50))
    feats = (rng.integers(0, 4, (m, 3)) / 8).astype(F)
    keys = np.where(coords[:, 1] % 97 == 96, -1, coords[:, 1] // 120)
    for c in (6, 26):
        _, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=cosd(6), what=(m, c))
        assert len(rec) == (m - 1) // 50 + 1
        check(coords, sc, keys, normals, feats, c, [0, m - 1, m], cos_min=cosd(6), tol2=F(0.05), what=(m, c))
        check(coords, sc, None, None, feats, c, tol2=F(0.02), oriented=True, what=(m, c))
        check(coords, sc, keys, normals, None, c, cos_min=F(-1), ref_normal=turning([20.0])[0], ref_cos_min=cosd(31), what=(m, c))


def nsim_rows(a, b, c):
    dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]                     # fp32 arrays: one rounding per operation
    return np.abs(dot) >= c


def fsim_rows(a, b, t):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= t


def lines_of_five(coords4, keys, normals, feats, cos_min, tol2):
    """The rule in CLOSED FORM for voxels (x in 0..4, y, z) whose lines along x never touch: a line falls into runs of
    consecutive voxels that are there, hold a key >= 0, and pass both predicates with their left neighbour; a run is named by
    its smallest row.  Vectorised over the lines, so half a million voxels take a second."""
    n = len(coords4)
    _, lid = np.unique(coords4[:, 2:4], axis=0, return_inverse=True)
    lid = lid.reshape(-1)
    row = np.full((lid.max() + 1, 5), -1, np.int64)
    row[lid, coords4[:, 1]] = np.arange(n)
    ok = (row >= 0) & (np.asarray(keys)[row] >= 0)
    run = np.zeros(row.shape, np.int64)
    for p in range(1, 5):
        a, b = row[:, p - 1], row[:, p]
        joined = ok[:, p - 1] & ok[:, p] & (np.asarray(keys)[a] == np.asarray(keys)[b]) & nsim_rows(normals[a], normals[b], cos_min) & \
            fsim_rows(feats[a], feats[b], tol2)
        run[:, p] = run[:, p - 1] + ~joined
    name = np.full((len(row), 5), n, np.int64)
    lines = np.broadcast_to(np.arange(len(row)).reshape(-1, 1), row.shape)
    np.minimum.at(name, (lines[ok], run[ok]), row[ok])
    piece = np.full(n, -1, np.int32)
    piece[row[ok]] = name[lines[ok], run[ok]]
    return piece


def test_one_full_grid_pass_and_77_rows():
    """2048 workgroups x 256 rows is one pass of the hook's grid: 524 365 voxels take a second pass of 77 rows.  Lines of five
    voxels, two apart in y and z (never neighbours, under any connectivity), the last one cut short.  The rule is evaluated in
    closed form here (``lines_of_five``), which is first held to ``patches_rule.py`` on the first 3 000 voxels."""
    m = 2048 * 256 + 77
    side = 324
    assert side * side * 5 >= m
    yz = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 1, 2) * 2
    pts = np.concatenate([np.broadcast_to(np.arange(5).reshape(1, 5, 1), (side * side, 5, 1)), np.broadcast_to(yz, (side * side, 5, 2))], 2)
    rng = np.random.default_rng(3)
    ordered = np.concatenate([np.zeros((m, 1), np.int64), pts.reshape(-1, 3)[:m]], 1).astype(np.int32)
    keys = np.where(rng.random(m) < 0.05, -1, 0)
    normals = turning(rng.choice([0.0, 8.0, 16.0, 60.0], m))
    feats = (rng.integers(0, 3, (m, 3)) / 32).astype(F)
    cos_min, tol2 = cosd(10), F(0.006)
    few = np.random.default_rng(4).permutation(3000)
    piece = lines_of_five(ordered[:3000][few], keys[:3000][few], normals[:3000][few], feats[:3000][few], cos_min, tol2)
    rule = P.similar_numpy(ordered[:3000][few], keys[:3000][few], normals[:3000][few], feats[:3000][few], 6, cos_min, tol2)[0]
    assert np.array_equal(piece, rule) and 1000 < len(np.unique(piece)) < 2700
    p = rng.permutation(m)
    coords, keys, normals, feats = ordered[p], keys[p], normals[p], feats[p]
    sc = scene_of(coords)
    assert sc.n[0] == m
    want = lines_of_five(coords, keys, normals, feats, cos_min, tol2)
    inv = rng.integers(0, m, 300_000)                                  # more vertices than one pass of the lift's grid
    for c in (6, 26):                                                  # under 26 the lines are still apart: the same pieces
        got = similar_gpu(sc, keys, normals, feats, c, inverse_map=inv, max_out=8, cos_min=cos_min, tol2=tol2)
        assert np.array_equal(got["piece"], want), c
        roots = np.flatnonzero(want == np.arange(m))
        assert got["n"] == len(roots) and got["records"]["root"].tolist() == roots[:8].tolist() and got["err"] == 0
        assert np.array_equal(got["full"], want[inv])


def test_offsets_each_connectivity_joins():
    up, tilted, side = turning([0.0])[0], turning([10.0])[0], turning([90.0])[0]
    joined = {c: 0 for c in CONN}
    for k in range(27):
        d = (k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1)
        if d == (0, 0, 0):
            continue
        coords = np.array([[0, 5, 5, 5], [0, 5 + d[0], 5 + d[1], 5 + d[2]]], np.int32)
        sc = scene_of(coords)
        for c in CONN:
            admitted = d in offsets(c)
            got = similar_gpu(sc, None, np.stack([up, tilted]), None, c, cos_min=cosd(15))
            assert got["piece"].tolist() == ([0, 0] if admitted else [0, 1]), (d, c)
            joined[c] += admitted
            assert similar_gpu(sc, None, np.stack([up, side]), None, c, cos_min=cosd(15))["piece"].tolist() == [0, 1]
            assert similar_gpu(sc, [3, 4], np.stack([up, up]), None, c, cos_min=cosd(15))["piece"].tolist() == [0, 1]
    assert joined == {6: 6, 18: 18, 26: 26}


def test_two_batch_samples_that_touch():
    # equal xyz in two batch samples, and neighbours across samples: never joined, however similar
    coords = np.array([[0, 1, 1, 1], [0, 2, 1, 1], [1, 1, 1, 1], [1, 2, 1, 1], [1, 3, 2, 2]], np.int32)
    sc = scene_of(coords)
    normals, feats = np.tile(turning([0.0]), (5, 1)), np.full((5, 3), 0.5, F)
    for c in CONN:
        got, _ = check(coords, sc, None, normals, feats, c, [3], cos_min=F(1), tol2=F(0))
        assert got["piece"].tolist() == [0, 0, 2, 2, 2 if c == 26 else 4]
        assert got["records"]["clicked"].tolist() == ([0, 1] if c == 26 else [0, 1, 0])


def test_serpentine():
    coords = serpentine()
    n = len(coords)
    assert n == 2599
    sc = scene_of(coords)
    normals, feats = np.tile(turning([30.0]), (n, 1)), np.full((n, 3), 0.25, F)
    for c in (6, 26):
        got = similar_gpu(sc, None, normals, feats, c, cos_min=cosd(1), tol2=F(0))
        assert (got["piece"] == 0).all() and got["n"] == 1            # one piece, named by the smallest row
        assert got["records"]["voxels"].tolist() == [2599] and got["records"]["hi"].tolist() == [[63, 78, 0]]
    # cut where the normal jumps: the lines come apart at their joints
    normals = turning(np.where(coords[:, 2] % 2 == 1, 80.0, 0.0))
    check(coords, sc, None, normals, None, 6, cos_min=cosd(15))
    again = similar_gpu(sc, None, normals, None, 6, cos_min=cosd(15))
    assert again["n"] == 40 + 39 and np.array_equal(again["raw"], similar_gpu(sc, None, normals, None, 6, cos_min=cosd(15))["raw"])


# ---------------------------------------------------------------------------------------------------- 2
def test_two_plates_at_a_right_angle():
    floor = plate(8, 8, 0)
    wall = floor[:, [0, 3, 2, 1]].copy()                               # x = 0, z = 0..7
    wall = wall[wall[:, 3] > 0]
    coords = np.concatenate([floor, wall])
    normals = np.concatenate([np.tile([0, 0, 1], (len(floor), 1)), np.tile([1, 0, 0], (len(wall), 1))]).astype(F)
    p = np.random.default_rng(0).permutation(len(coords))
    coords, normals = coords[p], normals[p]
    sc = scene_of(coords)
    for c in CONN:
        got, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=cosd(15))
        assert sorted(rec["voxels"].tolist()) == [56, 64]              # two patches at 15 degrees
        assert len(set(piece[normals[:, 2] == 1].tolist())) == 1
        got, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=F(0))
        assert rec["voxels"].tolist() == [120]                         # one at cos_min = 0: the dot of the two is exactly 0
    # `oriented`: the wall turned round joins the floor's opposite side only unoriented
    flipped = np.where(normals[:, 2:3] == 1, normals, -normals)
    _, (_, rec) = check(coords, sc, None, flipped * np.where(coords[:, 2:3] % 2 == 0, 1, -1).astype(F), None, 6, cos_min=cosd(15))
    assert sorted(rec["voxels"].tolist()) == [56, 64]
    _, (_, rec) = check(coords, sc, None, flipped * np.where(coords[:, 2:3] % 2 == 0, 1, -1).astype(F), None, 6, cos_min=cosd(15),
                        oriented=True)
    assert len(rec) == 16                                              # stripes along y: 8 on the floor, 8 on the wall


def test_quarter_cylinder():
    # 19 columns of 6 voxels; the normal turns 5 degrees per column, 0 .. 90
    coords = plate(19, 6)
    p = np.random.default_rng(1).permutation(len(coords))
    coords = coords[p]
    normals = turning(5.0 * coords[:, 1])
    sc = scene_of(coords)
    _, (piece, rec) = check(coords, sc, None, normals, None, 26, cos_min=cosd(6))
    assert rec["voxels"].tolist() == [114]                             # chain: one patch, though its ends are at right angles
    _, (piece, rec) = check(coords, sc, None, normals, None, 26, cos_min=cosd(4))
    assert len(rec) == 19
    ref = turning([45.0])[0]
    for deg, widths in ((15.0, (5, 7)), (17.5, (7, 7)), (2.0, (1, 1))):  # (at exactly 15 degrees the two border columns may round either way)
        got, (piece, rec) = check(coords, sc, None, normals, None, 26, cos_min=F(-1), ref_normal=ref, ref_cos_min=cosd(deg))
        columns = np.unique(coords[piece >= 0, 1])
        assert len(rec) == 1 and widths[0] <= len(columns) <= widths[1] and columns.tolist() == list(range(columns[0], columns[-1] + 1))
        assert 9 in columns and rec["voxels"][0] == 6 * len(columns) and (piece[np.isin(coords[:, 1], columns, invert=True)] == -1).all()
    # both: the chain at 4 degrees breaks every column, the reference keeps the band
    _, (piece, rec) = check(coords, sc, None, normals, None, 26, cos_min=cosd(4), ref_normal=ref, ref_cos_min=cosd(17.5))
    assert rec["voxels"].tolist() == [6] * 7


def test_colour_alone():
    board = plate(8, 8)
    board = board[np.random.default_rng(2).permutation(64)]
    feats = np.repeat(((board[:, 1] + board[:, 2]) % 2).reshape(-1, 1), 3, 1).astype(F)
    sc = scene_of(board)
    _, (_, rec) = check(board, sc, None, None, feats, 6, tol2=F(0.01))
    assert len(rec) == 64                                              # faces only: no neighbour of a field has its colour
    _, (_, rec) = check(board, sc, None, None, feats, 26, tol2=F(0.01))
    assert rec["voxels"].tolist() == [32, 32]                          # through the corners: the two colours
    _, (_, rec) = check(board, sc, None, None, feats, 6, tol2=F(3))
    assert rec["voxels"].tolist() == [64]                              # q = 3 exactly: AT the tolerance
    _, (_, rec) = check(board, sc, None, None, feats, 6, tol2=np.nextafter(F(3), F(0)))
    assert len(rec) == 64
    _, (piece, rec) = check(board, sc, None, None, feats, 26, tol2=F(0), ref_feat=[1, 1, 1], ref_tol2=F(0.5))
    assert rec["voxels"].tolist() == [32] and (piece[feats[:, 0] == 0] == -1).all()
    # a ramp: steps of 1/64 with one of 1/4 every 16 voxels; tol = 1/32 in one channel
    coords, at = line(64, seed=5)
    level = coords[:, 1] / 64 + (coords[:, 1] // 16) / 4
    feats = np.stack([level, np.zeros(64), np.ones(64)], 1).astype(F)
    sc = scene_of(coords)
    _, (_, rec) = check(coords, sc, None, None, feats, 6, tol2=F(1 / 32) ** 2)
    assert rec["voxels"].tolist() == [16] * 4
    _, (_, rec) = check(coords, sc, None, None, feats, 6, tol2=F(0.3) ** 2)
    assert rec["voxels"].tolist() == [64]
    _, (_, rec) = check(coords, sc, None, None, feats, 6, tol2=F(1 / 128) ** 2)
    assert len(rec) == 64


def test_zero_and_nan_normals():
    coords = plate(6, 6)[np.random.default_rng(3).permutation(36)]
    normals = np.tile(turning([0.0]), (36, 1))
    zero, nan = (coords[:, 1] == 2) & (coords[:, 2] < 3), (coords[:, 1] == 4) & (coords[:, 2] >= 3)
    normals[zero], normals[nan, 1] = 0, np.nan
    sc = scene_of(coords)
    for c in CONN:
        _, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=cosd(15))
        # no special case: a zero or NaN normal is admissible (its key is >= 0) and joins nobody
        assert (rec["voxels"] == 1).sum() == 6 and rec["voxels"].max() == 30 and (piece >= 0).all()
        _, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=F(0))
        assert (rec["voxels"] == 1).sum() == 3 and rec["voxels"].max() == 33       # a zero's dot is 0 >= 0; a NaN still fails
        _, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=F(-1), oriented=True)
        assert (rec["voxels"] == 1).sum() == 3
        _, (piece, rec) = check(coords, sc, None, normals, None, c, cos_min=cosd(15), ref_normal=[0, 0, 1], ref_cos_min=cosd(15))
        assert (piece[zero | nan] == -1).all() and rec["voxels"].tolist() == [30]
        check(coords, sc, None, normals, np.where(nan.reshape(-1, 1), np.nan, np.full((36, 3), 0.5)).astype(F), c, cos_min=F(0), tol2=F(1))


# ---------------------------------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def synthetic():
    sc = make_scene(3000, seed=5)
    rng = np.random.default_rng(5)
    p = rng.permutation(len(sc["coords"]))
    coords, labels = sc["coords"][p], sc["labels"][p].astype(np.int64)
    n = len(coords)
    # normals: a smooth field of the position plus a few outliers; colours: per object, with noise
    angle = 4.0 * coords[:, 1] + 7.0 * coords[:, 2] + np.where(rng.random(n) < 0.05, 90.0, 0.0)
    normals = turning(angle)
    feats = (np.stack([labels % 3, (labels // 3) % 3, labels % 2], 1) / 4 + rng.normal(scale=0.02, size=(n, 3))).astype(F)
    return coords, labels, scene_of(coords), normals, feats


@pytest.mark.parametrize("c", CONN)
def test_synthetic_scene(synthetic, c):
    coords, labels, sc, normals, feats = synthetic
    n = len(coords)
    rng = np.random.default_rng(n + c)
    clicks = rng.integers(0, n, 40).tolist() + [-1, n, 2 ** 31 - 1]
    holes = np.where(rng.random(n) < 0.1, -1, noisy(labels, seed=n))
    settings = dict(cos_min=cosd(12), tol2=F(0.1) ** 2)
    got, (piece, rec) = check(coords, sc, holes, normals, feats, c, clicks, what=("both", c), **settings)
    assert rec["clicked"].any() and not rec["clicked"].all() and (piece[holes < 0] == -1).all() and len(rec) > 50
    print(f"n={n} connectivity={c}: {len(rec)} patches, {(rec['voxels'] == 1).sum()} singletons, largest {rec['voxels'].max()}")
    check(coords, sc, labels, normals, None, c, clicks, what=("normals", c), cos_min=cosd(12), oriented=True)
    check(coords, sc, None, None, feats, c, what=("colours", c), tol2=F(0.1) ** 2)
    check(coords, sc, holes, normals, feats, c, clicks, what=("reference", c), ref_normal=normals[7], ref_cos_min=cosd(40),
          ref_feat=feats[7], ref_tol2=F(0.6) ** 2, **settings)
    # two calls give the same bytes; a smaller max_out reports the true count and writes the first records
    first = similar_gpu(sc, holes, normals, feats, c, clicks, **settings)
    assert np.array_equal(first["raw"], got["raw"]) and np.array_equal(first["piece"], got["piece"])
    few = similar_gpu(sc, holes, normals, feats, c, clicks, max_out=7, **settings)
    assert few["n"] == first["n"] > 7 and len(few["records"]) == 7
    assert np.array_equal(few["records"], first["records"][:7]) and (few["raw"][7 * 40:] == 0x5a).all()
    none = similar_gpu(sc, holes, normals, feats, c, clicks, max_out=0, **settings)
    assert none["n"] == first["n"] and np.array_equal(none["piece"], first["piece"])
    # the lift, and an inverse-map entry out of range
    inv = rng.integers(0, n, 2 * n + 3)
    got = similar_gpu(sc, holes, normals, feats, c, inverse_map=inv, **settings)
    want, err = lift_numpy(got["piece"], inv, SENTINEL)
    assert err == 0 and got["err"] == 0 and np.array_equal(got["full"], want) and np.array_equal(got["piece"], first["piece"])
    inv[[0, n, 2 * n + 2]] = [n, -1, 2 ** 40]
    got = similar_gpu(sc, holes, normals, feats, c, inverse_map=inv, **settings)
    want, err = lift_numpy(got["piece"], inv, SENTINEL)
    assert err == BAD_INDEX == got["err"] and np.array_equal(got["full"], want) and (got["full"][[0, n, 2 * n + 2]] == SENTINEL).all()
    # no key at all: no piece
    got = similar_gpu(sc, np.full(n, -1), normals, feats, c, **settings)
    assert got["n"] == 0 and (got["piece"] == -1).all() and (got["raw"] == 0x5a).all()


@pytest.mark.parametrize("c", CONN)
def test_neither_array_is_label_pieces(synthetic, c):
    coords, labels, sc, _, _ = synthetic
    n = len(coords)
    keys = np.where(np.random.default_rng(c).random(n) < 0.1, -1, noisy(labels, seed=c))
    clicks = [0, 5, n - 1, n]
    inv = _dev(np.random.default_rng(1).integers(0, n, n + 9), np.int64)
    outs = []
    for call in (V.label_pieces, V.similar_pieces):
        piece = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
        full = torch.full((n + 9,), SENTINEL, dtype=torch.int32, device=DEV)
        records = torch.full((20 * PIECE.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
        count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
        call(sc, _dev(keys, np.int32), connectivity=c, click_rows=clicks, inverse_map=inv, piece_qv=piece, piece_full=full,
             records=records, count=count)
        outs.append([t.cpu().numpy() for t in (piece, full, records, count)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert outs[0][3][0] > 20                                          # (the record list overflowed in both, alike)
    # keys = NULL is keys = 0
    zeros, null = similar_gpu(sc, np.zeros(n), connectivity=c), similar_gpu(sc, None, connectivity=c)
    assert np.array_equal(zeros["piece"], null["piece"]) and np.array_equal(zeros["raw"], null["raw"]) and null["n"] >= 1
    assert (null["records"]["key"] == 0).all()


# ---------------------------------------------------------------------------------------------------- 4
def vote_gpu(scene, source, keys, labels, min_voxels, share, click_rows=(), n_classes=256, capacity=64, normals=None):
    """The partition of ``keys`` by label_pieces or by similar_pieces (with equal normals everywhere: the same partition), then
    view.vote_pieces with that call's workspace: (labels_out, summary dict, piece)."""
    n = scene.n[0]
    ws = V.vote_workspace(n, DEV, capacity, n_classes)
    if source == "label":
        piece = V.label_pieces(scene, _dev(keys, np.int32), 26, workspace=ws)[0]
    else:
        piece = V.similar_pieces(scene, _dev(keys, np.int32), _dev(np.tile(turning([0.0]), (n, 1)) if normals is None else normals, F),
                                 cos_min=cosd(15), workspace=ws)[0]
    lab = _dev(labels, np.int32)
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    summary = torch.full((V.VOTE_SUMMARY.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
    got = V.vote_pieces(scene, lab, piece, ws, min_voxels, share, click_rows, n_classes, capacity, labels_out=out, summary=summary)
    assert got[0] is out and got[1] is summary
    return out.cpu().numpy(), V.read_vote_summary(summary.cpu().numpy()), piece.cpu().numpy()


def same_vote(scene, source, keys, labels, min_voxels, share, click_rows=(), n_classes=256, capacity=64, normals=None):
    got, summary, piece = vote_gpu(scene, source, keys, labels, min_voxels, share, click_rows, n_classes, capacity, normals)
    want, rule = P.vote_numpy(piece, labels, min_voxels, share, click_rows, n_classes, capacity)
    assert summary == rule, (summary, rule)
    assert (got == SENTINEL).all() if want is None else np.array_equal(got, want)
    return got, summary


@pytest.mark.parametrize("source", ["label", "similar"])
def test_vote_known_answers(source):
    # three runs of 6, 6 and 3 voxels along x, a voxel apart, and a voxel without a key: pieces 0, 6, 12 and none
    xs = list(range(0, 6)) + list(range(7, 13)) + list(range(14, 17)) + [18]
    coords = np.array([[0, x, 0, 0] for x in xs], np.int32)
    sc = scene_of(coords)
    keys = np.array([0] * 15 + [-1])
    piece = vote_gpu(sc, source, keys, np.zeros(16), 1, (1, 1))[2]
    assert piece.tolist() == [0] * 6 + [6] * 6 + [12] * 3 + [-1]
    # a tie goes to the lowest label
    labels = np.array([5, 5, 5, 2, 2, 2] + [1] * 6 + [7, 7, 4] + [9])
    out, s = same_vote(sc, source, keys, labels, 3, (1, 2))
    assert out.tolist() == [2] * 6 + [1] * 6 + [7] * 3 + [9] and s["relabelled_voxels"] == 4 and s["uniform_pieces"] == 1
    # a share of exactly num / den passes, one vote fewer fails
    labels = np.array([3, 3, 3, 3, 8, 8] + [3, 3, 3, 8, 8, 8] + [0] * 4)
    out, s = same_vote(sc, source, keys, labels, 4, (2, 3))
    assert out.tolist() == [3] * 6 + [3, 3, 3, 8, 8, 8] + [0] * 4 and s["below_share_pieces"] == 1 and s["eligible_pieces"] == 2
    out, s = same_vote(sc, source, keys, labels, 4, (65536, 65536))
    assert np.array_equal(out, labels) and s["below_share_pieces"] == 2
    # a blocking click
    for clicks, blocked in (([4], True), ([0], False), ([4, 0], True), ([-1, 99, 2 ** 31 - 1], False), ([15], False)):
        out, s = same_vote(sc, source, keys, labels, 6, (2, 3), clicks)
        assert (out[4] == 8) == blocked and s["blocked_pieces"] == int(blocked)
    # a piece below min_voxels
    labels = np.array([1] * 12 + [7, 7, 4, 0])
    out, s = same_vote(sc, source, keys, labels, 4, (1, 2))
    assert np.array_equal(out, labels) and s["eligible_pieces"] == 2
    out, s = same_vote(sc, source, keys, labels, 3, (1, 2))
    assert out[14] == 7
    # overflow writes nothing
    out, s = same_vote(sc, source, keys, labels, 3, (1, 2), capacity=2)
    assert (out == SENTINEL).all() and s["err"] == P.OVERFLOW and s["eligible_pieces"] == 3
    same_vote(sc, source, keys, labels, 3, (1, 2), capacity=3)
    same_vote(sc, source, keys, labels, 20, (1, 2), capacity=0)
    # a label out of range casts no vote and keeps its label
    labels = np.array([1, 1, 1, 1, 300, 2] + [1] * 6 + [-5, 7, 7, 0])
    out, s = same_vote(sc, source, keys, labels, 3, (1, 2))
    assert out.tolist() == [1, 1, 1, 1, 300, 1] + [1] * 6 + [-5, 7, 7, 0] and s["err"] == P.BAD_LABEL
    out, s = same_vote(sc, source, keys, np.where(labels == 7, 4, labels), 3, (1, 2), n_classes=4)
    assert s["err"] == P.BAD_LABEL and out[13] == 4


@pytest.mark.parametrize("source", ["label", "similar"])
def test_vote_noisy_labelling_and_capacity(synthetic, source):
    coords, labels, sc, normals, _ = synthetic
    n = len(coords)
    noise = noisy(labels, seed=n)
    clicks = np.random.default_rng(1).integers(0, n, 30).tolist()
    k = int(noise.max()) + 1
    # the partition: by the true objects (label_pieces) / by the objects and the normals (similar_pieces)
    kw = dict(n_classes=k, normals=None if source == "label" else normals)
    got, s = same_vote(sc, source, labels, noise, 8, (2, 3), clicks, capacity=1024, **kw)
    assert s["relabelled_pieces"] >= 1 and s["relabelled_voxels"] >= s["relabelled_pieces"]
    assert s["eligible_pieces"] >= s["uniform_pieces"] + s["relabelled_pieces"] + s["blocked_pieces"] + s["below_share_pieces"]
    print(f"{source}: {s}")
    need = s["eligible_pieces"]
    small, t = same_vote(sc, source, labels, noise, 8, (2, 3), clicks, capacity=need - 1, **kw)
    assert t["err"] == P.OVERFLOW and t["eligible_pieces"] == need and (small == SENTINEL).all()
    exact, t = same_vote(sc, source, labels, noise, 8, (2, 3), clicks, capacity=need, **kw)
    assert np.array_equal(exact, got) and t == s
    same_vote(sc, source, labels, noise, 1, (1, 1), clicks, capacity=n, **kw)
    same_vote(sc, source, labels, np.where(noise == 2, 300, noise), 8, (1, 2), clicks, capacity=1024, **kw)


# ---------------------------------------------------------------------------------------------------- 5
def test_refusals():
    coords = plate(5, 5)
    sc = scene_of(coords)
    n = 25
    keys = _dev(np.zeros(n), np.int32)
    f3 = _dev(np.tile(turning([0.0]), (n, 1)), F)
    good = dict(scene=sc, keys=keys, normals=f3, feats=f3)
    V.similar_pieces(**good)
    for bad in (dict(connectivity=8), dict(keys=keys[:24]), dict(keys=keys.long()), dict(keys=keys.cpu()), dict(normals=f3[:24]),
                dict(normals=f3.double()), dict(feats=f3.cpu()), dict(feats=f3[:, :2]), dict(feats=f3.t()), dict(click_rows=[0] * 257),
                dict(piece_full=keys), dict(inverse_map=keys), dict(piece_qv=keys[:3]), dict(scene=None), dict(cos_min=1.01),
                dict(tol2=-1.0), dict(ref_cos_min=float("nan")), dict(ref_tol2=float("inf")), dict(ref_normal=[0, 0, float("nan")]),
                dict(ref_normal=[0, 0, 1], normals=None), dict(ref_feat=[0, 0, 1], feats=None), dict(oriented=3),
                dict(count=torch.zeros(1, dtype=torch.int32, device=DEV)), dict(records=torch.zeros(80, device=DEV))):
        with pytest.raises(ValueError):
            V.similar_pieces(**dict(good, **bad))
    ws = V.vote_workspace(n, DEV, 8, 4)
    piece = V.similar_pieces(workspace=ws, **good)[0]
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    vote = dict(scene=sc, labels=keys, piece_qv=piece, workspace=ws, min_voxels=8, share=(2, 3), n_classes=4, capacity=8)
    V.vote_pieces(**vote)
    for bad in (dict(labels_out=keys), dict(n_classes=0), dict(n_classes=257), dict(capacity=-1), dict(capacity=1000),
                dict(min_voxels=0), dict(share=(3, 2)), dict(share=(0, 2)), dict(share=(1, 65537)), dict(piece_qv=piece[:5]),
                dict(workspace=ws[:256]), dict(workspace=ws[4:]), dict(summary=torch.zeros(8, dtype=torch.uint8, device=DEV)),
                dict(click_rows=[0] * 257), dict(labels=keys.cpu())):
        with pytest.raises(ValueError):
            V.vote_pieces(**dict(vote, **bad))
    # the library's own checks: nothing is launched
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    piece_out = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)

    def similar(**kw):
        a = L.SimilarPiecesArgs()
        base = dict(scene=sc.handle.value, n=n, keys_dev=keys, piece_qv_dev=piece_out, n_out_dev=count, workspace_dev=ws,
                    workspace_bytes=ws.numel(), connectivity=26, normal_qv_dev=f3, feat_qv_dev=f3, cos_min=1.0, ref_cos_min=1.0)
        for k, v in dict(base, **kw).items():
            if k in ("ref_normal", "ref_feat"):
                getattr(a, k)[:] = v
            else:
                setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_similar_pieces", byref(a), None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(scene=None), dict(n=24), dict(connectivity=7), dict(n_clicks=257), dict(n_clicks=-1), dict(max_out=-1),
                dict(max_out=1), dict(n_full=-1), dict(n_full=3), dict(n_out_dev=None), dict(piece_qv_dev=None),
                dict(workspace_dev=None), dict(workspace_bytes=64), dict(workspace_dev=ws.data_ptr() + 4),
                dict(cos_min=1.5), dict(cos_min=-1.5), dict(cos_min=nan), dict(ref_cos_min=inf), dict(ref_cos_min=-2.0),
                dict(tol2=-1.0), dict(tol2=inf), dict(tol2=nan), dict(ref_tol2=-0.5), dict(ref_tol2=nan),
                dict(ref_flags=1, normal_qv_dev=None), dict(ref_flags=2, feat_qv_dev=None), dict(ref_flags=4), dict(ref_flags=-1),
                dict(ref_normal=[0, nan, 0]), dict(ref_feat=[inf, 0, 0]), dict(oriented=2)):
        assert similar(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [SENTINEL] * 2 and (piece_out.cpu().numpy() == SENTINEL).all()
    assert similar() == OK and similar(keys_dev=None, normal_qv_dev=None, ref_flags=2, ref_feat=[0, 0, 1], ref_tol2=0.5) == OK
    assert count.cpu().tolist() == [1, 0] and (piece_out.cpu().numpy() == 0).all()

    summary = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)

    def vote_status(**kw):
        a = L.VotePiecesArgs()
        base = dict(scene=sc.handle.value, n=n, labels_dev=keys, piece_qv_dev=piece, labels_out_dev=piece_out, summary_dev=summary,
                    workspace_dev=ws, workspace_bytes=ws.numel(), min_voxels=8, n_classes=4, capacity=8, share_num=2, share_den=3)
        for k, v in dict(base, **kw).items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_vote_pieces", byref(a), None)

    piece_out.fill_(SENTINEL)
    for bad in (dict(scene=None), dict(n=24), dict(n_clicks=257), dict(n_clicks=-1), dict(n_classes=0), dict(n_classes=257),
                dict(capacity=-1), dict(capacity=100000), dict(min_voxels=0), dict(share_num=0), dict(share_num=4), dict(share_den=65537),
                dict(share_num=65537, share_den=65537), dict(summary_dev=None), dict(labels_dev=None), dict(piece_qv_dev=None),
                dict(labels_out_dev=None), dict(labels_out_dev=keys), dict(workspace_dev=None), dict(workspace_bytes=64),
                dict(workspace_dev=ws.data_ptr() + 4)):
        assert vote_status(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert summary.cpu().tolist() == [SENTINEL] * 8 and (piece_out.cpu().numpy() == SENTINEL).all()
    assert vote_status() == OK
    assert summary.cpu().tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and (piece_out.cpu().numpy() == 0).all()
