"""-m gpu: the connected pieces of a labelling and the despeckle step (a3d_label_pieces, a3d_absorb_pieces in
csrc/session_pieces.hip; view.label_pieces, view.absorb_pieces).  The rules are restated in ``pieces_rule.py``; everything is
integer, so every comparison is exact.

1  which offsets each connectivity joins, batch samples, one voxel, lines across the wave and the 128-row pad, a wall, the
   serpentine (graph diameter 2 598)
2  synthetic scenes, permuted: ground-truth and noisy keys, keys of -1, keys up to 2^31 - 1, the hash-table scenes; every
   record field; max_out below the count; the lift and an inverse-map entry out of range; two calls bit-identical
3  absorb: the known answers of the rule, the capacity, the noisy labelling
4  the wrappers' and the library's refusals
"""
import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from pieces_rule import BAD_INDEX, OVERFLOW, PIECE, absorb_numpy, lift_numpy, noisy, offsets, pieces_numpy, serpentine
from session_kit import DEV, _dev, byref, status

pytestmark = pytest.mark.gpu

SENTINEL = -77
CONN = (6, 18, 26)
INVALID, OK = -1, 0


# ---------------------------------------------------------------------------------------------------- the adaptors
def scene_of(coords4):
    return Scene(torch.from_numpy(np.ascontiguousarray(coords4, np.int32)).to(DEV))


def pieces_gpu(scene, keys, connectivity, click_rows=(), inverse_map=None, max_out=1024, workspace=None):
    """view.label_pieces, numpy in / numpy out; every output starts as a sentinel."""
    n = scene.n[0]
    piece = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    records = torch.full((max_out * PIECE.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    kw = {}
    if inverse_map is not None:
        kw = dict(inverse_map=_dev(inverse_map, np.int64),
                  piece_full=torch.full((len(inverse_map),), SENTINEL, dtype=torch.int32, device=DEV))
    got = V.label_pieces(scene, _dev(keys, np.int32), connectivity, click_rows, piece_qv=piece, records=records, count=count,
                         workspace=workspace, **kw)
    assert got[0] is piece and got[2] is records and got[3] is count
    raw = records.cpu().numpy()
    rec, n_pieces, err = V.read_pieces(raw, count.cpu().numpy())
    return dict(piece=piece.cpu().numpy(), full=None if got[1] is None else got[1].cpu().numpy(), records=rec, n=n_pieces,
                err=err, raw=raw, piece_dev=piece, workspace=got[4])


def rows(rec):
    return [(int(r["root"]), int(r["key"]), int(r["voxels"]), int(r["clicked"]), r["lo"].tolist(), r["hi"].tolist()) for r in rec]


def same_pieces(got, coords4, keys, connectivity, click_rows=(), what=None):
    piece, rec = pieces_numpy(coords4, keys, connectivity, click_rows)
    assert got["piece"].dtype == np.int32 and np.array_equal(got["piece"], piece), what
    assert got["n"] == len(rec) and got["err"] == 0, (what, got["n"], len(rec))
    kept = rec[:len(got["records"])]
    for field in PIECE.names:                    # root, key, voxels, clicked, lo, hi
        assert np.array_equal(got["records"][field], kept[field]), (what, field)
    return piece, rec


def absorb_gpu(coords4, labels, min_voxels, connectivity, click_rows=(), n_classes=256, capacity=64, scene=None):
    """label_pieces on the labels, then view.absorb_pieces with the same workspace: (labels_out, summary dict)."""
    scene = scene or scene_of(coords4)
    n = scene.n[0]
    ws = V.pieces_workspace(n, DEV, capacity, n_classes)
    lab = _dev(labels, np.int32)
    piece = V.label_pieces(scene, lab, connectivity, click_rows, workspace=ws)[0]
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    summary = torch.full((V.ABSORB_SUMMARY.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
    got = V.absorb_pieces(scene, lab, piece, ws, min_voxels, connectivity, click_rows, n_classes, capacity, labels_out=out,
                          summary=summary)
    assert got[0] is out and got[1] is summary
    return out.cpu().numpy(), V.read_absorb_summary(summary.cpu().numpy())


def same_absorb(coords4, labels, min_voxels, connectivity, click_rows=(), n_classes=256, capacity=64, scene=None):
    got, summary = absorb_gpu(coords4, labels, min_voxels, connectivity, click_rows, n_classes, capacity, scene)
    want, rule = absorb_numpy(coords4, labels, min_voxels, connectivity, click_rows, n_classes, capacity)
    assert summary == rule, (summary, rule)
    if want is None:
        assert (got == SENTINEL).all()
    else:
        assert np.array_equal(got, want)
    return got, summary


# ---------------------------------------------------------------------------------------------------- 1
def test_offsets_each_connectivity_joins():
    joined = {c: 0 for c in CONN}
    for k in range(27):
        d = (k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1)
        if d == (0, 0, 0):
            continue
        coords = np.array([[0, 5, 5, 5], [0, 5 + d[0], 5 + d[1], 5 + d[2]]], np.int32)
        sc = scene_of(coords)
        for c in CONN:
            got = pieces_gpu(sc, [3, 3], c)
            admitted = d in offsets(c)
            assert admitted == (1 <= sum(abs(x) for x in d) <= {6: 1, 18: 2, 26: 3}[c])
            assert got["piece"].tolist() == ([0, 0] if admitted else [0, 1]), (d, c)
            assert got["n"] == (1 if admitted else 2)
            joined[c] += admitted
            assert pieces_gpu(sc, [3, 4], c)["piece"].tolist() == [0, 1]         # neighbours, but not the same key
    assert joined == {6: 6, 18: 18, 26: 26}


def test_small_shapes():
    # equal xyz in two batch samples, and neighbours across samples: never joined
    coords = np.array([[0, 1, 1, 1], [0, 2, 1, 1], [1, 1, 1, 1], [1, 2, 1, 1], [1, 3, 2, 2]], np.int32)
    sc = scene_of(coords)
    for c in CONN:
        got = pieces_gpu(sc, [7, 7, 7, 7, 7], c, click_rows=[3])
        assert got["piece"].tolist() == [0, 0, 2, 2, 2 if c == 26 else 4]
        same_pieces(got, coords, [7, 7, 7, 7, 7], c, [3])
        assert got["records"]["clicked"].tolist() == ([0, 1] if c == 26 else [0, 1, 0])
    # one voxel; one voxel without a key
    one = np.array([[0, -3, 4, 9]], np.int32)
    sc = scene_of(one)
    got = pieces_gpu(sc, [5], 26, click_rows=[0])
    assert got["piece"].tolist() == [0] and got["n"] == 1
    assert rows(got["records"]) == [(0, 5, 1, 1, [-3, 4, 9], [-3, 4, 9])]
    got = pieces_gpu(sc, [-1], 6)
    assert got["piece"].tolist() == [-1] and got["n"] == 0 and len(got["records"]) == 0
    # lines of 37 and of 129 voxels (the latter crosses the 128-row pad), shuffled, cut into pieces by the keys
    for m in (37, 129):
        rng = np.random.default_rng(m)
        line = np.stack([np.zeros(m), np.arange(m), np.full(m, 2), np.full(m, -1)], 1).astype(np.int32)[rng.permutation(m)]
        sc = scene_of(line)
        for keys in (np.zeros(m, np.int64), (line[:, 1] // 10) % 2, np.where(line[:, 1] == m // 2, -1, 4)):
            for c in CONN:
                piece, rec = same_pieces(pieces_gpu(sc, keys, c), line, keys, c, what=(m, c))
        assert len(rec) == 2 and rec["voxels"].sum() == m - 1
    # a one-voxel wall of another key between two plates of one key
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    plates = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1).astype(np.int32)[np.random.default_rng(1).permutation(len(g))]
    keys = np.where(plates[:, 3] == 1, 2, 1)
    sc = scene_of(plates)
    for c in CONN:
        piece, rec = same_pieces(pieces_gpu(sc, keys, c), plates, keys, c)
        assert len(rec) == 3 and sorted(rec["voxels"].tolist()) == [16, 16, 16]


def test_serpentine():
    coords = serpentine()
    assert len(coords) == 2599
    sc = scene_of(coords)
    keys = np.full(len(coords), 9)
    for c in (6, 26):
        got = pieces_gpu(sc, keys, c)
        assert (got["piece"] == 0).all() and got["n"] == 1            # one piece, named by the smallest row
        assert rows(got["records"]) == [(0, 9, 2599, 0, [0, 0, 0], [63, 78, 0])]
        same_pieces(got, coords, keys, c)
    again = pieces_gpu(sc, keys, 6)
    assert np.array_equal(again["piece"], got["piece"]) and np.array_equal(again["raw"], pieces_gpu(sc, keys, 6)["raw"])


# ---------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module", params=[(3000, 5), (5000, 2)], ids=["3000", "5000"])
def synthetic(request):
    n, seed = request.param
    sc = make_scene(n, seed=seed)
    p = np.random.default_rng(seed).permutation(len(sc["coords"]))
    coords, labels = sc["coords"][p], sc["labels"][p].astype(np.int64)
    return coords, labels, scene_of(coords)


@pytest.mark.parametrize("c", CONN)
def test_synthetic_scenes(synthetic, c):
    coords, labels, sc = synthetic
    n = len(coords)
    rng = np.random.default_rng(n + c)
    clicks = rng.integers(0, n, 40).tolist() + [-1, n, 2 ** 31 - 1]
    noise = noisy(labels, seed=n)
    holes = np.where(rng.random(n) < 0.1, -1, noise)
    big = np.where(noise % 2 == 1, 2 ** 31 - 1 - noise, noise)
    for name, keys in (("ground truth", labels), ("noisy", noise), ("holes", holes), ("large keys", big)):
        got = pieces_gpu(sc, keys, c, clicks, max_out=2048)
        piece, rec = same_pieces(got, coords, keys, c, clicks, what=(name, c))
        assert rec["clicked"].any() and not rec["clicked"].all()
        print(f"n={n} connectivity={c} {name}: {len(rec)} pieces, {(rec['voxels'] == 1).sum()} singletons")
    assert (piece >= 0).all() and (pieces_gpu(sc, holes, c)["piece"][holes < 0] == -1).all()
    # two calls give the same bytes; a smaller max_out reports the true count and writes the first records
    first, second = pieces_gpu(sc, noise, c, clicks, max_out=2048), pieces_gpu(sc, noise, c, clicks, max_out=2048)
    assert np.array_equal(first["raw"], second["raw"]) and np.array_equal(first["piece"], second["piece"])
    few = pieces_gpu(sc, noise, c, clicks, max_out=7)
    assert few["n"] == first["n"] > 7 and len(few["records"]) == 7
    assert np.array_equal(few["records"], first["records"][:7]) and (few["raw"][7 * 40:] == 0x5a).all()
    none = pieces_gpu(sc, noise, c, clicks, max_out=0)
    assert none["n"] == first["n"] and np.array_equal(none["piece"], first["piece"])
    # the lift, and an inverse-map entry out of range
    inv = rng.integers(0, n, 2 * n + 3)
    got = pieces_gpu(sc, holes, c, inverse_map=inv)
    want, err = lift_numpy(got["piece"], inv, SENTINEL)
    assert err == 0 and got["err"] == 0 and np.array_equal(got["full"], want)
    inv[[0, n, 2 * n + 2]] = [n, -1, 2 ** 40]
    got = pieces_gpu(sc, holes, c, inverse_map=inv)
    want, err = lift_numpy(got["piece"], inv, SENTINEL)
    assert err == BAD_INDEX == got["err"] and np.array_equal(got["full"], want) and (got["full"][[0, n, 2 * n + 2]] == SENTINEL).all()
    # no key at all: no piece
    got = pieces_gpu(sc, np.full(n, -1), c)
    assert got["n"] == 0 and (got["piece"] == -1).all() and (got["raw"] == 0x5a).all()


@pytest.mark.parametrize("name", ["sparse_far", "compact_plus_outlier"])
def test_hash_table_scenes(name):
    from test_gpu_scene import CASES, _random_coords
    coords = _random_coords(800, 60000, 3, negative=True) if name == "sparse_far" else CASES[name]()
    sc = scene_of(coords)
    assert sc.grid_dims is None                  # the lookup went through the hash table
    rng = np.random.default_rng(3)
    for c in CONN:
        for keys in (np.zeros(len(coords), np.int64), rng.integers(0, 3, len(coords))):
            same_pieces(pieces_gpu(sc, keys, c, [0, 5]), coords, keys, c, [0, 5], what=(name, c))


# ---------------------------------------------------------------------------------------------------- 3
def _plate(nx=5, ny=5):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g, np.zeros((len(g), 1), np.int64)], 1).astype(np.int32)


def test_absorb_known_answers():
    plate = _plate()
    at = lambda x, y: int(np.flatnonzero((plate[:, 1] == x) & (plate[:, 2] == y))[0])
    # one foreign voxel in the middle is absorbed
    lab = np.full(25, 3)
    lab[at(2, 2)] = 7
    for c in CONN:
        got, s = same_absorb(plate, lab, 8, c)
        assert (got == 3).all() and s == dict(small_pieces=1, relabelled_pieces=1, relabelled_voxels=1, kept_isolated=0, err=0)
    # a vote tie goes to the lowest label: the left half 5, the right half 2, the speck on the middle column between them
    lab = np.where(plate[:, 1] < 2, 5, 2)
    lab[plate[:, 1] == 2] = np.where(plate[plate[:, 1] == 2, 2] < 2, 5, 2)
    lab[at(2, 2)] = 9
    got, s = same_absorb(plate, lab, 2, 6)
    votes = {int(l): int(sum(lab[at(2 + dx, 2 + dy)] == l for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))) for l in (2, 5)}
    assert votes == {2: 2, 5: 2} and got[at(2, 2)] == 2 and s["relabelled_pieces"] == 1
    # a speck with no neighbour at all is kept and counted; a speck that holds a clicked row is kept
    far = np.concatenate([plate, [[0, 40, 40, 40]]]).astype(np.int32)
    lab = np.full(26, 3)
    lab[at(1, 1)] = 4
    got, s = same_absorb(far, lab, 8, 26, click_rows=[at(1, 1)])
    assert np.array_equal(got, lab) and s == dict(small_pieces=1, relabelled_pieces=0, relabelled_voxels=0, kept_isolated=1, err=0)
    got, s = same_absorb(far, lab, 8, 26)
    assert got[at(1, 1)] == 3 and got[25] == 3 and s["small_pieces"] == 2 and s["kept_isolated"] == 1
    # two adjacent specks of different labels each vote with the other's INPUT label: the corner 8 sees one 9 and one 1 (a
    # tie: the lowest), the 9 beside it one 8 and two 1 ...
    lab = np.full(25, 1)
    lab[at(0, 0)], lab[at(1, 0)] = 8, 9
    got, s = same_absorb(plate, lab, 2, 6)
    assert got[at(0, 0)] == 1 and got[at(1, 0)] == 1 and s["relabelled_pieces"] == 2
    edge = _plate(2, 1)                          # ... and two voxels alone swap their labels: one step, on the input
    got, s = same_absorb(edge, [8, 9], 2, 6)
    assert got.tolist() == [9, 8] and s["relabelled_voxels"] == 2
    # a piece of exactly min_voxels voxels is kept, one of min_voxels - 1 is not
    lab = np.full(25, 1)
    lab[[at(0, 0), at(1, 0), at(2, 0)]] = 6
    got, s = same_absorb(plate, lab, 3, 6)
    assert np.array_equal(got, lab) and s["small_pieces"] == 0
    got, s = same_absorb(plate, lab, 4, 6)
    assert (got == 1).all() and s["relabelled_voxels"] == 3


def test_absorb_noisy_labelling_and_capacity(synthetic):
    coords, labels, sc = synthetic
    noise = noisy(labels, seed=len(coords))
    clicks = np.random.default_rng(1).integers(0, len(coords), 30).tolist()
    for c in CONN:
        got, s = same_absorb(coords, noise, 8, c, clicks, n_classes=int(noise.max()) + 1, capacity=1024, scene=sc)
        assert s["relabelled_pieces"] > 50 and s["small_pieces"] == s["relabelled_pieces"] + s["kept_isolated"]
    need = s["small_pieces"]
    # capacity too small: nothing is written, the need is reported; exactly enough: the same answer
    small, t = same_absorb(coords, noise, 8, 26, clicks, n_classes=int(noise.max()) + 1, capacity=need - 1, scene=sc)
    assert t["err"] == OVERFLOW and t["small_pieces"] == need and (small == SENTINEL).all()
    exact, t = same_absorb(coords, noise, 8, 26, clicks, n_classes=int(noise.max()) + 1, capacity=need, scene=sc)
    assert np.array_equal(exact, got) and t == s


# ---------------------------------------------------------------------------------------------------- 4
def test_refusals():
    coords = _plate()
    sc = scene_of(coords)
    n = 25
    keys = _dev(np.zeros(n), np.int32)
    ws = V.pieces_workspace(n, DEV, 8, 4)
    piece = V.label_pieces(sc, keys, 26, workspace=ws)[0]
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    for bad in (dict(connectivity=8), dict(connectivity=0), dict(keys=keys[:24]), dict(keys=keys.long()), dict(keys=keys.cpu()),
                dict(click_rows=[0] * 257), dict(piece_full=out), dict(inverse_map=keys), dict(piece_qv=out[:3]),
                dict(count=torch.zeros(1, dtype=torch.int32, device=DEV)), dict(records=torch.zeros(80, device=DEV)),
                dict(scene=None)):
        with pytest.raises(ValueError):
            V.label_pieces(**dict(dict(scene=sc, keys=keys), **bad))
    good = dict(scene=sc, labels=keys, piece_qv=piece, workspace=ws, min_voxels=8, n_classes=4, capacity=8)
    V.absorb_pieces(**good)
    for bad in (dict(connectivity=27), dict(labels_out=keys), dict(n_classes=0), dict(n_classes=257), dict(capacity=-1),
                dict(capacity=1000), dict(min_voxels=-1), dict(piece_qv=piece[:5]), dict(workspace=ws[:256]),
                dict(summary=torch.zeros(8, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            V.absorb_pieces(**dict(good, **bad))
    # the library's own checks: nothing is launched
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device=DEV)
    piece_out = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)

    def label(**kw):
        a = L.LabelPiecesArgs()
        base = dict(scene=sc.handle.value, n=n, keys_dev=keys, piece_qv_dev=piece_out, n_out_dev=count, workspace_dev=ws,
                    workspace_bytes=ws.numel(), connectivity=26)
        for k, v in dict(base, **kw).items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_label_pieces", byref(a), None)

    assert status("a3d_label_pieces", None, None) == INVALID and status("a3d_absorb_pieces", None, None) == INVALID
    for bad in (dict(scene=None), dict(n=24), dict(connectivity=7), dict(n_clicks=257), dict(n_clicks=-1), dict(max_out=-1),
                dict(max_out=1), dict(n_full=-1), dict(n_full=3), dict(n_out_dev=None), dict(keys_dev=None),
                dict(piece_qv_dev=None), dict(workspace_dev=None), dict(workspace_bytes=64),
                dict(workspace_dev=ws.data_ptr() + 4)):
        assert label(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [SENTINEL] * 2 and (piece_out.cpu().numpy() == SENTINEL).all()
    assert label() == OK
    assert count.cpu().tolist() == [1, 0] and (piece_out.cpu().numpy() == 0).all()
    assert L.load().a3d_pieces_workspace_bytes(-1) == 0 and L.load().a3d_absorb_workspace_bytes(10, 4, 257) == 0
