"""No GPU: the host restatement of the pieces rule (``pieces_rule.py``) against ``scipy.ndimage.label``, known answers of the
absorb rule, and the spot ranking of ``guide(regions="connected")``."""
import numpy as np
import pytest
from scipy import ndimage

from agile3d_amd.session import MAX_SPOTS, rank_spots
from agile3d_amd.synthetic import make_scene
from pieces_rule import OVERFLOW, absorb_numpy, lift_numpy, noisy, offsets, pieces_numpy, serpentine


def scipy_pieces(coords4, keys, connectivity):
    """Per key and batch sample ``scipy.ndimage.label`` on the dense grid; the root is the min row of each component."""
    coords4, keys = np.asarray(coords4, np.int64), np.asarray(keys, np.int64)
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    piece = np.full(len(keys), -1, np.int64)
    lo = coords4[:, 1:].min(0)
    shape = tuple(coords4[:, 1:].max(0) - lo + 1)
    for b in np.unique(coords4[:, 0]):
        for key in np.unique(keys[(coords4[:, 0] == b) & (keys >= 0)]):
            rows = np.flatnonzero((coords4[:, 0] == b) & (keys == key))
            grid = np.zeros(shape, bool)
            cell = tuple((coords4[rows, 1:] - lo).T)
            grid[cell] = True
            comp = ndimage.label(grid, structure)[0][cell]
            for c in np.unique(comp):
                piece[rows[comp == c]] = rows[comp == c].min()
    return piece


@pytest.mark.parametrize("connectivity", (6, 18, 26))
@pytest.mark.parametrize("n, seed", ((3000, 5), (5000, 2)))
def test_rule_equals_scipy_label(n, seed, connectivity):
    sc = make_scene(n, seed=seed)
    p = np.random.default_rng(seed).permutation(len(sc["coords"]))
    coords, labels = sc["coords"][p], sc["labels"][p].astype(np.int64)
    for name, keys in (("ground truth", labels), ("noisy", noisy(labels, seed=len(coords)))):
        piece, rec = pieces_numpy(coords, keys, connectivity)
        assert np.array_equal(piece, scipy_pieces(coords, keys, connectivity)), name
        assert rec["voxels"].sum() == len(coords) and np.array_equal(rec["root"], np.unique(piece))
        assert np.array_equal(rec["key"], keys[rec["root"]]) and (np.diff(rec["root"]) > 0).all()
        for r in rec[:: max(1, len(rec) // 8)]:
            member = coords[piece == r["root"], 1:]
            assert r["voxels"] == len(member) and np.array_equal(r["lo"], member.min(0)) and np.array_equal(r["hi"], member.max(0))
        assert (len(rec) < 100) == (name == "ground truth")           # tens of pieces; hundreds, mostly singletons, with the noise


def test_connectivity_and_batches():
    assert [len(offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    for d in offsets(26):
        pair = np.array([[0, 5, 5, 5], [0, 5 + d[0], 5 + d[1], 5 + d[2]]])
        for c in (6, 18, 26):
            joined = sum(abs(x) for x in d) <= {6: 1, 18: 2, 26: 3}[c]
            assert pieces_numpy(pair, [1, 1], c)[0].tolist() == ([0, 0] if joined else [0, 1])
            assert np.array_equal(pieces_numpy(pair, [1, 1], c)[0], scipy_pieces(pair, [1, 1], c))
    two = np.array([[0, 1, 1, 1], [1, 1, 1, 1], [1, 2, 1, 1]])
    assert pieces_numpy(two, [4, 4, 4], 26)[0].tolist() == [0, 1, 1]
    assert pieces_numpy(two, [4, -1, 4], 26)[0].tolist() == [0, -1, 2]
    piece, rec = pieces_numpy(two, [4, 4, 4], 6, click_rows=[2, 7, -1])
    assert rec["clicked"].tolist() == [0, 1] and rec["lo"].tolist() == [[1, 1, 1], [1, 1, 1]] and rec["hi"][1].tolist() == [2, 1, 1]
    full, err = lift_numpy(piece, [2, 0, 3, -1], -9)
    assert full.tolist() == [1, 0, -9, -9] and err == 1


def test_serpentine_is_one_piece():
    coords = serpentine()
    assert len(coords) == 2599 and len(np.unique(coords, axis=0)) == 2599
    for c in (6, 26):
        piece, rec = pieces_numpy(coords, np.zeros(2599), c)
        assert (piece == 0).all() and len(rec) == 1 and rec["voxels"][0] == 2599
    # the graph diameter under 6: a breadth-first search from one end of the path
    where = {tuple(c[1:]): i for i, c in enumerate(coords.tolist())}
    start = where[(0, 0, 0)]
    dist, frontier = {start: 0}, [start]
    while frontier:
        nxt = []
        for i in frontier:
            x, y, z = coords[i, 1:].tolist()
            for dx, dy, dz in offsets(6):
                j = where.get((x + dx, y + dy, z + dz))
                if j is not None and j not in dist:
                    dist[j] = dist[i] + 1
                    nxt.append(j)
        frontier = nxt
    assert max(dist.values()) == 2598


def _plate(nx=5, ny=5):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g, np.zeros((len(g), 1), np.int64)], 1)


def test_absorb_known_answers():
    plate = _plate()
    at = lambda x, y: int(np.flatnonzero((plate[:, 1] == x) & (plate[:, 2] == y))[0])
    lab = np.full(25, 3)
    lab[at(2, 2)] = 7
    out, s = absorb_numpy(plate, lab, 8, 26)
    assert (out == 3).all() and s == dict(small_pieces=1, relabelled_pieces=1, relabelled_voxels=1, kept_isolated=0, err=0)
    assert np.array_equal(absorb_numpy(plate, lab, 1, 26)[0], lab)                  # nothing has fewer than 1 voxel
    assert np.array_equal(absorb_numpy(plate, lab, 8, 26, click_rows=[at(2, 2)])[0], lab)
    # a tie goes to the lowest label: two votes for 5 (left, below), two for 2 (right, above)
    lab = np.where(plate[:, 1] < 2, 5, 2)
    lab[plate[:, 1] == 2] = np.where(plate[plate[:, 1] == 2, 2] < 2, 5, 2)
    lab[at(2, 2)] = 9
    assert absorb_numpy(plate, lab, 2, 6)[0][at(2, 2)] == 2
    lab[at(2, 3)] = 5                                                               # a third vote for 5
    assert absorb_numpy(plate, lab, 2, 6)[0][at(2, 2)] == 5
    # isolated in space: kept and counted
    far = np.concatenate([plate, [[0, 40, 40, 40]]])
    out, s = absorb_numpy(far, np.full(26, 3), 8, 26)
    assert (out == 3).all() and s["small_pieces"] == 1 and s["kept_isolated"] == 1 and s["relabelled_pieces"] == 0
    # one step on the INPUT labels: two voxels alone swap
    out, s = absorb_numpy(_plate(2, 1), [8, 9], 2, 6)
    assert out.tolist() == [9, 8] and s["relabelled_voxels"] == 2
    # exactly min_voxels is kept
    lab = np.full(25, 1)
    lab[[at(0, 0), at(1, 0), at(2, 0)]] = 6
    assert np.array_equal(absorb_numpy(plate, lab, 3, 6)[0], lab) and (absorb_numpy(plate, lab, 4, 6)[0] == 1).all()
    # the capacity
    lab = np.full(25, 1)
    lab[[at(0, 0), at(4, 4), at(2, 2)]] = [6, 7, 8]
    out, s = absorb_numpy(plate, lab, 2, 6, capacity=2)
    assert out is None and s["err"] == OVERFLOW and s["small_pieces"] == 3
    assert (absorb_numpy(plate, lab, 2, 6, capacity=3)[0] == 1).all()


def test_spot_ranking():
    rec = [dict(root=40, voxels=3), dict(root=7, voxels=9), dict(root=12, voxels=3), dict(root=90, voxels=1)]
    assert rank_spots(rec) == [1, 2, 0, 3]                                          # by size; ties to the lower root
    assert rank_spots(rec, 2) == [1, 2] and rank_spots(rec, 0) == [] and rank_spots([]) == []
    many = [dict(root=r, voxels=1 + r % 3) for r in range(600)]
    got = rank_spots(many)
    assert len(got) == MAX_SPOTS == 255 and got[:3] == [2, 5, 8] and all(many[k]["voxels"] >= 2 for k in got)
    structured = np.array([(5, 2), (1, 2), (3, 4)], dtype=[("root", "<i4"), ("voxels", "<i4")])
    assert rank_spots(structured) == [2, 1, 0]
    with pytest.raises(ValueError):
        rank_spots(rec, -1)
