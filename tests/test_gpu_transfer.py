"""-m gpu: the point index and the bulk nearest query -- a3d_point_index_create / a3d_point_index_nearest
(csrc/session_transfer.hip) -- against the brute-force rule restated in ``transfer_rule.py``: rows, the BYTES of d2, the carried
labels and the summary's counts, all exact.  The restatement knows nothing of cells, keys or tables, so every case here is a
case against the index: sizes at the edges of the launches, one long list and many short ones, coordinates on cell borders
and on both sides of zero, the ends of the key range, the cutoff to the last bit, ties across cells, sets far from the
origin, rows and queries that are not finite, and the reaches for which the index is bypassed."""

import numpy as np
import pytest
import torch

import transfer_rule as R
from agile3d_amd import lib as L
from agile3d_amd import view as V
from session_kit import DEV, _dev, status

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY_PASS = 1024 * 256          # rows one pass of the key kernel's grid covers (kTiFat x kTiFatBlocks)
QUERY_PASS = 256 * 2048        # queries one pass of the query kernel's grid covers (kTiB x kTiQueryBlocks)


def run(src, queries, cell, r, labels=None, fill=0, check=False):
    """The library on numpy arrays: the outputs start as sentinels, so that an untouched entry shows."""
    src, q = np.ascontiguousarray(src, F32).reshape(-1, 3), np.ascontiguousarray(queries, F32).reshape(-1, 3)
    index = V.point_index_create(_dev(src, F32), cell)
    m = len(q)
    nearest = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((m,), -7.0, dtype=torch.float32, device=DEV)
    lab_out = None if labels is None else torch.full((m,), -7, dtype=torch.int32, device=DEV)
    out = V.point_index_nearest(index, _dev(q, F32), r, labels_src=None if labels is None else _dev(labels, np.int32), fill=fill,
                                nearest=nearest, d2=d2, labels=lab_out)
    host = out[3].cpu().numpy()
    index.close()
    res = dict(nearest=nearest.cpu().numpy(), d2=d2.cpu().numpy(), labels=None if labels is None else lab_out.cpu().numpy())
    res.update(V.read_transfer_summary(host, check=check))
    return res


def check(src, queries, cell, r, labels=None, fill=0, chunk=256):
    got = run(src, queries, cell, r, labels, fill)
    want = R.nearest(src, queries, r, labels, fill, chunk=chunk)
    assert got["nearest"].tolist() == want["nearest"].tolist()
    assert got["d2"].tobytes() == want["d2"].tobytes()
    if labels is not None:
        assert got["labels"].tolist() == want["labels"].tolist()
    for k in ("matched", "unmatched", "nonfinite", "source_left_out"):
        assert got[k] == want[k], k
    assert got["err"] == (R.UNKEYABLE if R.unkeyable(src, cell) else 0)
    return got


def cloud(n, seed, box=2.0):
    return np.random.default_rng(seed).uniform(0.0, box, (n, 3)).astype(F32)


# ------------------------------------------------------------------------------------------- sizes
def test_source_and_query_sizes_at_their_edges():
    q = cloud(65, 1, 0.6)
    for n in (1, 2, 63, 64, 65, 255, 256, 257):
        got = check(cloud(n, n, 0.6), q, 0.2, 0.1, labels=np.arange(n) * 3 + 1, fill=-5)
        assert n < 64 or got["matched"] > 0
    src = cloud(257, 2, 0.6)
    for m in (1, 64, 65):
        check(src, cloud(m, 100 + m, 0.6), 0.2, 0.1)


def test_one_pass_of_the_key_grid_and_77_rows():
    src = cloud(KEY_PASS + 77, 3)
    src[::1001] = np.nan
    got = check(src, cloud(64, 4), 0.1, 0.05, chunk=8)
    assert got["matched"] >= 60 and got["source_left_out"] == len(src[::1001])


def test_one_pass_of_the_query_grid_and_77_queries():
    src = cloud(33, 5, 1.0)
    got = check(src, cloud(QUERY_PASS + 77, 6, 1.0), 0.5, 0.25, labels=np.arange(33), chunk=1 << 14)
    assert 0 < got["unmatched"] and got["matched"] > QUERY_PASS // 4


# ------------------------------------------------------------------------------------------- long and short lists
def test_300_points_in_one_cell_and_every_point_in_its_own():
    rng = np.random.default_rng(7)
    crowd = (0.25 + rng.uniform(0.01, 0.24, (300, 3))).astype(F32)          # all in cell (1, 1, 1) of 0.25
    assert len(np.unique(np.floor(crowd / F32(0.25)), axis=0)) == 1
    got = check(crowd, np.concatenate([crowd[::7] + F32(0.001), rng.uniform(0.0, 0.75, (200, 3)).astype(F32)]), 0.25, 0.125)
    assert got["matched"] > 60
    g = np.arange(6, dtype=F32) * F32(0.25) + F32(0.125)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)                 # 216 cells, one point each
    assert len(np.unique(np.floor(lattice / F32(0.25)), axis=0)) == 216
    got = check(lattice[rng.permutation(216)], rng.uniform(-0.2, 1.7, (500, 3)).astype(F32), 0.25, 0.125)
    assert 0 < got["matched"] < 500


# ------------------------------------------------------------------------------------------- cell borders, signs, the key range
def test_coordinates_at_exact_multiples_of_the_cell_on_both_sides_of_zero():
    cell = F32(0.25)
    k = np.arange(-3, 4, dtype=F32) * cell
    src = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)                     # 343 points ON cell corners
    rng = np.random.default_rng(8)
    eps = np.nextafter(F32(0), F32(1))
    q = np.concatenate([src, src + F32(0.125), src - F32(0.125), src + eps, src - eps, np.nextafter(src, F32(-9)), np.nextafter(src, F32(9)),
                        rng.uniform(-1, 1, (300, 3)).astype(F32), src[:1] + np.array([0.125, 0, 0], F32)])
    got = check(src, q, cell, cell / 2)
    assert got["nearest"][:343].tolist() == list(range(343))       # floor, not truncation: -0.25 lies in cell -1, and is found
    # the last query lies an exact half cell from rows 0 and 49, its neighbours along x: the lower row, at exactly the reach
    assert got["nearest"][-1] == 0 and got["d2"][-1] == F32(0.015625)


def test_the_ends_of_the_key_range():
    """cell_size 1: sources in the cells -2^20 and +2^20, the last that can be keyed.  A query beside them has neighbour cells at
    -2^20 - 1 / 2^20 + 1, which are outside the key range and must be skipped, not wrapped onto another cell; the two end cells
    themselves share a key (the key wraps modulo 2^21), which may cost time and never an answer."""
    e = float(1 << 20)
    src = np.array([[-e + 0.25, 0.5, 0.5], [e + 0.25, 0.5, 0.5], [0.5, -e + 0.75, 0.5], [0.5, 0.5, e + 0.5], [e - 0.5, 0.5, 0.5],
                    [-e + 1.25, 0.5, 0.5]], F32)
    assert np.abs(np.floor(src)).max() == e
    q = np.array([[-e + 0.125, 0.5, 0.5], [e + 0.5, 0.5, 0.5], [0.5, -e + 0.5, 0.5], [0.5, 0.5, e + 0.75], [-e - 0.125, 0.5, 0.5],
                  [e + 1.5, 0.5, 0.5], [e + 0.125, 0.5, 0.5], [-e + 0.875, 0.5, 0.5], [0.5, 0.5, 0.5], [3 * e, 0.5, 0.5], [-1e30, 0, 0]], F32)
    got = check(src, q, 1.0, 0.5)
    assert got["nearest"].tolist() == [0, 1, 2, 3, 0, -1, 1, 5, -1, -1, -1] and got["err"] == 0


def test_a_source_beyond_the_key_range_is_flagged_and_the_wrapper_raises():
    src = np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.25 * ((1 << 20) + 1)], [0.3, 0.1, 0.1]], F32)
    got = run(src, src, 0.25, 0.125)                                # the row is left out: the others answer as the rule says ...
    assert R.unkeyable(src, 0.25) and got["err"] == V.TRANSFER_UNKEYABLE and got["nearest"].tolist() == [0, -1, 2]
    with pytest.raises(ValueError, match="cells"):                  # ... and the summary's decoder refuses to speak for such an index
        run(src, src, 0.25, 0.125, check=True)
    assert run(src, src, 0.5, 0.125, check=True)["nearest"].tolist() == [0, 1, 2]      # larger cells: within range


# ------------------------------------------------------------------------------------------- the cutoff, ties
def test_the_cutoff_to_the_last_bit():
    r = F32(0.05)
    src = np.array([[0, 0, 0], [1, 1, 1]], F32)
    q = []
    for base in src:
        for axis in range(3):
            for sign in (1, -1):
                for d in (r, np.nextafter(r, F32(1)), np.nextafter(r, F32(0))):
                    p = base.copy()
                    p[axis] += F32(sign) * d
                    q.append(p)
    q = np.asarray(q, F32)
    got = check(src, q, 2 * r, r)                                   # max_distance == cell_size / 2 exactly
    want = [0, -1, 0] * 6                                           # about the origin the differences are exact: at r in, one ulp beyond out
    assert got["nearest"][:18].tolist() == want and got["d2"][0].tobytes() == F32(r * r).tobytes()
    check(src, q, 1.0, r)                                           # the same reach in far larger cells
    # the library's own refusal one ulp above half a cell (the wrapper refuses it too, so the entry point is called as it is)
    index = V.point_index_create(_dev(src, F32), float(2 * r))
    out, summ = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(40, dtype=torch.uint8, device=DEV)
    call = lambda *a: status("a3d_point_index_nearest", *a)
    qd = _dev(src, F32)
    ok = (index.handle, qd.data_ptr(), 2, float(r), None, 0, out.data_ptr(), None, None, summ.data_ptr(), None)
    assert call(*ok) == 0
    bad = lambda i, value: ok[:i] + (value,) + ok[i + 1:]
    for args in (bad(3, float(np.nextafter(r, F32(1)))), bad(3, 0.0), bad(3, -0.01), bad(3, float("nan")), bad(2, -1), bad(2, 1 << 31),
                 bad(1, None), bad(6, None), bad(9, None), bad(0, None), bad(8, out.data_ptr()), bad(4, out.data_ptr()),
                 bad(9, summ.data_ptr() + 4)):
        assert call(*args) == L.A3D_ERR_INVALID, args
    assert b"a3d_point_index_nearest" in L.load().a3d_last_error()
    torch.cuda.synchronize()
    index.close()


def test_ties_go_to_the_lowest_row_whatever_the_cells():
    rng = np.random.default_rng(9)
    base = cloud(200, 10, 1.0)
    src = np.concatenate([base, base[::3], base[::5]])             # exact duplicates at higher rows
    src = src[rng.permutation(len(src))]
    got = check(src, np.concatenate([base, base + F32(0.01)]), 0.2, 0.1)
    first = {p.tobytes(): i for i, p in reversed(list(enumerate(src)))}
    assert got["nearest"][:200].tolist() == [first[p.tobytes()] for p in base]
    # midway between two points in DIFFERENT cells, both exactly 0.125 away: the lower row, in both orders of the rows
    a, b, q = [0.125, 0.1, 0.1], [0.375, 0.1, 0.1], np.array([[0.25, 0.1, 0.1]], F32)
    for pair in ([a, b], [b, a]):
        got = check(np.array(pair, F32), q, 0.25, 0.125)
        assert got["nearest"].tolist() == [0] and got["d2"].tolist() == [0.015625]
    corners = np.array([[x, y, z] for z in (0.1875, 0.3125) for y in (0.1875, 0.3125) for x in (0.1875, 0.3125)], F32)   # eight cells
    for order in (np.arange(8), np.arange(8)[::-1], rng.permutation(8)):
        assert check(corners[order], np.full((1, 3), 0.25, F32), 0.25, 0.125)["nearest"].tolist() == [0]


# ------------------------------------------------------------------------------------------- random sets, far from the origin
@pytest.fixture(scope="module")
def random_sets():
    rng = np.random.default_rng(11)
    src = rng.uniform(0.0, 2.0, (5000, 3))
    q = np.concatenate([src[:2500] + rng.uniform(-0.03, 0.03, (2500, 3)), rng.uniform(-0.1, 2.1, (2500, 3))])
    return src, q


@pytest.mark.parametrize("shift", [0.0, 1000.0, -1000.0])
def test_random_sets_in_a_2_m_box(random_sets, shift):
    src, q = random_sets
    got = check((src + shift).astype(F32), (q + shift).astype(F32), 0.1, 0.05, labels=np.arange(5000) % 251, fill=255)
    assert 2500 <= got["matched"] < 5000


def test_random_sources_on_a_plane(random_sets):
    src, q = (a.copy() for a in random_sets)
    src[:, 2] = 0.3
    q[:, 2] = 0.3 + (q[:, 2] - 1.0) * 0.04
    got = check(src.astype(F32), q.astype(F32), 0.1, 0.05)
    assert 1500 <= got["matched"] < 5000


# ------------------------------------------------------------------------------------------- rows and queries that are not finite
def test_rows_and_queries_that_are_not_finite():
    src = cloud(500, 12, 0.5)
    odd = np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [np.nan, np.nan, np.nan]], F32)
    src[[0, 17, 256, 499]] = odd
    q = np.concatenate([cloud(100, 13, 0.5), odd, src[[1, 16, 255]]])
    got = check(src, q, 0.1, 0.05, labels=np.arange(500), fill=-1)
    assert got["source_left_out"] == 4 and got["nonfinite"] == 4 and not np.isin(got["nearest"], [0, 17, 256, 499]).any()
    assert got["nearest"][100:104].tolist() == [-1] * 4 and np.isinf(got["d2"][100:104]).all()
    none = check(np.concatenate([odd, odd]), q, 0.1, 0.05, labels=np.arange(8), fill=9)         # a source of such rows only
    assert none["matched"] == 0 and none["source_left_out"] == 8 and set(none["labels"].tolist()) == {9}


def test_empty_source_and_no_queries():
    got = check(np.zeros((0, 3), F32), cloud(70, 14), 0.1, 0.05, labels=np.zeros(0, np.int32), fill=4)
    assert got["unmatched"] == 70 and set(got["labels"].tolist()) == {4}
    got = check(cloud(70, 14), np.zeros((0, 3), F32), 0.1, 0.05, labels=np.arange(70))
    assert (got["matched"], got["unmatched"], got["nonfinite"]) == (0, 0, 0)


# ------------------------------------------------------------------------------------------- where r2 is not a normal number
def test_reaches_whose_square_is_not_a_normal_number():
    """max_distance below 2^-63 (r2 rounds to 0 or a subnormal) or from 2^64 on (r2 = +inf): the 27 cells no longer enclose what the
    rule accepts, and the library tests every row instead.  The rule is the same."""
    rng = np.random.default_rng(15)
    tiny = (rng.integers(-1000, 1000, (300, 3)) * 1e-22).astype(F32)                            # within 2^20 cells of 2e-25
    got = check(tiny, np.concatenate([tiny[::2], tiny[:50] + F32(3e-23)]), 2e-25, 1e-25)
    assert got["matched"] >= 150                              # d2 underflows to 0 <= r2 == 0 far beyond "max_distance"
    got = check(tiny, tiny, 4e-20, 2e-20)                     # r2 = 4e-40, a subnormal
    assert got["matched"] == 300
    big = (rng.uniform(-1, 1, (300, 3)) * 1e24).astype(F32)
    got = check(big, (rng.uniform(-1, 1, (80, 3)) * 3e24).astype(F32), 4e20, 2e20)               # r2 = +inf: everything is in reach
    assert got["matched"] == 80
    check(np.array([[3e38, 0, 0], [0, 1e20, 0]], F32), np.array([[-3e38, 0, 0], [0, 0, 0]], F32), 1e38, 2e20)   # d2 = +inf is accepted


# ------------------------------------------------------------------------------------------- labels, repeatability
def test_labels_are_the_gather_by_nearest_and_two_calls_give_the_same_bytes():
    src, q = cloud(3000, 16, 1.0), cloud(3000, 17, 1.2)
    labels = np.random.default_rng(18).integers(-5, 300, 3000).astype(np.int32)
    a = run(src, q, 0.1, 0.05, labels, fill=-77)
    assert a["labels"].tolist() == np.where(a["nearest"] >= 0, labels[np.maximum(a["nearest"], 0)], -77).tolist()
    assert 0 < a["unmatched"] < 3000
    b = run(src, q, 0.1, 0.05, labels, fill=-77)
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("nearest", "d2", "labels"))
    # without d2 and without labels: the same rows; an index in a workspace of the caller's, larger than needed
    dev_src, dev_q = _dev(src, F32), _dev(q, F32)
    ws = torch.empty(V.point_index_workspace(3000, DEV).shape[0] + 4096, dtype=torch.uint8, device=DEV)
    index = V.point_index_create(dev_src, 0.1, workspace=ws)
    nearest, d2, lab, _ = V.point_index_nearest(index, dev_q, 0.05, d2=False)
    assert d2 is None and lab is None and nearest.cpu().numpy().tobytes() == a["nearest"].tobytes()
    assert V.point_index_nearest(index, dev_q, 0.025)[0].cpu().numpy().tolist() == R.nearest(src, q, 0.025)["nearest"].tolist()   # a shorter reach, the same index
    index.close()
    with pytest.raises(ValueError, match="index"):
        V.point_index_nearest(index, dev_q, 0.05)
