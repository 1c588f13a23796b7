"""Host side of the label transfer (no GPU): the brute-force rule's restatement (``transfer_rule.py``) on hand-made cases; every
``ValueError`` the ``view.py`` wrappers of the point index raise before the library is reached; the entry points' own refusals
that need no index; the workspace size at its edges.  ``test_gpu_transfer.py`` holds the kernels to the same restatement bit
for bit (and, with a real index, the refusals of the query that need one)."""
import ctypes as C

import numpy as np
import pytest

import transfer_rule as R
from pick_rule import fp32_rule_argmin

F32 = np.float32


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


# ------------------------------------------------------------------------------------------- the restatement
def test_rule_on_hand_made_cases():
    src = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [0.25, 0, 0], [np.inf, 1, 1]], F32)
    q = np.array([[0, 0, 0], [0.9, 0, 0], [0.5, 0.5, 0.5], [np.nan, 0, 0], [0.125, 0, 0], [0, -np.inf, 0]], F32)
    r = R.nearest(src, q, 0.25, labels=[10, 11, 12, 13, 14, 15], fill=-3)
    # a duplicate gives the lowest row; 0.1 away is in reach; nothing within 0.25 of the cube's centre; a NaN query; a query
    # midway between rows 0 and 4 (both 0.125 away) gives the lower; an infinite query
    assert r["nearest"].tolist() == [0, 1, -1, -1, 0, -1]
    assert r["labels"].tolist() == [10, 11, -3, -3, 10, -3]
    assert r["d2"][[0, 4]].tolist() == [0.0, 0.015625] and np.isinf(r["d2"][[2, 3, 5]]).all()
    d = F32(1) - F32(0.9)
    assert r["d2"][1].tobytes() == F32(d * d).tobytes()
    assert (r["matched"], r["unmatched"], r["nonfinite"], r["source_left_out"]) == (3, 1, 2, 2)
    # with everything in reach it is a3d_nearest_rows' first arg-min over the finite rows
    rng = np.random.default_rng(1)
    src, q = rng.uniform(-1, 1, (300, 3)).astype(F32), rng.uniform(-1, 1, (40, 3)).astype(F32)
    got = R.nearest(src, q, 10.0)["nearest"]
    assert got.tolist() == [fp32_rule_argmin(src, p) for p in q]


def test_rule_cutoff_is_inclusive_in_fp32():
    r = F32(0.05)
    src = np.zeros((1, 3), F32)
    for axis in range(3):
        at, beyond = np.zeros((1, 3), F32), np.zeros((1, 3), F32)
        at[0, axis], beyond[0, axis] = r, np.nextafter(r, F32(1))
        assert R.nearest(src, at, r)["nearest"].tolist() == [0] and R.nearest(src, -at, r)["nearest"].tolist() == [0]
        assert R.nearest(src, beyond, r)["nearest"].tolist() == [-1]
    # r2 is rounded once: a d2 that equals it bit for bit is in reach, whatever the real numbers say
    assert R.nearest(src, at, r)["d2"].tobytes() == F32(r * r).tobytes()


def test_rule_where_r2_is_not_a_normal_number():
    tiny = np.array([[0, 0, 0], [1e-30, 0, 0]], F32)
    r = R.nearest(tiny, tiny, 1e-25)                         # r2 == 0: only d2 == 0 is in reach, which 1e-30 apart is
    assert r["nearest"].tolist() == [0, 0] and r["d2"].tolist() == [0.0, 0.0]
    far = np.array([[3e38, 0, 0], [0, 1, 0]], F32)
    r = R.nearest(far, np.array([[-3e38, 0, 0], [0, 0, 0]], F32), 1e20)     # r2 == +inf accepts a d2 of +inf
    assert r["nearest"].tolist() == [0, 1] and np.isinf(r["d2"][0]) and r["d2"][1] == 1.0     # (both rows are +inf away from the first)
    r = R.nearest(far[:1], np.array([[-3e38, 0, 0]], F32), 1e20)
    assert r["nearest"].tolist() == [0] and r["matched"] == 1


def test_rule_edges_and_unkeyable():
    none = R.nearest(np.zeros((0, 3), F32), np.zeros((2, 3), F32), 1.0, labels=np.zeros(0, np.int32), fill=7)
    assert none["nearest"].tolist() == [-1, -1] and none["labels"].tolist() == [7, 7] and none["unmatched"] == 2
    assert R.nearest(np.zeros((3, 3), F32), np.zeros((0, 3), F32), 1.0)["nearest"].shape == (0,)
    only_odd = R.nearest(np.full((4, 3), np.nan, F32), np.zeros((1, 3), F32), 1.0)
    assert only_odd["nearest"].tolist() == [-1] and only_odd["source_left_out"] == 4
    cell = F32(0.5)
    assert not R.unkeyable([[-(1 << 19), 0, 1 << 19]], cell)            # cells -2^20 and 2^20: the last that can be keyed
    assert not R.unkeyable([[(1 << 19) + 0.25, 0, 0]], cell)           # still floor = 2^20
    assert R.unkeyable([[0, (1 << 19) + 0.5, 0]], cell) and R.unkeyable([[-(1 << 19) - 0.25, 0, 0]], cell)
    assert not R.unkeyable([[np.inf, 0, 0], [np.nan, 1e30, 0]], cell)  # rows that are not finite are left out, not unkeyable


# ------------------------------------------------------------------------------------------- the wrappers' refusals
def test_wrappers_refuse_before_the_library():
    import torch
    from agile3d_amd import view as V
    _lib()
    assert (V.TRANSFER_UNKEYABLE, V.POINT_INDEX_MAX_CELLS) == (R.UNKEYABLE, R.MAX_CELLS) and V.TRANSFER_SUMMARY.itemsize == 40
    xyz = torch.zeros((4, 3), dtype=torch.float32)
    for bad in (xyz, None, np.zeros((4, 3), np.float32)):
        with pytest.raises(ValueError, match="GPU"):
            V.point_index_create(bad, 0.1)

    class OnGpu(torch.Tensor):                          # a stand-in for a device tensor: the host checks are reached without a GPU
        device = torch.device("cuda", 0)
    fake = lambda t: t.as_subclass(OnGpu)
    dev = OnGpu.device
    ws = fake(torch.zeros(1 << 20, dtype=torch.uint8))
    for name, bad in (("xyz", dict(xyz=fake(torch.zeros((4, 2))))), ("xyz", dict(xyz=fake(torch.zeros((4, 3), dtype=torch.float64)))),
                      ("xyz", dict(xyz=fake(torch.zeros((3, 4)).t()))), ("cell_size", dict(cell_size=0.0)),
                      ("cell_size", dict(cell_size=-1.0)), ("cell_size", dict(cell_size=np.nan)), ("cell_size", dict(cell_size=np.inf)),
                      ("cell_size", dict(cell_size=1e39)), ("cell_size", dict(cell_size=1e-50)),
                      ("workspace", dict(workspace=fake(torch.zeros(256, dtype=torch.uint8)))),
                      ("workspace", dict(workspace=fake(torch.zeros(1 << 20, dtype=torch.float32)))),
                      ("workspace", dict(workspace=torch.zeros(1 << 20, dtype=torch.uint8)))):
        with pytest.raises(ValueError, match=name):
            V.point_index_create(**dict(dict(xyz=fake(xyz), cell_size=0.1, workspace=ws), **bad))
    # the query: an index that is closed or none at all, then every argument against an index that only looks open
    closed = V.PointIndex(None, None, 4, 0.5, dev)
    q = fake(torch.zeros((5, 3)))
    for index in (closed, None, object()):
        with pytest.raises(ValueError, match="index"):
            V.point_index_nearest(index, q, 0.25)
    index = V.PointIndex(C.c_void_p(0), None, 4, 0.5, dev)
    try:
        base = dict(index=index, queries=q, max_distance=0.25, nearest=fake(torch.zeros(5, dtype=torch.int32)), d2=False,
                    summary=fake(torch.zeros(40, dtype=torch.uint8)))      # (every output given: nothing is allocated on a device)
        lab = fake(torch.zeros(4, dtype=torch.int32))
        for name, bad in (("queries", dict(queries=torch.zeros((5, 3)))), ("queries", dict(queries=np.zeros((5, 3), np.float32))),
                          ("queries", dict(queries=fake(torch.zeros((5, 2))))), ("queries", dict(queries=fake(torch.zeros((5, 3), dtype=torch.float64)))),
                          ("max_distance", dict(max_distance=0.0)), ("max_distance", dict(max_distance=-0.1)),
                          ("max_distance", dict(max_distance=np.nan)), ("max_distance", dict(max_distance=np.inf)),
                          ("max_distance", dict(max_distance=0.26)), ("max_distance", dict(max_distance=np.nextafter(F32(0.25), F32(1)))),
                          ("labels_src", dict(labels_src=fake(torch.zeros(5, dtype=torch.int32)))),
                          ("labels_src", dict(labels_src=fake(torch.zeros(4, dtype=torch.int64)))),
                          ("labels_src", dict(labels_src=torch.zeros(4, dtype=torch.int32))),
                          ("labels", dict(labels=fake(torch.zeros(5, dtype=torch.int32)))),
                          ("labels", dict(labels_src=lab, labels=fake(torch.zeros(4, dtype=torch.int32)))),
                          ("fill", dict(labels_src=lab, fill=1 << 31)), ("fill", dict(labels_src=lab, fill=0.5)),
                          ("nearest", dict(nearest=fake(torch.zeros(4, dtype=torch.int32)))), ("nearest", dict(nearest=fake(torch.zeros(5)))),
                          ("d2", dict(d2=fake(torch.zeros(5, dtype=torch.int32)))), ("summary", dict(summary=fake(torch.zeros(39, dtype=torch.uint8))))):
            with pytest.raises(ValueError, match=name):
                V.point_index_nearest(**dict(base, **bad))
    finally:
        index.handle = None                             # (nothing to free)
    # the summary's decoding, and what its error word raises
    rec = lambda err: np.array([(5, 2, 1, 3, err, 0)], V.TRANSFER_SUMMARY).view(np.uint8)
    assert V.read_transfer_summary(rec(0)) == dict(matched=5, unmatched=2, nonfinite=1, source_left_out=3, err=0)
    assert V.read_transfer_summary(rec(V.TRANSFER_UNKEYABLE), check=False)["err"] == V.TRANSFER_UNKEYABLE
    with pytest.raises(ValueError, match="cells"):
        V.read_transfer_summary(rec(V.TRANSFER_UNKEYABLE))
    with pytest.raises(RuntimeError, match="sort"):
        V.read_transfer_summary(rec(V.TRANSFER_SORT_FAILED))


# ------------------------------------------------------------------------------------------- the entry points' own refusals
def test_workspace_size_at_its_edges():
    _, L = _lib()
    assert L.a3d_point_index_workspace_bytes(-1) == 0 and L.a3d_point_index_workspace_bytes(1 << 31) == 0
    assert L.a3d_point_index_workspace_bytes(1 << 40) == 0
    sizes = [L.a3d_point_index_workspace_bytes(n) for n in (0, 1, 1000, 1 << 20, (1 << 31) - 1)]
    assert all(b > 0 and b % 256 == 0 for b in sizes) and sizes == sorted(sizes)
    for n, b in zip((1000, 1 << 20, (1 << 31) - 1), sizes[2:]):
        # the sort's pairs twice, the sorted points, a table of at least 2 n slots (key and value)
        assert b >= n * (2 * 12 + 16) + 2 * n * 12


def test_library_refuses_without_a_gpu():
    lib, L = _lib()
    assert C.sizeof(lib.TransferSummary) == 40
    out = C.c_void_p(123)
    create = lambda *a: L.a3d_point_index_create(*a)
    ws, big = 1 << 20, 1 << 30                          # (addresses that are never followed: every call is refused first)
    for args in ((None, 4, 0.1, ws, big, None, C.byref(out)),             # rows without coordinates
                 (256, -1, 0.1, ws, big, None, C.byref(out)), (256, 1 << 31, 0.1, ws, big, None, C.byref(out)),
                 (256, 4, 0.0, ws, big, None, C.byref(out)), (256, 4, -0.5, ws, big, None, C.byref(out)),
                 (256, 4, float("nan"), ws, big, None, C.byref(out)), (256, 4, float("inf"), ws, big, None, C.byref(out)),
                 (256, 4, 0.1, None, big, None, C.byref(out)), (256, 4, 0.1, ws + 8, big, None, C.byref(out)),
                 (256, 4, 0.1, ws, big, None, None)):
        assert create(*args) == lib.A3D_ERR_INVALID, args
        assert b"a3d_point_index_create" in L.a3d_last_error()
    assert out.value is None                            # a refused call leaves no handle behind
    need = L.a3d_point_index_workspace_bytes(4)
    assert create(256, 4, 0.1, ws, need - 1, None, C.byref(out)) == lib.A3D_ERR_WORKSPACE and b"too small" in L.a3d_last_error()
    # the query without an index, whatever else it is given
    assert L.a3d_point_index_nearest(None, 256, 4, 0.05, None, 0, 256, None, None, 256, None) == lib.A3D_ERR_INVALID
    assert b"a3d_point_index_nearest" in L.a3d_last_error()
    L.a3d_point_index_destroy(None)                     # as free(NULL)
