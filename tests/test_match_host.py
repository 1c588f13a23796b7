"""Host side of the query by example (no GPU): the rule's restatement (``match_rule.py``) on hand-made cases; the caller's
prototype step of ``view.prototype_table`` against it; every ``ValueError`` the ``view.py`` wrappers raise before the library is
reached; the entry points' own refusals that need no device memory; the ranking of candidates on plain records.
``test_gpu_match.py`` holds the kernels to the same restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import match_rule as R

F32 = np.float32
Q = F32(2.0 ** -20)


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def example(seed=0):
    """One fp32 [128] row whose channels are multiples of 2^-20 (|f| < 4)."""
    return (np.random.default_rng(seed).integers(-(1 << 21), 1 << 21, R.CHANNELS) * np.float64(Q)).astype(F32)


# ------------------------------------------------------------------------------------------- the restatement
def test_a_single_example_is_its_own_prototype():
    e = example()
    assert (e.astype(np.float64) / R.QUANTUM == np.rint(e.astype(np.float64) / R.QUANTUM)).all()
    p = R.prototypes(np.stack([example(1), e, example(2)]), [-1, 3, -1], n_classes=5)
    assert p["count"].tolist() == [0, 0, 0, 1, 0] and (p["examples"], p["examples_left_out"], p["err"]) == (1, 0, 0)
    table = R.prototype_table(p["sums"], p["count"])
    assert sorted(table) == [3] and table[3].tobytes() == e.tobytes()          # an empty class gets no prototype
    # the mean of two: in fixed point, rounded once
    a, b = example(3), example(4)
    p = R.prototypes(np.stack([a, b]), [0, 0], n_classes=1)
    want = ((np.rint(a / np.float64(Q)) + np.rint(b / np.float64(Q))) / 2.0 * R.QUANTUM).astype(F32)
    assert R.prototype_table(p["sums"], p["count"])[0].tobytes() == want.tobytes()


def test_threshold_of_exactly_one():
    e = example()
    off = e.copy()
    # one channel moved by 2^-10: 1 - cos is of SECOND order in the angle, about (2^-10 / |e|)^2 / 2 > 1e-10 here, far above
    # the 1e-16 a double resolves (a change of one fp32 ulp, 1e-17 in 1 - cos, would be below it and pass)
    off[17] += F32(2.0 ** -10)
    ortho = np.zeros(R.CHANNELS, F32)
    ortho[0], ortho[1] = e[1], -e[0]                                         # dot == 0 exactly (e[0] e[1] - e[1] e[0])
    assert e[0] != 0 and e[1] != 0
    feats = np.stack([e, 2 * e, F32(0.5) * e, off, ortho, -e])
    r = R.match(feats, e[None], [7], 1.0)
    assert r["match_qv"].tolist() == [7, 7, 7, -1, -1, -1]                   # the equality is met exactly, one ulp off fails
    assert r["best_qv"].tolist() == [0] * 6 and r["matched"][7] == 3 and r["matched"].sum() == 3
    assert r["score_qv"][:3].tolist() == [1.0, 1.0, 1.0] and r["score_qv"][4] == 0.0 and r["score_qv"][5] == -1.0
    assert 0.99999 < r["score_qv"][3] <= 1.0
    # an orthogonal voxel fails at cos_min = 0 too (dot > 0 is part of the test), an opposite one as well
    r0 = R.match(feats, e[None], [7], 0.0)
    assert r0["match_qv"].tolist() == [7, 7, 7, 7, -1, -1]


def test_ties_and_the_order_of_the_scan():
    e, other = example(), example(5)
    v = (e + F32(0.25) * other).astype(F32)
    r = R.match(v[None], np.stack([e, e]), [4, 9], 0.5)
    assert (r["match_qv"].tolist(), r["best_qv"].tolist()) == ([4], [0])     # two identical prototypes: the lower index wins
    r = R.match(v[None], np.stack([other, e, 2 * e, e]), [1, 2, 3, 4], 0.5)
    assert (r["match_qv"].tolist(), r["best_qv"].tolist()) == ([2], [1])     # 2 e has e's cosine exactly: no replacement
    # best counts prototypes that do not pass; signs: a zero dot beats a negative one, the smaller negative cosine loses
    r = R.match(e[None], np.stack([-e, (-e - other).astype(F32)]), [1, 2], 0.9)
    assert (r["match_qv"].tolist(), r["best_qv"].tolist()) == ([-1], [1]) and -1.0 < r["score_qv"][0] < 0.0
    ortho = np.zeros(R.CHANNELS, F32)
    ortho[0], ortho[1] = e[1], -e[0]
    assert R.match(e[None], np.stack([-e, ortho, -e]), [1, 2, 3], 0.9)["best_qv"].tolist() == [1]
    # a zero prototype takes part in nothing; alone, the voxel has no best
    zero = np.zeros(R.CHANNELS, F32)
    r = R.match(e[None], np.stack([zero, e]), [1, 2], 0.9)
    assert (r["match_qv"].tolist(), r["best_qv"].tolist()) == ([2], [1])
    r = R.match(e[None], zero[None], [1], 0.0)
    assert (r["match_qv"].tolist(), r["best_qv"].tolist(), r["score_qv"].tolist(), r["err"]) == ([-1], [-1], [0.0], 0)


def test_rows_that_cannot_be_scored_and_examples_left_out():
    e = example()
    nan, inf, big, zero = e.copy(), e.copy(), e.copy(), np.zeros(R.CHANNELS, F32)
    nan[5], inf[127], big[0] = np.nan, -np.inf, F32(2.0 ** 20) + F32(0.125)
    edge = e.copy()
    edge[0] = F32(2.0 ** 20)                                                 # X == 2^40: the last value that is accepted
    feats = np.stack([e, nan, inf, big, zero, edge])
    p = R.prototypes(feats, [1, 1, 1, 1, 1, 1], n_classes=2)
    assert (p["examples"], p["examples_left_out"], p["count"].tolist()) == (3, 3, [0, 3])     # nan, inf, big are left out whole
    assert p["sums"][1, 0] == int(np.rint(e[0] / np.float64(Q))) + 0 + (1 << 40)            # e, zero, edge
    r = R.match(feats, e[None], [1], 0.5, candidate=[1, 1, 1, 1, 1, 0])
    assert r["rows_nonfinite"] == 2 and r["best_qv"].tolist() == [0, -1, -1, 0, -1, -1]       # big is finite: it is scored
    assert r["match_qv"].tolist() == [1, -1, -1, -1, -1, -1] and r["score_qv"][[1, 2, 4, 5]].tolist() == [0.0] * 4
    # class values outside -1 .. n_classes-1: the bit, and the row is no example
    p = R.prototypes(feats[:3], [-2, 2, 0], n_classes=2)
    assert (p["err"], p["examples"], p["examples_left_out"]) == (R.BAD_CLASS, 0, 1)
    # the match's error bits: a prototype that is not finite, a class outside 0..255, an index outside the rows
    r = R.match(feats[:1], np.stack([nan, e]), [1, 256], 0.5, inverse_map=[0, 1, -1, 0])
    assert r["err"] == R.BAD_PROTOTYPE | R.BAD_CLASS | R.BAD_INDEX and r["match_qv"].tolist() == [256] and r["matched"].sum() == 0
    assert r["match_full"].tolist() == [256, -7, -7, 256] and r["score_full"].tolist() == [1.0, -7.0, -7.0, 1.0]


def test_sums_do_not_depend_on_the_order_of_the_rows():
    rng = np.random.default_rng(6)
    feats = rng.standard_normal((300, R.CHANNELS)).astype(F32)
    classes = rng.integers(-1, 4, 300)
    a = R.prototypes(feats, classes, n_classes=4)
    perm = rng.permutation(300)
    b = R.prototypes(feats[perm], classes[perm], n_classes=4)
    assert a["sums"].tobytes() == b["sums"].tobytes() and a["count"].tolist() == b["count"].tolist()
    assert a["count"].sum() == (classes >= 0).sum()


def test_view_prototype_table_is_the_rules_host_step():
    import torch
    from agile3d_amd import view as V
    rng = np.random.default_rng(7)
    p = R.prototypes(rng.standard_normal((500, R.CHANNELS)).astype(F32) * F32(3.0), rng.integers(-1, 6, 500), n_classes=7)
    assert p["count"][6] == 0
    want = R.prototype_table(p["sums"], p["count"])
    for got in (V.prototype_table(p["sums"], p["count"]), V.prototype_table(torch.from_numpy(p["sums"]), torch.from_numpy(p["count"])).numpy()):
        assert got.dtype == F32 and got.shape == (7, R.CHANNELS) and not got[6].any()        # no prototype: a zero row
        assert all(got[c].tobytes() == want[c].tobytes() for c in want)
    assert (V.MATCH_QUANTUM, V.MATCH_CHANNELS, V.MATCH_MAX_PROTOTYPES) == (R.QUANTUM, R.CHANNELS, R.MAX_PROTOTYPES)
    assert (V.MATCH_BAD_CLASS, V.MATCH_BAD_INDEX, V.MATCH_BAD_PROTOTYPE) == (R.BAD_CLASS, R.BAD_INDEX, R.BAD_PROTOTYPE)
    for bad in ((p["sums"].astype(np.int32), p["count"]), (p["sums"], p["count"][:3]), (p["sums"][:, :5], p["count"]),
                (torch.from_numpy(p["sums"]), p["count"]), (p["sums"], p["count"].astype(np.int64))):
        with pytest.raises(ValueError):
            V.prototype_table(*bad)


# ------------------------------------------------------------------------------------------- the wrappers' refusals
def test_wrappers_refuse_before_the_library():
    import torch
    from agile3d_amd import view as V
    _lib()

    class OnGpu(torch.Tensor):                          # a stand-in for a device tensor: the host checks are reached without a GPU
        device = torch.device("cuda", 0)
    fake = lambda t: t.as_subclass(OnGpu)
    feats = fake(torch.zeros((5, 128)))
    for bad in (torch.zeros((5, 128)), None, np.zeros((5, 128), np.float32)):
        with pytest.raises(ValueError, match="GPU"):
            V.feature_prototypes(bad, fake(torch.zeros(5, dtype=torch.int32)))
        with pytest.raises(ValueError, match="GPU"):
            V.feature_match(bad, np.ones((1, 128), np.float32), fake(torch.zeros(1, dtype=torch.int32)), 0.9)
    base = dict(feats=feats, classes=fake(torch.zeros(5, dtype=torch.int32)), n_classes=4, sums=fake(torch.zeros((4, 128), dtype=torch.int64)),
                count=fake(torch.zeros(4, dtype=torch.int32)), summary=fake(torch.zeros(24, dtype=torch.uint8)))
    for name, bad in (("feats", dict(feats=fake(torch.zeros((5, 127))))), ("feats", dict(feats=fake(torch.zeros((5, 128), dtype=torch.float64)))),
                      ("feats", dict(feats=fake(torch.zeros((128, 5)).t()))), ("feats", dict(feats=fake(torch.zeros(640)))),
                      ("classes", dict(classes=fake(torch.zeros(4, dtype=torch.int32)))), ("classes", dict(classes=fake(torch.zeros(5, dtype=torch.int64)))),
                      ("classes", dict(classes=torch.zeros(5, dtype=torch.int32))), ("classes", dict(classes=None)),
                      ("n_classes", dict(n_classes=0)), ("n_classes", dict(n_classes=257)), ("n_classes", dict(n_classes=2.5)),
                      ("sums", dict(sums=fake(torch.zeros((3, 128), dtype=torch.int64)))), ("sums", dict(sums=fake(torch.zeros((4, 128), dtype=torch.int32)))),
                      ("count", dict(count=fake(torch.zeros(5, dtype=torch.int32)))), ("summary", dict(summary=fake(torch.zeros(23, dtype=torch.uint8))))):
        with pytest.raises(ValueError, match=name):
            V.feature_prototypes(**dict(base, **bad))
    protos = fake(torch.ones((3, 128)))
    i32 = lambda *shape: fake(torch.zeros(shape, dtype=torch.int32))
    base = dict(feats=feats, protos=protos, proto_class=i32(3), cos_min=0.9, match_qv=i32(5), best_qv=i32(5), score_qv=fake(torch.zeros(5)),
                summary=fake(torch.zeros(2064, dtype=torch.uint8)))           # (every output given: nothing is allocated on a device)
    lift = dict(inverse_map=fake(torch.zeros(9, dtype=torch.int64)), match_full=i32(9), score_full=fake(torch.zeros(9)))
    host = np.ones((2, 128), np.float32)
    for name, bad in (("feats", dict(feats=fake(torch.zeros((5, 64))))), ("feats", dict(feats=fake(torch.zeros((5, 128), dtype=torch.float16)))),
                      ("protos", dict(protos=fake(torch.ones((3, 127))))), ("protos", dict(protos=fake(torch.ones((0, 128))))),
                      ("protos", dict(protos=fake(torch.ones((257, 128))))), ("protos", dict(protos=fake(torch.ones((128, 3)).t()))),
                      ("protos", dict(protos=np.ones((2, 128), np.float64))), ("protos", dict(protos=np.ones((0, 128), np.float32))),
                      ("protos", dict(protos=np.ones((257, 128), np.float32))), ("protos", dict(protos=np.ones(128, np.float32))),
                      ("protos must be finite", dict(protos=np.where(np.arange(256).reshape(2, 128) == 200, np.nan, host).astype(np.float32))),
                      ("protos must be finite", dict(protos=torch.full((2, 128), float("inf")))),
                      ("proto_class", dict(proto_class=i32(2))), ("proto_class", dict(proto_class=fake(torch.zeros(3, dtype=torch.int64)))),
                      ("proto_class", dict(proto_class=torch.zeros(3, dtype=torch.int32))),
                      ("cos_min", dict(cos_min=-0.01)), ("cos_min", dict(cos_min=1.0001)), ("cos_min", dict(cos_min=np.nan)),
                      ("cos_min", dict(cos_min=np.inf)), ("cos_min", dict(cos_min=None)), ("cos_min", dict(cos_min="high")),
                      ("candidate", dict(candidate=fake(torch.zeros(4, dtype=torch.uint8)))), ("candidate", dict(candidate=fake(torch.zeros(5, dtype=torch.bool)))),
                      ("candidate", dict(candidate=torch.zeros(5, dtype=torch.uint8))),
                      ("inverse_map", dict(lift, inverse_map=fake(torch.zeros(9, dtype=torch.int32)))),
                      ("inverse_map", dict(match_full=i32(9))), ("inverse_map", dict(score_full=fake(torch.zeros(9)))),
                      ("match_full", dict(lift, match_full=i32(8))), ("score_full", dict(lift, score_full=i32(9))),
                      ("match_qv", dict(match_qv=i32(4))), ("best_qv", dict(best_qv=fake(torch.zeros(5)))), ("score_qv", dict(score_qv=i32(5))),
                      ("summary", dict(summary=fake(torch.zeros(2063, dtype=torch.uint8))))):
        with pytest.raises(ValueError, match=name):
            V.feature_match(**dict(base, **bad))
    # the summaries' decoding
    rec = np.zeros(1, V.MATCH_SUMMARY)
    rec["matched"][0, [1, 255]], rec["rows_nonfinite"], rec["err"] = (5, 7), 3, V.MATCH_BAD_INDEX
    s = V.read_match_summary(rec.view(np.uint8))
    assert s["matched"].tolist() == [0, 5] + [0] * 253 + [7] and (s["rows_nonfinite"], s["err"]) == (3, V.MATCH_BAD_INDEX)
    rec = np.array([(9, 2, V.MATCH_BAD_CLASS, 0)], V.PROTOTYPES_SUMMARY)
    assert V.read_prototypes_summary(rec.view(np.uint8)) == dict(examples=9, examples_left_out=2, err=V.MATCH_BAD_CLASS)


# ------------------------------------------------------------------------------------------- the entry points' own refusals
def test_library_refuses_without_a_gpu():
    lib, L = _lib()
    assert (C.sizeof(lib.PrototypesSummary), C.sizeof(lib.FeaturePrototypesArgs)) == (24, 56)
    assert (C.sizeof(lib.MatchSummary), C.sizeof(lib.FeatureMatchArgs)) == (2064, 120)
    assert (lib.A3D_MATCH_CHANNELS, lib.A3D_MATCH_QUANTUM_BITS, lib.A3D_MATCH_MAX_PROTOTYPES) == (128, 20, 256)
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "agile3d_hip.h")).read()
    for name in ("CHANNELS", "QUANTUM_BITS", "FIXED_BITS", "MAX_PROTOTYPES", "CHUNK", "BAD_CLASS", "BAD_INDEX", "BAD_PROTOTYPE"):
        value = __import__("re").search(rf"#define A3D_MATCH_{name}\s+(\d+)", hdr).group(1)
        assert int(value) == getattr(lib, f"A3D_MATCH_{name}"), name
    assert L.a3d_feature_prototypes(None, None) == lib.A3D_ERR_INVALID and b"a3d_feature_prototypes" in L.a3d_last_error()
    assert L.a3d_feature_match(None, None) == lib.A3D_ERR_INVALID and b"a3d_feature_match" in L.a3d_last_error()
    at = 1 << 20                                         # (an address that is never followed: every call is refused first)

    def protos_args(**kw):
        a = lib.FeaturePrototypesArgs(feats_dev=at, classes_dev=at, n=4, sums_dev=at, count_dev=at, summary_dev=at, n_classes=3)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for bad in (dict(n=-1), dict(n=1 << 22), dict(n_classes=0), dict(n_classes=257), dict(feats_dev=None), dict(classes_dev=None),
                dict(feats_dev=at + 8), dict(sums_dev=None), dict(sums_dev=at + 4), dict(count_dev=None), dict(summary_dev=None),
                dict(summary_dev=at + 4)):
        assert L.a3d_feature_prototypes(C.byref(protos_args(**bad)), None) == lib.A3D_ERR_INVALID, bad
        assert b"a3d_feature_prototypes" in L.a3d_last_error()

    def match_args(**kw):
        a = lib.FeatureMatchArgs(feats_dev=at, n=4, protos_dev=at, proto_class_dev=at, match_qv_dev=at, best_qv_dev=at, score_qv_dev=at,
                                 summary_dev=at, cos_min=0.9, k=2)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    lift = dict(inverse_map_dev=at, n_full=6, match_full_dev=at, score_full_dev=at)
    for bad in (dict(n=-1), dict(n=1 << 31), dict(k=0), dict(k=257), dict(feats_dev=None), dict(feats_dev=at + 4), dict(protos_dev=None),
                dict(proto_class_dev=None), dict(match_qv_dev=None), dict(best_qv_dev=None), dict(score_qv_dev=None),
                dict(summary_dev=None), dict(summary_dev=at + 4), dict(cos_min=-0.5), dict(cos_min=1.5), dict(cos_min=float("nan")),
                dict(n_full=6), dict(match_full_dev=at), dict(score_full_dev=at), dict(lift, match_full_dev=None),
                dict(lift, score_full_dev=None), dict(lift, n_full=-1), dict(lift, n_full=1 << 31)):
        assert L.a3d_feature_match(C.byref(match_args(**bad)), None) == lib.A3D_ERR_INVALID, bad
        assert b"a3d_feature_match" in L.a3d_last_error()


# ------------------------------------------------------------------------------------------- the candidates' ranking
def test_candidates_are_ranked_by_depth_on_plain_records():
    from agile3d_amd.session import rank_candidates, rank_spots
    regions = [dict(root=40, key=2, voxels=30), dict(root=7, key=1, voxels=30), dict(root=90, key=1, voxels=55), dict(root=3, key=1, voxels=9)]
    order = rank_spots(regions)
    assert order == [2, 1, 0, 3]                                             # by size, ties to the lower root
    spots = [regions[k] for k in order]
    clusters = [dict(cluster_id=96 * 3, row=41, label=3, pred=0, error_size=0.25), dict(cluster_id=96 * 1, row=95, label=1, pred=0, error_size=0.5),
                dict(cluster_id=96 * 4, row=5, label=4, pred=0, error_size=0.75), dict(cluster_id=96 * 2, row=8, label=2, pred=0, error_size=0.25)]
    coords = {41: (1.0, 2.0, 3.0), 95: (4.0, 5.0, 6.0), 5: (7.0, 8.0, 9.0), 8: (0.5, 0.25, 0.125)}
    got = rank_candidates(clusters, spots, coords, 10)
    assert [c["row"] for c in got] == [5, 95, 8, 41]                         # deepest first; equal depths in ascending pseudo id
    assert got[0] == dict(point=[7.0, 8.0, 9.0], row=5, object=1, voxels=9, root=3, depth=0.75)
    assert got[3] == dict(point=[1.0, 2.0, 3.0], row=41, object=2, voxels=30, root=40, depth=0.25)
    assert rank_candidates(clusters, spots, coords.__getitem__, 2) == got[:2] and rank_candidates(clusters, spots, coords, 0) == []
    assert rank_candidates([], [], coords, 5) == []
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            rank_candidates(clusters, spots, coords, bad)
