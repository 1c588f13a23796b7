"""Host side of smooth patches, the magic wand and the snap (no GPU): ``a3d_similar_pair`` -- the pair predicate exported by
the function the kernel calls -- against the restatement (``patches_rule.py``) bit for bit, its symmetry, the restatement's
components against a brute-force transitive closure, the known answers of the vote, ``session.patch_thresholds``, every
``ValueError`` the ``view.py`` wrappers raise before the library is reached, and the library's refusal of a call without a
scene.  ``test_gpu_patches.py`` holds the kernels to the same restatement by equality."""
import ctypes as C
import types

import numpy as np
import pytest

import patches_rule as P
from pieces_rule import neighbours

F = np.float32
FP = C.POINTER(C.c_float)


def _lib():
    import __graft_entry__ as g
    g.build()
    from agile3d_amd import lib
    return lib, lib.load()


def _pair(L, na, nb, fa, fb, cos_min, tol2, oriented):
    p = lambda a: None if a is None else a.ctypes.data_as(FP)
    return L.a3d_similar_pair(p(na), p(nb), p(fa), p(fb), float(cos_min), float(tol2), int(oriented))


def _unit(rng, k):
    v = rng.normal(size=(k, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _dot(a, b):
    return (F(a[0]) * F(b[0]) + F(a[1]) * F(b[1])) + F(a[2]) * F(b[2])


def _q(a, b):
    d = [F(a[k]) - F(b[k]) for k in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


# ------------------------------------------------------------------------------------------- the exported predicate
def test_similar_pair_is_the_restatement():
    _, L = _lib()
    rng = np.random.default_rng(0)
    k = 100_000
    na = _unit(rng, k)
    nb = np.where(rng.random((k, 1)) < 0.7, na + rng.normal(scale=0.25, size=(k, 3)).astype(F), _unit(rng, k)).astype(F)
    nb[rng.random(k) < 0.3] *= F(-1)                                  # antiparallel: what `oriented` tells apart
    nb = np.ascontiguousarray(nb)
    fa = rng.random((k, 3)).astype(F)
    fb = np.ascontiguousarray(np.where(rng.random((k, 1)) < 0.7, fa + rng.normal(scale=0.05, size=(k, 3)).astype(F), rng.random((k, 3)))).astype(F)
    cos = np.cos(np.radians(rng.choice([0.0, 5.0, 15.0, 30.0, 90.0, 180.0], k))).astype(F)
    tol2 = (rng.choice([0.0, 0.02, 0.1, 0.5], k).astype(F)) ** 2
    oriented = rng.integers(0, 2, k)
    which = rng.integers(0, 3, k)                                     # normals, colours, both
    seen = set()
    for i in range(k):
        n_ = (na[i], nb[i]) if which[i] != 1 else (None, None)
        f_ = (fa[i], fb[i]) if which[i] != 0 else (None, None)
        got = _pair(L, *n_, *f_, cos[i], tol2[i], oriented[i])
        want = P.pair_numpy(*n_, *f_, cos[i], tol2[i], bool(oriented[i]))
        assert got == int(want), (i, na[i], nb[i], fa[i], fb[i], cos[i], tol2[i], oriented[i])
        assert got == _pair(L, *n_[::-1], *f_[::-1], cos[i], tol2[i], oriented[i])          # symmetric on every pair
        seen.add((int(which[i]), got))
    assert seen == {(w, g) for w in range(3) for g in (0, 1)}


def test_similar_pair_at_the_threshold():
    _, L = _lib()
    rng = np.random.default_rng(1)
    a, b = _unit(rng, 2000), _unit(rng, 2000)
    fa, fb = rng.random((2000, 3)).astype(F), rng.random((2000, 3)).astype(F)
    for i in range(2000):
        dot, q = _dot(a[i], b[i]), _q(fa[i], fb[i])
        for oriented, value in ((1, dot), (0, np.abs(dot))):
            if -1 <= value <= 1:
                assert _pair(L, a[i], b[i], None, None, value, 0, oriented) == 1                     # AT the threshold: joined
                assert _pair(L, a[i], b[i], None, None, np.nextafter(value, F(2)), 0, oriented) == 0    # one ulp above: not
                assert P.nsim(a[i], b[i], value, oriented) and not P.nsim(a[i], b[i], np.nextafter(value, F(2)), oriented)
        assert _pair(L, None, None, fa[i], fb[i], 1, q, 0) == 1 and P.fsim(fa[i], fb[i], q)
        assert _pair(L, None, None, fa[i], fb[i], 1, np.nextafter(q, F(-1)), 0) == 0 and not P.fsim(fa[i], fb[i], np.nextafter(q, F(-1)))
        # both tests: either one failing fails the pair
        assert _pair(L, a[i], b[i], fa[i], fb[i], np.abs(dot), q, 0) == 1
        assert _pair(L, a[i], b[i], fa[i], fb[i], np.nextafter(np.abs(dot), F(2)), q, 0) == 0
        assert _pair(L, a[i], b[i], fa[i], fb[i], np.abs(dot), np.nextafter(q, F(-1)), 0) == 0
    # a product that an FMA would round differently: the dot is built from three roundings
    # (1 + 2^-12)^2 rounds to 1 + 2^-11, so the sum is 0; a multiply-add fused with either product keeps 2^-24
    for order in ((0, 1, 2), (1, 0, 2)):
        x = np.array([1 + 2.0 ** -12, 1, 0], F)[list(order)]
        y = np.array([1 + 2.0 ** -12, -(1 + 2.0 ** -11), 0], F)[list(order)]
        assert _dot(x, y) == F(0) and float(x[order[0]]) * float(y[order[0]]) + float(x[order[1]]) * float(y[order[1]]) == 2.0 ** -24
        assert _pair(L, x, y, None, None, 2.0 ** -30, 0, 1) == 0 and _pair(L, x, y, None, None, 0.0, 0, 1) == 1


def test_similar_pair_zero_nan_oriented():
    lib, L = _lib()
    z, e, m = np.zeros(3, F), np.array([0, 0, 1], F), np.array([0, 0, -1], F)
    nan, inf = np.array([np.nan, 0, 1], F), np.array([np.inf, 0, 0], F)
    # no special case for a zero normal: its dot is 0
    assert _pair(L, z, e, None, None, 0.5, 0, 0) == 0 and _pair(L, z, z, None, None, 2.0 ** -149, 0, 0) == 0
    assert _pair(L, z, e, None, None, 0.0, 0, 0) == 1 and _pair(L, z, e, None, None, -1.0, 0, 1) == 1
    # oriented on and off
    assert _pair(L, e, m, None, None, 0.9, 0, 0) == 1 and _pair(L, e, m, None, None, 0.9, 0, 1) == 0
    assert _pair(L, e, m, None, None, -1.0, 0, 1) == 1
    # any comparison with a NaN fails, at the loosest threshold too; inf - inf is a NaN
    assert _pair(L, nan, e, None, None, -1.0, 0, 1) == 0 and _pair(L, nan, nan, None, None, -1.0, 0, 0) == 0
    assert _pair(L, None, None, nan, nan, 1, 3e38, 0) == 0 and _pair(L, None, None, inf, inf, 1, 3e38, 0) == 0
    assert _pair(L, None, None, inf, z, 1, 3e38, 0) == 0                                   # q = inf > any finite tolerance
    assert _pair(L, e, e, nan, nan, 1.0, 1.0, 0) == 0 and _pair(L, None, None, None, None, 1, 0, 0) == 1
    for args in ((nan, e, None, None), (None, None, nan, e), (z, z, None, None), (e, m, z, e)):
        for oriented in (0, 1):
            assert _pair(L, *args, 0.25, 0.5, oriented) == int(P.pair_numpy(*args, 0.25, 0.5, bool(oriented)))
    # a pointer without its partner, an `oriented` that is no flag
    assert _pair(L, e, None, None, None, 1, 0, 0) == -1 and _pair(L, None, None, None, e, 1, 0, 0) == -1
    assert _pair(L, e, e, None, None, 1, 0, 2) == -1 and b"a3d_similar_pair" in L.a3d_last_error()
    from agile3d_amd import view as V
    assert V.similar_pair(e, m, cos_min=0.9) is True and V.similar_pair(e, m, cos_min=0.9, oriented=True) is False
    assert V.similar_pair(feat_a=[0, 0, 0], feat_b=[0.5, 0, 0], tol2=0.25) is True
    assert V.similar_pair(e, e, [0, 0, 0], [0.5, 0, 0], 1.0, np.nextafter(F(0.25), F(0))) is False


# ------------------------------------------------------------------------------------------- the restatement's components
def _random_lattice(rng):
    box = rng.integers(1, 5, 3)
    cells = np.stack(np.meshgrid(*[np.arange(s) for s in box], indexing="ij"), -1).reshape(-1, 3)
    keep = cells[rng.random(len(cells)) < rng.uniform(0.5, 1.0)]
    if len(keep) == 0:
        keep = cells[:1]
    batch = rng.integers(0, 2, (len(keep), 1)) if rng.random() < 0.3 else np.zeros((len(keep), 1), np.int64)
    return np.concatenate([batch, keep - rng.integers(0, 3)], 1)[rng.permutation(len(keep))]


def test_restatement_against_transitive_closure():
    rng = np.random.default_rng(2)
    directions = np.array([[0, 0, 1], [0, 0, -1], [0, np.sin(0.2), np.cos(0.2)], [0, np.sin(0.4), np.cos(0.4)], [1, 0, 0],
                           [0, 0, 0]], F)
    several = 0
    for case in range(200):
        coords = _random_lattice(rng)
        n = len(coords)
        keys = [None, rng.integers(-1, 2, n)][rng.integers(2)]
        normals = directions[rng.integers(0, len(directions), n)] if rng.random() < 0.8 else None
        feats = (rng.integers(0, 4, (n, 3)) / 4).astype(F) if rng.random() < 0.6 else None
        c = int(rng.choice([6, 18, 26]))
        kw = dict(cos_min=F(np.cos(rng.choice([0.1, 0.25, 0.5]))), tol2=F(rng.choice([0.0, 0.07, 0.2])), oriented=bool(rng.integers(2)))
        if normals is not None and rng.random() < 0.4:
            kw.update(ref_normal=directions[rng.integers(0, 5)], ref_cos_min=F(np.cos(0.3)))
        if feats is not None and rng.random() < 0.4:
            kw.update(ref_feat=np.array([0.25, 0.5, 0.25], F), ref_tol2=F(0.3))
        piece, rec = P.similar_numpy(coords, keys, normals, feats, c, **kw)
        # independently: admissibility, every edge, the closure
        k_ = np.zeros(n, np.int64) if keys is None else keys
        ok = [bool(k_[i] >= 0 and ("ref_normal" not in kw or P.nsim(normals[i], kw["ref_normal"], kw["ref_cos_min"], kw["oriented"]))
                   and ("ref_feat" not in kw or P.fsim(feats[i], kw["ref_feat"], kw["ref_tol2"]))) for i in range(n)]
        edges = [(i, j) for i, js in enumerate(neighbours(coords, c)) for j in js
                 if ok[i] and ok[j] and k_[i] == k_[j] and P.pair_numpy(
                     None if normals is None else normals[i], None if normals is None else normals[j],
                     None if feats is None else feats[i], None if feats is None else feats[j], kw["cos_min"], kw["tol2"], kw["oriented"])]
        want = P.closure_numpy(n, edges, ok)
        assert np.array_equal(piece, want), case
        assert rec["root"].tolist() == sorted(set(want[want >= 0].tolist())) and rec["voxels"].sum() == (want >= 0).sum()
        several += len(rec) > 1
    assert several > 100


# ------------------------------------------------------------------------------------------- the vote
def test_vote_known_answers():
    piece = np.array([0] * 6 + [6] * 6 + [12] * 3 + [-1])
    # a tie goes to the lowest label: 3 x 5 and 3 x 2 in piece 0; (1, 2) asks for half
    labels = np.array([5, 5, 5, 2, 2, 2] + [1] * 6 + [7, 7, 4] + [9])
    out, s = P.vote_numpy(piece, labels, 3, (1, 2))
    assert out.tolist() == [2] * 6 + [1] * 6 + [7] * 3 + [9]
    assert s == dict(eligible_pieces=3, uniform_pieces=1, relabelled_pieces=2, relabelled_voxels=4, blocked_pieces=0,
                     below_share_pieces=0, err=0)
    # a share of exactly num / den passes, one vote fewer fails
    labels = np.array([3, 3, 3, 3, 8, 8] + [3, 3, 3, 8, 8, 8] + [0] * 4)
    out, s = P.vote_numpy(piece, labels, 4, (2, 3))
    assert out.tolist() == [3] * 6 + [3, 3, 3, 8, 8, 8] + [0] * 4
    assert (s["eligible_pieces"], s["relabelled_pieces"], s["relabelled_voxels"], s["below_share_pieces"]) == (2, 1, 2, 1)
    # a blocking click: a clicked row of another label in the piece; a click of the winner's label does not block, nor does a
    # click outside the rows
    for clicks, blocked in (([4], True), ([0], False), ([4, 0], True), ([-1, 99], False), ([15], False)):
        out, s = P.vote_numpy(piece, labels, 6, (2, 3), clicks)
        assert (out[4] == 8) == blocked and s["blocked_pieces"] == int(blocked) and s["relabelled_pieces"] == int(not blocked)
    # a piece below min_voxels is not eligible: the 3-voxel piece stays
    labels = np.array([1] * 12 + [7, 7, 4, 0])
    out, s = P.vote_numpy(piece, labels, 4, (1, 2))
    assert np.array_equal(out, labels) and s["eligible_pieces"] == 2 and s["uniform_pieces"] == 2
    out, s = P.vote_numpy(piece, labels, 3, (1, 2))
    assert out[14] == 7 and s["eligible_pieces"] == 3
    # overflow writes nothing and reports the capacity needed; exactly enough is enough
    out, s = P.vote_numpy(piece, labels, 3, (1, 2), capacity=2)
    assert out is None and s == dict(eligible_pieces=3, uniform_pieces=0, relabelled_pieces=0, relabelled_voxels=0,
                                     blocked_pieces=0, below_share_pieces=0, err=P.OVERFLOW)
    assert P.vote_numpy(piece, labels, 3, (1, 2), capacity=3)[1]["err"] == 0
    # a label out of range casts no vote and keeps its label
    labels = np.array([1, 1, 1, 1, 300, 2] + [1] * 6 + [-5, 7, 7, 0])
    out, s = P.vote_numpy(piece, labels, 3, (1, 2))
    assert out.tolist() == [1, 1, 1, 1, 300, 1] + [1] * 6 + [-5, 7, 7, 0] and s["err"] == P.BAD_LABEL
    assert (s["relabelled_pieces"], s["relabelled_voxels"], s["uniform_pieces"]) == (1, 1, 1)


# ------------------------------------------------------------------------------------------- settings, refusals
def test_patch_thresholds():
    from agile3d_amd.session import WAND_MODES, patch_thresholds
    cos_min, tol2 = patch_thresholds(15.0, 0.1)
    assert cos_min.dtype == F and cos_min == F(np.cos(np.radians(15.0))) and tol2.dtype == F and tol2 == F(0.1) * F(0.1)
    assert patch_thresholds(None, None) == (None, None) and patch_thresholds(0, None) == (F(1), None)
    assert patch_thresholds(180, 0)[0] == F(-1) and patch_thresholds(None, 0)[1] == F(0)
    for bad in ((-1, None), (181, None), (float("nan"), None), (None, -0.1), (None, float("inf")), (None, 1e30),
                (None, float("nan"))):
        with pytest.raises(ValueError):
            patch_thresholds(*bad)
    assert WAND_MODES == ("chain", "seed", "both")


def test_wrappers_refuse_before_the_library():
    import torch
    from agile3d_amd import view as V
    assert V.similar_settings(0.5, 0.25, True, [0, 0, 1], -1.0, None, 0.0) == (0.5, 0.25, 1, 1, [0.0, 0.0, 1.0], -1.0, [0.0] * 3, 0.0)
    assert V.similar_settings(ref_feat=(0.5, 0.5, 0.5), ref_tol2=4.0)[3] == V.SIMILAR_REF_FEAT == P.REF_FEAT
    assert V.SIMILAR_REF_NORMAL == P.REF_NORMAL
    for name, bad in (("cos_min", dict(cos_min=1.5)), ("cos_min", dict(cos_min=-1.001)), ("cos_min", dict(cos_min=float("nan"))),
                      ("ref_cos_min", dict(ref_cos_min=float("inf"))), ("ref_cos_min", dict(ref_cos_min=2)),
                      ("tol2", dict(tol2=-1e-9)), ("tol2", dict(tol2=float("inf"))), ("tol2", dict(tol2=1e39)),
                      ("ref_tol2", dict(ref_tol2=float("nan"))), ("ref_tol2", dict(ref_tol2=-1)),
                      ("ref_normal", dict(ref_normal=[0, 0])), ("ref_normal", dict(ref_normal=[0, 0, float("nan")])),
                      ("ref_feat", dict(ref_feat=[0, float("inf"), 0])), ("oriented", dict(oriented=2)),
                      ("oriented", dict(oriented=None))):
        with pytest.raises(ValueError, match=name):
            V.similar_settings(**bad)
        with pytest.raises(ValueError, match=name):
            V.similar_pieces(types.SimpleNamespace(handle=C.c_void_p(0), n=[5]), **bad)
    scene = types.SimpleNamespace(handle=C.c_void_p(0), n=[5])
    f3, i5 = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32)
    for name, bad in (("scene", dict(scene=None)), ("scene", dict(scene=object())), ("connectivity", dict(connectivity=8)),
                      ("reference", dict(ref_normal=[0, 0, 1])), ("reference", dict(ref_feat=[0, 0, 1], normals=f3)),
                      ("GPU", dict(normals=f3)), ("GPU", dict(keys=i5)), ("GPU", dict())):
        with pytest.raises(ValueError, match=name):
            V.similar_pieces(**dict(dict(scene=scene), **bad))
    for name, bad in (("normal_a", dict(normal_a=[0, 0, 1])), ("normal_a", dict(feat_b=[0, 0, 1])),
                      ("normal_a", dict(normal_a=[0, 0], normal_b=[0, 0, 1])), ("cos_min", dict(cos_min=3)),
                      ("tol2", dict(tol2=-1)), ("oriented", dict(oriented="yes"))):
        with pytest.raises(ValueError, match=name):
            V.similar_pair(**bad)
    assert V.vote_settings(8, (2, 3)) == (8, 2, 3, 256, 1024) and V.vote_settings(1, [65536, 65536], 1, 0) == (1, 65536, 65536, 1, 0)
    for name, bad in (("min_voxels", dict(min_voxels=0)), ("min_voxels", dict(min_voxels=2.5)), ("share", dict(share=(0, 3))),
                      ("share", dict(share=(4, 3))), ("share", dict(share=(1, 65537))), ("share", dict(share=0.5)),
                      ("share", dict(share=(1, 2, 3))), ("share", dict(share=(0.5, 1))), ("n_classes", dict(n_classes=0)),
                      ("n_classes", dict(n_classes=257)), ("capacity", dict(capacity=-1))):
        with pytest.raises(ValueError, match=name):
            V.vote_settings(**dict(dict(min_voxels=8, share=(2, 3)), **bad))
        with pytest.raises(ValueError, match=name):
            V.vote_pieces(**dict(dict(scene=scene, labels=i5, piece_qv=i5, workspace=None, min_voxels=8, share=(2, 3)), **bad))
    for name, bad in (("scene", dict(scene=None)), ("GPU", dict())):
        with pytest.raises(ValueError, match=name):
            V.vote_pieces(**dict(dict(scene=scene, labels=i5, piece_qv=i5, workspace=None), **bad))
    host = np.array([(9, 1, 2, 30, 4, 5, 2, 0)], V.VOTE_SUMMARY).view(np.uint8)
    assert V.read_vote_summary(host) == dict(eligible_pieces=9, uniform_pieces=1, relabelled_pieces=2, relabelled_voxels=30,
                                             blocked_pieces=4, below_share_pieces=5, err=2)
    assert tuple(V.read_vote_summary(host)) == P.VOTE_FIELDS and (V.VOTE_OVERFLOW, V.VOTE_BAD_LABEL) == (P.OVERFLOW, P.BAD_LABEL)


def test_library_refuses_without_a_scene():
    lib, L = _lib()
    assert C.sizeof(lib.SimilarPiecesArgs) == 1192 and C.sizeof(lib.VotePiecesArgs) == 1112 and C.sizeof(lib.VoteSummary) == 32
    assert L.a3d_vote_workspace_bytes(-1, 4, 4) == 0 and L.a3d_vote_workspace_bytes(10, -1, 4) == 0
    assert L.a3d_vote_workspace_bytes(10, 4, 0) == 0 and L.a3d_vote_workspace_bytes(10, 4, 257) == 0
    for n, cap, k in ((0, 0, 1), (1, 1, 256), (1000, 64, 20)):
        nbytes = L.a3d_vote_workspace_bytes(n, cap, k)
        assert nbytes >= L.a3d_pieces_workspace_bytes(n) + 4 * (n + cap + cap * k) and nbytes % 256 == 0
    assert L.a3d_similar_pieces(None, None) == lib.A3D_ERR_INVALID and L.a3d_vote_pieces(None, None) == lib.A3D_ERR_INVALID
    a = lib.SimilarPiecesArgs()
    a.n, a.connectivity, a.cos_min = 0, 26, 1.0
    a.n_out_dev = 256                                                 # (never looked at: the scene is checked first)
    assert L.a3d_similar_pieces(C.byref(a), None) == lib.A3D_ERR_INVALID
    assert b"a3d_similar_pieces" in L.a3d_last_error()
    v = lib.VotePiecesArgs()
    v.n, v.min_voxels, v.n_classes, v.share_num, v.share_den = 0, 8, 256, 2, 3
    v.summary_dev = 256
    assert L.a3d_vote_pieces(C.byref(v), None) == lib.A3D_ERR_INVALID
    assert b"a3d_vote_pieces" in L.a3d_last_error()
