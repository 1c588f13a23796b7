"""-m gpu: the query by example's kernels -- a3d_feature_prototypes / a3d_feature_match (csrc/session_match.hip) -- against the
rule restated in ``match_rule.py``.  sums, count, match_qv, best_qv, the summaries' counters and error words and match_full are
compared BIT FOR BIT, on every row of every case.  score_qv / score_full are compared within 1 fp32 ulp: the rule's score is a
double rounded once to fp32, and the kernel's double lies within a few double ulps of it (its division and square root may
differ from numpy's in the last bit), which moves the rounded fp32 value by at most one step.

Row counts: 1, 63, 64, 65, 257 (the match's tile is 64 rows, the prototypes' workgroup takes 4 rows a pass) and one count that
makes a workgroup of each kernel walk its grid a second time.  Prototype counts: 1, 2, 256 and the LDS chunk of 16 +- 1."""
import numpy as np
import pytest
import torch

import match_rule as R
from agile3d_amd import lib as L
from agile3d_amd import view as V
from session_kit import DEV, _dev, byref, status

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK = L.A3D_MATCH_CHUNK
MATCH_PASS = 64 * 768          # rows one pass of the match kernel's grid covers (kMmRows x kMmBlocks)
PROTO_PASS = 4 * 1024          # rows one pass of the prototype kernel's grid covers (kMpWaves x kMpBlocks)


def data(n, k, seed, planted=True):
    """``(feats fp32 [n, 128], protos fp32 [k, 128])``: standard normal, and every third row a near-duplicate (noise of 0.1 to
    0.6 a channel: cosines on both sides of 0.9) of a multiple of some prototype, so that voxels pass at 0.9."""
    rng = np.random.default_rng(seed)
    feats, protos = rng.standard_normal((n, 128)).astype(F32), rng.standard_normal((k, 128)).astype(F32)
    if planted:
        rows = np.arange(0, n, 3)
        which = rng.integers(0, k, len(rows))
        noise = rng.standard_normal((len(rows), 128)) * rng.uniform(0.1, 0.6, (len(rows), 1))
        feats[rows] = ((protos[which] + noise) * rng.uniform(0.5, 2.0, (len(rows), 1))).astype(F32)
    return feats, protos


def run_match(feats, protos, proto_class, cos_min, candidate=None, inverse_map=None):
    """The library on numpy arrays: the outputs start as sentinels, so that an untouched entry shows."""
    n = len(feats)
    out = dict(match_qv=torch.full((n,), -7, dtype=torch.int32, device=DEV), best_qv=torch.full((n,), -7, dtype=torch.int32, device=DEV),
               score_qv=torch.full((n,), -7.0, dtype=torch.float32, device=DEV))
    if inverse_map is not None:
        out.update(match_full=torch.full((len(inverse_map),), -7, dtype=torch.int32, device=DEV),
                   score_full=torch.full((len(inverse_map),), -7.0, dtype=torch.float32, device=DEV))
    got = V.feature_match(_dev(feats, F32).reshape(-1, 128), _dev(protos, F32).reshape(-1, 128), _dev(proto_class, np.int32), cos_min,
                          candidate=None if candidate is None else _dev(candidate, np.uint8),
                          inverse_map=None if inverse_map is None else _dev(inverse_map, np.int64), **out)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(V.read_match_summary(got[5].cpu().numpy()))
    return res


def check_match(feats, protos, proto_class, cos_min, candidate=None, inverse_map=None):
    got = run_match(feats, protos, proto_class, cos_min, candidate, inverse_map)
    want = R.match(feats, protos, proto_class, cos_min, candidate, inverse_map)
    for name in ("match_qv", "best_qv") + (("match_full",) if inverse_map is not None else ()):
        assert got[name].tobytes() == want[name].tobytes(), (name, np.flatnonzero(got[name] != want[name])[:8])
    for name in ("score_qv",) + (("score_full",) if inverse_map is not None else ()):
        ulps = R.ulps(got[name], want[name])
        print(f"{name}: n={len(feats)} k={len(protos)} max ulps {ulps.max() if len(ulps) else 0}")
        assert np.isfinite(got[name]).all() and (ulps <= 1).all(), (name, ulps.max())
    assert got["matched"].tolist() == want["matched"].tolist()
    assert (got["rows_nonfinite"], got["err"]) == (want["rows_nonfinite"], want["err"])
    return got


def run_prototypes(feats, classes, n_classes):
    sums = torch.full((n_classes, 128), -7, dtype=torch.int64, device=DEV)
    count = torch.full((n_classes,), -7, dtype=torch.int32, device=DEV)
    got = V.feature_prototypes(_dev(feats, F32).reshape(-1, 128), _dev(classes, np.int32), n_classes, sums=sums, count=count)
    return dict(sums=sums.cpu().numpy(), count=count.cpu().numpy(), **V.read_prototypes_summary(got[2].cpu().numpy()))


def check_prototypes(feats, classes, n_classes):
    got, want = run_prototypes(feats, classes, n_classes), R.prototypes(feats, classes, n_classes)
    assert got["sums"].tobytes() == want["sums"].tobytes() and got["count"].tobytes() == want["count"].tobytes()
    assert {k: got[k] for k in ("examples", "examples_left_out", "err")} == {k: want[k] for k in ("examples", "examples_left_out", "err")}
    return got


# ------------------------------------------------------------------------------------------- the match: sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_match_row_counts(n):
    feats, protos = data(n, 5, n)
    got = check_match(feats, protos, [3, 0, 255, 7, 3], 0.9, inverse_map=np.random.default_rng(n).integers(0, n, 2 * n + 1))
    assert n < 63 or 0 < got["matched"].sum() < n
    check_match(feats, protos, [3, 0, 255, 7, 3], 0.9, candidate=np.arange(n) % 4 != 1)


@pytest.mark.parametrize("k", [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 256])
def test_match_prototype_counts(k):
    feats, protos = data(130, k, 100 + k)
    protos[k // 2] = protos[0]                                               # (k > 1) a duplicate of a lower index, in a later chunk
    got = check_match(feats, protos, np.arange(k)[::-1] % 256, 0.9)
    assert got["matched"].sum() > 10 and (k == 1 or k // 2 not in got["best_qv"])
    check_match(feats, protos, np.arange(k) % 7, 0.0, candidate=np.arange(130) % 3 != 0, inverse_map=np.arange(130)[::-1])


def test_match_a_workgroup_walks_its_grid_twice():
    n = MATCH_PASS + 64 + 13
    feats, protos = data(n, 3, 9)
    inv = np.concatenate([np.arange(n), np.random.default_rng(9).integers(0, n, 2049 * 256 + 5 - n)])      # the lift's grid, too
    got = check_match(feats, protos, [1, 2, 3], 0.9, inverse_map=inv)
    assert 1000 < got["matched"].sum() < n


# ------------------------------------------------------------------------------------------- the match: the rule's edges
def test_match_threshold_of_exactly_one_and_ties():
    rng = np.random.default_rng(3)
    e = (rng.integers(-(1 << 21), 1 << 21, 128) * 2.0 ** -20).astype(F32)
    off, ortho = e.copy(), np.zeros(128, F32)
    off[17] += F32(2.0 ** -10)
    ortho[0], ortho[1] = e[1], -e[0]
    feats = np.stack([e, 2 * e, F32(0.5) * e, off, ortho, -e, np.zeros(128, F32)])
    got = check_match(feats, e[None], [7], 1.0)
    assert got["match_qv"].tolist() == [7, 7, 7, -1, -1, -1, -1] and got["score_qv"][:3].tolist() == [1.0] * 3
    assert check_match(feats, e[None], [7], 0.0)["match_qv"].tolist() == [7, 7, 7, 7, -1, -1, -1]
    other = rng.standard_normal(128).astype(F32)
    v = (e + F32(0.25) * other).astype(F32)[None]
    assert check_match(v, np.stack([e, e]), [4, 9], 0.5)["match_qv"].tolist() == [4]
    protos = np.stack([other] + [e, 2 * e] * 9 + [e])                        # e's equals in the second chunk: no replacement
    got = check_match(v, protos, np.arange(20), 0.5)
    assert (got["match_qv"].tolist(), got["best_qv"].tolist()) == ([1], [1])
    got = check_match(e[None], np.stack([-e, ortho, -e, np.zeros(128, F32)]), [1, 2, 3, 4], 0.9)      # signs, a zero prototype
    assert (got["match_qv"].tolist(), got["best_qv"].tolist()) == ([-1], [1])
    got = check_match(e[None], np.zeros((1, 128), F32), [1], 0.0)
    assert (got["best_qv"].tolist(), got["score_qv"].tolist()) == ([-1], [0.0])


def test_match_rows_and_prototypes_that_are_not_finite_and_bad_classes():
    feats, protos = data(200, 4, 11)
    feats[[0, 64, 199], [5, 127, 0]] = [np.nan, np.inf, -np.inf]
    feats[7] = 0.0
    feats[9] *= F32(1e30)                                                    # finite and huge: scored all the same
    got = check_match(feats, protos, [1, 2, 3, 4], 0.9, inverse_map=np.arange(200))
    assert got["rows_nonfinite"] == 3 and got["best_qv"][[0, 64, 199, 7]].tolist() == [-1] * 4 and got["best_qv"][9] >= 0
    protos[1, 100] = np.nan
    protos[2, 3] = np.inf
    got = check_match(feats, protos, [1, 2, 3, 256], 0.9)                    # on the device: the wrapper takes the caller's word
    assert got["err"] == V.MATCH_BAD_PROTOTYPE | V.MATCH_BAD_CLASS and not np.isin(got["best_qv"], [1, 2]).any()
    assert got["matched"][1] > 0 and (got["match_qv"] == 256).any()
    assert check_match(feats, protos[:1], [-1], 0.9)["err"] == V.MATCH_BAD_CLASS


def test_match_inverse_map_out_of_range_is_flagged_and_not_followed():
    feats, protos = data(100, 2, 12)
    inv = np.arange(150) % 100
    inv[[0, 77, 149]] = [-1, 100, 1 << 40]
    got = check_match(feats, protos, [1, 2], 0.9, inverse_map=inv)
    assert got["err"] == V.MATCH_BAD_INDEX and got["match_full"][[0, 77, 149]].tolist() == [-7] * 3
    assert got["score_full"][[0, 77, 149]].tolist() == [-7.0] * 3


def test_match_refusals_of_the_entry_point_and_two_calls_agree():
    feats, protos = data(300, 17, 13)
    a, b = (run_match(feats, protos, np.arange(17), 0.9, inverse_map=np.arange(300)) for _ in range(2))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("match_qv", "best_qv", "score_qv", "match_full", "score_full", "matched"))
    f, p, c = _dev(feats, F32), _dev(protos, F32), _dev(np.arange(17), np.int32)
    out, summ = torch.zeros(300, dtype=torch.int32, device=DEV), torch.zeros(2064, dtype=torch.uint8, device=DEV)

    def call(**kw):
        args = L.FeatureMatchArgs(feats_dev=f.data_ptr(), n=300, protos_dev=p.data_ptr(), proto_class_dev=c.data_ptr(), match_qv_dev=out.data_ptr(),
                                  best_qv_dev=out.data_ptr(), score_qv_dev=out.data_ptr(), summary_dev=summ.data_ptr(), cos_min=0.9, k=17)
        for k, v in kw.items():
            setattr(args, k, v)
        return status("a3d_feature_match", byref(args), None)
    assert call() == 0
    for bad in (dict(k=0), dict(k=257), dict(cos_min=1.5), dict(cos_min=float("nan")), dict(n=-1), dict(feats_dev=f.data_ptr() + 4),
                dict(summary_dev=None), dict(n_full=5), dict(inverse_map_dev=out.data_ptr(), n_full=5)):
        assert call(**bad) == L.A3D_ERR_INVALID, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- the prototypes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, PROTO_PASS + 4 + 3])
def test_prototype_row_counts(n):
    rng = np.random.default_rng(n)
    feats = (rng.standard_normal((n, 128)) * 4).astype(F32)
    classes = rng.integers(-1, 40, n)                                       # classes in LDS (below 32) and beyond
    got = check_prototypes(feats, classes, 40)
    assert got["examples"] == (classes >= 0).sum()
    check_prototypes(feats, np.zeros(n), 1)                                  # every row one class: the most contended sums


def test_prototypes_in_two_row_orders_are_byte_identical_and_256_classes():
    rng = np.random.default_rng(21)
    feats = (rng.standard_normal((3000, 128)) * 100).astype(F32)
    classes = rng.integers(-1, 256, 3000)
    classes[:300] = 255
    a = check_prototypes(feats, classes, 256)
    perm = rng.permutation(3000)
    b = run_prototypes(feats[perm], classes[perm], 256)
    assert a["sums"].tobytes() == b["sums"].tobytes() and a["count"].tobytes() == b["count"].tobytes() and a["count"][255] >= 300


def test_prototypes_rows_left_out_and_class_values_out_of_range():
    rng = np.random.default_rng(22)
    feats = rng.standard_normal((100, 128)).astype(F32)
    feats[[3, 40, 41, 99], [0, 127, 64, 5]] = [np.nan, np.inf, F32(2.0 ** 20) + F32(0.125), -np.inf]
    feats[50, 9], feats[51, 9] = F32(2.0 ** 20), -F32(2.0 ** 20)             # |X| == 2^40: accepted
    feats[99, 7] = np.nan                                                    # (class -1: never read as an example)
    classes = rng.integers(0, 3, 100)
    classes[99] = -1
    got = check_prototypes(feats, classes, 3)
    assert (got["examples"], got["examples_left_out"], got["err"]) == (96, 3, 0)
    classes[[10, 11, 12]] = [-2, 3, 1 << 20]
    got = check_prototypes(feats, classes, 3)
    assert (got["examples"], got["examples_left_out"], got["err"]) == (93, 3, V.MATCH_BAD_CLASS)
    # a single example of multiples of the quantum is its own prototype; through the caller's step on the device
    e = (rng.integers(-(1 << 21), 1 << 21, 128) * 2.0 ** -20).astype(F32)
    sums, count, _ = V.feature_prototypes(_dev(np.stack([feats[0], e]), F32), _dev([-1, 2], np.int32), 4)
    table = V.prototype_table(sums, count)
    assert table.is_cuda and table[2].cpu().numpy().tobytes() == e.tobytes() and not table[[0, 1, 3]].any()


def test_prototype_table_on_the_device_has_the_hosts_bits():
    rng = np.random.default_rng(23)
    feats = (rng.standard_normal((2000, 128)) * 50).astype(F32)
    classes = rng.integers(-1, 9, 2000)
    sums, count, _ = V.feature_prototypes(_dev(feats, F32), _dev(classes, np.int32), 10)
    want = R.prototype_table(sums.cpu().numpy(), count.cpu().numpy())
    got = V.prototype_table(sums, count).cpu().numpy()
    assert sorted(want) == list(range(9)) and all(got[c].tobytes() == want[c].tobytes() for c in want) and not got[9].any()
