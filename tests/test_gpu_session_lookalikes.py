"""-m gpu: more objects like this one, through the session (InteractiveSession.lookalikes, lookalike_at).  A scene of 3200
voxels carries a PLANTED feature field through ``features=``: four separated discs share one feature direction with small
noise (and so does a speck of a few voxels), the rest of the scan is orthogonal to it; one disc is labelled by a click plus
``infer(logits=...)``.  Every result is also held to the rule's restatement (``match_rule.py``) run on the same field: the
matched object of every voxel bit for bit, the score within one fp32 ulp (test_gpu_match.py derives the bound).

1  lookalikes(obj=1) finds exactly the three other discs with their voxel counts; each suggested row is its disc's deepest
   voxel by a float64 brute force; min_voxels drops the speck; the similarity view's colours; guide() afterwards answers as
   before: nothing was invalidated
2  within="background" leaves out a disc labelled as object 2, "all" takes it in; selection= with obj=
3  obj=None with two objects and two feature directions: every matched voxel carries the object of the nearer prototype
4  lookalike_at on an object's pixel, on a background pixel and on one that shows nothing; the ValueErrors
5  without features=, on the random-weight model: the restatement run on a host copy of the backbone's output
"""
import numpy as np
import pytest
import torch

import match_rule as R
from session_kit import DEV, _model, intrinsic, look_at

pytestmark = pytest.mark.gpu
F32 = np.float32
CENTRES, RADII = np.array([[0.2, 0.2], [0.6, 0.2], [0.2, 0.6], [0.6, 0.6]]), (0.11, 0.09, 0.08, 0.07)
SPECK, SPECK_RADIUS = np.array([0.4, 0.4]), 0.016


@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


def lattice(seed=0):
    """A 40 x 40 x 2 lattice with one point per 2 cm voxel (jittered by +-6 mm inside it), shuffled: 3200 voxels, and no two
    of them equally deep in a disc (as test_gpu_session_pieces.py builds its scene)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    xyz = ((g + 0.5) * 0.02 + rng.uniform(-0.006, 0.006, g.shape)).astype(F32)
    return xyz[rng.permutation(len(xyz))]


def blob_of(coords):
    """0..3: the disc a point lies in (by its x, y), 4: the speck, -1: neither."""
    xy = coords[:, :2].astype(np.float64)
    out = np.full(len(xy), -1)
    for k, (c, r) in enumerate(zip(CENTRES, RADII)):
        out[np.linalg.norm(xy - c, axis=1) < r] = k
    out[np.linalg.norm(xy - SPECK, axis=1) < SPECK_RADIUS] = 4
    return out


def field(blob, direction_of, seed=1, noise=0.02):
    """fp32 [n, 128]: a voxel of blob b holds ``scale * (direction_of[b] + noise)``, a voxel of no blob a standard normal
    vector made orthogonal to every direction."""
    rng = np.random.default_rng(seed)
    n = len(blob)
    dirs = np.stack(list(direction_of.values()))
    q, _ = np.linalg.qr(dirs.T)                                            # an orthonormal basis of the directions' span
    f = rng.standard_normal((n, 128))
    f -= (f @ q) @ q.T
    for b, d in direction_of.items():
        rows = np.flatnonzero(blob == b)
        f[rows] = (d + noise * rng.standard_normal((len(rows), 128))) * rng.uniform(0.5, 2.0, (len(rows), 1))
    return f.astype(F32)


def directions(seed=2):
    rng = np.random.default_rng(seed)
    d1, u = rng.standard_normal(128), rng.standard_normal(128)
    d1 /= np.linalg.norm(d1)
    u -= (u @ d1) * d1
    u /= np.linalg.norm(u)
    d2 = d1 + 0.6 * u                                                      # cos(d1, d2) = 0.857
    return d1, d2 / np.linalg.norm(d2)


def deepest(coords, member):
    """(row, depth, relative lead over the second deepest) of the member farthest from every non-member, in float64."""
    x = coords.astype(np.float64)
    rows = np.flatnonzero(member)
    d = np.sqrt(((x[member][:, None, :] - x[~member][None]) ** 2).sum(2)).min(1)
    top = np.sort(d)[::-1]
    return int(rows[d.argmax()]), float(top[0]), float((top[0] - top[1]) / top[0])


def labelled(model, objects):
    """A session on the lattice whose voxels carry object k + 1 inside disc ``objects[k]`` and 0 elsewhere: one click per object,
    then logits replayed.  Returns ``(ses, coords fp32 [n, 3] in voxel order, blob int [n])``."""
    from agile3d_amd.session import InteractiveSession
    xyz = lattice()
    ses = InteractiveSession(model, voxel_size=0.02).load_scene(xyz, np.full(xyz.shape, 0.5, F32) + (xyz * F32(0.3)))
    coords = ses.raw_coords_qv.cpu().numpy()
    assert len(coords) == 3200                                             # (one point per voxel)
    blob = blob_of(coords)
    logits = np.full((len(coords), 1 + len(objects)), -3.0, F32)
    logits[:, 0] = 1.0
    for k, b in enumerate(objects):
        ses.click(coords[deepest(coords, blob == b)[0]], k + 1)
        logits[blob == b, k + 1] = 4.0
    ses.infer(logits=torch.from_numpy(logits).to(DEV))
    want = np.zeros(len(coords), np.int32)
    for k, b in enumerate(objects):
        want[blob == b] = k + 1
    assert np.array_equal(ses._labels_qv.cpu().numpy(), want)
    return ses, coords, blob


def restated(feats, classes, ids, cos_min, candidate=None, own=False):
    """``(match_qv, score_qv, example counts)`` of the rule for the example classes ``classes`` and the objects ``ids``."""
    p = R.prototypes(feats, classes, max(ids) + 1)
    table = R.prototype_table(p["sums"], p["count"])
    protos = np.stack([table.get(c, np.zeros(128, F32)) for c in ids])
    r = R.match(feats, protos, ids, cos_min, candidate)
    match = r["match_qv"].copy()
    if own:
        match[match == classes] = -1
    return match, r["score_qv"], {c: int(p["count"][c]) for c in ids if p["count"][c] > 0}


def holds(res, match, score, inverse_map):
    assert res.match_qv.cpu().numpy().tobytes() == match.tobytes()
    assert (R.ulps(res.score_qv.cpu().numpy(), score) <= 1).all()
    assert torch.equal(res.score_full, res.score_qv[inverse_map])


# ---------------------------------------------------------------------------------------------------- 1
def test_the_three_other_discs(model_002):
    ses, coords, blob = labelled(model_002, [0])
    sizes = [int((blob == k).sum()) for k in range(5)]
    assert min(sizes[:4]) > 40 and 0 < sizes[4] < 8 and len(set(sizes[:4])) == 4
    d1, _ = directions()
    feats = field(blob, {k: d1 for k in range(5)})
    fdev = torch.from_numpy(feats).to(DEV)
    before = ses.guide()
    res = ses.lookalikes(obj=1, features=fdev)
    classes = np.where(blob == 0, 1, -1)
    match, score, counts = restated(feats, classes, [1], 0.9, candidate=(blob != 0))
    holds(res, match, score, ses.inverse_map)
    assert np.array_equal(match, np.where(np.isin(blob, [1, 2, 3, 4]), 1, -1))        # the planted field, and nothing else
    assert (res.n_regions, res.n_regions_searched, len(res.candidates)) == (3, 3, 3)  # the speck is below min_voxels = 8
    assert res.prototypes == counts == {1: sizes[0]} and (res.examples_left_out, res.rows_nonfinite) == (0, 0)
    assert (res.cos_min, res.min_voxels, res.within, res.connectivity) == (0.9, 8, "background", 26)
    want = sorted((deepest(coords, blob == k) + (k,) for k in (1, 2, 3)), key=lambda w: -w[1])
    assert min(w[2] for w in want) >= 1e-4, want                          # no tie the fp32 search could break differently
    for c, (row, depth, _, k) in zip(res.candidates, want):
        assert set(c) == {"point", "row", "object", "voxels", "root", "depth"}
        assert c["row"] == row and blob[c["row"]] == k and c["object"] == 1, (c, row)
        assert abs(c["depth"] - depth) <= 1e-5 * depth and np.array_equal(np.float32(c["point"]), coords[row])
        assert c["voxels"] == sizes[k] and c["root"] == int(np.flatnonzero(blob == k).min())
    assert ses.lookalikes(obj=1, features=fdev, max_candidates=1).candidates == res.candidates[:1]
    # min_voxels = 1 keeps the speck; a threshold nothing reaches finds nothing, in one round trip and without a search
    small = ses.lookalikes(obj=1, features=fdev, min_voxels=1)
    assert (small.n_regions, len(small.candidates)) == (4, 4) and small.candidates[-1]["voxels"] == sizes[4]
    assert blob[small.candidates[-1]["row"]] == 4
    fewer = ses.lookalikes(obj=1, features=fdev, min_voxels=sizes[2])                # the threshold is inclusive
    assert fewer.n_regions == sum(s >= sizes[2] for s in sizes[1:4])
    orth = ses.lookalikes(obj=1, features=torch.from_numpy(field(blob, {0: d1})).to(DEV))
    assert (orth.n_regions, orth.candidates) == (0, []) and int((orth.match_qv >= 0).sum()) == 0
    # the similarity view: own * (1 - s) + palette * s on the matched vertices, their own colour elsewhere
    inv = ses.inverse_map.cpu().numpy()
    own, s = ses.colors_full.cpu().numpy(), np.clip(res.score_full.cpu().numpy(), F32(0), F32(1))[:, None]
    faded = (own * (F32(1.0) - s)).astype(F32) + (ses.palette[1][None] * s).astype(F32)
    assert np.array_equal(res.colors.cpu().numpy(), np.where((match[inv] >= 0)[:, None], faded, own))
    # a candidate is taken as a new object by click(); nothing was invalidated: guide() answers as before
    after = ses.guide()
    assert after.suggestions == before.suggestions and torch.equal(after.colors, before.colors)
    row, _ = ses.click(res.candidates[0]["point"], 2)
    assert row == res.candidates[0]["row"]


# ---------------------------------------------------------------------------------------------------- 2
def test_within_and_selection(model_002):
    ses, coords, blob = labelled(model_002, [0, 1])
    sizes = [int((blob == k).sum()) for k in range(5)]
    d1, _ = directions()
    feats = field(blob, {k: d1 for k in range(5)})
    fdev = torch.from_numpy(feats).to(DEV)
    classes = np.where(blob == 0, 1, -1)
    back = ses.lookalikes(obj=1, features=fdev)
    holds(back, *restated(feats, classes, [1], 0.9, candidate=(blob != 0) & (blob != 1))[:2], ses.inverse_map)
    assert sorted(c["voxels"] for c in back.candidates) == sorted(sizes[2:4]) and back.n_regions == 2
    every = ses.lookalikes(obj=1, features=fdev, within="all")
    holds(every, *restated(feats, classes, [1], 0.9, own=True)[:2], ses.inverse_map)
    assert sorted(c["voxels"] for c in every.candidates) == sorted(sizes[1:4]) and every.within == "all"
    assert {blob[c["row"]] for c in every.candidates} == {1, 2, 3} and int((every.match_qv[torch.from_numpy(blob == 0).to(DEV)] >= 0).sum()) == 0
    # selection= with obj=: the voxels of the selected vertices are the examples, whatever the labelling says
    inv = ses.inverse_map.cpu().numpy()
    sel = torch.from_numpy(blob[inv] == 2).to(DEV)
    picked = ses.lookalikes(obj=3, selection=sel, features=fdev)
    match, score, counts = restated(feats, np.where(blob == 2, 3, -1), [3], 0.9, candidate=np.isin(blob, [-1, 3, 4]))
    holds(picked, match, score, ses.inverse_map)
    assert picked.prototypes == counts == {3: sizes[2]} and [c["voxels"] for c in picked.candidates] == [sizes[3]]
    assert picked.candidates[0]["object"] == 3 and blob[picked.candidates[0]["row"]] == 3
    as_bytes = ses.lookalikes(obj=3, selection=sel.to(torch.uint8), features=fdev)
    assert as_bytes.candidates == picked.candidates
    with pytest.raises(ValueError, match="obj"):
        ses.lookalikes(selection=sel, features=fdev)
    with pytest.raises(ValueError, match="example"):
        ses.lookalikes(obj=1, selection=torch.zeros_like(sel), features=fdev)
    with pytest.raises(ValueError, match="selection"):
        ses.lookalikes(obj=1, selection=sel[:-1], features=fdev)


# ---------------------------------------------------------------------------------------------------- 3
def test_every_object_and_the_nearer_prototype(model_002):
    ses, coords, blob = labelled(model_002, [0, 1])
    d1, d2 = directions()
    feats = field(blob, {0: d1, 1: d2, 2: d1, 3: d2, 4: d2})
    res = ses.lookalikes(features=torch.from_numpy(feats).to(DEV), cos_min=0.8)
    classes = np.where(blob == 0, 1, np.where(blob == 1, 2, -1))
    match, score, counts = restated(feats, classes, [1, 2], 0.8, candidate=~np.isin(blob, [0, 1]))
    holds(res, match, score, ses.inverse_map)
    assert res.prototypes == counts and sorted(counts) == [1, 2]
    # both prototypes pass on the discs (cos(d1, d2) = 0.857 > 0.8): the nearer one decides
    assert np.array_equal(match[blob == 2], np.full((blob == 2).sum(), 1)) and np.array_equal(match[blob == 3], np.full((blob == 3).sum(), 2))
    assert sorted((c["object"], int(blob[c["row"]])) for c in res.candidates) == [(1, 2), (2, 3)]
    one = ses.lookalikes(obj=2, features=torch.from_numpy(feats).to(DEV), cos_min=0.95)
    assert [(c["object"], int(blob[c["row"]])) for c in one.candidates] == [(2, 3)] and sorted(one.prototypes) == [2]


# ---------------------------------------------------------------------------------------------------- 4
def test_lookalike_at_and_the_refusals(model_002):
    ses, coords, blob = labelled(model_002, [0])
    d1, _ = directions()
    fdev = torch.from_numpy(field(blob, {k: d1 for k in range(5)})).to(DEV)
    w, h = 96, 72
    view = ses.render(intrinsic(w, h), look_at([0.4, 0.4, 1.2], [0.4, 0.4, 0.0], up=(0.0, 1.0, 0.0)), w, h, radius=0.015)   # from above
    image = ses.label_image(view).cpu().numpy()
    assert (image == 1).any() and (image == 0).any()
    v, u = np.argwhere(image == 1)[0]
    want = ses.lookalikes(obj=1, features=fdev)
    got = ses.lookalike_at(view, u, v, features=fdev)
    assert got.candidates == want.candidates and torch.equal(got.match_qv, want.match_qv) and len(got.candidates) == 3
    v, u = np.argwhere(image == 0)[0]
    with pytest.raises(ValueError, match="background"):
        ses.lookalike_at(view, u, v, features=fdev)
    assert (image < 0).any()
    v, u = np.argwhere(image < 0)[0]
    with pytest.raises(ValueError, match="nothing"):
        ses.lookalike_at(view, u, v, features=fdev)
    for bad in (dict(within="label"), dict(cos_min=1.5), dict(cos_min=-0.1), dict(cos_min=float("nan")), dict(cos_min=None),
                dict(min_voxels=0), dict(max_candidates=-1), dict(connectivity=4), dict(obj=2), dict(obj=0), dict(obj=1.5),
                dict(features=fdev[:, :64]), dict(features=fdev[:-1]), dict(features=fdev.double()), dict(features=fdev.cpu()),
                dict(features=fdev.cpu().numpy())):
        with pytest.raises(ValueError):
            ses.lookalikes(**dict(dict(obj=1, features=fdev), **bad))
    ses.reset()
    with pytest.raises(ValueError, match="example"):
        ses.lookalikes(features=fdev)                                      # no object yet
    with pytest.raises(ValueError):
        ses.lookalikes(obj=1, features=fdev)


# ---------------------------------------------------------------------------------------------------- 5
def test_on_the_backbones_own_features(model_002):
    ses, coords, blob = labelled(model_002, [0, 3])
    feats = ses._backbone[0].F
    assert feats.dtype == torch.float32 and tuple(feats.shape) == (3200, 128)
    host = feats.cpu().numpy()
    classes = np.where(blob == 0, 1, np.where(blob == 3, 2, -1))
    for kw, ids, cls, cand, own in ((dict(), [1, 2], classes, ~np.isin(blob, [0, 3]), False),
                                    (dict(obj=2, within="all", cos_min=0.97), [2], np.where(blob == 3, 2, -1), None, True)):
        res = ses.lookalikes(**kw)
        match, score, counts = restated(host, cls, ids, kw.get("cos_min", 0.9), candidate=cand, own=own)
        print(f"backbone features, {kw}: {int((match >= 0).sum())} of 3200 voxels matched, {res.n_regions} regions")
        holds(res, match, score, ses.inverse_map)
        assert res.prototypes == counts and res.rows_nonfinite == 0 and res.examples_left_out == 0
        keys = np.where(match >= 0, match, -1)
        assert sum(c["voxels"] for c in res.candidates) <= int((keys >= 0).sum())
        assert all(match[c["row"]] == c["object"] for c in res.candidates)
