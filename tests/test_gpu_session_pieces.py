"""-m gpu: where in space a label lies, through the session (InteractiveSession.pieces, piece_at, despeckle,
guide(regions="connected")).  The rules are restated in ``pieces_rule.py`` and ``guide_rule.py``; logits are replayed through
``infer(logits=...)``.

1  pieces() against the rule on the session's own voxel rows; piece_at on a rendered pixel, on a cloud and on a mesh
2  despeckle() against the rule lifted through the inverse map; it leaves clicks(), preview() and a following guide() alone
3  two disjoint contested spots of one (winner, runner-up) pair: guide() suggests one click, guide(regions="connected") two,
   each the deepest voxel of its spot by a float64 brute force; guide() itself is unchanged bit for bit
"""
import numpy as np
import pytest
import torch

from agile3d_amd.synthetic import make_scene
from guide_rule import guide_numpy
from pieces_rule import absorb_numpy, noisy, pieces_numpy
from session_kit import DEV, _model, bits, intrinsic, jittered_grid, look_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


def _session(model, xyz, col, lab=None, faces=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=0.02).load_scene(xyz, col, lab, faces=faces)


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene at full resolution: every voxel's point plus a second vertex 4 mm beside it, shuffled
    (as test_gpu_session_guide.py builds its scene)."""
    sc = make_scene(5_000, seed=6, voxel_size=0.02)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def voxel_coords(ses):
    """int [n_voxels, 4] (b, x, y, z) of the session's voxel rows, as its scene was built from them."""
    return ses._scene_handle().coords.cpu().numpy().astype(np.int64)


def speckled(ses, scene, seed=0):
    """Three objects clicked, then logits replayed whose arg-max is the ground truth folded onto the objects 0..3 with 5 % of
    the voxels relabelled at random: objects in a few large pieces plus specks."""
    xyz, _, lab = scene
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:3]
    for k, i in enumerate(inst):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    ori = ses.labels_qv_ori.cpu().numpy()
    folded = np.zeros(len(ori), np.int64)
    for k, i in enumerate(inst):
        folded[ori == i] = k + 1
    want = noisy(folded, seed)
    logits = np.full((len(ori), 4), -2.0, np.float32)
    logits[np.arange(len(ori)), want] = 3.0
    res = ses.infer(logits=torch.from_numpy(logits).to(DEV))
    return res, logits


def record_tuple(r):
    return (int(r["root"]), int(r["key"]), int(r["voxels"]), int(r["clicked"]), r["lo"].tolist(), r["hi"].tolist())


# ---------------------------------------------------------------------------------------------------- 1
def test_pieces_against_the_rule(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    coords = voxel_coords(ses)
    n = len(coords)
    # from load_scene on: everything is background, one piece per connected part of the scan
    first = ses.pieces()
    piece, rec = pieces_numpy(coords, np.zeros(n), 26)
    assert np.array_equal(first.piece_qv.cpu().numpy(), piece) and first.n_pieces == len(rec) and first.object_pieces.tolist() == [len(rec)]
    speckled(ses, scene)
    labels = ses._labels_qv.cpu().numpy()
    clicks = [r for rows in ses.click_idx.values() for r in rows]
    inv = ses.inverse_map.cpu().numpy()
    for c in (6, 18, 26):
        got = ses.pieces(connectivity=c)
        piece, rec = pieces_numpy(coords, labels, c, clicks)
        assert np.array_equal(got.piece_qv.cpu().numpy(), piece) and np.array_equal(got.piece_full.cpu().numpy(), piece[inv])
        assert got.n_pieces == len(rec) > 100 and got.connectivity == c
        assert [record_tuple(r) for r in got.records] == [record_tuple(r) for r in rec]
        assert got.object_pieces.tolist() == np.bincount(rec["key"], minlength=4).tolist() and got.records["clicked"].sum() >= 3
    # another labelling of the same voxels; more pieces than the first buffer holds: the call is made again
    scattered = np.random.default_rng(1).integers(0, 200, n)                # next to no two neighbours agree
    got = ses.pieces(labels=torch.from_numpy(scattered.astype(np.int32)).to(DEV))
    piece, rec = pieces_numpy(coords, scattered, 26, clicks)
    assert got.n_pieces == len(rec) > 1024 and np.array_equal(got.records["root"], rec["root"])
    assert np.array_equal(got.piece_qv.cpu().numpy(), piece)
    with pytest.raises(ValueError):
        ses.pieces(connectivity=4)


def test_piece_at_on_a_cloud(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    speckled(ses, scene)
    pieces = ses.pieces()
    w, h = 96, 72
    k, e = ses.default_view(w, h)
    view = ses.render(k, e, w, h, radius=0.03)
    ids = view.ids.cpu().numpy()
    piece_full = pieces.piece_full.cpu().numpy()
    by_root = {int(r["root"]): r for r in pieces.records}
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 50 and (ids < 0).any()
    for v, u in shown[:: len(shown) // 12]:
        want = by_root[int(piece_full[ids[v, u]])]
        assert record_tuple(ses.piece_at(view, u, v, pieces)) == record_tuple(want)
        assert record_tuple(ses.piece_at(view, u, v)) == record_tuple(want)          # computed on the spot: the same
    v, u = np.argwhere(ids < 0)[0]
    assert ses.piece_at(view, u, v, pieces) is None
    with pytest.raises(ValueError):
        ses.piece_at(view, w, 0, pieces)


def test_piece_at_on_a_mesh(model_002):
    xyz, faces = jittered_grid(20, 20, seed=3)
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32), faces=faces)
    ses.click(xyz[5], 1)
    ses.click(xyz[300], 2)
    n = ses.raw_coords_qv.shape[0]
    ses.infer(logits=torch.from_numpy(np.random.default_rng(0).normal(0, 2, (n, 3)).astype(np.float32)).to(DEV))
    pieces = ses.pieces()
    piece_full = pieces.piece_full.cpu().numpy()
    by_root = {int(r["root"]): r for r in pieces.records}
    w, h = 64, 48
    view = ses.render(intrinsic(w, h), look_at([0.95, 0.95, 2.0], [0.95, 0.95, 0.0], up=(0.0, 1.0, 0.0)), w, h)     # from above
    ids, wu, wv = (t.cpu().numpy() for t in (view.ids, view.u, view.v))
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 100
    for v, u in shown[:: len(shown) // 16]:
        a, b = wu[v, u], wv[v, u]
        ww = np.float32(np.float32(1.0) - a) - b
        corner = 0 if (ww >= a and ww >= b) else (1 if a >= b else 2)         # the heaviest corner, ties to the lower one
        vertex = faces[ids[v, u]][corner]
        assert record_tuple(ses.piece_at(view, u, v, pieces)) == record_tuple(by_root[int(piece_full[vertex])])


# ---------------------------------------------------------------------------------------------------- 2
def test_despeckle(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    res, logits = speckled(ses, scene)
    coords = voxel_coords(ses)
    labels = ses._labels_qv.cpu().numpy()
    clicks = [r for rows in ses.click_idx.values() for r in rows]
    inv = ses.inverse_map.cpu().numpy()
    before = dict(clicks=ses.clicks(), preview=[t.cpu().numpy() for t in ses.preview()], guide=ses.guide(),
                  labels_qv=ses._labels_qv.clone(), logits=ses._guide_logits[0].clone())
    for min_voxels, c in ((8, 26), (2, 6), (1, 26)):
        got = ses.despeckle(min_voxels=min_voxels, connectivity=c)
        want, rule = absorb_numpy(coords, labels, min_voxels, c, clicks)
        assert np.array_equal(got.labels_qv.cpu().numpy(), want) and np.array_equal(got.labels_full.cpu().numpy(), want[inv])
        assert {k: getattr(got, k) for k in ("small_pieces", "relabelled_pieces", "relabelled_voxels", "kept_isolated")} == \
            {k: rule[k] for k in ("small_pieces", "relabelled_pieces", "relabelled_voxels", "kept_isolated")}
        assert (rule["relabelled_pieces"] > 50) == (min_voxels > 1)
        # colours: the palette entry of the object, the vertex's own for the background
        colors = got.colors.cpu().numpy()
        full = want[inv]
        assert np.array_equal(colors[full > 0], ses.palette[full[full > 0]]) and np.array_equal(colors[full == 0], col[full == 0])
        # IoU against the relabelled ground truth, in float64
        gt = ses.new_labels.cpu().numpy()
        ious = [((full == k) & (gt == k)).sum() / max(((full == k) | (gt == k)).sum(), 1) for k in (1, 2, 3)]
        assert abs(got.miou - np.mean(ious)) < 1e-6
    assert got.relabelled_pieces == 0 and np.array_equal(got.labels_qv.cpu().numpy(), labels)      # min_voxels = 1: nothing is small
    default = ses.despeckle()
    assert default.min_voxels == 8 and default.connectivity == 26 and default.miou > res.miou        # the specks were errors
    # no state changed
    assert ses.clicks() == before["clicks"] and torch.equal(ses._labels_qv, before["labels_qv"])
    assert torch.equal(ses._guide_logits[0], before["logits"])
    for a, b in zip(ses.preview(), before["preview"]):
        assert np.array_equal(a.cpu().numpy(), b)
    after = ses.guide()
    assert after.suggestions == before["guide"].suggestions and torch.equal(after.colors, before["guide"].colors)
    assert torch.equal(after.margin_full, before["guide"].margin_full)
    # the result shows through the existing view calls
    w, h = 48, 36
    k, e = ses.default_view(w, h)
    view = ses.render(k, e, w, h, colors=default.colors, radius=0.03)
    ses.annotate(view, labels=default.labels_full)
    # without ground truth: no IoU
    bare = _session(model_002, xyz, col)
    bare.click(xyz[0], 1)
    bare.infer(logits=torch.from_numpy(logits).to(DEV))
    assert bare.despeckle().miou is None


# ---------------------------------------------------------------------------------------------------- 3
def two_spot_scene(seed=0):
    """A 40 x 40 x 2 lattice with one point per 2 cm voxel (jittered by +-6 mm inside it), so that neighbouring points are
    neighbouring voxels, and logits [n, 2] as a function of the coordinates: the background wins everywhere; object 1 comes
    within 0.5 of it inside two discs (radii 11 cm and 8 cm) at opposite corners, and nowhere else."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    xyz = ((g + 0.5) * 0.02 + rng.uniform(-0.006, 0.006, g.shape)).astype(np.float32)
    centres, radii = np.array([[0.2, 0.2], [0.6, 0.6]]), (0.11, 0.08)

    def spot_of(coords):
        d = np.linalg.norm(coords[:, None, :2].astype(np.float64) - centres[None], axis=2)
        return np.where(d[:, 0] < radii[0], 0, np.where(d[:, 1] < radii[1], 1, -1))

    def logits_at(coords):
        x = np.zeros((len(coords), 2), np.float32)
        x[:, 0] = 2.0
        x[:, 1] = np.where(spot_of(coords) >= 0, 1.5, -5.0)
        return x
    return xyz[rng.permutation(len(xyz))], spot_of, logits_at


def deepest(coords, member):
    """(row, depth, relative lead over the second deepest) of the member farthest from every non-member, in float64."""
    x = coords.astype(np.float64)
    rows = np.flatnonzero(member)
    d = np.sqrt(((x[member][:, None, :] - x[~member][None]) ** 2).sum(2)).min(1)
    top = np.sort(d)[::-1]
    return int(rows[d.argmax()]), float(top[0]), float((top[0] - top[1]) / top[0])


def test_two_spots_of_one_pair(model_002):
    xyz, spot_of, logits_at = two_spot_scene()
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32))
    coords = ses.raw_coords_qv.cpu().numpy()
    assert len(coords) == 3200                                            # (one point per voxel)
    corner = int(np.argmax(coords[:, 0] - coords[:, 1]))                  # far from both discs
    row, _ = ses.click(coords[corner], 1)
    assert row == corner and spot_of(coords)[corner] < 0
    x = logits_at(coords)
    ses.infer(logits=torch.from_numpy(x).to(DEV))
    spot = spot_of(coords)
    sizes = [int((spot == k).sum()) for k in (0, 1)]
    assert min(sizes) > 20 and sizes[0] > sizes[1]
    # as it was: the two discs are ONE region of the pair (runner-up 1, winner 0) and get ONE suggestion
    pairs = ses.guide()
    assert pairs.n_contested == sum(sizes) and len(pairs.suggestions) == 1 and pairs.n_spots is None
    assert set(pairs.suggestions[0]) == {"row", "point", "object", "current", "size"}
    both = deepest(coords, spot >= 0)
    assert both[2] >= 1e-4 and pairs.suggestions[0]["row"] == both[0]     # the deeper of the two
    # connected: two spots, a suggestion inside each, each the deepest voxel of ITS spot
    g = ses.guide(regions="connected")
    assert (g.n_spots, g.n_spots_searched, len(g.suggestions)) == (2, 2, 2)
    want = [deepest(coords, spot == k) for k in (0, 1)]
    assert min(w[2] for w in want) >= 1e-4, want                          # no tie the fp32 search could break differently
    assert want[0][1] > want[1][1]                                        # ranked by depth: the larger disc first
    vox = voxel_coords(ses)
    piece, rec = pieces_numpy(vox, np.where(spot >= 0, 256, -1), 26)
    assert len(rec) == 2
    for s, (row, depth, _), k in zip(g.suggestions, want, (0, 1)):
        assert s["row"] == row and spot[s["row"]] == k and (s["object"], s["current"]) == (1, 0), (s, row)
        assert abs(s["size"] - depth) <= 1e-5 * depth and np.array_equal(np.float32(s["point"]), coords[row])
        assert s["voxels"] == sizes[k] and s["root"] == int(np.flatnonzero(spot == k).min()) == int(piece[row])
    assert ses.guide(regions="connected", max_suggestions=1).suggestions == g.suggestions[:1]
    for field in ("labels_qv", "runner_qv", "margin_qv", "margin_full", "colors"):
        assert torch.equal(getattr(g, field), getattr(pairs, field)), field
    # guide() with no argument is what it was before the new mode ran: bit for bit, and the rule's
    again = ses.guide()
    rule = guide_numpy(x, [corner], [1], 1.0)
    assert again.suggestions == pairs.suggestions and again.n_spots is None and again.least_confident == pairs.least_confident
    assert np.array_equal(again.labels_qv.cpu().numpy(), rule["label"]) and np.array_equal(again.runner_qv.cpu().numpy(), rule["runner"])
    assert np.array_equal(bits(again.margin_qv.cpu().numpy()), bits(rule["margin"]))
    for field in ("labels_qv", "runner_qv", "margin_qv", "margin_full", "colors"):
        assert torch.equal(getattr(again, field), getattr(pairs, field)), field
    assert again.object_contested.tolist() == pairs.object_contested.tolist() == rule["contested_per_label"][:2].tolist()
    with pytest.raises(ValueError):
        ses.guide(regions="islands")


def test_connected_whole_scene_and_none(model_002, scene):
    """Constant logits without a clicked voxel among their rows: ONE spot covers every voxel of a connected scan and has no
    border; the existing fallback holds -- the least confident voxel, ``size = inf``.  Sure logits: no spot, no suggestion."""
    xyz, _, _ = two_spot_scene()
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32))
    n = ses.raw_coords_qv.shape[0]
    ses.click(xyz[0], 1)
    flat = torch.zeros((n, 2), device=DEV)
    ses.infer(logits=flat)
    ses._guide_logits = (flat, {"0": []})
    g = ses.guide(regions="connected")
    assert (g.n_spots, g.n_spots_searched, g.n_contested) == (1, 1, n)
    assert g.suggestions == [{"row": 0, "point": [float(c) for c in ses.raw_coords_qv[0].cpu()], "object": 1, "current": 0,
                              "size": float("inf"), "voxels": n, "root": 0}]
    sure = torch.zeros((n, 2), device=DEV)
    sure[:, 0] = 9.0
    ses.infer(logits=sure)
    g = ses.guide(regions="connected")
    assert (g.n_spots, g.n_spots_searched, g.suggestions) == (0, 0, [])
