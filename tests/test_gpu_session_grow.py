"""-m gpu: growing a selection along the surface through the session (InteractiveSession.grow, grow_at, shrink).  The rule is
restated in ``grow_rule.py`` and applied to the session's own voxel rows and inverse map; everything is integer, so every
comparison is exact.  Logits are replayed through ``infer(logits=...)``.

1  grow from a select() result, a tensor, a list of rows: every field of the GrowResult against the rule, under each kind of
   ``within``; no session state changes
2  grow_at on a rendered pixel, a cloud and a mesh: the vertex shown is selected, within="label" stays on its object, a
   background pixel gives None
3  paint(grow_result) changes exactly the vertices not painted so yet; shrink against the rule
4  grow("clicks", within="label"): every voxel's owner is a clicked voxel, every clicked voxel owns itself
5  a radius beyond the step bound raises; a GrowResult of another scene raises
"""
import numpy as np
import pytest
import torch

import grow_rule as G
from agile3d_amd.synthetic import make_scene
from session_kit import DEV, _model, intrinsic, jittered_grid, look_at

pytestmark = pytest.mark.gpu
VS = 0.02


@pytest.fixture(scope="module")
def model_002():
    return _model(VS)


def _session(model, xyz, col, lab=None, faces=None):
    from agile3d_amd.session import InteractiveSession
    return InteractiveSession(model, voxel_size=VS).load_scene(xyz, col, lab, faces=faces)


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene at full resolution: every voxel's point plus a second vertex 4 mm beside it, shuffled
    (as test_gpu_session_pieces.py builds its scene)."""
    sc = make_scene(5_000, seed=6, voxel_size=VS)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def annotated(ses, scene, wrong=0.1):
    """Three objects and the background clicked (two clicks on the first object), then logits replayed whose arg-max is the
    ground truth folded onto the objects 0..3 with a share ``wrong`` of the voxels relabelled at random."""
    xyz, _, lab = scene
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:3]
    for k, i in enumerate(inst):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == inst[0])[-1]], 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    ori = ses.labels_qv_ori.cpu().numpy()
    want = np.zeros(len(ori), np.int64)
    for k, i in enumerate(inst):
        want[ori == i] = k + 1
    rng = np.random.default_rng(1)
    flip = rng.uniform(size=len(ori)) < wrong
    want[flip] = rng.integers(0, 4, int(flip.sum()))
    clicked = [r for rows in ses.click_idx.values() for r in rows]
    logits = np.full((len(ori), 4), -2.0, np.float32)
    logits[np.arange(len(ori)), want] = 3.0
    return ses.infer(logits=torch.from_numpy(logits).to(DEV)), clicked


def voxel_coords(ses):
    """int [n_voxels, 4] (b, x, y, z) of the session's voxel rows, as its scene was built from them."""
    return ses._scene_handle().coords.cpu().numpy().astype(np.int64)


def state_of(ses):
    manual = None if ses._manual is None else tuple(t.clone() for t in ses._manual)
    return ses.clicks(), ses._labels_qv.clone(), None if ses._labels_last is None else ses._labels_last.clone(), manual


def same_state(ses, before):
    clicks, labels_qv, labels_last, manual = state_of(ses)
    assert clicks == before[0] and torch.equal(labels_qv, before[1])
    assert (labels_last is None) == (before[2] is None) and (labels_last is None or torch.equal(labels_last, before[2]))
    assert (manual is None) == (before[3] is None) and (manual is None or all(torch.equal(a, b) for a, b in zip(manual, before[3])))


def check_grow(ses, got, want, cost, limit, connectivity, within):
    for name, field in (("selected", "selected_full"), ("dist_full", "dist_full"), ("dist_qv", "dist_qv"), ("owner_qv", "owner_qv")):
        t = getattr(got, name)
        assert t.dtype == (torch.uint8 if name == "selected" else torch.int32) and np.array_equal(t.cpu().numpy(), want[field]), name
    s = want["summary"]
    assert (got.count, got.reached_voxels, got.seeds) == (s["selected"], s["reached"], s["seeds"]) and s["err"] == 0
    unit = VS / 1024.0 if cost == G.METRIC_COST else VS
    assert got.max_distance == s["max_dist"] * unit
    assert (got.limit, got.cost, got.connectivity, got.within) == (limit, cost, connectivity, within)


def view_of(ses, w=96, h=72):
    k, e = ses.default_view(w, h)
    return ses.render(k, e, w, h, radius=0.03)


# ---------------------------------------------------------------------------------------------------- 1
def test_grow_against_the_rule(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    annotated(ses, scene)
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    n, n_full = len(coords), len(xyz)
    labels = ses._labels_qv.cpu().numpy()
    view = view_of(ses)
    sel = ses.select(view, ses.region_mask(view, stroke=[(30.0, 30.0), (50.0, 40.0)], radius=3.0))
    s = sel.selected.cpu().numpy()
    assert 0 < sel.count < n_full // 2
    before = state_of(ses)
    radius = 5 * VS
    limit = int(np.floor(np.float64(radius) / np.float64(VS) * 1024.0))
    assert limit in (5120, 5119)
    rule = lambda **kw: G.grow_all(coords, kw.pop("keys", None), kw.pop("cost", G.METRIC_COST), kw.pop("limit", limit),
                                   kw.pop("connectivity", 26), inverse_map=inv, n_full=n_full, **kw)
    # a SelectResult, the same as a uint8 and as a bool tensor; a radius in world units
    got = ses.grow(sel, radius=radius)
    want = rule(seed_full=s)
    check_grow(ses, got, want, G.METRIC_COST, limit, 26, "all")
    assert got.count > sel.count and got.seeds == len(set(inv[s != 0].tolist()))
    assert (got.selected.cpu().numpy()[s != 0] == 1).all()             # the seeds' own vertices are selected
    for same in (sel.selected, sel.selected != 0, got):                 # (a GrowResult seeds with what it selected)
        again = ses.grow(same, radius=radius)
        check_grow(ses, again, want if same is not got else rule(seed_full=want["selected_full"]), G.METRIC_COST, limit, 26, "all")
    # hops; each connectivity; each kind of within
    for c in (6, 18, 26):
        check_grow(ses, ses.grow(sel, steps=4, connectivity=c), rule(seed_full=s, cost=(1, 1, 1), limit=4, connectivity=c),
                   (1, 1, 1), 4, c, "all")
    got = ses.grow(sel, steps=6, within="label")
    check_grow(ses, got, rule(seed_full=s, cost=(1, 1, 1), limit=6, keys=labels), (1, 1, 1), 6, 26, "label")
    assert got.count < ses.grow(sel, steps=6).count                     # the labelling's borders stop the walk
    mask = coords[:, 1] % 7 != 0                                        # slabs: planes x = 7 k cannot be walked on
    for within, keys in ((torch.from_numpy(mask).to(DEV), np.where(mask, 0, -1)),
                         (torch.from_numpy(mask.astype(np.uint8)).to(DEV), np.where(mask, 0, -1)),
                         (torch.from_numpy((coords[:, 2] // 9 - 1).astype(np.int32)).to(DEV), coords[:, 2] // 9 - 1)):
        got = ses.grow(sel, radius=radius, within=within)
        check_grow(ses, got, rule(seed_full=s, keys=keys), G.METRIC_COST, limit, 26, "keys")
    # a list of voxel rows; limit 0 selects the seeds' voxels only
    rows = [3, 17, n - 1]
    got = ses.grow(rows, steps=0)
    check_grow(ses, got, rule(seed_qv=np.bincount(rows, minlength=n).astype(np.uint8), cost=(1, 1, 1), limit=0), (1, 1, 1), 0, 26, "all")
    assert got.seeds == got.reached_voxels == 3 and got.max_distance == 0.0 and got.count == int(np.isin(inv, rows).sum())
    same_state(ses, before)
    for bad in (lambda: ses.grow(sel), lambda: ses.grow(sel, radius=0.1, steps=2), lambda: ses.grow(sel, radius=-1.0),
                lambda: ses.grow(sel, steps=1.5), lambda: ses.grow(sel, steps=2, connectivity=9),
                lambda: ses.grow(sel, steps=2, within="object"), lambda: ses.grow(sel, steps=2, within=torch.zeros(n, device=DEV)),
                lambda: ses.grow(sel, steps=2, within=torch.zeros(n - 1, dtype=torch.int32, device=DEV)),
                lambda: ses.grow("click", steps=2), lambda: ses.grow([n], steps=2), lambda: ses.grow([-1], steps=2),
                lambda: ses.grow(sel.selected[:-1], steps=2), lambda: ses.grow(sel.selected.cpu(), steps=2),
                lambda: ses.grow(3.5, steps=2), lambda: ses.shrink(sel), lambda: ses.shrink(sel.selected[:-1], steps=1),
                lambda: ses.grow_at(view, 0, 0), lambda: ses.grow_at(view, 96, 0, steps=1)):
        with pytest.raises(ValueError):
            bad()
    same_state(ses, before)


# ---------------------------------------------------------------------------------------------------- 2
def test_grow_at_on_a_cloud(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    annotated(ses, scene)
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    labels = ses._labels_qv.cpu().numpy()
    view = view_of(ses)
    ids = view.ids.cpu().numpy()
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 50 and (ids < 0).any()
    before = state_of(ses)
    spilled = 0
    for v, u in shown[:: len(shown) // 8]:
        vertex = int(ids[v, u])
        seed = np.bincount([vertex], minlength=len(xyz)).astype(np.uint8)
        got = ses.grow_at(view, u, v, radius=0.15)
        limit = got.limit
        assert limit == int(np.floor(np.float64(0.15) / np.float64(VS) * 1024.0))
        want = G.grow_all(coords, labels, G.METRIC_COST, limit, 26, seed_full=seed, inverse_map=inv, n_full=len(xyz))
        check_grow(ses, got, want, G.METRIC_COST, limit, 26, "label")
        picked = got.selected.cpu().numpy() != 0
        assert picked[vertex] and got.seeds == 1 and int(got.dist_full[vertex]) == 0
        assert (labels[inv[picked]] == labels[inv[vertex]]).all()       # no vertex of another label
        anywhere = ses.grow_at(view, u, v, radius=0.15, within="all")
        check_grow(ses, anywhere, G.grow_all(coords, None, G.METRIC_COST, limit, 26, seed_full=seed, inverse_map=inv, n_full=len(xyz)),
                   G.METRIC_COST, limit, 26, "all")
        spilled += anywhere.count > got.count
    assert spilled > 0                                                  # somewhere the walk without keys crosses a border
    v, u = np.argwhere(ids < 0)[0]
    assert ses.grow_at(view, u, v, radius=0.15) is None and ses.grow_at(view, u, v, steps=3, within="all") is None
    same_state(ses, before)


def test_grow_at_on_a_mesh(model_002):
    xyz, faces = jittered_grid(40, 40, seed=3)
    xyz = (xyz * 0.15).astype(np.float32)                               # vertices 15 mm apart: neighbouring voxels of 20 mm
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32), faces=faces)
    ses.click(xyz[5], 1)
    ses.click(xyz[900], 2)
    n = ses.raw_coords_qv.shape[0]
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    side = np.where(coords[:, 1] < np.median(coords[:, 1]), 1, 2)       # two objects, a straight border between them
    logits = np.full((n, 3), -2.0, np.float32)
    logits[np.arange(n), side] = 3.0
    ses.infer(logits=torch.from_numpy(logits).to(DEV))
    labels = ses._labels_qv.cpu().numpy()
    assert set(labels.tolist()) == {1, 2}
    w, h = 64, 48
    mid = float(xyz[:, 0].mean())
    view = ses.render(intrinsic(w, h), look_at([mid, mid, 0.8], [mid, mid, 0.0], up=(0.0, 1.0, 0.0)), w, h)           # from above
    ids, wu, wv = (t.cpu().numpy() for t in (view.ids, view.u, view.v))
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 100 and (ids < 0).any()
    stopped = 0
    for v, u in shown[:: len(shown) // 10]:
        a, b = wu[v, u], wv[v, u]
        ww = np.float32(np.float32(1.0) - a) - b
        corner = 0 if (ww >= a and ww >= b) else (1 if a >= b else 2)         # the heaviest corner, ties to the lower one
        vertex = int(faces[ids[v, u]][corner])
        seed = np.bincount([vertex], minlength=len(xyz)).astype(np.uint8)
        got = ses.grow_at(view, u, v, steps=5, connectivity=18)
        check_grow(ses, got, G.grow_all(coords, labels, (1, 1, 1), 5, 18, seed_full=seed, inverse_map=inv, n_full=len(xyz)),
                   (1, 1, 1), 5, 18, "label")
        picked = got.selected.cpu().numpy() != 0
        assert picked[vertex] and (labels[inv[picked]] == labels[inv[vertex]]).all() and got.count > 20
        stopped += got.count < ses.grow_at(view, u, v, steps=5, connectivity=18, within="all").count
    assert stopped > 0
    v, u = np.argwhere(ids < 0)[0]
    assert ses.grow_at(view, u, v, steps=5) is None


# ---------------------------------------------------------------------------------------------------- 3
def test_paint_and_shrink(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    annotated(ses, scene)
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    view = view_of(ses)
    sel = ses.select(view, ses.region_mask(view, stroke=[(40.0, 36.0)], radius=8.0), through=True)
    s = sel.selected.cpu().numpy() != 0
    assert sel.count > 50
    k = 3
    grown = ses.grow(sel, steps=k)
    g = grown.selected.cpu().numpy() != 0
    assert (g[s]).all() and grown.count == g.sum() > sel.count
    # paint: exactly the grown vertices that are not painted so yet
    assert ses.paint(sel, 2) == sel.count
    assert ses.paint(grown, 2) == grown.count - sel.count
    assert ses.paint(grown, 2) == 0 and ses.corrected().overridden == grown.count
    assert ses.erase(grown) == grown.count
    # shrink, against the rule
    before = state_of(ses)
    for steps, c in ((k, 26), (1, 6), (0, 26)):
        back = ses.shrink(grown, steps=steps, connectivity=c)
        want = G.shrink_numpy(coords, inv, g, (1, 1, 1), steps, c)
        assert back.selected.dtype == torch.uint8 and np.array_equal(back.selected.cpu().numpy(), want) and back.count == want.sum()
        assert (back.limit, back.cost, back.connectivity, back.within) == (steps, (1, 1, 1), c, "all")
        held = np.zeros(len(coords), bool)
        held[inv[g]] = True
        from_outside = G.grow_numpy(coords, None, (1, 1, 1), steps, c, seed_qv=(~held).astype(np.uint8))[0]
        assert np.array_equal(back.dist_qv.cpu().numpy(), from_outside) and back.seeds == (~held).sum()
    back = ses.shrink(grown, steps=k)
    kept = back.selected.cpu().numpy() != 0
    from_outside = G.grow_numpy(coords, None, (1, 1, 1), k, 26, seed_qv=(~held).astype(np.uint8))[0]
    interior = s & (from_outside[inv] < 0)                              # the vertices of s whose voxel is interior to the grown set
    assert interior.sum() > 20 and kept[interior].all() and not kept[~g].any() and kept.sum() < g.sum()
    assert ses.shrink(grown, steps=0).count == grown.count              # limit 0 takes nothing away
    metric = ses.shrink(grown, radius=2 * VS)
    assert np.array_equal(metric.selected.cpu().numpy(), G.shrink_numpy(coords, inv, g, G.METRIC_COST, metric.limit, 26))
    assert metric.limit in (2048, 2047) and metric.cost == G.METRIC_COST
    same_state(ses, before)


# ---------------------------------------------------------------------------------------------------- 4
def test_grow_from_the_clicks(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    _, clicked = annotated(ses, scene)
    coords, inv = voxel_coords(ses), ses.inverse_map.cpu().numpy()
    labels = ses._labels_qv.cpu().numpy()
    n = len(coords)
    assert len(set(clicked)) == 5
    before = state_of(ses)
    got = ses.grow("clicks", steps=40, within="label")
    want = G.grow_all(coords, labels, (1, 1, 1), 40, 26, seed_qv=np.bincount(clicked, minlength=n).astype(np.uint8),
                      inverse_map=inv, n_full=len(xyz))
    check_grow(ses, got, want, (1, 1, 1), 40, 26, "label")
    owner = got.owner_qv.cpu().numpy()
    assert set(owner[owner >= 0].tolist()) == set(clicked) and all(owner[r] == r for r in clicked) and got.seeds == 5
    assert (labels[owner[owner >= 0]] == labels[owner >= 0]).all()     # a voxel's owner is a click of its own object
    two = [r for r in ses.click_idx["1"]]
    assert len(two) == 2 and all((owner == r).sum() > 1 for r in two)  # the object with two clicks is split between them
    same_state(ses, before)


# ---------------------------------------------------------------------------------------------------- 5
def test_the_step_bound_and_a_stale_result(model_002, scene):
    xyz, col, lab = scene
    ses = _session(model_002, xyz, col, lab)
    ses.click(xyz[0], 1)
    got = ses.grow("clicks", radius=1024 * VS)                          # the largest radius taken: 1024 voxel steps
    assert got.limit // 1024 in (1024, 1023) and got.seeds == 1 and got.reached_voxels > 100
    for bad in (lambda: ses.grow("clicks", radius=1025 * VS + 1e-6), lambda: ses.grow("clicks", steps=1025),
                lambda: ses.shrink(got, radius=30.0), lambda: ses.grow_at(view_of(ses), 0, 0, steps=4000)):
        with pytest.raises(ValueError, match="pieces"):
            bad()
    ses.load_scene(xyz[:500], col[:500], lab[:500])
    ses.click(xyz[0], 1)
    for stale in (lambda: ses.paint(got, 1), lambda: ses.erase(got), lambda: ses.grow(got, steps=1), lambda: ses.shrink(got, steps=1)):
        with pytest.raises(ValueError):
            stale()
    fresh = ses.grow("clicks", steps=2)
    assert tuple(fresh.selected.shape) == (500,) and ses.paint(fresh, 1) == fresh.count
