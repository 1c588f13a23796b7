"""-m gpu: where the segmentation is unsure (a3d_session_guide in csrc/session_guide.hip; view.session_guide;
InteractiveSession.guide, confidence_at).  The rules are restated in ``guide_rule.py``.

1  the voxel pass, bit for bit against the restatement, outputs pre-filled with sentinels: row counts around the wave, the
   workgroup's tile and beyond one pass of the grid, 2 .. 256 columns (one row per thread up to 32 columns, fewer beyond),
   logits drawn from five values so that ties are common, rows built for every order of winner and runner-up, clicks at
   the first and the last row, twice on one row, outside the rows, and as many as the call takes
2  the summary record against the restatement, twice the same; no finite margin; a NaN row
3  the full-resolution pass, colours by their bits: labels beyond the palette, the background, margins 0 and inf, no inverse
   map, an inverse-map entry out of range
4  the wrapper's and the library's own refusals
5  guide()'s suggestions against the CPU oracle's error clusters on jittered lattices with three logit cones
6  the session: when guide() is allowed, what it returns, the confidence view, confidence_at, the suggested click taken
"""
import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.synthetic import make_scene
from guide_rule import BAD_INDEX, NAN_MARGIN, blend_numpy, guide_numpy, lift_numpy
from oracle import clicks as oc
from session_kit import DEV, _dev, _model, bits, byref, intrinsic, jittered_grid, look_at, status

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 4099)
COLUMNS = (2, 3, 11, 21, 64, 256)
VALUES = np.array([-1.5, 0.0, 0.25, 2.0, 2.0, 3.5], np.float32)          # five values, one twice as likely
SENTINEL = -77
INVALID, OK = -1, 0                                                       # A3D_ERR_INVALID, A3D_OK (include/agile3d_hip.h)


# ---------------------------------------------------------------------------------------------------- the adaptor
def guide_gpu(logits, click_rows=(), click_objs=(), threshold=1.0, vertices=None):
    """view.session_guide, numpy in / numpy out.  ``vertices``: ``dict(inverse_map (or None), colors, palette, doubt,
    full_margin)`` for the full-resolution half.  Every output starts as a sentinel."""
    n = len(logits)
    lab, run, want = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3))
    mar = torch.full((n,), float(SENTINEL), dtype=torch.float32, device=DEV)
    summary = torch.full((V.GUIDE_SUMMARY.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)
    kw = {}
    if vertices is not None:
        m = len(vertices["colors"])
        inv = vertices["inverse_map"]
        kw = dict(inverse_map=None if inv is None else _dev(inv, np.int64), colors=_dev(vertices["colors"], np.float32),
                  palette=_dev(vertices["palette"], np.float32), doubt_color=vertices["doubt"],
                  full_margin=vertices["full_margin"], margin_full=torch.full((m,), float(SENTINEL), dtype=torch.float32, device=DEV),
                  colors_out=torch.full((m, 3), float(SENTINEL), dtype=torch.float32, device=DEV))
    got = V.session_guide(_dev(logits, np.float32), list(click_rows), list(click_objs), threshold, labels=lab,
                          runner=run, margin=mar, want=want, summary=summary, **kw)
    assert got[0] is lab and got[1] is run and got[2] is mar and got[3] is want and got[6] is summary
    host = summary.cpu().numpy()
    out = dict(label=lab.cpu().numpy(), runner=run.cpu().numpy(), margin=mar.cpu().numpy(), want=want.cpu().numpy(),
               summary_bytes=host, **V.read_guide_summary(host))
    if vertices is not None:
        out.update(margin_full=got[4].cpu().numpy(), colors=got[5].cpu().numpy())
    return out


def same_voxels(got, rule, what):
    for k in ("label", "runner", "want"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], rule[k]), (what, k)
    nan = np.isnan(rule["margin"])
    assert np.array_equal(np.isnan(got["margin"]), nan), what
    assert np.array_equal(bits(got["margin"])[~nan], bits(rule["margin"])[~nan]), what


def same_summary(got, rule, what):
    assert np.array_equal(got["voxels"], rule["voxels"]) and np.array_equal(got["contested"], rule["contested_per_label"]), what
    assert got["least"] == rule["least"] and got["err"] == rule["err"], (what, got["least"], rule["least"])


def logits_for(n, c, rng):
    """fp32 [n, c] drawn from VALUES, the first rows built by hand: the maximum in the first column; in the last; the
    runner-up before the winner; behind it; all columns equal; the maximum twice (the first wins, the second is the
    runner-up with margin 0)."""
    x = VALUES[rng.integers(0, len(VALUES), (n, c))]
    special = np.full((6, c), -1.5, np.float32)
    special[0, 0] = 3.5
    special[1, c - 1] = 3.5
    special[2, [0, c - 1]] = [2.0, 3.5]
    special[3, [0, c - 1]] = [3.5, 2.0]
    special[4] = 0.25
    special[5, [0, c - 1]] = 3.5
    x[:min(n, 6)] = special[:n]
    return x


def clicks_for(n, c, rng, how):
    if how == "none":
        return [], []
    if how == "edges":                           # first and last row, one row twice with two objects, rows outside
        rows = [0, n - 1, n // 2, n, -1, n // 2, 2 ** 31 - 1]
        objs = [c - 1, 1, 0, 1, 1, c - 1, 0]
        return rows, objs
    rows = rng.integers(0, n, L.A3D_MAX_CLICKS).tolist()                 # as many as the call takes, duplicates among them
    return rows, rng.integers(0, c, L.A3D_MAX_CLICKS).tolist()


# ---------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("c", COLUMNS)
def test_voxel_pass_against_the_rule(c):
    rng = np.random.default_rng(c)
    for n in ROWS:
        x = logits_for(n, c, rng)
        for how, threshold in (("none", 1.0), ("edges", 1.75), ("full", 0.25)):
            rows, objs = clicks_for(n, c, rng, how)
            rule = guide_numpy(x, rows, objs, threshold)
            got = guide_gpu(x, rows, objs, threshold)
            same_voxels(got, rule, (n, c, how))
            same_summary(got, rule, (n, c, how))
            assert rule["err"] == 0 and (rule["margin"] >= 0).all()
        if n >= 6:
            plain = guide_numpy(x, [], [], 1.0)
            assert plain["label"][:6].tolist() == [0, c - 1, c - 1, 0, 0, 0]
            assert plain["runner"][:6].tolist() == [1, 0, 0, c - 1, 1, c - 1] and plain["margin"][4] == 0 == plain["margin"][5]
            assert plain["contested"].any() and not plain["contested"].all()


@pytest.mark.parametrize("c", (2, 3))
def test_voxel_pass_beyond_one_pass_of_the_grid(c):
    n = 300_001                                  # > 1024 workgroups x 256 rows: the grid comes round again
    rng = np.random.default_rng(100 + c)
    x = logits_for(n, c, rng)
    rows, objs = clicks_for(n, c, rng, "edges")
    rule = guide_numpy(x, rows, objs, 1.0)
    got = guide_gpu(x, rows, objs, 1.0)
    same_voxels(got, rule, (n, c))
    same_summary(got, rule, (n, c))
    assert np.array_equal(guide_gpu(x, rows, objs, 1.0)["summary_bytes"], got["summary_bytes"])


def test_summary_record():
    rng = np.random.default_rng(5)
    n, c = 4099, 11
    x = rng.normal(0, 2, (n, c)).astype(np.float32)                  # (continuous: no margin is 0 unless a row is built so)
    x[3000] = x[77] = 1.0                        # two rows of margin 0: the lower one is the least confident
    rows, objs = [0, n - 1], [3, 4]
    rule = guide_numpy(x, rows, objs, 0.5)
    assert rule["least"] == (77, 0.0) and 0 < rule["contested"].sum() < n and rule["voxels"].sum() == n
    first, second = guide_gpu(x, rows, objs, 0.5), guide_gpu(x, rows, objs, 0.5)
    same_summary(first, rule, "first")
    assert np.array_equal(first["summary_bytes"], second["summary_bytes"])            # run to run the same bytes
    # the smallest margin at the last row of a tile's last thread
    x[77], x[3000] = rng.normal(0, 2, (2, c)).astype(np.float32)
    x[2047, :] = 0.0
    x[2047, 5] = 1e-30
    rule = guide_numpy(x, rows, objs, 0.5)
    assert rule["least"] == (2047, float(np.float32(1e-30)))
    same_summary(guide_gpu(x, rows, objs, 0.5), rule, "tiny margin")
    # every row clicked: no finite margin
    few = x[:200]
    every = guide_gpu(few, list(range(200)), [1 + k % 5 for k in range(200)], 0.5)
    rule = guide_numpy(few, list(range(200)), [1 + k % 5 for k in range(200)], 0.5)
    same_voxels(every, rule, "all clicked")
    same_summary(every, rule, "all clicked")
    assert every["least"] is None and np.isinf(every["margin"]).all() and every["contested"].sum() == 0
    assert every["summary_bytes"].view(V.GUIDE_SUMMARY)["least_key"][0] == 0                        # its complement: row -1
    # one NaN row: bit 0, not contested, label and runner columns of the row
    bad = x.copy()
    bad[1234, 0] = np.nan                        # the scan starts on it and never leaves: label 0, margin NaN
    rule = guide_numpy(bad, rows, objs, 0.5)
    got = guide_gpu(bad, rows, objs, 0.5)
    same_voxels(got, rule, "nan")
    same_summary(got, rule, "nan")
    assert got["err"] == NAN_MARGIN and np.isnan(got["margin"][1234]) and got["want"][1234] == got["label"][1234]
    assert 0 <= got["label"][1234] < c and 0 <= got["runner"][1234] < c and got["least"][0] != 1234


# ---------------------------------------------------------------------------------------------------- 3
def test_full_resolution_pass():
    rng = np.random.default_rng(9)
    n, c, m = 700, 40, 5003                      # 39 objects over a palette of 7: labels wrap
    x = (rng.normal(0, 2, (n, c))).astype(np.float32)
    x[:50] = 0.0                                 # margin 0, label 0: the doubt colour whatever the vertex's own
    x[50:100, 0] = 30.0                          # background, sure
    x[100:150] = 0.0
    x[100:150, 17] = 1.0                         # margin 1 on object 17
    rows, objs = list(range(150, 170)), [1 + k for k in range(20)]      # clicked: margin inf
    palette = rng.uniform(0, 1, (7, 3)).astype(np.float32)
    own = rng.uniform(0, 1, (m, 3)).astype(np.float32)
    inv = rng.integers(0, n, m)
    inv[:n] = rng.permutation(n)                 # every voxel shows
    doubt = (0.9, 0.95, 1.0)
    for full_margin, inverse_map, colors in ((4.0, inv, own), (3.0, inv, own), (0.7, None, own[:n])):
        v = dict(inverse_map=inverse_map, colors=colors, palette=palette, doubt=doubt, full_margin=full_margin)
        got = guide_gpu(x, rows, objs, 1.0, vertices=v)
        rule = guide_numpy(x, rows, objs, 1.0)
        same_voxels(got, rule, full_margin)
        margin_full, valid, err = lift_numpy(rule["margin"], inverse_map, np.float32(SENTINEL))
        label_full = lift_numpy(rule["label"], inverse_map, 0)[0]
        assert valid.all() and err == 0 and got["err"] == 0
        assert np.array_equal(bits(got["margin_full"]), bits(margin_full))
        want = blend_numpy(label_full, margin_full, colors, palette, doubt, full_margin)
        assert np.array_equal(bits(got["colors"]), bits(want)), full_margin
        src = np.arange(n) if inverse_map is None else inverse_map
        zero, sure_bg, clicked = src < 50, (src >= 50) & (src < 100), (src >= 150) & (src < 170)
        assert zero.any() and sure_bg.any() and clicked.any() and (label_full > 6).any()
        assert np.array_equal(got["colors"][zero], np.broadcast_to(np.float32(doubt), (zero.sum(), 3)))   # exactly doubt
        assert np.array_equal(got["colors"][sure_bg], colors[sure_bg])                                     # exactly its own
        wrapped = 1 + (label_full[clicked] - 1) % 6
        assert np.array_equal(got["colors"][clicked], palette[wrapped]) and np.isinf(got["margin_full"][clicked]).all()
    # an inverse-map entry out of range: bit 1, the vertex untouched
    worse = inv.copy()
    worse[[0, 2500, m - 1]] = [n, -1, 2 ** 40]
    got = guide_gpu(x, rows, objs, 1.0, vertices=dict(inverse_map=worse, colors=own, palette=palette, doubt=doubt, full_margin=4.0))
    margin_full, valid, err = lift_numpy(guide_numpy(x, rows, objs, 1.0)["margin"], worse, np.float32(SENTINEL))
    assert err == BAD_INDEX and got["err"] == BAD_INDEX and (~valid).sum() == 3
    assert np.array_equal(bits(got["margin_full"]), bits(margin_full))
    assert (got["colors"][~valid] == SENTINEL).all() and (got["colors"][valid] != SENTINEL).all()
    # no voxels at all: every vertex is out of range; no vertices: only the voxels
    none = guide_gpu(np.zeros((0, 3), np.float32), vertices=dict(inverse_map=None, colors=own[:4], palette=palette, doubt=doubt,
                                                                 full_margin=4.0))
    assert none["err"] == BAD_INDEX and (none["colors"] == SENTINEL).all() and none["least"] is None and none["voxels"].sum() == 0
    only = guide_gpu(x, rows, objs, 1.0, vertices=dict(inverse_map=np.zeros(0, np.int64), colors=np.zeros((0, 3), np.float32),
                                                       palette=palette, doubt=doubt, full_margin=4.0))
    same_voxels(only, guide_numpy(x, rows, objs, 1.0), "no vertices")


# ---------------------------------------------------------------------------------------------------- 4
def test_wrapper_refusals():
    x = _dev(np.zeros((5, 3)), np.float32)
    col, pal, inv = _dev(np.zeros((7, 3)), np.float32), _dev(np.zeros((4, 3)), np.float32), _dev(np.zeros(7), np.int64)
    good = dict(logits=x, click_rows=[1], click_objs=[2], threshold=1.0)
    full = dict(good, inverse_map=inv, colors=col, palette=pal)
    V.session_guide(**good), V.session_guide(**full)
    for bad in (dict(good, logits=x.cpu()), dict(good, logits=x.double()), dict(good, logits=x[:, :1].contiguous()),
                dict(good, logits=torch.zeros((2, 257), device=DEV)), dict(good, logits=x.t()), dict(good, logits=x[0]),
                dict(good, click_rows=[1, 2]), dict(good, click_objs=[256]), dict(good, click_objs=[-1]),
                dict(good, click_rows=[0] * 257, click_objs=[0] * 257), dict(good, threshold=0.0), dict(good, threshold=-1.0),
                dict(good, threshold=float("nan")), dict(good, threshold=float("inf")), dict(good, threshold=1e39),
                dict(good, full_margin=0.0), dict(good, full_margin=float("inf")), dict(good, full_margin=float("nan")),
                dict(good, inverse_map=inv), dict(good, margin_full=torch.zeros(7, device=DEV)),
                dict(full, palette=None), dict(full, palette=pal[:1]), dict(full, palette=torch.zeros((257, 3), device=DEV)),
                dict(full, inverse_map=inv[:6]), dict(full, inverse_map=inv.int()), dict(full, colors=col[:, :2].contiguous()),
                dict(full, doubt_color=(1.0, 1.0)), dict(full, colors_out=torch.zeros((6, 3), device=DEV)),
                dict(good, labels=torch.zeros(5, device=DEV)), dict(good, margin=torch.zeros(4, device=DEV)),
                dict(good, summary=torch.zeros(100, dtype=torch.uint8, device=DEV)),
                dict(good, summary=torch.zeros(V.GUIDE_SUMMARY.itemsize + 4, dtype=torch.uint8, device=DEV)[4:])):
        with pytest.raises(ValueError):
            V.session_guide(**bad)


def test_library_refusals():
    n, m = 5, 7
    x, col, pal = _dev(np.zeros((n, 3)), np.float32), _dev(np.zeros((m, 3)), np.float32), _dev(np.zeros((4, 3)), np.float32)
    lab, run, want = (torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3))
    mar = torch.full((n,), float(SENTINEL), dtype=torch.float32, device=DEV)
    mfull, cout = torch.full((m,), float(SENTINEL), device=DEV), torch.full((m, 3), float(SENTINEL), device=DEV)
    summary = torch.full((V.GUIDE_SUMMARY.itemsize,), 0x5a, dtype=torch.uint8, device=DEV)

    def call(**kw):
        a = L.SessionGuideArgs()
        for k, v in kw.items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_session_guide", byref(a), None)

    voxels = dict(logits_dev=x, n_qv=n, n_classes=3, labels_qv_dev=lab, runner_qv_dev=run, margin_qv_dev=mar, want_qv_dev=want,
                  summary_dev=summary, threshold=1.0, full_margin=4.0)
    full = dict(voxels, n_full=m, colors_full_dev=col, palette_dev=pal, n_palette=4, margin_full_dev=mfull, colors_out_dev=cout)
    assert status("a3d_session_guide", None, None) == INVALID
    inf, nan = float("inf"), float("nan")
    for bad in (dict(voxels, n_classes=1), dict(voxels, n_classes=257), dict(voxels, n_classes=0), dict(voxels, n_qv=-1),
                dict(voxels, n_qv=2 ** 31), dict(voxels, n_full=-1), dict(voxels, n_clicks=-1),
                dict(voxels, n_clicks=L.A3D_MAX_CLICKS + 1), dict(voxels, threshold=0.0), dict(voxels, threshold=-1.0),
                dict(voxels, threshold=inf), dict(voxels, threshold=nan), dict(voxels, full_margin=0.0),
                dict(voxels, full_margin=-2.0), dict(voxels, full_margin=inf), dict(voxels, full_margin=nan),
                dict(voxels, summary_dev=None), dict(voxels, logits_dev=None), dict(voxels, labels_qv_dev=None),
                dict(voxels, runner_qv_dev=None), dict(voxels, margin_qv_dev=None), dict(voxels, want_qv_dev=None),
                dict(full, colors_full_dev=None), dict(full, palette_dev=None), dict(full, margin_full_dev=None),
                dict(full, colors_out_dev=None), dict(full, n_palette=1), dict(full, n_palette=257)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert lab.cpu().tolist() == [SENTINEL] * n and (cout.cpu().numpy() == SENTINEL).all()          # nothing was launched
    assert (summary.cpu().numpy() == 0x5a).all()
    assert call(**dict(voxels, n_qv=0, logits_dev=None, labels_qv_dev=None)) == OK                  # an absent half
    assert V.read_guide_summary(summary.cpu().numpy())["voxels"].sum() == 0
    assert call(**dict(full, inverse_map_dev=None)) == OK
    assert lab.cpu().tolist() == [0] * n and run.cpu().tolist() == [1] * n and mar.cpu().tolist() == [0.0] * n
    assert want.cpu().tolist() == [1] * n and mfull.cpu().tolist() == [0.0] * n + [SENTINEL] * (m - n)
    got = V.read_guide_summary(summary.cpu().numpy())
    assert got["voxels"][0] == n and got["contested"][0] == n and got["least"] == (0, 0.0) and got["err"] == BAD_INDEX


# ---------------------------------------------------------------------------------------------------- 5, 6: the session
@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


def _session(model, xyz, col, faces=None):
    from agile3d_amd.session import InteractiveSession
    ses = InteractiveSession(model, voxel_size=0.02)
    return ses.load_scene(xyz, col, None, faces=faces)


def cone_scene(shape, seed):
    """The construction the suggestions were checked on: a jittered lattice of ``shape`` points 5 cm apart (+-2 cm), K = 3
    logit cones ``6 - 50 d / extent`` (d: the distance to the cone's centre, extent: the lattice's longest side) over a zero
    background, N(0, 0.15) noise on every logit.  Returns (xyz fp32 [n, 3], the three centres fp32 [3, 3], a function of
    coordinates that gives the logits fp32 [n, 4])."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = shape
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3) * 0.05
    xyz = (g + rng.uniform(-0.02, 0.02, g.shape)).astype(np.float32)
    extent = 0.05 * max(shape)
    centres = xyz[[int(np.argmin(((g - np.array(f) * [nx, ny, nz] * 0.05) ** 2).sum(1))) for f in
                   ((0.25, 0.3, 0.5), (0.72, 0.35, 0.5), (0.45, 0.75, 0.5))]]
    noise = np.random.default_rng(seed + 1000).normal(0, 0.15, (nx, ny, nz, 4))      # per lattice cell: the logits are a function
    #                                                                                  of the coordinates, whatever order they come in

    def logits_at(coords):
        d = np.linalg.norm(coords[:, None, :].astype(np.float64) - centres[None].astype(np.float64), axis=2)
        cones = 6.0 - 50.0 * d / extent
        cell = np.rint(coords.astype(np.float64) / 0.05).astype(np.int64)              # (the jitter stays below half a cell)
        x = np.concatenate([np.zeros((len(coords), 1)), cones], 1) + noise[cell[:, 0], cell[:, 1], cell[:, 2]]
        return x.astype(np.float32)
    return xyz, centres, logits_at


def relative_leads(pred, want, coords):
    """Per error cluster, in float64: (largest outside distance - second largest) / largest over the cluster's points; a
    cluster of one point leads by 1."""
    p, w, x = np.asarray(pred), np.asarray(want), np.asarray(coords, np.float64)
    ids = np.where(p != w, 96 * w + 11 * p, -1)
    out = {}
    for cid in np.unique(ids[ids >= 0]):
        member = ids == cid
        d = np.sqrt(((x[member][:, None, :] - x[~member][None]) ** 2).sum(2)).min(1)
        top = np.sort(d)[::-1]
        out[int(cid)] = 1.0 if len(top) == 1 else float((top[0] - top[1]) / top[0])
    return out


@pytest.mark.parametrize("seed", range(6))
def test_suggestions_against_the_oracle(model_002, seed):
    xyz, centres, logits_at = cone_scene((24, 24, 3), seed)
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32))
    for k, centre in enumerate(centres):
        ses.click(centre, k + 1)
    coords = ses.raw_coords_qv.cpu().numpy()
    assert len(coords) == 24 * 24 * 3                                     # (no two points share a 2 cm voxel)
    x = logits_at(coords)
    ses.infer(logits=torch.from_numpy(x).to(DEV))
    g = ses.guide(threshold=1.0, max_suggestions=100)
    rows = [r for key in ses.click_idx for r in ses.click_idx[key]]
    objs = [int(key) for key in ses.click_idx for _ in ses.click_idx[key]]
    rule = guide_numpy(x, rows, objs, 1.0)
    assert np.array_equal(g.labels_qv.cpu().numpy(), rule["label"]) and np.array_equal(g.runner_qv.cpu().numpy(), rule["runner"])
    assert g.n_contested == rule["contested"].sum() and g.least_confident == rule["least"]
    # the oracle on the same coordinates as float64: torch.cdist in fp32 takes |a|^2 + |b|^2 - 2ab beyond a few rows, which
    # at 1 m from the origin and 5 cm sizes is itself 1e-5 off; the library's distances are exact fp32 from the differences
    clusters = oc.error_clusters(torch.from_numpy(rule["label"]), torch.from_numpy(rule["want"]),
                                 torch.from_numpy(coords.astype(np.float64)))
    leads = relative_leads(rule["label"], rule["want"], coords)
    print(f"seed {seed}: {len(coords)} voxels, {len(clusters)} clusters, {int(rule['contested'].sum())} contested, "
          f"smallest relative lead {min(leads.values()):.2e}")
    assert len(clusters) >= 6 and sorted(leads) == [c["cluster_id"] for c in clusters]
    assert min(leads.values()) >= 1e-4, leads                             # no tie the fp32 search could break differently
    ranked = sorted(clusters, key=lambda c: c["error_size"], reverse=True)                # stable: ties keep ascending id
    assert len(g.suggestions) == len(ranked)
    for s, c in zip(g.suggestions, ranked):
        assert (s["row"], s["object"], s["current"]) == (c["row"], c["label"], c["pred"]), (s, c)
        assert abs(s["size"] - c["error_size"]) <= 1e-5 * c["error_size"], (s, c)
        assert np.array_equal(np.float32(s["point"]), coords[c["row"]]) and s["object"] == rule["runner"][c["row"]]
    assert ses.guide(max_suggestions=2).suggestions == g.suggestions[:2]


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene at full resolution: every voxel's point plus a second vertex 4 mm beside it, shuffled
    (as test_gpu_session_edit.py builds its scene)."""
    sc = make_scene(5_000, seed=6, voxel_size=0.02)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def _clicked(ses, scene, n_objects=3):
    xyz, _, lab = scene
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:n_objects]
    for k, i in enumerate(inst):
        ses.click(xyz[np.flatnonzero(lab == i)[0]], k + 1)
    ses.click(xyz[np.flatnonzero(lab == 0)[0]], 0)
    return ses


def test_guide_describes_the_last_inference_only(model_002, scene):
    ses = _session(model_002, scene[0], scene[1])
    with pytest.raises(ValueError, match=r"infer\(\)"):
        ses.guide()
    _clicked(ses, scene)
    with pytest.raises(ValueError, match=r"infer\(\)"):
        ses.guide()
    ses.infer()
    ses.guide()
    ses.click(scene[0][5], 1)
    with pytest.raises(ValueError, match=r"infer\(\)"):
        ses.guide()
    with pytest.raises(ValueError):
        ses.confidence_at(ses.render(*ses.default_view(32, 24), 32, 24), 3, 3)
    ses.infer()
    ses.guide()
    assert ses.undo()["index"] == 4
    with pytest.raises(ValueError, match=r"infer\(\)"):
        ses.guide()
    for edit in (lambda: ses.redo(), lambda: ses.remove_click(0), lambda: ses.reset(),
                 lambda: ses.restore_clicks({"0": [3], "1": [9]}, {"0": [0], "1": [1]}), lambda: ses.load_scene(scene[0], scene[1])):
        if ses.num_clicks == 0:
            _clicked(ses, scene)
        ses.infer()
        ses.guide()
        edit()
        with pytest.raises(ValueError, match=r"infer\(\)"):
            ses.guide()
    for bad in (dict(threshold=0.0), dict(full_margin=float("inf")), dict(doubt_color=(1.0, 2.0)), dict(max_suggestions=-1)):
        _clicked(ses, scene) if ses.num_clicks == 0 else None
        ses.infer()
        with pytest.raises(ValueError):
            ses.guide(**bad)


def test_guide_through_the_session(model_002, scene):
    xyz, col, _ = scene
    ses = _clicked(_session(model_002, xyz, col), scene)
    res = ses.infer()
    logits = ses._guide_logits[0].cpu().numpy()
    g = ses.guide()
    assert torch.equal(g.labels_qv, ses._labels_qv)                       # what infer() computed, row for row
    rows = [r for key in ses.click_idx for r in ses.click_idx[key]]
    objs = [int(key) for key in ses.click_idx for _ in ses.click_idx[key]]
    rule = guide_numpy(logits, rows, objs, 1.0)
    for got, want in ((g.labels_qv, rule["label"]), (g.runner_qv, rule["runner"])):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(bits(g.margin_qv.cpu().numpy()), bits(rule["margin"]))
    inv = ses.inverse_map.cpu().numpy()
    assert np.array_equal(bits(g.margin_full.cpu().numpy()), bits(rule["margin"][inv]))
    assert torch.equal(g.margin_full, g.margin_qv[ses.inverse_map])
    want_col = blend_numpy(rule["label"][inv], rule["margin"][inv], col, ses.palette, (1.0, 1.0, 1.0), 4.0)
    assert np.array_equal(bits(g.colors.cpu().numpy()), bits(want_col))
    assert torch.equal(ses._colors_last, res.colors)                      # the default view stays the inference's
    assert g.object_voxels.tolist() == rule["voxels"][:4].tolist() and g.object_contested.tolist() == rule["contested_per_label"][:4].tolist()
    assert g.least_confident == rule["least"] and g.n_contested == rule["contested"].sum() and len(g.suggestions) <= 5
    assert g.suggestions == ses.guide(max_suggestions=5).suggestions
    # the confidence view renders as it is, and confidence_at reads the vertex under a pixel
    w, h = 96, 72
    k, e = ses.default_view(w, h)
    view = ses.render(k, e, w, h, colors=g.colors, radius=0.03)
    ids = view.ids.cpu().numpy()
    margin_full = g.margin_full.cpu().numpy()
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 50 and (ids < 0).any()
    for v, u in shown[:: len(shown) // 12]:
        assert ses.confidence_at(view, u, v) == float(margin_full[ids[v, u]])
    v, u = np.argwhere(ids < 0)[0]
    assert ses.confidence_at(view, u, v) is None
    with pytest.raises(ValueError):
        ses.confidence_at(view, w, 0)
    # the follow-up: take the first suggestion, infer again
    if g.suggestions:
        s = g.suggestions[0]
        assert s["object"] == rule["runner"][s["row"]] and s["current"] == rule["label"][s["row"]] and s["size"] > 0
        row, _ = ses.click(s["point"], s["object"])
        assert row == s["row"]
        again = ses.infer()
        assert int(ses._labels_qv[row]) == s["object"] and again.num_obj == 3
        assert ses.guide().labels_qv[row] == s["object"]


def test_constant_logits(model_002, scene):
    """Constant logits: every voxel but the clicked ones is contested (label 0, runner-up 1, margin 0).  The clicked voxels
    are never contested, so the region keeps a border -- them -- and its deepest voxel is the one farthest from every click.
    A region WITHOUT a border needs logits without a clicked voxel, which ``infer()`` never keeps (it refuses to run without
    a click); that path of ``guide()`` is driven here by handing it such a state: the suggestion is then the least
    confident voxel alone, with ``size = inf``, and nothing raises."""
    xyz, col, _ = scene
    ses = _clicked(_session(model_002, xyz, col), scene)
    n = ses.raw_coords_qv.shape[0]
    flat = torch.zeros((n, 4), device=DEV)
    ses.infer(logits=flat)
    g = ses.guide()
    clicked = sorted({r for rows in ses.click_idx.values() for r in rows})
    assert g.n_contested == n - len(clicked) and g.least_confident == (min(set(range(clicked[-1] + 2)) - set(clicked)), 0.0)
    assert g.object_contested.tolist() == [n - len(clicked), 0, 0, 0] and len(g.suggestions) == 1
    coords = ses.raw_coords_qv.cpu().numpy().astype(np.float64)
    depth = np.sqrt(((coords[:, None] - coords[clicked][None]) ** 2).sum(2)).min(1)
    s = g.suggestions[0]
    assert (s["object"], s["current"]) == (1, 0) and np.isfinite(s["size"])
    assert abs(s["size"] - depth.max()) <= 1e-5 * depth.max() and depth[s["row"]] >= depth.max() * (1 - 1e-5)
    # no clicked voxel among the logits' rows: one region, no border
    ses._guide_logits = (flat, {"0": []})
    g = ses.guide()
    assert g.n_contested == n and g.least_confident == (0, 0.0)
    assert g.suggestions == [{"row": 0, "point": [float(c) for c in ses.raw_coords_qv[0].cpu()], "object": 1, "current": 0,
                              "size": float("inf")}]
    assert ses.guide(max_suggestions=0).suggestions == []


def test_confidence_at_on_a_mesh(model_002):
    """On a mesh the pixel's vertex is the heaviest corner of its face, ties to the lower corner: ``object_at``'s."""
    xyz, faces = jittered_grid(20, 20, seed=3)
    ses = _session(model_002, xyz, np.full(xyz.shape, 0.5, np.float32), faces=faces)
    ses.click(xyz[5], 1)
    ses.click(xyz[300], 2)
    n = ses.raw_coords_qv.shape[0]
    ses.infer(logits=torch.from_numpy(np.random.default_rng(0).normal(0, 2, (n, 3)).astype(np.float32)).to(DEV))
    g = ses.guide()
    w, h = 64, 48
    view = ses.render(intrinsic(w, h), look_at([0.95, 0.95, 2.0], [0.95, 0.95, 0.0], up=(0.0, 1.0, 0.0)), w, h)     # from above
    ids, wu, wv = (t.cpu().numpy() for t in (view.ids, view.u, view.v))
    margin_full = g.margin_full.cpu().numpy()
    labels_full = g.labels_qv.cpu().numpy()[ses.inverse_map.cpu().numpy()]
    shown = np.argwhere(ids >= 0)
    assert len(shown) > 100
    for v, u in shown[:: len(shown) // 16]:
        a, b = wu[v, u], wv[v, u]
        ww = np.float32(np.float32(1.0) - a) - b
        corner = 0 if (ww >= a and ww >= b) else (1 if a >= b else 2)
        vertex = faces[ids[v, u]][corner]
        assert ses.confidence_at(view, u, v) == float(margin_full[vertex])
        assert ses.object_at(view, u, v, labels=g.labels_qv[ses.inverse_map].contiguous()) == labels_full[vertex]
