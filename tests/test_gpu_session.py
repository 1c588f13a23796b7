"""-m gpu: the headless interactive session (agile3d_amd/session.py on csrc/session.hip).  Reads tests/golden only.
The library is reached through ``session_kit.py``'s adaptors over ``agile3d_amd.view``; the rules are in ``pick_rule.py``.

1  a3d_nearest_rows against the float64 brute-force arg-min (fixture scenes, synthetic 80 k / 300 k rows x 64 queries)
2  a3d_pick_ray against a float64 statement of the pick rule
3  a3d_session_paint against numpy and against the colours / labels the reference's get_next_click produced
4  InteractiveSession == the existing public path (forward_mask -> clicks.argmax_labels -> [inverse_map]), bit for bit
5  the reference's bookkeeping, record line and files, replayed from the fixtures (recorded logits go in through
   ``infer(logits=)``: labels, colours, IoU string, file names and contents are then compared with what the
   reference's get_next_click wrote; the model call itself is covered by 4)
6  determinism, reset(), no state left from a previous scene; load_scene_dir == load_scene on the same arrays
7  refusals
"""
import copy
import os
from datetime import datetime

import numpy as np
import pytest
import torch

import session_kit
from agile3d_amd import clicks as K
from agile3d_amd import lib as L
from agile3d_amd.synthetic import make_scene
from pick_rule import U, fp32_rule_argmin, paint_numpy, pick_rule_f64
from session_kit import CASES, DEV, _model, f64_argmin, load_session_case, nearest_rows, pick_ray, session_paint

pytestmark = pytest.mark.gpu


def check_nearest(rows, queries, got, max_under=0.02):
    """``got`` must equal the float64 arg-min (first index) wherever float64 can speak for the fp32 rule.

    The bound.  The inputs are fp32 numbers, so float64 evaluates d^2 = dx^2 + dy^2 + dz^2 of them with a relative error
    of ~1e-16: it is the exact value for this purpose.  The kernel computes dx = fl(x - qx): ONE rounding, relative to
    the difference (not to the coordinates -- that is the point of the difference form), |dx_fp32 - dx| <= u |dx|,
    u = 2^-24.  dx^2 then carries (1 + u)^2 from dx and (1 + u) from the product: <= 3u (+ O(u^2)) relative.  The two
    additions of non-negative terms add <= u each: the computed d^2 is within 5u + O(u^2) < 6u of the exact one,
    relatively.  Two rows a (best) and b keep their order in fp32 whenever d_b^2 (1 - 6u) > d_a^2 (1 + 6u), which holds if
    d_b^2 - d_a^2 > 6u (d_a^2 + d_b^2); as d_a^2 <= d_b^2 it is enough that the gap exceeds 12u d_b^2.  The test uses
    16u x d_second^2 = 2^-20 d_second^2 -- derived from the magnitude of the DISTANCE; the coordinate magnitude (50 m in
    the translated scene) does not enter, which is why the kernel is exact where |a|^2 + |b|^2 - 2ab is not.  Rows that
    tie exactly in float64 must be bit-identical rows (duplicates, where the lowest index must win); a float64 tie
    between different rows counts as "under the bound".  At most ``max_under`` of the queries may be under the bound."""
    rows64 = rows.astype(np.float64)
    under = 0
    for qi, q in enumerate(queries):
        d2 = ((rows64 - q.astype(np.float64)) ** 2).sum(1)
        best = int(d2.argmin())
        ties = np.flatnonzero(d2 == d2[best])
        rest = d2[d2 > d2[best]]
        second = rest.min() if len(rest) else np.inf
        informative = (rows[ties] == rows[best]).all() and second - d2[best] > 16 * U * second
        if informative:
            assert got[qi] == best, (qi, got[qi], best, d2[best], second)
        else:
            under += 1
        assert got[qi] == fp32_rule_argmin(rows, q), (qi, "the fp32 rule itself, bit for bit")
    assert under <= max_under * len(queries), f"{under} of {len(queries)} queries under the bound: uninformative"


# ---------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", CASES)
def test_nearest_rows_fixture_scenes(name):
    c, _ = load_session_case(name)
    xyz32 = c["coords_full"].astype(np.float32)
    qv = xyz32[c["unique_map"]]
    got = nearest_rows([qv, xyz32], c["click_points"])
    # every reference-run fixture row (where the reference's find_nearest equals the float64 arg-min) matches exactly
    assert np.array_equal(got[0], c["click_rows_qv"]) and np.array_equal(got[1], c["click_rows_full"])
    check_nearest(qv, c["click_points"], got[0], max_under=0.0)
    check_nearest(xyz32, c["click_points"], got[1], max_under=0.0)
    # and random queries over the scene's extent, 64 per call
    rng = np.random.default_rng(5)
    q = (rng.uniform(xyz32.min(0), xyz32.max(0), (64, 3))).astype(np.float32)
    got = nearest_rows([qv, xyz32], q)
    check_nearest(qv, q, got[0])
    check_nearest(xyz32, q, got[1])


@pytest.mark.parametrize("n,shift", [(80_000, (0.0, 0.0, 0.0)), (300_000, (50.3, -48.7, 1.2))])
def test_nearest_rows_synthetic(n, shift):
    """64 queries against a synthetic scene: random points near the surface, queries EQUAL to a row (distance 0), and rows
    that are exact duplicates of earlier rows -- some of them the nearest row of a query (the lowest index must win)."""
    sc = make_scene(n, seed=11)
    rows = (sc["raw_xyz"] + np.asarray(shift, np.float32)).astype(np.float32)
    assert n <= len(rows) <= 1.01 * n                                # make_scene(seed 11): 80 021 and 300 816 rows
    rng = np.random.default_rng(n)
    src = rng.choice(len(rows) // 2, 200, replace=False)
    dst = len(rows) // 2 + rng.choice(len(rows) // 2, 200, replace=False)
    rows[dst] = rows[src]                                            # duplicates at higher indices
    q = np.empty((64, 3), np.float32)
    q[:40] = rows[rng.choice(len(rows), 40)] + rng.normal(0, 0.02, (40, 3)).astype(np.float32)
    q[40:52] = rows[rng.choice(len(rows), 12)]                       # equal to a row
    q[52:58] = rows[dst[:6]]                                         # equal to a duplicated row: index src must win
    q[58:] = rows[src[6:12]] + np.float32(1e-4)
    got = nearest_rows([rows], q)[0]
    check_nearest(rows, q, got)
    assert np.array_equal(got[52:58], src[:6])
    d0 = ((rows[got[40:52]] - q[40:52]) ** 2).sum(1)
    assert (d0 == 0).all()
    # two sources of different sizes in one call, one query
    got2 = nearest_rows([rows[:1000], rows], q[:1])
    assert got2[1, 0] == got[0] and got2[0, 0] == f64_argmin(rows[:1000], q[0])


# ---------------------------------------------------------------------------------------------------- 2
def _pick_scene():
    """A 20 k-point cloud plus, far above it (nothing else within metres), the points of the constructed cases."""
    xyz = make_scene(20_000, seed=4)["raw_xyz"].astype(np.float32)
    hi = xyz.max(0)
    n = len(xyz)
    cases = {}
    # two points on one ray: the nearer one wins although it is stored later
    o, d = np.array([1.0, 1.0, hi[2] + 5.0], np.float32), np.array([0.6, 0.8, 0.0], np.float32)
    extra = [o + np.float32(3.0) * d, o + np.float32(2.0) * d]
    cases["two on one ray"] = (o, d, n + 1)
    # equal t, different perpendicular distance: d = +x and both points share x, so t = 2 exactly in fp32 and float64;
    # the one closer to the ray wins although it is stored later
    o = np.array([1.0, 1.0, hi[2] + 8.0], np.float32)
    extra += [o + np.array([2.0, 0.02, 0.0], np.float32), o + np.array([2.0, 0.01, 0.0], np.float32)]
    cases["equal t"] = (o, np.array([1.0, 0.0, 0.0], np.float32), n + 3)
    # an exact duplicate of a vertex on the ray: equal t, equal distance -> the lower index
    o = np.array([1.0, 1.0, hi[2] + 11.0], np.float32)
    extra += [o + np.array([2.0, 0.01, 0.0], np.float32)] * 2
    cases["duplicate"] = (o, np.array([1.0, 0.0, 0.0], np.float32), n + 4)
    return np.concatenate([xyz, np.stack(extra)]).astype(np.float32), n, cases


def _draw_rays(xyz, n_cloud, r, rng, counts, cap=60):
    """``counts[kind]`` rays of every kind, each REDRAWN until it meets the margin condition (at most ``cap`` draws): the
    first two candidates differ in t by >= 1e-3, no point lies within 1e-4 of the cylinder surface or of the plane t = 0."""
    lo, hi = xyz[:n_cloud].min(0), xyz[:n_cloud].max(0)

    def unit():
        v = rng.normal(size=3)
        return (v / np.linalg.norm(v)).astype(np.float32)

    def draw(kind):
        if kind == "hit":                                # from outside the room towards a point of the scene
            d = unit()
            return (xyz[rng.integers(n_cloud)] - np.float32(4.0) * d + rng.normal(0, 0.005, 3).astype(np.float32)).astype(np.float32), d
        if kind == "inside":                             # starts inside the cloud
            return rng.uniform(lo + 0.2, hi - 0.2).astype(np.float32), unit()
        return (hi + np.float32(1.0)).astype(np.float32), np.abs(unit())   # "miss": leaves the scene behind

    rays = []
    for kind, cnt in counts.items():
        for _ in range(cnt):
            for _try in range(cap):
                o, d = draw(kind)
                d = (d / np.float32(np.linalg.norm(d.astype(np.float64)))).astype(np.float32)
                want, gap, surface, plane = pick_rule_f64(xyz, o, d, r)
                if gap >= 1e-3 and surface >= 1e-4 and plane >= 1e-4:
                    break
            else:
                raise AssertionError(f"no {kind} ray met the margin condition in {cap} draws")
            rays.append((kind, o, d))
    return rays


def test_pick_ray_against_float64_rule():
    """Rays that hit, miss, start inside the cloud, two points on one ray -- every ray drawn until it meets the margin
    condition, which is then asserted on ALL rays used -- and the two tie rules on constructed points whose t (and
    distance) are bitwise equal in fp32 and float64, so that no margin is involved."""
    rng = np.random.default_rng(3)
    xyz, n_cloud, cases = _pick_scene()
    dev = torch.from_numpy(xyz).to(DEV)
    r = 0.03
    rays = _draw_rays(xyz, n_cloud, r, rng, {"hit": 24, "inside": 8, "miss": 6})
    rays.append(("two on one ray",) + cases["two on one ray"][:2])
    assert len(rays) == 39
    hits = misses = 0
    for kind, o, d in rays:
        want, gap, surface, plane = pick_rule_f64(xyz, o, d, r)
        assert gap >= 1e-3 and surface >= 1e-4 and plane >= 1e-4, (kind, gap, surface, plane)     # the margin condition
        got, p = pick_ray(dev, o, d, r)
        assert got == want, (kind, got, want)
        if want >= 0:
            assert np.array_equal(p, xyz[want])
            hits += 1
        else:
            misses += 1
        if kind == "hit":
            assert want >= 0
        if kind == "miss":
            assert want == -1
        if kind == "two on one ray":
            assert want == cases[kind][2]
    assert hits >= 25 and misses >= 6
    # ties: equal t -> the smaller perpendicular distance; equal t and distance -> the lower index
    for kind in ("equal t", "duplicate"):
        o, d, expect = cases[kind]
        want, gap, _, _ = pick_rule_f64(xyz, o, d, r)
        assert gap == 0.0 and want == expect, (kind, gap, want)
        assert pick_ray(dev, o, d, r)[0] == expect, kind


# ---------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", CASES)
def test_session_paint_fixture_scenes(name):
    c, meta = load_session_case(name)
    xyz32, col32 = c["coords_full"].astype(np.float32), c["colors_full"].astype(np.float32)
    pal = c["palette"]
    cube_col = np.stack([c["background_click_color"] if o == 0 else pal[o] for o in c["click_objs"]])
    cubes_all = np.concatenate([c["click_points"], cube_col], 1).astype(np.float32)
    for j, step in enumerate(meta["steps"]):
        lq = c[f"step{j}_logits"].argmax(1).astype(np.int32)
        for o, rows in step["click_idx"].items():
            lq[rows] = int(o)
        # without cubes: what the reference's get_next_click / get_colors produced
        lab, col, err = session_paint(lq, c["inverse_map"], xyz32, col32, pal, [], 0.1)
        assert err == 0
        assert np.array_equal(lab, c[f"step{j}_mask"])
        assert np.array_equal(col, c[f"step{j}_colors"])
        # with the cubes of the clicks so far (gui.py:276-298,327 in numpy, fp32)
        cubes = cubes_all[:step["num_clicks"]]
        lab, col, err = session_paint(lq, c["inverse_map"], xyz32, col32, pal, cubes, 0.1)
        want_lab, want_col = paint_numpy(lq, c["inverse_map"], xyz32, col32, pal, cubes, 0.1)
        assert err == 0 and np.array_equal(lab, want_lab) and np.array_equal(col, want_col)
        assert (col != c[f"step{j}_colors"]).any()                     # the cubes changed something
    # a short palette wraps, overlapping cubes: the later one wins
    lq = (np.arange(len(c["unique_map"])) % 7).astype(np.int32)
    cubes = np.array([[*xyz32[5], 1, 0, 0], [*(xyz32[5] + np.float32(0.05)), 0, 1, 0]], np.float32)
    lab, col, err = session_paint(lq, c["inverse_map"], xyz32, col32, pal[:4], cubes, 0.15)
    want_lab, want_col = paint_numpy(lq, c["inverse_map"], xyz32, col32, pal[:4], cubes, 0.15)
    assert err == 0 and np.array_equal(lab, want_lab) and np.array_equal(col, want_col)
    assert tuple(col[5]) == (0.0, 1.0, 0.0)
    # an inverse map that points outside the voxels is reported, not followed
    bad = c["inverse_map"].copy()
    bad[3] = len(c["unique_map"])
    assert session_paint(lq, bad, xyz32, col32, pal, [], 0.1)[2] & 1


# ---------------------------------------------------------------------------------------------------- 4..7
@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


@pytest.fixture(scope="module")
def model_005():
    return session_kit.model_005()


def _synthetic_full(n_target, seed):
    """A ~n_target-voxel synthetic scene at full resolution: every voxel's point plus a second vertex 4 mm beside it."""
    sc = make_scene(n_target, seed=seed, voxel_size=0.02)
    rng = np.random.default_rng(seed)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def _script(xyz, lab, seed, n_clicks=14):
    """(point, object) clicks over 4 objects and background: points a few millimetres off vertices of distinct instances."""
    rng = np.random.default_rng(seed)
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:4]
    pattern = [1, 2, 0, 1, 3, 2, 0, 3, 4, 1, 2, 0, 4, 3][:n_clicks]
    out = []
    for o in pattern:
        v = rng.choice(np.flatnonzero(lab == (inst[o - 1] if o else 0)))
        out.append(((xyz[v] + rng.normal(0, 0.003, 3)).astype(np.float32), o))
    return out


def test_session_equals_public_path(model_002):
    from agile3d_amd.session import InteractiveSession
    xyz, col, lab = _synthetic_full(20_000, seed=2)
    ses = InteractiveSession(model_002, voxel_size=0.02)
    ses.load_scene(xyz, col, lab, name="synthetic")
    assert ses.raw_coords_qv.shape[0] >= 20_000             # 21 515 voxels (2 x 19 814 vertices)
    script = _script(xyz, lab, seed=9)
    assert len(script) >= 12 and len({o for _, o in script}) >= 4
    ci, ct, n = {"0": []}, {"0": []}, 0
    checked = 0
    for point, obj in script:
        row_qv, row_full = ses.click(point, obj)
        ci.setdefault(str(obj), []).append(row_qv)
        ct.setdefault(str(obj), []).append(n)
        n += 1
        assert ses.click_idx == ci and ses.click_time_idx == ct
        if len(ci) < 2:
            continue
        res = ses.infer()
        # by hand, on the public API, with the same click dictionaries
        out = model_002.forward_mask(*ses._backbone, click_idx=[copy.deepcopy(ci)], click_time_idx=[copy.deepcopy(ct)])
        pred_qv = K.argmax_labels(out["pred_masks"][0], ci)
        want = pred_qv[ses.inverse_map]
        assert res.labels_full.dtype == torch.int32 and torch.equal(res.labels_full, want)
        miou, per_obj = K.mean_iou_scene(pred_qv, ses.new_labels, ses.inverse_map)
        assert res.miou == miou.item() and res.iou_per_object == per_obj
        assert res.num_obj == len(ci) - 1 and res.avg_clicks == round(n / (len(ci) - 1), 1)
        # colours: palette of the label, the vertex's own colour on background
        lf = res.labels_full.long()
        pal = torch.from_numpy(ses.palette).to(DEV)
        assert torch.equal(res.colors, torch.where((lf > 0)[:, None], pal[lf], ses.colors_full))
        checked += 1
    assert checked >= 12
    # the relabelled ground truth: object k = the instance under its first click
    want_nl = np.zeros(len(lab), np.int32)
    qv_lab = ses.labels_qv_ori.cpu().numpy()
    for k in range(1, 5):
        want_nl[lab == qv_lab[ci[str(k)][0]]] = k
    assert np.array_equal(ses.new_labels.cpu().numpy(), want_nl) and len(np.unique(want_nl)) >= 4
    # the scene's first-layer cache served the passes (every call got the SAME pcd_features object)
    from agile3d_amd.engine import _kv_cache_mb
    if _kv_cache_mb() > 0:
        assert ses._backbone[0]._a3d.kv0 is not None and ses._backbone[0]._a3d.mask_calls >= 24


@pytest.mark.parametrize("name", CASES)
def test_reference_bookkeeping_and_files(name, model_005, tmp_path):
    """Replays the fixture's scripted clicks through click() and feeds the recorded logits through infer(logits=).
    (The model call itself is test_session_equals_public_path's.)

    What is compared, and where it comes from.  REFERENCE-RUN: the voxel row and the vertex of every click (the
    reference's ``find_nearest``), and everything ``get_next_click`` produced from the recorded logits -- labels
    (``object_mask``), colours (its ``get_colors``), the IoU (``mean_iou_scene``), the record line, the names and contents
    of the mask and click files.  THE GENERATOR'S STATEMENT OF THE RULE, not a run of the reference: the click
    dictionaries, ``click_positions`` and the relabelled ground truth between the model calls.  That state is kept by
    the GUI's event handler (gui.py:290-331), which needs a window; make_session_goldens.py keeps it by the rule the
    handler states, so for these three the test pins the session to a second, independent writing of the same rule
    (the click files' dictionaries went THROUGH the reference's ``np.save`` but were built by the generator)."""
    from agile3d_amd.session import InteractiveSession
    c, meta = load_session_case(name)
    clock = datetime.fromisoformat(meta["clock"])
    ses = InteractiveSession(model_005, voxel_size=meta["voxel_size"], palette=c["palette"], clock=lambda: clock,
                             background_click_color=c["background_click_color"])
    ses.load_scene(c["coords_full"], c["colors_full"], c["labels_full"], name=meta["name"], out_dir=str(tmp_path))
    assert torch.equal(ses.inverse_map.cpu(), torch.from_numpy(c["inverse_map"]))
    steps = {s["num_clicks"]: (j, s) for j, s in enumerate(meta["steps"])}
    for i, (p, o) in enumerate(zip(c["click_points"], c["click_objs"])):
        row_qv, row_full = ses.click(p, int(o))
        assert (row_qv, row_full) == (int(c["click_rows_qv"][i]), int(c["click_rows_full"][i]))
        if i + 1 not in steps:
            continue
        j, step = steps[i + 1]
        assert ses.click_idx == step["click_idx"] and ses.click_time_idx == step["click_time"]
        assert np.array_equal(ses.new_labels.cpu().numpy(), c[f"step{j}_new_labels"])
        res = ses.infer(logits=torch.from_numpy(c[f"step{j}_logits"]).to(DEV))
        assert np.array_equal(res.labels_full.cpu().numpy(), c[f"step{j}_mask"])
        assert np.array_equal(res.colors.cpu().numpy(), c[f"step{j}_colors"])
        assert np.float32(res.miou) == c[f"step{j}_miou"]
        assert res.record == meta["record"][j]
        assert os.path.basename(res.mask_path) == step["mask_file"] and os.path.basename(res.click_path) == step["click_file"]
        mask = np.load(res.mask_path)
        assert mask.dtype == np.int64 and np.array_equal(mask, c[f"step{j}_mask"])
        saved = np.load(res.click_path, allow_pickle=True).item()
        assert saved == {"click_idx": step["click_idx"], "click_time": step["click_time"]}
    assert ses.click_idx == meta["click_idx"] and ses.click_time_idx == meta["click_time_idx"]
    assert ses.click_positions == meta["click_positions"]
    assert np.array_equal(ses.new_labels.cpu().numpy(), c["new_labels"])
    with open(os.path.join(str(tmp_path), "iou_record.csv")) as f:
        assert f.readlines() == meta["record"]


def test_load_scene_dir_equals_load_scene(model_002, tmp_path):
    """``load_scene_dir`` on the InteractiveDataLoader layout -- a point-cloud ``scan.ply`` without labels and a
    triangle-mesh ``scan.ply`` with a ``label.ply`` -- gives the state ``load_scene`` gives on the same arrays."""
    from agile3d_amd.ply import is_triangular_mesh, write_ply
    from agile3d_amd.session import InteractiveSession
    xyz, col, lab = _synthetic_full(3_000, seed=12)
    rgb = np.round(col * 255).astype(np.uint8)
    faces = np.random.default_rng(0).integers(0, len(xyz), (500, 3)).astype(np.int32)
    cloud, mesh = tmp_path / "scene_0042_cloud", tmp_path / "scene_mesh_a"
    for d in (cloud, mesh):
        os.makedirs(d)
    assert write_ply(str(cloud / "scan.ply"), [xyz, rgb], ["x", "y", "z", "red", "green", "blue"])
    assert write_ply(str(mesh / "scan.ply"), [xyz, rgb], ["x", "y", "z", "red", "green", "blue"], triangular_faces=faces)
    assert write_ply(str(mesh / "label.ply"), [xyz, lab], ["x", "y", "z", "label"])
    assert not is_triangular_mesh(str(cloud / "scan.ply")) and is_triangular_mesh(str(mesh / "scan.ply"))
    want = InteractiveSession(model_002, voxel_size=0.02)
    for folder, labels, name in ((cloud, None, "0042_cloud"), (mesh, lab, "mesh_a")):
        out = str(tmp_path / ("out_" + name))
        ses = InteractiveSession(model_002, voxel_size=0.02)
        ses.load_scene_dir(str(folder), out_dir=out)
        want.load_scene(xyz.astype(np.float64), rgb.astype(np.float64) / 255.0, labels, name=name)
        assert ses.scene_name == name == want.scene_name and ses.out_dir == out
        assert os.path.isdir(os.path.join(out, "masks")) and os.path.isdir(os.path.join(out, "clicks"))
        assert torch.equal(ses.coords_full, want.coords_full) and torch.equal(ses.coords_full.cpu(), torch.from_numpy(xyz))
        assert torch.equal(ses.colors_full, want.colors_full)
        assert torch.equal(ses.colors_full.cpu(), torch.from_numpy((rgb.astype(np.float64) / 255.0).astype(np.float32)))
        assert torch.equal(ses.inverse_map, want.inverse_map) and torch.equal(ses.raw_coords_qv, want.raw_coords_qv)
        if labels is None:
            assert ses.labels_full_ori is None and ses.new_labels is None
        else:
            assert torch.equal(ses.labels_full_ori.cpu(), torch.from_numpy(lab)) and torch.equal(ses.labels_qv_ori, want.labels_qv_ori)
        # and the scene works: one click, one inference, the files land under out_dir
        ses.click(xyz[0], 1)
        res = ses.infer()
        assert (res.miou is None) == (labels is None) and os.path.exists(res.mask_path) and os.path.exists(res.click_path)
        assert os.path.exists(os.path.join(out, "iou_record.csv"))


def _run_script(ses, script):
    outs = []
    for point, obj in script:
        rows = ses.click(point, obj)
        if len(ses.click_idx) < 2:
            continue
        res = ses.infer(paint_cubes=True)
        outs.append((rows, res.labels_full.clone(), res.colors.clone(), res.miou))
    return outs, copy.deepcopy((ses.click_idx, ses.click_time_idx, ses.click_positions)), ses.new_labels.clone()


def _same(a, b):
    assert a[1] == b[1] and torch.equal(a[2], b[2]) and len(a[0]) == len(b[0])
    for x, y in zip(a[0], b[0]):
        assert x[0] == y[0] and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3]


def test_determinism_reset_and_scene_hygiene(model_002):
    from agile3d_amd.session import InteractiveSession
    xa, ca, la = _synthetic_full(6_000, seed=5)
    xb, cb, lb = _synthetic_full(5_000, seed=6)
    sb = _script(xb, lb, seed=1, n_clicks=8)
    ses = InteractiveSession(model_002, voxel_size=0.02)
    ses.load_scene(xb, cb, lb)
    first = _run_script(ses, sb)
    ses.reset()
    assert ses.num_clicks == 0 and ses.click_idx == {"0": []} and int(ses.new_labels.abs().sum()) == 0
    again = _run_script(ses, sb)
    _same(first, again)                                   # reset(), then the same script
    fresh = InteractiveSession(model_002, voxel_size=0.02)
    fresh.load_scene(xb, cb, lb)
    _same(first, _run_script(fresh, sb))                  # the same script twice
    # scene B after scene A (with clicks and an inference on A) == scene B alone
    ses.load_scene(xa, ca, la)
    _run_script(ses, _script(xa, la, seed=2, n_clicks=6))
    ses.load_scene(xb, cb, lb)
    assert ses.num_clicks == 0 and ses.click_idx == {"0": []} and ses.new_labels.shape[0] == len(xb)
    lab0, col0 = ses.preview()
    assert int(lab0.abs().sum()) == 0 and torch.equal(col0, ses.colors_full)      # nothing of A's labels or cubes
    _same(first, _run_script(ses, sb))


def test_refusals(model_002):
    from agile3d_amd.session import InteractiveSession
    xyz, col, lab = _synthetic_full(3_000, seed=8)
    ses = InteractiveSession(model_002, voxel_size=0.02)
    with pytest.raises(RuntimeError):
        ses.click(xyz[0], 1)                              # no scene yet
    ses.load_scene(xyz, col, lab)
    hi = xyz.max(0)
    assert ses.pick(hi + 1.0, [0.0, 0.0, 1.0]) is None   # a ray that leaves the scene behind: "clicked on nothing"
    top = xyz[np.argmax(xyz[:, 2])]
    hit = ses.pick(top + np.array([0, 0, 2.0], np.float32), [0.0, 0.0, -3.0])    # (the direction is normalised)
    assert hit is not None and np.allclose(hit[:2], top[:2], atol=0.02)
    with pytest.raises(ValueError):
        ses.infer()                                       # no click: the reference returns early, here it is an error
    with pytest.raises(ValueError):
        ses.click(xyz[0], 2)                              # object 2 before object 1: a gap
    ses.click(xyz[0], 0)
    with pytest.raises(ValueError):
        ses.infer()                                       # only background clicks: no object to segment
    ses.click(xyz[1], 1)
    with pytest.raises(ValueError):
        ses.click(xyz[2], 3)
    assert ses.infer().num_obj == 1
    with pytest.raises(ValueError):
        ses.pick([0, 0, 0], [0, 0, 0])
    # more queries than the decoder serves
    n_max = L.A3D_MAX_QUERIES - model_002.num_bg_queries
    ses.num_clicks = n_max                                # (as if n_max clicks had been made)
    with pytest.raises(ValueError):
        ses.click(xyz[3], 1)
    model_002.train()
    try:
        with pytest.raises(ValueError):
            InteractiveSession(model_002, voxel_size=0.02)   # a training-mode model
    finally:
        model_002.eval()
