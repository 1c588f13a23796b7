"""-m gpu: editing the session's clicks (a3d_session_edit in csrc/session_edit.hip; view.session_edit; InteractiveSession.undo,
redo, remove_click, restore_clicks, restore_file, click_at).  The rules are restated in ``edit_rule.py``.

1  the kernel, bit for bit against the restatement, outputs pre-filled with a sentinel: sizes around the workgroup and beyond
   one pass of the grid, 0 / 1 / 2 / 255 objects, instance ids 0, -1 and 2^31 - 1, one instance under two objects, labels
   nobody claims; the remap with identity, shift and all-zero tables, n = 0, the values -1 and 256; either half alone
2  the library's own refusals
3  the session on a ~5 k-voxel synthetic scene: undo == a fresh replay without the last click, redo == the state before,
   remove_click of an object's only click == a fresh replay of the survivors under their new ids, restore_file == the
   session that wrote the file, click_at == the marker annotate draws on top
"""
import copy

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.synthetic import make_scene
from annotate_rule import annotate_rule, marker_cover
from edit_rule import list_truth, relabel_numpy, remap_numpy, removal_lut
from pick_rule import fp32_rule_argmin, paint_numpy
from session_kit import DEV, _dev, _model, byref, status

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 4099, 300_001)        # 300 001 > 1024 workgroups x 256 rows: a second pass
SPECIAL = (0, -1, 2 ** 31 - 1)
SENTINEL = -77
INVALID, OK = -1, 0                                                 # A3D_ERR_INVALID, A3D_OK (include/agile3d_hip.h)


# ---------------------------------------------------------------------------------------------------- 1
def edit_gpu(labels_ori=None, instances=None, labels=None, lut=None):
    """view.session_edit, numpy in / numpy out: (new_labels or None, remapped labels or None, flag or None)."""
    new = err = lab = None
    kw = {}
    if labels_ori is not None:
        new = torch.full((len(labels_ori),), SENTINEL, dtype=torch.int32, device=DEV)
        kw.update(labels_ori=_dev(labels_ori, np.int32), new_labels=new,
                  instances=_dev(instances, np.int32) if len(instances) else None)
    if labels is not None:
        lab, err = _dev(labels, np.int32), torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
        kw.update(labels=lab, lut=lut, err=err)
    got = V.session_edit(**kw)
    assert got[0] is new and got[1] is lab and got[2] is err
    return (None if new is None else new.cpu().numpy(), None if lab is None else lab.cpu().numpy(),
            None if err is None else int(err.cpu()[0]))


def _instances(n_objects, rng):
    """``n_objects`` instance ids: the special values first, random ids after them, and -- from two objects on -- object
    ``n_objects`` standing for the instance of object 1 as well (the higher id must win); plus ids no object claims."""
    pool = np.array(list(SPECIAL) + rng.choice(np.arange(1, 5000), 300, replace=False).tolist(), np.int64)
    inst = pool[:n_objects].copy()
    if n_objects >= 2:
        inst[-1] = inst[0]
    if n_objects >= 8:
        inst[5] = inst[2]
    unclaimed = np.concatenate([pool[n_objects:n_objects + 20], [-2, 2 ** 31 - 2, -2 ** 31, 5001]])
    return inst.astype(np.int32), unclaimed.astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_relabel_against_the_rule(n):
    rng = np.random.default_rng(n)
    for n_objects in (0, 1, 2, 255):
        inst, unclaimed = _instances(n_objects, rng)
        values = np.concatenate([inst, unclaimed])
        labels_ori = values[rng.integers(0, len(values), n)]
        labels_ori[-1] = values[0]                                             # the last row is claimed (by object 1, or by its rival)
        if n > len(values):
            labels_ori[rng.permutation(n - 1)[:len(values)]] = values          # every value appears
        want = relabel_numpy(labels_ori, inst)
        got, _, _ = edit_gpu(labels_ori, inst)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, n_objects)
        if n > len(values):
            assert set(np.unique(want)) == set(range(n_objects + 1)) - ({1} if n_objects >= 2 else set()) - ({3} if n_objects >= 8 else set())
            assert (want[np.isin(labels_ori, unclaimed)] == 0).all()
            if n_objects >= 2:
                assert (want[labels_ori == inst[0]] == n_objects).all()        # the same instance under two objects
        # both halves in one call give what each gives alone
        labels = rng.integers(0, 256, max(n // 3, 1)).astype(np.int32)
        lut = removal_lut(7)
        both = edit_gpu(labels_ori, inst, labels, lut)
        assert np.array_equal(both[0], want) and np.array_equal(both[1], remap_numpy(labels, lut)[0]) and both[2] == 0


@pytest.mark.parametrize("n", SIZES)
def test_remap_against_the_rule(n):
    rng = np.random.default_rng(n + 1)
    labels = rng.integers(0, 256, n).astype(np.int32)
    labels[0] = 255
    for lut in (removal_lut(None), removal_lut(1), removal_lut(40), removal_lut(255), np.zeros(256, np.uint8),
                rng.integers(0, 256, 256).astype(np.uint8)):
        want, flag = remap_numpy(labels, lut)
        _, got, err = edit_gpu(labels=labels, lut=lut)                         # the remap half alone
        assert flag == 0 and err == 0 and got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(edit_gpu(labels=labels, lut=removal_lut(None))[1], labels)
    # values outside 0 .. 255 flag and become 0 -- at the last row, the first, and every other one
    for where in ([n - 1], [0], list(range(0, n, 2))):
        bad = labels.copy()
        bad[where] = np.where(np.arange(len(where)) % 2 == 0, -1, 256)
        want, flag = remap_numpy(bad, removal_lut(3))
        _, got, err = edit_gpu(labels=bad, lut=removal_lut(3))
        assert flag == 1 and err != 0 and np.array_equal(got, want) and (got[where] == 0).all()
    for extreme in (-2 ** 31, 2 ** 31 - 1):
        bad = labels.copy()
        bad[n // 2] = extreme
        _, got, err = edit_gpu(labels=bad, lut=removal_lut(None))
        assert err != 0 and got[n // 2] == 0 and np.array_equal(np.delete(got, n // 2), np.delete(labels, n // 2))


def test_empty_inputs_and_wrapper_refusals():
    empty = np.zeros(0, np.int32)
    got = edit_gpu(empty, np.array([3, 4], np.int32), empty, removal_lut(2))   # n = 0: nothing launched, the flag cleared
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2] == 0
    assert edit_gpu(labels=empty, lut=removal_lut(None))[2] == 0
    assert edit_gpu(np.array([5, 6], np.int32), empty)[0].tolist() == [0, 0]   # no object: all background
    ori, lab = _dev([1, 2, 3], np.int32), _dev([1, 2], np.int32)
    for bad in (dict(), dict(instances=ori), dict(lut=removal_lut(None)), dict(labels_ori=ori, lut=removal_lut(None)),
                dict(labels=lab), dict(labels=lab, lut=np.arange(255)), dict(labels=lab, lut=np.arange(256) + 1),
                dict(labels=lab, lut=np.arange(256.0)), dict(labels=lab.long(), lut=removal_lut(None)),
                dict(labels_ori=ori, instances=ori.long()), dict(labels_ori=ori, new_labels=lab),
                dict(labels_ori=ori.cpu()), dict(labels_ori=ori, instances=torch.zeros(256, dtype=torch.int32, device=DEV)),
                dict(labels=lab, lut=removal_lut(None), err=torch.zeros(2, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            V.session_edit(**bad)


# ---------------------------------------------------------------------------------------------------- 2
def test_library_refusals():
    ori, new, inst = _dev([1, 2, 3], np.int32), torch.full((3,), SENTINEL, dtype=torch.int32, device=DEV), _dev([2], np.int32)
    lab, err = _dev([1, 2], np.int32), torch.zeros(1, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = L.SessionEditArgs()
        for k, v in kw.items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        return status("a3d_session_edit", byref(a), None)

    good = dict(labels_ori_dev=ori, instances_dev=inst, new_labels_dev=new, n_full=3, n_objects=1)
    remap = dict(labels_dev=lab, n_labels=2, err_dev=err)
    assert status("a3d_session_edit", None, None) == INVALID
    for bad in (dict(good, n_full=-1), dict(good, n_objects=-1), dict(good, n_objects=256), dict(good, new_labels_dev=None),
                dict(good, labels_ori_dev=None), dict(good, instances_dev=None), dict(remap, n_labels=-1),
                dict(remap, labels_dev=None), dict(remap, err_dev=None), dict(good, **dict(remap, err_dev=None))):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert new.cpu().tolist() == [SENTINEL] * 3 and lab.cpu().tolist() == [1, 2]          # nothing was launched
    assert call() == OK and call(**dict(good, n_full=0, new_labels_dev=None)) == OK
    assert call(**good) == OK and new.cpu().tolist() == [0, 1, 0]


# ---------------------------------------------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def model_002():
    return _model(0.02)


@pytest.fixture(scope="module")
def scene():
    """A ~5 k-voxel synthetic scene at full resolution (as test_gpu_session.py builds its scenes): every voxel's point
    plus a second vertex 4 mm beside it, shuffled."""
    sc = make_scene(5_000, seed=6, voxel_size=0.02)
    rng = np.random.default_rng(6)
    raw = sc["raw_xyz"]
    xyz = np.concatenate([raw, raw + rng.uniform(-0.004, 0.004, raw.shape).astype(np.float32)]).astype(np.float32)
    col = np.concatenate([sc["feats"], sc["feats"]]).astype(np.float32)
    lab = np.concatenate([sc["labels"], sc["labels"]]).astype(np.int32)
    p = rng.permutation(len(xyz))
    return xyz[p], col[p], lab[p]


def _script(xyz, lab, pattern, seed=1):
    """(point, object) clicks: points a few millimetres off vertices of four distinct instances / of the background."""
    rng = np.random.default_rng(seed)
    inst = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() > 50][:4]
    assert len(inst) == 4
    out = []
    for o in pattern:
        v = rng.choice(np.flatnonzero(lab == (inst[o - 1] if o else 0)))
        out.append(((xyz[v] + rng.normal(0, 0.003, 3)).astype(np.float32), o))
    return out


def _session(model, scene, labels=True, **kw):
    from agile3d_amd.session import InteractiveSession
    ses = InteractiveSession(model, voxel_size=0.02)
    ses.load_scene(scene[0], scene[1], scene[2] if labels else None, **kw)
    return ses


def _state(ses):
    torch.cuda.synchronize()
    return dict(dicts=copy.deepcopy((ses.click_idx, ses.click_time_idx, ses.click_positions)),
                keys=[list(d) for d in (ses.click_idx, ses.click_time_idx, ses.click_positions)], n=ses.num_clicks,
                clicks=ses.clicks(), cubes=ses._cubes.copy(), cubes_dev=ses._cubes_dev.cpu().numpy(),
                new_labels=None if ses.new_labels is None else ses.new_labels.cpu().numpy())


def _same_state(a, b):
    assert a["dicts"] == b["dicts"] and a["keys"] == b["keys"] and a["n"] == b["n"] and a["clicks"] == b["clicks"]
    assert np.array_equal(a["cubes"], b["cubes"]) and np.array_equal(a["cubes_dev"], b["cubes_dev"])
    assert np.array_equal(a["cubes"], a["cubes_dev"]) and np.array_equal(a["new_labels"], b["new_labels"])


def _same_inference(a, b):
    ra, rb = a.infer(), b.infer()
    assert torch.equal(ra.labels_full, rb.labels_full) and torch.equal(ra.colors, rb.colors) and ra.miou == rb.miou
    assert ra.iou_per_object == rb.iou_per_object and ra.num_obj == rb.num_obj
    return ra


def _truth(ses, scene):
    pairs = [(c["obj"], c["row_qv"]) for c in ses.clicks()]
    return list_truth(pairs, ses.labels_qv_ori.cpu().numpy(), scene[2])


def test_undo_and_redo_equal_fresh_replays(model_002, scene):
    script = _script(*scene[::2], pattern=[1, 2, 0, 1, 3, 2, 0, 3, 4, 1])
    ses = _session(model_002, scene)
    assert 4_000 <= ses.raw_coords_qv.shape[0] <= 7_000
    assert ses.undo() is None and ses.redo() is None and ses.num_clicks == 0            # nothing to take back
    for i, (p, o) in enumerate(script):
        ses.click(p, o)
        if i == 5:
            ses.infer()
    full = _state(ses)
    assert np.array_equal(full["new_labels"], _truth(ses, scene)) and len(np.unique(full["new_labels"])) == 5
    fresh = {}
    for n in (8, 9, 10):
        fresh[n] = _session(model_002, scene)
        for p, o in script[:n]:
            fresh[n].click(p, o)
    _same_state(full, _state(fresh[10]))
    # undo: the 10th click, one of three of object 1
    removed = ses.undo()
    assert removed == dict(full["clicks"][9], id_map={1: 1, 2: 2, 3: 3, 4: 4}) and removed["index"] == 9 and removed["obj"] == 1
    nine = _state(ses)
    _same_state(nine, _state(fresh[9]))
    assert np.array_equal(nine["new_labels"], _truth(ses, scene)) and not nine["cubes"][9:].any()
    _same_inference(ses, fresh[9])
    # redo: the state before the undo
    assert ses.redo() == full["clicks"][9] and ses.redo() is None
    _same_state(_state(ses), full)
    _same_inference(ses, fresh[10])
    # two undos: the second takes object 4's only click, and object 4 with it
    qv10 = ses._labels_qv.cpu().numpy()
    assert (qv10 == 4).any()
    ses.undo()
    removed = ses.undo()
    assert removed["obj"] == 4 and removed["index"] == 8 and removed["id_map"] == {1: 1, 2: 2, 3: 3, 4: 0}
    _same_state(_state(ses), _state(fresh[8]))
    assert "4" not in ses.click_idx and not (ses.new_labels == 4).any()
    assert np.array_equal(ses._labels_qv.cpu().numpy(), np.where(qv10 == 4, 0, qv10))
    assert np.array_equal(ses._labels_last.cpu().numpy(), np.where(qv10 == 4, 0, qv10)[ses.inverse_map.cpu().numpy()])
    # ... and two redos bring it back under its id -- without its voxels, until the next inference
    assert ses.redo()["obj"] == 4
    _same_state(_state(ses), nine)
    assert not (ses._labels_qv == 4).any()
    assert ses.redo()["index"] == 9
    _same_state(_state(ses), full)
    _same_inference(ses, fresh[10])
    # a click after an undo: nothing to redo
    ses.undo()
    ses.click(*script[9])
    assert ses.redo() is None
    _same_state(_state(ses), full)
    for edit in (lambda: ses.reset(), lambda: ses.remove_click(0), lambda: ses.restore_clicks({"0": [3]}, {"0": [0]}),
                 lambda: ses.load_scene(*scene)):
        ses.reset()
        ses.click(*script[0])
        ses.click(*script[1])
        assert ses.undo()["index"] == 1
        edit()
        assert ses.redo() is None                                                       # they empty the stack as well


def test_remove_an_objects_only_click(model_002, scene):
    xyz, col, lab = scene
    script = _script(xyz, lab, pattern=[1, 2, 0, 1, 3, 3, 0, 4, 4, 1], seed=2)
    ses = _session(model_002, scene)
    for p, o in script:
        ses.click(p, o)
    ses.infer()
    old_qv = ses._labels_qv.cpu().numpy()
    assert set(np.unique(old_qv)) >= {1, 2, 3, 4}
    for bad in (-1, 10):
        with pytest.raises(IndexError):
            ses.remove_click(bad)
    removed = ses.remove_click(1)                                                       # object 2's only click; 3 and 4 lie above
    lut = removal_lut(2)
    assert removed["obj"] == 2 and removed["index"] == 1 and removed["id_map"] == {1: 1, 2: 0, 3: 2, 4: 3}
    assert np.array_equal(np.float32(removed["point"]), script[1][0]) and ses.redo() is None
    fresh = _session(model_002, scene)
    for p, o in script[:1] + script[2:]:
        fresh.click(p, int(lut[o]))
    _same_state(_state(ses), _state(fresh))
    assert ses.click_idx.keys() == {"0", "1", "2", "3"} and ses.click_time_idx["1"] == [0, 2, 8]
    assert np.array_equal(ses.new_labels.cpu().numpy(), _truth(ses, scene))
    # what the view shows: the last inference renumbered, the removed object's voxels background, the surviving cubes
    want_lab, want_col = paint_numpy(lut[old_qv].astype(np.int32), ses.inverse_map.cpu().numpy(), xyz, col, ses.palette,
                                     ses._cubes[:9], ses.cube_size)
    assert np.array_equal(ses._labels_last.cpu().numpy(), want_lab) and np.array_equal(ses._colors_last.cpu().numpy(), want_col)
    got_lab, got_col = ses.preview()
    assert np.array_equal(got_lab.cpu().numpy(), want_lab) and np.array_equal(got_col.cpu().numpy(), want_col)
    assert (old_qv == 2).sum() > 0 and (want_lab == 3).any() and not (want_lab == 4).any()
    _same_inference(ses, fresh)
    # the earliest click of an object that keeps a later one: ids stay, the instance follows the later click
    ses.reset()
    for p, o in script:
        ses.click(p, o)
    removed = ses.remove_click(4)                                                       # object 3: clicks 4 and 5
    assert removed["id_map"] == {1: 1, 2: 2, 3: 3, 4: 4} and ses.click_time_idx["3"] == [4]
    assert np.array_equal(ses.new_labels.cpu().numpy(), _truth(ses, scene))
    # ... also when the later click lies on another instance and behind a higher object's first click: (1), (2), (3), (2)
    ses.reset()
    for (p, _), o in zip((script[0], script[1], script[4], script[7]), (1, 2, 3, 2)):
        ses.click(p, o)
    first = ses.new_labels.cpu().numpy()
    qv_lab = ses.labels_qv_ori.cpu().numpy()
    a, b = (int(qv_lab[c["row_qv"]]) for c in ses.clicks()[1::2])
    assert a != b and (first[lab == a] == 2).all() and (first[lab == b] == 0).all()
    assert ses.remove_click(1)["id_map"] == {1: 1, 2: 2, 3: 3} and list(ses.click_idx) == ["0", "1", "3", "2"]
    moved = ses.new_labels.cpu().numpy()
    assert np.array_equal(moved, _truth(ses, scene)) and (moved[lab == a] == 0).all() and (moved[lab == b] == 2).all()
    assert ses.infer().num_obj == 3


def test_restore_file_and_restore_clicks(model_002, scene, tmp_path):
    xyz, col, lab = scene
    script = _script(xyz, lab, pattern=[1, 2, 0, 1, 3, 2, 0, 3, 4, 1], seed=3)
    ses = _session(model_002, scene, out_dir=str(tmp_path))
    for p, o in script:
        ses.click(p, o)
    res = ses.infer()
    other = _session(model_002, scene)
    other.click(xyz[0], 1)                                                              # (restore starts from reset())
    assert other.restore_file(res.click_path) is other
    assert other.click_idx == ses.click_idx and other.click_time_idx == ses.click_time_idx and other.num_clicks == 10
    assert torch.equal(other.new_labels, ses.new_labels)
    qv = ses.raw_coords_qv.cpu().numpy()
    for c in other.clicks():                                                            # a file keeps rows, not points
        assert np.array_equal(np.float32(c["point"]), qv[c["row_qv"]]) and c["row_full"] == fp32_rule_argmin(xyz, qv[c["row_qv"]])
        assert c["position"] == xyz[c["row_full"]].tolist()
    assert np.array_equal(other._cubes[:10, :3], qv[[c["row_qv"] for c in other.clicks()]])
    got = other.infer()
    assert torch.equal(got.labels_full, res.labels_full) and torch.equal(got.colors, res.colors) and got.miou == res.miou
    # a refusal leaves the session as it was
    before = _state(other)
    n_qv = len(qv)
    for idx, time in (({"0": [], "2": [1]}, {"0": [], "2": [0]}), ({"0": [1], "1": [2]}, {"0": [0], "1": [2]}),
                      ({"0": [], "1": [n_qv]}, {"0": [], "1": [0]}),
                      ({"0": list(range(300)), "1": [1]}, {"0": list(range(300)), "1": [300]})):
        with pytest.raises(ValueError):
            other.restore_clicks(idx, time)
    with pytest.raises(ValueError):
        np.save(str(tmp_path / "other.npy"), {"clicks": 1})
        other.restore_file(str(tmp_path / "other.npy"))
    _same_state(_state(other), before)
    # more clicks than one nearest-rows launch serves (64), time order unlike dictionary order
    rng = np.random.default_rng(0)
    rows = rng.choice(n_qv, 70, replace=False)
    objs = np.concatenate([[1, 2, 3], rng.integers(0, 4, 67)])
    times = rng.permutation(70)
    idx = {str(k): rows[objs == k].tolist() for k in range(4)}
    time = {str(k): times[objs == k].tolist() for k in range(4)}
    other.restore_clicks(idx, time)
    assert other.click_idx == {k: [r for _, r in sorted(zip(time[k], v))] for k, v in idx.items()} and other.num_clicks == 70
    assert other.click_time_idx == {k: sorted(v) for k, v in time.items()}
    order = np.argsort(times)
    assert [c["row_qv"] for c in other.clicks()] == rows[order].tolist() and [c["obj"] for c in other.clicks()] == objs[order].tolist()
    assert [c["row_full"] for c in other.clicks()] == [fp32_rule_argmin(xyz, qv[r]) for r in rows[order]]
    assert np.array_equal(other.new_labels.cpu().numpy(), _truth(other, scene))
    assert other.infer().num_obj == 3


def test_click_at_names_the_marker_on_top(model_002, scene):
    """A scene without ground truth (the relabel half is then skipped): clicks picked through pixels of a render, so that
    their markers show; ``click_at`` at every marker's centre == the restated cover rule; a removed click's marker is gone."""
    xyz = scene[0]
    ses = _session(model_002, scene, labels=False)
    w, h = 160, 120
    k, e = ses.default_view(w, h)
    res = ses.render(k, e, w, h, radius=0.03)
    ids, t = res.ids.cpu().numpy(), res.t.cpu().numpy()
    assert ses.click_at(res, 5, 5) is None                                              # no click yet
    picked = []                                                                         # pixels that show a vertex, 20 apart or more (the scene fills rows 36 .. 83)
    for v in range(14, h - 14):
        for u in range(14, w - 14):
            if ids[v, u] >= 0 and all(max(abs(u - a), abs(v - b)) >= 20 for a, b in picked):
                picked.append((u, v))
    picked = picked[:10]
    assert len(picked) == 10
    for (u, v), obj in zip(picked, [1, 2, 0, 1, 3, 2, 0, 3, 4, 1]):
        ses.click(ses.pick_from_render(res, u, v), obj)
    assert ses.new_labels is None

    def want_image():
        cubes = ses._cubes[:ses.num_clicks]
        rows, kept = V.marker_table(res.camera, cubes[:, :3], cubes[:, 3:], return_kept=True)
        label = np.where(ids >= 0, 0, -1)                                               # no inference: all background
        return rows, kept, annotate_rule(res.rgb.cpu().numpy(), label, t, rows, 6.0, 4.5, ses.cube_size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))

    rows, kept, want = want_image()
    shown = ses.annotate(res).cpu().numpy()
    assert len(rows) == 10 and kept.tolist() == list(range(10)) and np.array_equal(shown, want)
    top, _ = marker_cover(t, rows, 6.0, 6.0, ses.cube_size)
    own = 0
    pixels = [(int(round(float(x))), int(round(float(y)))) for x, y in rows[:, :2]]      # the markers' centre pixels
    for i, (u, v) in enumerate(pixels):
        assert 0 <= u < w and 0 <= v < h and max(abs(u - picked[i][0]), abs(v - picked[i][1])) < 7    # (the vertex lies within 3 cm of the
        #                                                                                 picked pixel's ray, not on it: centres stay >= 8 apart) 
        assert ses.click_at(res, u, v) == (None if top[v, u] < 0 else int(kept[top[v, u]]))
        own += ses.click_at(res, u, v) == i
    assert own >= 5
    for u, v in ((0, 0), (w - 1, h - 1), (pixels[0][0] + 6, pixels[0][1]), (pixels[0][0] + 7, pixels[0][1])):
        assert ses.click_at(res, u, v) == (None if top[v, u] < 0 else int(kept[top[v, u]]))
    small, _ = marker_cover(t, rows, 2.0, 2.0, 0.0)
    u, v = pixels[4]
    assert ses.click_at(res, u + 3, v, marker_px=2.0, depth_slack=0.0) == (None if small[v, u + 3] < 0 else int(kept[small[v, u + 3]]))
    for bad in (dict(u=w, v=0), dict(u=0, v=-1), dict(u=0, v=0, marker_px=-1.0), dict(u=0, v=0, depth_slack=float("nan"))):
        with pytest.raises(ValueError):
            ses.click_at(res, **bad)
    # the viewer's "delete the click under the pointer"
    victim = next(i for i, (u, v) in enumerate(pixels) if ses.click_at(res, u, v) == i and i not in (0, 9))
    u, v = pixels[victim]
    removed = ses.remove_click(ses.click_at(res, u, v))
    assert removed["index"] == victim and ses.num_clicks == 9
    rows, kept, want = want_image()
    after = ses.annotate(res).cpu().numpy()
    assert len(rows) == 9 and np.array_equal(after, want)
    assert ses.click_at(res, u, v) is None and (after[v, u] != shown[v, u]).any()       # the marker is gone
    assert np.array_equal(after[v, u], ses.annotate(res, markers=False).cpu().numpy()[v, u])
    assert ses.undo()["index"] == 8 and ses.redo()["index"] == 8 and ses.num_clicks == 9
