"""CPU: the rules behind the session's editable click list -- ``click_state``, ``remove_from_clicks``, ``instance_rows``,
``restore_lut``, ``clicks_from_dicts`` (what ``restore_clicks`` refuses) and ``marker_hit`` (what ``click_at`` answers) --
pure functions of ``agile3d_amd/session.py``, held to ``edit_rule.py`` and ``annotate_rule.py``.  No library, no GPU."""
import numpy as np
import pytest

from agile3d_amd import lib as L
from agile3d_amd import view as V
from agile3d_amd.session import (camera_from_matrices, click_state, clicks_from_dicts, instance_rows, marker_hit,
                                 remove_from_clicks, restore_lut)
from annotate_rule import marker_cover
from edit_rule import list_truth, relabel_numpy, remap_numpy, removal_lut
from session_kit import intrinsic, load_session_case, look_at


def _click(obj, row, full=None):
    full = row + 1000 if full is None else full
    return {"obj": obj, "point": (0.5 * row, 1.0, -2.0), "row_qv": row, "row_full": full, "position": [float(full), 0.25, 0.5]}


def _list(*objs):
    return [_click(o, 10 + i) for i, o in enumerate(objs)]


def _pairs(clicks):
    return [(c["obj"], c["row_qv"]) for c in clicks]


def test_click_state_reproduces_the_fixture_dictionaries():
    c, meta = load_session_case("near")
    xyz32 = c["coords_full"].astype(np.float32)
    clicks = [{"obj": int(o), "point": tuple(map(float, p)), "row_qv": int(r), "row_full": int(f), "position": xyz32[f].tolist()}
              for p, o, r, f in zip(c["click_points"], c["click_objs"], c["click_rows_qv"], c["click_rows_full"])]
    idx, times, positions = click_state(clicks)
    assert idx == meta["click_idx"] and times == meta["click_time_idx"] and positions == meta["click_positions"]
    assert list(idx) == list(meta["click_idx"]) == ["0", "1", "2", "3", "4"]         # key order: "0", then by first click
    for step in meta["steps"]:                                                        # and every prefix the fixture recorded
        idx, times, _ = click_state(clicks[:step["num_clicks"]])
        assert idx == step["click_idx"] and times == step["click_time"]
        assert list(idx) == list(step["click_idx"])
    assert click_state([]) == ({"0": []}, {"0": []}, {"0": []})
    assert click_state(_list(1, 1))[0] == {"0": [], "1": [10, 11]}                    # "0" is there also when empty
    assert click_state(_list(0, 2, 1))[0] == {"0": [10], "2": [11], "1": [12]}                # ids 1..2, in any order
    for bad in ((2,), (1, 3), (0, 2, 2), (-1,), (1, 256)):
        with pytest.raises(ValueError):
            click_state(_list(*bad))


def test_remove_the_last_and_a_middle_click():
    clicks = _list(1, 2, 0, 1, 3, 2, 0, 3)
    frozen = [dict(c) for c in clicks]
    # the last click: its object keeps another one
    new, lut = remove_from_clicks(clicks, 7)
    assert new == clicks[:7] and np.array_equal(lut, np.arange(256)) and lut.dtype == np.uint8 and lut.shape == (256,)
    # a middle click of an object that keeps others: the times behind it drop by one, ids stay
    new, lut = remove_from_clicks(clicks, 3)
    assert new == clicks[:3] + clicks[4:] and np.array_equal(lut, removal_lut(None))
    idx, times, positions = click_state(new)
    assert idx == {"0": [12, 16], "1": [10], "2": [11, 15], "3": [14, 17]}
    assert times == {"0": [2, 5], "1": [0], "2": [1, 4], "3": [3, 6]}
    assert positions["3"] == [clicks[4]["position"], clicks[7]["position"]]
    # a background click
    new, lut = remove_from_clicks(clicks, 2)
    assert _pairs(new) == _pairs(clicks[:2] + clicks[3:]) and np.array_equal(lut, np.arange(256))
    assert clicks == frozen                                                           # the argument is left alone
    for bad in (-1, 8, 100):
        with pytest.raises(IndexError):
            remove_from_clicks(clicks, bad)
    with pytest.raises(IndexError):
        remove_from_clicks([], 0)


def test_remove_an_objects_only_click_renumbers_the_objects_above():
    clicks = _list(1, 2, 0, 3, 4, 3, 1, 4)
    new, lut = remove_from_clicks(clicks, 1)                                          # object 2's only click
    assert [c["obj"] for c in new] == [1, 0, 2, 3, 2, 1, 3]
    assert [c["row_qv"] for c in new] == [10, 12, 13, 14, 15, 16, 17]
    assert np.array_equal(lut, removal_lut(2)) and lut.dtype == np.uint8
    assert lut[:6].tolist() == [0, 1, 0, 2, 3, 4] and lut[255] == 254
    idx, times, _ = click_state(new)
    assert idx == {"0": [12], "1": [10, 16], "2": [13, 15], "3": [14, 17]}
    assert times == {"0": [1], "1": [0, 5], "2": [2, 4], "3": [3, 6]}
    # the highest object, and the only object
    new, lut = remove_from_clicks(_list(1, 2, 0), 1)
    assert _pairs(new) == [(1, 10), (0, 12)] and np.array_equal(lut, removal_lut(2))
    new, lut = remove_from_clicks(_list(0, 1), 1)
    assert _pairs(new) == [(0, 10)] and np.array_equal(lut, removal_lut(1)) and click_state(new)[0] == {"0": [10]}
    # the table that takes a renumbering back: surviving ids return to where they were
    for k in (None, 1, 2, 7, 255):
        lut, back = removal_lut(k), restore_lut(removal_lut(k))
        old = np.array([j for j in range(256) if j != k])
        assert np.array_equal(back[lut[old]], old) and back.dtype == np.uint8


def test_remove_the_earliest_click_of_an_object_moves_its_instance():
    """(1), (2), (3), (2) minus index 1: ids stay -- object 2 still has a click -- but its instance now comes from the
    later click, which follows the first click of the higher object 3."""
    labels_qv = np.arange(100, 200)                        # voxel row r carries instance 100 + r
    labels_full = np.array([110, 111, 112, 113, 0, 7, 113, 111], np.int32)
    clicks = _list(1, 2, 3, 2)
    assert instance_rows(clicks) == [10, 11, 12]
    assert np.array_equal(list_truth(_pairs(clicks), labels_qv, labels_full), [1, 2, 3, 0, 0, 0, 0, 2])
    new, lut = remove_from_clicks(clicks, 1)
    assert np.array_equal(lut, np.arange(256)) and [c["obj"] for c in new] == [1, 3, 2]
    assert instance_rows(new) == [10, 13, 12]
    idx, times, _ = click_state(new)
    assert idx == {"0": [], "1": [10], "3": [12], "2": [13]} and times == {"0": [], "1": [0], "3": [1], "2": [2]}
    want = list_truth(_pairs(new), labels_qv, labels_full)
    assert np.array_equal(want, [1, 0, 3, 2, 0, 0, 2, 0])
    assert np.array_equal(relabel_numpy(labels_full, labels_qv[instance_rows(new)]), want)
    # two objects on one instance: the higher id wins, whichever was clicked first
    both = [_click(1, 20), _click(2, 21), _click(3, 20)]
    assert np.array_equal(relabel_numpy([120, 121], labels_qv[instance_rows(both)]), [3, 2])
    assert instance_rows([]) == [] and instance_rows(_list(0, 0)) == []
    with pytest.raises(ValueError):
        instance_rows(_list(1, 3))
    # the remap rule's own edges
    got, flag = remap_numpy([0, 3, 255, -1, 256], removal_lut(2))
    assert got.tolist() == [0, 2, 254, 0, 0] and flag == 1 and remap_numpy([1, 2], removal_lut(None))[1] == 0


def test_restore_refusals():
    ok_idx, ok_time = {"0": [5], "1": [7, 8], "2": [9]}, {"0": [2], "1": [0, 3], "2": [1]}
    assert clicks_from_dicts(ok_idx, ok_time, 10, 4) == [(1, 7), (2, 9), (0, 5), (1, 8)]
    assert clicks_from_dicts({"0": []}, {"0": []}, 10, 4) == []
    assert clicks_from_dicts({"1": [3], "0": []}, {"0": [], "1": [0]}, 10, 4) == [(1, 3)]        # dict order is free
    refused = {
        "a missing key": ({"0": [], "2": [1]}, {"0": [], "2": [0]}),
        "no background key": ({"1": [1]}, {"1": [0]}),
        "a key that is no id": ({"0": [], "1": [1], "x": [2]}, {"0": [], "1": [0], "x": [1]}),
        "integer keys": ({0: [], 1: [1]}, {0: [], 1: [0]}),
        "different keys": ({"0": [], "1": [1]}, {"0": [], "1": [0], "2": []}),
        "an object without a click": ({"0": [1], "1": []}, {"0": [0], "1": []}),
        "rows and times of different lengths": ({"0": [], "1": [1, 2]}, {"0": [], "1": [0]}),
        "a time twice": ({"0": [1], "1": [2]}, {"0": [0], "1": [0]}),
        "a gap in the times": ({"0": [1], "1": [2]}, {"0": [0], "1": [2]}),
        "times from 1": ({"0": [], "1": [2]}, {"0": [], "1": [1]}),
        "a negative time": ({"0": [1], "1": [2]}, {"0": [-1], "1": [0]}),
        "a row behind the table": ({"0": [], "1": [10]}, {"0": [], "1": [0]}),
        "a negative row": ({"0": [], "1": [-1]}, {"0": [], "1": [0]}),
        "too many clicks": ({"0": [1, 2, 3], "1": [4, 5]}, {"0": [0, 1, 2], "1": [3, 4]}),
        "no dictionaries": ([[1]], [[0]]),
        "empty": ({}, {}),
    }
    for why, (idx, time) in refused.items():
        with pytest.raises(ValueError):
            clicks_from_dicts(idx, time, 10, 4)
            pytest.fail(why)


def test_marker_hit_is_annotates_cover_rule():
    """``marker_hit`` at every pixel of a small image == ``annotate_rule.marker_cover``'s top marker; ``marker_table``'s kept
    indices name the points that stayed."""
    w, h = 40, 30
    cam = camera_from_matrices(intrinsic(w, h), look_at([0.0, -4.0, 0.5], [0.0, 0.0, 0.0]), w, h)
    rng = np.random.default_rng(4)
    points = np.concatenate([rng.uniform(-1.5, 1.5, (9, 3)), [[0.0, -9.0, 0.5]], rng.uniform(-1.5, 1.5, (2, 3))])   # one behind the camera
    points[3] = points[1] + [0.02, 0.0, 0.0]                    # two markers on top of each other: the later one wins
    colors = rng.uniform(0, 1, (12, 3))
    rows, kept = V.marker_table(cam, points, colors, return_kept=True)
    assert kept.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11] and np.array_equal(rows, V.marker_table(cam, points, colors))
    t = rng.uniform(2.0, 6.0, (h, w)).astype(np.float32)       # a surface now in front of a marker, now behind it
    t[::3, ::2] = np.inf
    for radius, slack in ((6.0, 0.1), (2.5, 0.0), (0.0, 1.0)):
        want, _ = marker_cover(t, rows, radius, radius, slack)
        got = np.array([[-1 if (k := marker_hit(rows, u, v, t[v, u], radius, slack)) is None else k for u in range(w)]
                        for v in range(h)])
        assert np.array_equal(got, want)
        assert radius == 0.0 or ((want >= 0).sum() > 20 and (want < 0).sum() > 20)
    u, v = int(round(float(rows[3, 0]))), int(round(float(rows[3, 1])))
    assert marker_hit(rows, u, v, np.inf, 6.0, 0.1) == 3       # not 1, which lies under it
    bad = rows.copy()
    bad[3, 4] = np.nan                                         # a row with a NaN covers nothing: the one under it shows
    assert marker_hit(bad, u, v, np.inf, 6.0, 0.1) == 1
    assert marker_hit(np.zeros((0, 6), np.float32), 3, 3, 1.0, 6.0, 0.1) is None


def test_edit_struct_matches_the_header():
    import ctypes as C
    assert C.sizeof(L.SessionEditArgs) == 7 * 8 + 2 * 4 + 256 and L.SessionEditArgs.lut.offset == 64
