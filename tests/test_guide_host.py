"""CPU: the host half of ``InteractiveSession.guide()`` -- ``rank_suggestions``, ``suggest_clicks``, the summary decoder --
and the known answers of the restated rule (``guide_rule.py``) the GPU tests hold ``a3d_session_guide`` to."""
import numpy as np
import pytest

from agile3d_amd import view as V
from agile3d_amd.session import rank_suggestions, suggest_clicks
from guide_rule import BAD_INDEX, F32, NAN_MARGIN, blend_numpy, guide_numpy, lift_numpy

COORDS = np.arange(30, dtype=np.float32).reshape(10, 3)


def _rec(label, pred, row, size):
    return {"cluster_id": 96 * label + 11 * pred, "row": row, "label": label, "pred": pred, "error_size": size}


def test_rank_suggestions_order_ties_and_limit():
    recs = [_rec(2, 1, 4, 0.25), _rec(1, 0, 7, 0.5), _rec(1, 2, 3, 0.25), _rec(0, 1, 9, 0.125)]    # ids 203, 96, 118, 11
    got = rank_suggestions(recs, COORDS, 5)
    assert [s["row"] for s in got] == [7, 3, 4, 9]                        # by size; the tie 118 before 203: ascending id
    assert got[0] == {"row": 7, "point": COORDS[7].tolist(), "object": 1, "current": 0, "size": 0.5}
    assert all(type(s["row"]) is int and type(s["size"]) is float and type(s["point"][0]) is float for s in got)
    assert rank_suggestions(recs[::-1], COORDS, 5) == got                 # whatever order the records come in
    assert rank_suggestions(recs, COORDS, 2) == got[:2] and rank_suggestions(recs, COORDS, 0) == []
    assert rank_suggestions([], COORDS, 5) == []
    assert rank_suggestions(recs, lambda row: COORDS[row], 5) == got      # a callable lookup
    for bad in (-1, 1.5):
        with pytest.raises(ValueError):
            rank_suggestions(recs, COORDS, bad)


def test_suggest_clicks_when_a_region_has_no_border():
    recs = [_rec(2, 1, 4, 0.25), _rec(1, 0, 7, 0.5)]
    assert suggest_clicks(recs, (3, 0.0), COORDS, 5) == rank_suggestions(recs, COORDS, 5)
    whole = [_rec(1, 0, 0, float("inf"))]                                 # the search's record of a region that covers every row
    assert suggest_clicks(whole, (6, 0.125), COORDS, 5) == [{"row": 6, "point": COORDS[6].tolist(), "object": 1, "current": 0,
                                                             "size": float("inf")}]
    assert suggest_clicks(whole, (6, 0.125), COORDS, 0) == [] and suggest_clicks(whole, None, COORDS, 5) == []
    assert suggest_clicks([_rec(1, 0, 0, float("nan"))], (2, 0.5), COORDS, 5)[0]["row"] == 2
    assert suggest_clicks([], None, COORDS, 5) == []


def test_read_guide_summary():
    rec = np.zeros(1, V.GUIDE_SUMMARY)
    rec["voxels"][0, :3] = [5, 4, 1]
    rec["contested"][0, 1] = 2
    rec["least_key"] = ~np.uint64((int(np.array([0.375], F32).view(np.uint32)[0]) << 32) | 1234)      # stored complemented
    rec["err"] = 2
    got = V.read_guide_summary(rec.view(np.uint8))
    assert got["voxels"][:4].tolist() == [5, 4, 1, 0] and got["contested"][:3].tolist() == [0, 2, 0]
    assert got["voxels"].dtype == np.int64 and got["least"] == (1234, 0.375) and got["err"] == 2
    rec["least_key"] = 0                                                  # the cleared record: no row
    assert V.read_guide_summary(rec.view(np.uint8))["least"] is None


# ---- the rule's own known answers, worked by hand ---------------------------------------------------------------------------
HAND = np.array([[1.0, 3.0, 2.5],        # label 1, runner 2 (behind the winner), margin 0.5: contested at threshold 1
                 [4.0, -1.0, 0.0],       # label 0, runner 2, margin 4
                 [0.0, 0.5, 2.0],        # label 2, runner 1 (before the winner), margin 1.5
                 [2.0, 2.0, 1.0]],       # a tie: label 0 (the first), runner 1, margin 0
                np.float32)


def test_the_rule_by_hand():
    g = guide_numpy(HAND, [], [], 1.0)
    assert g["label"].tolist() == [1, 0, 2, 0] and g["runner"].tolist() == [2, 2, 1, 1]
    assert g["margin"].tolist() == [0.5, 4.0, 1.5, 0.0] and g["margin"].dtype == np.float32
    assert g["contested"].tolist() == [True, False, False, True] and g["want"].tolist() == [2, 0, 2, 1]
    assert g["voxels"][:3].tolist() == [2, 1, 1] and g["contested_per_label"][:3].tolist() == [1, 1, 0]
    assert g["least"] == (3, 0.0) and g["err"] == 0
    assert guide_numpy(HAND, [], [], 0.5)["contested"].tolist() == [False, False, False, True]     # strictly below


def test_the_rule_margin_zero_tie():
    g = guide_numpy(np.zeros((3, 4), np.float32), [], [], 1.0)
    assert g["label"].tolist() == [0, 0, 0] and g["runner"].tolist() == [1, 1, 1] and g["margin"].tolist() == [0.0] * 3
    assert g["want"].tolist() == [1, 1, 1] and g["least"] == (0, 0.0)                               # ties: the lowest row
    assert np.signbit(g["margin"]).sum() == 0


def test_the_rule_clicked_rows():
    g = guide_numpy(HAND, [3, 7, -1], [2, 1, 1], 1.0)                     # rows 7 and -1 lie outside: ignored
    assert g["label"].tolist() == [1, 0, 2, 2] and g["runner"].tolist() == [2, 2, 1, 2]
    assert g["margin"].tolist() == [0.5, 4.0, 1.5, np.inf] and g["want"].tolist() == [2, 0, 2, 2]
    assert g["voxels"][:3].tolist() == [1, 1, 2] and g["contested_per_label"][:3].tolist() == [0, 1, 0]
    assert g["least"] == (0, 0.5)
    twice = guide_numpy(HAND, [0, 3, 0], [2, 2, 0], 1.0)                  # row 0 clicked twice: the last entry wins
    assert twice["label"].tolist() == [0, 0, 2, 2] and twice["margin"][0] == np.inf and twice["least"] == (2, 1.5)
    every = guide_numpy(HAND, [0, 1, 2, 3], [1, 1, 1, 1], 1.0)
    assert every["least"] is None and not every["contested"].any() and every["voxels"][1] == 4


def test_the_rule_nan_row():
    x = HAND.copy()
    x[1, 1] = np.nan
    g = guide_numpy(x, [], [], 1.0)
    assert g["err"] == NAN_MARGIN and g["label"][1] == 0 and g["runner"][1] == 1 and np.isnan(g["margin"][1])
    assert not g["contested"][1] and g["want"][1] == 0 and g["least"] == (3, 0.0)
    x[1] = [np.inf, np.inf, 0.0]                                          # inf - inf
    assert guide_numpy(x, [], [], 1.0)["err"] == NAN_MARGIN


def test_lift_and_blend_by_hand():
    margin = np.array([0.0, 2.0, 4.0, np.inf, 8.0], np.float32)
    out, valid, err = lift_numpy(margin, [4, 0, 5, -1, 3], np.float32(-7))
    assert out.tolist() == [8.0, 0.0, -7.0, -7.0, np.inf] and valid.tolist() == [True, True, False, False, True] and err == BAD_INDEX
    assert lift_numpy(margin, None, np.float32(-7))[0].tolist() == margin.tolist() and lift_numpy(margin, None, 0)[2] == 0
    pal = np.array([[9, 9, 9], [1, 0, 0], [0, 1, 0]], np.float32)         # two objects
    own = np.full((5, 3), 0.25, np.float32)
    doubt = (1.0, 1.0, 0.5)
    got = blend_numpy([1, 2, 0, 3, 4], margin, own, pal, doubt, 4.0)      # labels 3 and 4 wrap to entries 1 and 2
    assert got.dtype == np.float32
    assert got[0].tolist() == [1.0, 1.0, 0.5]                             # margin 0: exactly the doubt colour
    assert got[1].tolist() == [0.5, 1.0, 0.25]                            # half way between object 2's green and the doubt colour
    assert got[2].tolist() == [0.25, 0.25, 0.25]                          # sure, background: the vertex's own colour
    assert got[3].tolist() == [1.0, 0.0, 0.0] and got[4].tolist() == [0.0, 1.0, 0.0]     # inf and 8 > full_margin: exactly base
