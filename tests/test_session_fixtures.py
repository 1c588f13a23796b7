"""CPU checks of the interactive-session fixtures (tests/golden/session_case_*.npz / .json, written by
make_session_goldens.py from the reference's own ``find_nearest`` / ``get_next_click``) and of the pure-Python
formatting helpers of ``agile3d_amd.session`` against the strings the reference wrote.  The loader is in ``session_kit.py``."""
from datetime import datetime

import numpy as np
import pytest

from session_kit import CASES, f64_argmin, load_session_case


@pytest.mark.parametrize("name", CASES)
def test_fixture_rows_are_the_float64_argmin(name):
    """Every scripted click is one where the reference's find_nearest was right: the float64 brute-force arg-min over the
    committed float32 rows equals the stored row, on the voxel rows and on the vertices."""
    c, meta = load_session_case(name)
    xyz32 = c["coords_full"].astype(np.float32)
    qv = xyz32[c["unique_map"]]
    assert len(c["click_points"]) >= 12
    for p, r_qv, r_full in zip(c["click_points"], c["click_rows_qv"], c["click_rows_full"]):
        assert f64_argmin(qv, p) == r_qv
        assert f64_argmin(xyz32, p) == r_full
    # the dictionaries are the rows in script order
    rows = {k: [] for k in meta["click_idx"]}
    for r, o in zip(c["click_rows_qv"].tolist(), c["click_objs"].tolist()):
        rows[str(o)].append(r)
    assert rows == meta["click_idx"]
    assert sorted(t for v in meta["click_time_idx"].values() for t in v) == list(range(len(c["click_objs"])))


@pytest.mark.parametrize("name", CASES)
def test_fixture_drop_rate_cap(name):
    """At most half of the candidate clicks were dropped for the reference's own rounding (the generator's cap)."""
    _, meta = load_session_case(name)
    assert meta["candidates"] >= len(meta["click_time_idx"]) and 2 * meta["dropped"] <= meta["candidates"]
    assert meta["candidates"] - meta["dropped"] == sum(len(v) for v in meta["click_idx"].values())


def test_far_scene_is_far():
    c, _ = load_session_case("far")
    lo, hi = c["coords_full"].min(0), c["coords_full"].max(0)
    assert lo[0] > 45 and hi[1] < -40          # ~50 m out, one axis negative
    n, _ = load_session_case("near")
    assert n["coords_full"].min() > -1 and n["coords_full"].max() < 8


@pytest.mark.parametrize("name", CASES)
def test_formatting_helpers_match_recorded_strings(name):
    from agile3d_amd import session as S
    c, meta = load_session_case(name)
    clock = datetime.fromisoformat(meta["clock"])
    assert len(meta["steps"]) == len(meta["record"]) >= 3
    for j, (step, line) in enumerate(zip(meta["steps"], meta["record"])):
        num_obj = len(step["click_idx"]) - 1
        num_clicks = sum(len(v) for v in step["click_idx"].values())
        assert num_clicks == step["num_clicks"]
        iou = S.format_iou(c[f"step{j}_miou"])
        assert S.record_line(clock, meta["name"], num_obj, num_clicks, iou) == line
        assert S.mask_file_name(num_clicks, num_obj, iou) == step["mask_file"]
        assert S.click_file_name(num_clicks, num_obj, iou) == step["click_file"]
    assert S.format_iou(None) == "NA"
    assert S.record_line(clock, "s", 3, 7, "NA").endswith("  s  NumObjects:3  AvgNumClicks:2.3  mIoU:NA\n")


def test_default_palette_is_ours_and_usable():
    from agile3d_amd.session import default_palette
    pal = default_palette()
    assert pal.shape == (21, 3) and pal.dtype == np.float32 and (pal >= 0).all() and (pal <= 1).all()
    assert len({tuple(r) for r in pal[1:].tolist()}) == 20            # distinct colours
    ref = load_session_case("near")[0]["palette"]
    assert not np.allclose(pal[1:11], ref[1:11], atol=1e-3)          # not the reference's table
