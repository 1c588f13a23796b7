"""No GPU: ``clicks.query_list`` -- the one place where a sample's click dictionaries become the decoder's query list
(``Engine.forward_mask`` and ``DecoderTape`` both call it)."""
import numpy as np
import pytest

from agile3d_amd.clicks import query_list


def test_one_object_one_click():
    assert query_list({"0": [], "1": [7]}, {"0": [], "1": [0]}) == ([7], [0], [1], [], [])


def test_ragged_counts_with_background_clicks_in_object_order():
    ci = {"2": [30], "0": [5, 6], "1": [10, 11, 12], "3": [40, 41]}         # dictionary order does not matter
    ct = {"2": [1], "0": [6, 7], "1": [0, 2, 3], "3": [4, 5]}
    assert query_list(ci, ct) == ([10, 11, 12, 30, 40, 41], [0, 2, 3, 1, 4, 5], [3, 1, 2], [5, 6], [6, 7])


def test_a_row_clicked_twice_is_kept_twice():
    assert query_list({"0": [3], "1": [3, 3]}, {"0": [2], "1": [0, 1]}) == ([3, 3], [0, 1], [2], [3], [2])


def test_numpy_rows_come_back_as_python_ints():
    rows, times, counts, bg_rows, bg_times = query_list({"0": np.array([9]), "1": np.array([4, 2], dtype=np.int64)},
                                                        {"0": np.array([2]), "1": [np.int32(0), np.int32(1)]})
    assert (rows, times, counts, bg_rows, bg_times) == ([4, 2], [0, 1], [2], [9], [2])
    assert all(type(v) is int for v in rows + times + bg_rows + bg_times)


def test_an_object_without_clicks_is_refused():
    with pytest.raises(ValueError, match=r"object 2 has no click \(the reference fails on an empty max, agile3d.py:353\)"):
        query_list({"0": [1], "1": [2], "2": []}, {"0": [1], "1": [0], "2": []})


@pytest.mark.parametrize("key", ["0", "1"])
def test_rows_and_times_of_different_lengths_are_refused(key):
    ci, ct = {"0": [1], "1": [2, 3]}, {"0": [2], "1": [0, 1]}
    ct[key] = ct[key] + [9]
    with pytest.raises(ValueError, match="length mismatch"):
        query_list(ci, ct)


def test_a_missing_background_key_is_refused():
    with pytest.raises(ValueError, match='"0"'):
        query_list({"1": [2], "2": [3]}, {"1": [0], "2": [1]})
    with pytest.raises(ValueError, match='"0"'):
        query_list({"0": [], "1": [2]}, {"1": [0]})
