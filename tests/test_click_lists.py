"""clicks.click_lists on the host: the one place a click dictionary becomes the (rows, objects) lists the library takes."""
import numpy as np

from agile3d_amd import clicks as pc


def test_click_lists_keep_dict_order_empties_and_repeats():
    rows, objs = pc.click_lists({"3": [7, 2], "0": [], "1": [2, 2, 9], 2: (5,)})
    assert rows.dtype == np.int32 and objs.dtype == np.int32
    assert rows.tolist() == [7, 2, 2, 2, 9, 5] and objs.tolist() == [3, 3, 1, 1, 1, 2]       # dict order, not sorted; repeats stay
    for nothing in (None, {}, {"0": [], "1": []}):
        rows, objs = pc.click_lists(nothing)
        assert rows.dtype == np.int32 and objs.dtype == np.int32 and rows.shape == objs.shape == (0,)
