"""The column slices of an input-gradient conv (``backward.input_grad_slices``: the conv kernels write 32, 64, 96 or a
multiple of 128 output columns) and the forward-kind -> input-gradient-kind table, on the CPU."""
import pytest

from agile3d_amd import backward as B
from agile3d_amd import lib as L

SLICES = {32: [(0, 32)], 64: [(0, 64)], 96: [(0, 96)], 128: [(0, 128)], 160: [(0, 128), (128, 32)],
          192: [(0, 128), (128, 64)], 224: [(0, 128), (128, 96)], 256: [(0, 256)],
          288: [(0, 128), (128, 128), (256, 32)], 384: [(0, 384)]}


@pytest.mark.parametrize("cin", sorted(SLICES))
def test_input_grad_slices_are_the_fixed_lists(cin):
    got = B.input_grad_slices(cin)
    assert got == SLICES[cin]
    # they tile [0, cin) with widths the kernels write
    assert got[0][0] == 0 and sum(w for _, w in got) == cin
    assert all(a + wa == b for (a, wa), (b, _) in zip(got, got[1:]))
    assert all(w in (32, 64, 96) or w % 128 == 0 for _, w in got)


def test_back_kind_is_an_involution():
    assert set(B.BACK_KIND) == {L.OP_CONV3, L.OP_DOWN, L.OP_UP, L.OP_LINEAR} == set(B._KVOL)
    assert all(B.BACK_KIND[B.BACK_KIND[k]] == k for k in B.BACK_KIND)
    assert B.BACK_KIND[L.OP_DOWN] == L.OP_UP and B.BACK_KIND[L.OP_CONV3] == L.OP_CONV3 and B.BACK_KIND[L.OP_LINEAR] == L.OP_LINEAR
    # the input gradient of a conv from level l to level l' runs from l' back to l
    for k in B.BACK_KIND:
        assert B.level_out(B.BACK_KIND[k], B.level_out(k, 2)) == 2
