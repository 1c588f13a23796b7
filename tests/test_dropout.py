"""CPU checks of the decoder dropout option: the model accepts 0 <= dropout < 1 with an unchanged parameter layout, and the
numpy restatement of the masks' RNG reproduces the Philox4x32-10 known-answer vectors of Random123."""
import numpy as np
import pytest

from dropout_ref import keep_mask, philox4x32_10


@pytest.mark.parametrize("key,ctr,want", [
    ((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(key, ctr, want):
    got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
    assert [int(x) for x in got] == list(want)


def test_keep_mask_is_a_function_of_the_logical_index():
    m = keep_mask(123, 1, 17, 0.5, 2, 5, 11)
    assert m.shape == (2, 5, 11) and set(np.unique(m)) <= {0, 1}
    # columns of a narrower tensor are a prefix of a wider one's (the counter does not depend on the column count) ...
    assert np.array_equal(keep_mask(123, 1, 17, 0.5, 2, 5, 7), m[:, :, :7])
    # ... and other samples / sites / seeds draw other masks
    assert not np.array_equal(keep_mask(123, 2, 17, 0.5, 2, 5, 11), m)
    assert not np.array_equal(keep_mask(123, 1, 18, 0.5, 2, 5, 11), m)
    assert not np.array_equal(keep_mask(124, 1, 17, 0.5, 2, 5, 11), m)
    assert keep_mask(5, 0, 0, 0.0, 1, 3, 9).all()


def test_model_accepts_dropout_with_the_same_parameters():
    from agile3d_amd import build_model, default_args
    m0 = build_model(default_args())
    m1 = build_model(default_args(dropout=0.1))
    assert m1.dropout == 0.1 and m0.dropout == 0.0
    s0, s1 = m0.state_dict(), m1.state_dict()
    assert list(s0) == list(s1)
    assert all(s0[k].shape == s1[k].shape for k in s0)


@pytest.mark.parametrize("p", [1.0, -0.1, 1.5])
def test_model_refuses_dropout_outside_the_unit_interval(p):
    from agile3d_amd import build_model, default_args
    with pytest.raises(ValueError):
        build_model(default_args(dropout=p))


def test_tape_refuses_bad_dropout():
    from agile3d_amd.train_decoder import DecoderTape
    with pytest.raises(ValueError):
        DecoderTape(None, None, None, None, None, dropout=1.0)
