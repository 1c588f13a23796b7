"""The scene tables' contract in numpy (tests/scene_rule.py) tried on the CPU: the checker accepts the rule's own tables on
the scenes the GPU tests use, agrees with the oracle's coordinate manager on level sizes and coordinate sets, and refuses
every kind of wrong table it exists to catch -- each for its own reason."""
import numpy as np
import pytest

import scene_cases as sc
import scene_rule as R
from agile3d_amd import lib as L
from oracle import backbone as ob
from test_gpu_scene import CASES as SEVEN


def _coords(name):
    return SEVEN[name]() if name in SEVEN else sc.CASES[name]()


@pytest.mark.parametrize("name", list(SEVEN) + sc.SMALL)
def test_checker_accepts_the_rule_and_agrees_with_the_oracle(name):
    coords = _coords(name)
    T = R.build_tables(coords)
    assert sorted(T) == sorted(R.table_keys())
    R.check_tables(coords, T)
    R.check_tables(coords, T, sample=50)
    lv = ob.SparseLevels(coords)
    for level in range(5):
        mine = R.level_coords(coords, level)
        assert lv.n(level) == len(mine) == T[level, L.TAB_XYZB].size // 4
        theirs = lv.levels[level].astype(np.int64)
        theirs = theirs[np.lexsort((theirs[:, 1], theirs[:, 2], theirs[:, 3], theirs[:, 0]))]
        assert np.array_equal(mine, theirs), level


def test_cases_have_the_sizes_and_lookup_structures_they_are_named_for():
    for n in (127, 128, 129, 1023, 1024, 1025, 2049):
        assert len(sc.CASES[f"compact{n}"]()) == n == len(sc.CASES[f"far{n}"]())
        assert R.grid_expected(sc.CASES[f"compact{n}"]()) is not None and R.grid_expected(sc.CASES[f"far{n}"]()) is None
    assert R.grid_expected(sc.CASES["box12_one_sample_64"]()) == (16, 16, 16)
    assert R.grid_expected(sc.CASES["box12_two_samples_128"]()) == (16, 16, 16)
    assert R.grid_expected(sc.CASES["box12_one_sample_63"]()) is None and len(sc.CASES["box12_one_sample_63"]()) == 63
    assert R.grid_expected(sc.CASES["box12_two_samples_127"]()) is None and len(sc.CASES["box12_two_samples_127"]()) == 127
    assert R.grid_expected(sc.CASES["corner_hi_20"]()) is not None and R.grid_expected(sc.CASES["corner_lo_20"]()) is not None
    assert sc.CASES["corner_hi_20"]()[:, 1:].max() == sc.HI and sc.CASES["corner_lo_20"]()[:, 1:].min() == sc.LO
    assert R.grid_expected(sc.CASES["range_corners"]()) is None and R.grid_expected(sc.CASES["batches_1023"]()) is None
    for name in sc.GRID_VS_HASH:
        assert R.grid_expected(sc.CASES[name]()) is not None


@pytest.mark.parametrize("name", ["compact1025", "compact2049"])
def test_siblings_straddle_the_first_block_edge(name):
    """Rows 1023 and 1024 of the Morton-sorted level 0 share their level-1 parent: head_flags reads keys[i - 1] across the edge
    of a 1024-voxel block, and a flag set wrongly there would split the parent in two."""
    c = sc.CASES[name]()
    m = sc.morton(c[:, 1:])
    order = np.argsort(m)
    a, b = c[order[1023], 1:] >> 1, c[order[1024], 1:] >> 1
    assert (a == b).all()


def test_neither_end_of_the_range_is_the_other_ends_neighbour():
    """The rule itself on the range's ends: (2^17 - 1, y, z) and (-2^17, y, z) are both rows, and neither is a hit of the
    other at any level."""
    coords = sc.CASES["range_corners"]()
    T = R.build_tables(coords)
    for level in range(5):
        x = T[level, L.TAB_XYZB].reshape(-1, 4).astype(np.int64)
        n = len(x)
        nbr = T[level, L.TAB_NBR27].reshape(27, -1)[:, :n]
        lo, hi = sc.LO >> level, sc.HI >> level
        for axis in range(3):
            assert (x[:, axis] == lo).any() and (x[:, axis] == hi).any()
        for k in range(27):
            hit = nbr[k] < n
            step = np.abs(x[nbr[k][hit]][:, :3] - x[hit][:, :3])
            assert (step <= 1).all() and (x[nbr[k][hit]][:, 3] == x[hit][:, 3]).all()


# ---- the checker is not vacuous: one mutation of a valid table set per case, each refused for its own reason
def _nbr(T, level=0):
    n = T[level, L.TAB_XYZB].size // 4
    return T[level, L.TAB_NBR27].reshape(27, -1), n


def _first(mask):
    k, i = np.nonzero(mask)
    return int(k[0]), int(i[0])


def m_hit_to_n(T, coords):
    nbr, n = _nbr(T)
    k, i = _first((nbr[:, :n] < n) & (np.arange(27)[:, None] != 13))
    nbr[k, i] = n


def m_miss_to_row(T, coords):
    nbr, n = _nbr(T)
    k, i = _first(nbr[:, :n] == n)
    nbr[k, i] = (i + 1) % n


def m_hit_to_other_sample(T, coords):
    nbr, n = _nbr(T)
    x = T[0, L.TAB_XYZB].reshape(-1, 4)
    k, i = _first((nbr[:, :n] < n) & (x[:, 3] == 0)[None, :])
    tgt = x[nbr[k, i]]
    twin = np.flatnonzero((x[:, :3] == tgt[:3]).all(1) & (x[:, 3] == 1))
    nbr[k, i] = twin[0]


def m_gmask_bit_cleared(T, coords):
    g = T[1, L.TAB_GMASK27]
    g[0] &= ~np.uint32(1 << 13)


def m_gmask_bit_set(T, coords):
    g = T[0, L.TAB_GMASK27]
    i = int(np.flatnonzero(g != (1 << 27) - 1)[0])
    free = [k for k in range(27) if not (int(g[i]) >> k) & 1]
    g[i] |= np.uint32(1 << free[0])


def m_pre27_off_by_one(T, coords):
    T[0, L.TAB_PRE27][3] += 1


def m_preup_total(T, coords):
    T[2, L.TAB_PREUP][-1] -= 1


def m_child_slots_swapped(T, coords):
    nC = T[1, L.TAB_XYZB].size // 4
    ch = T[0, L.TAB_CHILD8].reshape(8, -1)
    n = T[0, L.TAB_XYZB].size // 4
    c = int(np.flatnonzero((ch[:, :nC] < n).sum(0) >= 2)[0])
    s = np.flatnonzero(ch[:, c] < n)[:2]
    ch[s, c] = ch[s[::-1], c]


def m_child_under_two_parents(T, coords):
    nC = T[1, L.TAB_XYZB].size // 4
    ch = T[0, L.TAB_CHILD8].reshape(8, -1)
    n = T[0, L.TAB_XYZB].size // 4
    s, c = _first(ch[:, :nC] == n)
    ch[s, c] = ch[:, (c + 1) % nC][ch[:, (c + 1) % nC] < n][0]


def m_up_hit_moved(T, coords):
    nC = T[2, L.TAB_XYZB].size // 4
    up = T[1, L.TAB_UP8].reshape(8, -1)
    s = int(np.flatnonzero(up[:, 5] < nC)[0])
    up[(s + 1) % 8, 5], up[s, 5] = up[s, 5], nC


def m_padding_not_n(T, coords):
    nbr, n = _nbr(T, 3)
    assert nbr.shape[1] > n
    nbr[4, -1] = 0


def m_origrow_twice(T, coords):
    o = T[0, L.TAB_ORIGROW]
    o[7] = o[8]


MUTATIONS = [
    (m_hit_to_n, "NBR27 level 0: .*existing neighbour .* reported missing"),
    (m_miss_to_row, "NBR27 level 0: .*points at row .* which holds"),
    (m_hit_to_other_sample, "NBR27 level 0: .*another batch sample"),
    (m_gmask_bit_cleared, "GMASK27 level 1: group 0 lacks an offset"),
    (m_gmask_bit_set, "GMASK27 level 0: group .* has an offset none of its 16 rows has"),
    (m_pre27_off_by_one, "PRE27 level 0: entry 3 is"),
    (m_preup_total, "PREUP level 2: total is"),
    (m_child_slots_swapped, "CHILD8 level 0: fine row .* sits at slot"),
    (m_child_under_two_parents, "CHILD8 level 0: fine row .* is listed 2 times"),
    (m_up_hit_moved, "UP8 level 1: virtual row 5 has its hit at slot"),
    (m_padding_not_n, "NBR27 level 3: a padding entry is not n"),
    (m_origrow_twice, "ORIGROW level 0: is not a permutation"),
]


@pytest.fixture(scope="module")
def valid():
    coords = sc.CASES["twin_samples_700"]()      # two samples with the same xyz: a hit can be sent to the other sample's twin
    T = R.build_tables(coords)
    R.check_tables(coords, T)
    return coords, T


@pytest.mark.parametrize("mutate,message", MUTATIONS, ids=[m[0].__name__[2:] for m in MUTATIONS])
def test_checker_refuses(valid, mutate, message):
    coords, T = valid
    T = {k: v.copy() for k, v in T.items()}
    before = {k: v.copy() for k, v in T.items()}
    mutate(T, coords)
    changed = [k for k in T if not np.array_equal(T[k], before[k])]
    assert len(changed) == 1 and (T[changed[0]] != before[changed[0]]).sum() <= 2, changed
    with pytest.raises(R.TableError, match=message) as e:
        R.check_tables(coords, T)
    assert (e.value.level, e.value.table) == changed[0]
