"""The contract of the scene tables (``A3D_TAB_*``, include/agile3d_hip.h) restated in vectorised numpy, independently of the
package (not collected; numpy only -- of ``agile3d_amd`` nothing but the table ids is imported, of ``oracle`` nothing).

``tables`` is a dict ``{(level, table id): flat array}`` with the arrays as ``a3d_scene_table`` hands them out.
``build_tables`` makes one valid set (rows sorted by batch, z, y, x; virtual rows sorted by child slot), ``check_tables`` holds
any set -- the library's row order is its own -- to the contract.  Everything is integer, so every check is an equality.

Keys: batch index (<= 1022, 10 bits) on top of three 18-bit fields z, y, x offset by 2^17 -- a ``uint64``.  A neighbour offset
that leaves [-2^17, 2^17) is masked as missing BEFORE it is packed: packed, it would carry into the next field."""
import numpy as np

from agile3d_amd.lib import (TAB_CHILD8, TAB_GMASK27, TAB_GMASKDOWN, TAB_GMASKUP, TAB_NBR27, TAB_ORIGROW, TAB_PRE27,
                             TAB_PREDOWN, TAB_PREUP, TAB_UP8, TAB_UPROWS, TAB_XYZB)

LEVELS = 5
COORD_OFF = 1 << 17          # coordinates live in [-2^17, 2^17)
MAX_BATCH = 1022
GRID_PAD, GRID_CELLS_PER_VOXEL = 2, 64
DENSE_BOX_CELLS = 1 << 25    # neighbour lookup: a dense box up to this many cells, sorted keys + searchsorted above
NAMES = {TAB_XYZB: "XYZB", TAB_NBR27: "NBR27", TAB_GMASK27: "GMASK27", TAB_CHILD8: "CHILD8", TAB_GMASKDOWN: "GMASKDOWN",
         TAB_UP8: "UP8", TAB_GMASKUP: "GMASKUP", TAB_UPROWS: "UPROWS", TAB_ORIGROW: "ORIGROW", TAB_PRE27: "PRE27",
         TAB_PREDOWN: "PREDOWN", TAB_PREUP: "PREUP"}
PER_LEVEL = (TAB_XYZB, TAB_NBR27, TAB_GMASK27, TAB_PRE27)                                    # levels 0 .. 4
PER_PAIR = (TAB_CHILD8, TAB_GMASKDOWN, TAB_UP8, TAB_GMASKUP, TAB_UPROWS, TAB_PREDOWN, TAB_PREUP)   # levels 0 .. 3


def table_keys():
    """Every (level, table id) the library serves."""
    return [(lv, t) for lv in range(LEVELS) for t in PER_LEVEL] + [(lv, t) for lv in range(LEVELS - 1) for t in PER_PAIR] + \
        [(0, TAB_ORIGROW)]


def npad_of(n):
    return (max(n, 1) + 127) // 128 * 128


def pack(b, x, y, z):
    """uint64 key of (b, x, y, z); all fields must be in range (mask first)."""
    b, x, y, z = (np.asarray(a).astype(np.int64) for a in (b, x, y, z))
    return ((b << 54) | ((z + COORD_OFF) << 36) | ((y + COORD_OFF) << 18) | (x + COORD_OFF)).astype(np.uint64)


def in_range(x, y, z):
    return (x >= -COORD_OFF) & (x < COORD_OFF) & (y >= -COORD_OFF) & (y < COORD_OFF) & (z >= -COORD_OFF) & (z < COORD_OFF)


def level_coords(coords, level):
    """Sorted distinct (b, x >> L, y >> L, z >> L) of the caller's rows, int64 [n_L, 4], in (b, z, y, x) order.  The shift is
    arithmetic: floor division for negative coordinates."""
    c = np.asarray(coords).astype(np.int64)
    assert c.ndim == 2 and c.shape[1] == 4
    assert c[:, 0].min() >= 0 and c[:, 0].max() <= MAX_BATCH and in_range(c[:, 1], c[:, 2], c[:, 3]).all()
    k = np.unique(pack(c[:, 0], c[:, 1] >> level, c[:, 2] >> level, c[:, 3] >> level))
    return unpack(k)


def unpack(k):
    k = np.asarray(k, np.uint64)            # a batch index from 512 up sets bit 63: shift as unsigned
    m, u = np.uint64((1 << 18) - 1), np.uint64
    return np.stack([(k >> u(54)).astype(np.int64), (k & m).astype(np.int64) - COORD_OFF,
                     ((k >> u(18)) & m).astype(np.int64) - COORD_OFF, ((k >> u(36)) & m).astype(np.int64) - COORD_OFF], 1)


def grid_expected(coords):
    """The level-0 lookup structure the header promises: the dense grid's (x, y, z) cell counts when the padded bounding box of
    the batch, times the number of samples, has at most 64 cells per voxel; None (the hash table) otherwise."""
    c = np.asarray(coords).astype(np.int64)
    dims = tuple(int(e) + 2 * GRID_PAD for e in c[:, 1:].max(0) - c[:, 1:].min(0) + 1)
    cells = (int(c[:, 0].max()) + 1) * dims[0] * dims[1] * dims[2]
    return dims if cells <= GRID_CELLS_PER_VOXEL * len(c) else None


class Lookup:
    """Row of a coordinate among ``bxyz`` (int64 [n, 4], distinct), -1 where there is none."""

    def __init__(self, bxyz):
        self.n = len(bxyz)
        self.lo = bxyz[:, 1:].min(0) - 1
        self.dim = bxyz[:, 1:].max(0) + 1 - self.lo + 1          # one empty cell on every side: the 3^3 offsets stay inside
        self.nb = int(bxyz[:, 0].max()) + 1
        if self.nb * int(self.dim[0]) * int(self.dim[1]) * int(self.dim[2]) <= DENSE_BOX_CELLS:
            self.box = np.full(self.nb * int(np.prod(self.dim)), -1, np.int32)
            cell = self._cell(bxyz[:, 0], bxyz[:, 1], bxyz[:, 2], bxyz[:, 3])
            self.box[cell] = np.arange(self.n, dtype=np.int32)
            assert (self.box[cell] == np.arange(self.n)).all(), "coordinates are not distinct"
        else:
            self.box = None
            keys = pack(bxyz[:, 0], bxyz[:, 1], bxyz[:, 2], bxyz[:, 3])
            self.order = np.argsort(keys, kind="stable")
            self.sorted = keys[self.order]
            assert (self.sorted[1:] != self.sorted[:-1]).all(), "coordinates are not distinct"

    def _cell(self, b, x, y, z):
        return ((b * self.dim[2] + (z - self.lo[2])) * self.dim[1] + (y - self.lo[1])) * self.dim[0] + (x - self.lo[0])

    def rows(self, b, x, y, z):
        """Coordinates within one step of an existing voxel (what the 3^3 offsets produce)."""
        ok = in_range(x, y, z)
        if self.box is not None:
            for a, v in enumerate((x, y, z)):
                ok = ok & (v >= self.lo[a]) & (v < self.lo[a] + self.dim[a])
            return np.where(ok, self.box[np.where(ok, self._cell(b, x, y, z), 0)], -1)
        k = pack(b, np.where(ok, x, 0), np.where(ok, y, 0), np.where(ok, z, 0))
        pos = np.minimum(np.searchsorted(self.sorted, k), self.n - 1)
        return np.where(ok & (self.sorted[pos] == k), self.order[pos], -1)


def offset27(k):
    """(dx, dy, dz) of kernel offset k: x fastest."""
    return k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1


def group_or(hit):
    """hit: bool [K, npad] -> uint32 [npad / 16]: bit k set where any of the group's 16 rows has a hit at offset k."""
    K, npad = hit.shape
    any16 = hit.reshape(K, npad // 16, 16).any(2)
    out = np.zeros(npad // 16, np.uint32)
    for k in range(K):
        out |= any16[k].astype(np.uint32) << np.uint32(k)
    return out


def popcount(a):
    a = a.astype(np.uint32)
    a = a - ((a >> 1) & np.uint32(0x55555555))
    a = (a & np.uint32(0x33333333)) + ((a >> 2) & np.uint32(0x33333333))
    a = (a + (a >> 4)) & np.uint32(0x0F0F0F0F)
    return ((a * np.uint32(0x01010101)) >> 24).astype(np.int64)


def tile_prefix(gmask):
    """int32 [ntile + 1]: before each 64-row tile (four 16-row groups) the (tile, offset) pairs of the tiles in front of it --
    a tile counts one pair per offset any of its four groups has; the last entry is the total."""
    per_tile = popcount(np.bitwise_or.reduce(gmask.reshape(-1, 4), axis=1))
    return np.concatenate([[0], np.cumsum(per_tile)]).astype(np.int32)


def slot_of(bxyz):
    return (bxyz[:, 1] & 1) + 2 * (bxyz[:, 2] & 1) + 4 * (bxyz[:, 3] & 1)


def parent_rows(fine, coarse_lookup):
    return coarse_lookup.rows(fine[:, 0], fine[:, 1] >> 1, fine[:, 2] >> 1, fine[:, 3] >> 1)


def build_tables(coords):
    """One valid table set of ``coords`` (int [n0, 4] rows (b, x, y, z), distinct)."""
    coords = np.asarray(coords)
    lv = [level_coords(coords, L) for L in range(LEVELS)]
    assert len(lv[0]) == len(coords), "duplicate voxel coordinates"
    look = [Lookup(c) for c in lv]
    T = {}
    c64 = coords.astype(np.int64)
    T[0, TAB_ORIGROW] = np.argsort(pack(c64[:, 0], c64[:, 1], c64[:, 2], c64[:, 3]), kind="stable").astype(np.int32)
    for L in range(LEVELS):
        c, n = lv[L], len(lv[L])
        npad = npad_of(n)
        T[L, TAB_XYZB] = np.stack([c[:, 1], c[:, 2], c[:, 3], c[:, 0]], 1).astype(np.int32).reshape(-1)
        nbr = np.full((27, npad), n, np.int32)
        for k in range(27):
            dx, dy, dz = offset27(k)
            r = look[L].rows(c[:, 0], c[:, 1] + dx, c[:, 2] + dy, c[:, 3] + dz)
            nbr[k, :n] = np.where(r >= 0, r, n)
        T[L, TAB_NBR27] = nbr.reshape(-1)
        T[L, TAB_GMASK27] = group_or(nbr < n)
        T[L, TAB_PRE27] = tile_prefix(T[L, TAB_GMASK27])
    for L in range(LEVELS - 1):
        f, n, nC = lv[L], len(lv[L]), len(lv[L + 1])
        npad, npadC = npad_of(n), npad_of(nC)
        par, slot = parent_rows(f, look[L + 1]), slot_of(f)
        child = np.full((8, npadC), n, np.int32)
        child[slot, par] = np.arange(n)
        T[L, TAB_CHILD8] = child.reshape(-1)
        T[L, TAB_GMASKDOWN] = group_or(child < n)
        T[L, TAB_PREDOWN] = tile_prefix(T[L, TAB_GMASKDOWN])
        uprows = np.zeros(npad, np.int32)
        uprows[:n] = np.argsort(slot, kind="stable")
        up = np.full((8, npad), nC, np.int32)
        up[slot[uprows[:n]], np.arange(n)] = par[uprows[:n]]
        T[L, TAB_UPROWS] = uprows
        T[L, TAB_UP8] = up.reshape(-1)
        T[L, TAB_GMASKUP] = group_or(up < nC)
        T[L, TAB_PREUP] = tile_prefix(T[L, TAB_GMASKUP])
    return T


class TableError(AssertionError):
    def __init__(self, level, table, what):
        super().__init__(f"{NAMES[table]} level {level}: {what}")
        self.level, self.table = level, table


def _need(cond, level, table, what):
    if not cond:
        raise TableError(level, table, what() if callable(what) else what)


def _is_permutation(a, n):
    return len(a) == n and (n == 0 or (a.min() >= 0 and a.max() < n and (np.bincount(a, minlength=n) == 1).all()))


def _check_masks(T, L, mask_tab, pre_tab, hit):
    got, want = T[L, mask_tab], group_or(hit)
    _need(got.dtype == np.uint32 and got.shape == want.shape, L, mask_tab, f"{got.shape} {got.dtype}, expected {want.shape} uint32")
    lack, extra = want & ~got, got & ~want
    _need(not lack.any(), L, mask_tab,
          lambda: f"group {int(np.flatnonzero(lack)[0])} lacks an offset one of its 16 rows has (bits {int(lack[lack != 0][0]):#x})")
    _need(not extra.any(), L, mask_tab,
          lambda: f"group {int(np.flatnonzero(extra)[0])} has an offset none of its 16 rows has (bits {int(extra[extra != 0][0]):#x})")
    pre, want_pre = T[L, pre_tab], tile_prefix(got)
    _need(pre.shape == want_pre.shape, L, pre_tab, f"length {len(pre)}, expected {len(want_pre)}")
    bad = np.flatnonzero(pre[:-1] != want_pre[:-1])
    _need(len(bad) == 0, L, pre_tab, lambda: f"entry {int(bad[0])} is {int(pre[bad[0]])}, the tiles before it hold {int(want_pre[bad[0]])} pairs")
    _need(pre[-1] == want_pre[-1], L, pre_tab, f"total is {int(pre[-1])}, the tiles hold {int(want_pre[-1])} pairs")


def check_tables(coords, tables, *, sample=None):
    """Hold ``tables`` to the header's contract for the caller's ``coords``; raises ``TableError`` (an AssertionError naming
    the table and level) at the first breach.  ``sample``: at a level with more rows than this, the 27 neighbour lookups are
    checked on that many seeded random rows plus the first and last 256; everything else stays exhaustive."""
    coords = np.asarray(coords)
    T = tables
    want = [level_coords(coords, L) for L in range(LEVELS)]
    bx, look = [], []
    for L in range(LEVELS):
        n = len(want[L])
        t = T[L, TAB_XYZB]
        _need(t.size == 4 * n, L, TAB_XYZB, f"{t.size // 4} rows, the level has {n}")
        t = t.reshape(-1, 4).astype(np.int64)
        _need(t[:, 3].min() >= 0 and t[:, 3].max() <= MAX_BATCH and in_range(t[:, 0], t[:, 1], t[:, 2]).all(), L, TAB_XYZB,
              "a coordinate outside the range")
        b = np.stack([t[:, 3], t[:, 0], t[:, 1], t[:, 2]], 1)
        _need(np.array_equal(unpack(np.sort(pack(b[:, 0], b[:, 1], b[:, 2], b[:, 3]))), want[L]), L, TAB_XYZB,
              "the rows are not the distinct (b, xyz >> level) of the input")
        bx.append(b)
        look.append(Lookup(b))
    n0 = len(coords)
    orig = T[0, TAB_ORIGROW]
    _need(_is_permutation(orig, n0), 0, TAB_ORIGROW, "is not a permutation of the caller's rows")
    c64 = coords.astype(np.int64)
    _need(np.array_equal(c64[orig], bx[0]), 0, TAB_ORIGROW, "XYZB does not hold the coordinates of the caller's row it names")

    for L in range(LEVELS):
        b, n = bx[L], len(bx[L])
        npad = npad_of(n)
        nbr = T[L, TAB_NBR27]
        _need(nbr.size == 27 * npad, L, TAB_NBR27, f"{nbr.size} entries, expected 27 x {npad}")
        nbr = nbr.reshape(27, npad)
        _need(nbr.min() >= 0 and nbr.max() <= n, L, TAB_NBR27, "an entry outside [0, n]")
        _need((nbr[:, n:] == n).all(), L, TAB_NBR27, "a padding entry is not n")
        if sample is not None and n > sample:
            rows = np.unique(np.concatenate([np.arange(min(256, n)), np.arange(max(n - 256, 0), n),
                                             np.random.default_rng(n).integers(0, n, sample)]))
        else:
            rows = np.arange(n)
        src = b[rows]
        for k in range(27):
            dx, dy, dz = offset27(k)
            tgt = src + np.array([0, dx, dy, dz])
            r = nbr[k, rows]
            hit = r < n
            held = b[np.where(hit, r, 0)]
            wrong = hit & (held != tgt).any(1)
            if wrong.any():
                i = int(np.flatnonzero(wrong)[0])
                other = " (a row of another batch sample)" if held[i, 0] != tgt[i, 0] else ""
                raise TableError(L, TAB_NBR27, f"offset {k} of row {int(rows[i])} points at row {int(r[i])}, which holds "
                                 f"{held[i].tolist()}, not {tgt[i].tolist()}{other}")
            there = look[L].rows(tgt[:, 0], tgt[:, 1], tgt[:, 2], tgt[:, 3])
            lost = ~hit & (there >= 0)
            _need(not lost.any(), L, TAB_NBR27, lambda: f"offset {k} of row {int(rows[np.flatnonzero(lost)[0]])}: an existing "
                  f"neighbour (row {int(there[np.flatnonzero(lost)[0]])}) is reported missing")
        _check_masks(T, L, TAB_GMASK27, TAB_PRE27, nbr < n)

    for L in range(LEVELS - 1):
        f, c, n, nC = bx[L], bx[L + 1], len(bx[L]), len(bx[L + 1])
        npad, npadC = npad_of(n), npad_of(nC)
        slot = slot_of(f)
        par = parent_rows(f, look[L + 1])
        assert (par >= 0).all()            # follows from the coordinate sets checked above
        child = T[L, TAB_CHILD8]
        _need(child.size == 8 * npadC, L, TAB_CHILD8, f"{child.size} entries, expected 8 x {npadC}")
        child = child.reshape(8, npadC)
        _need(child.min() >= 0 and child.max() <= n, L, TAB_CHILD8, "an entry outside [0, n]")
        _need((child[:, nC:] == n).all(), L, TAB_CHILD8, "a padding entry is not n")
        s_idx, c_idx = np.nonzero(child < n)
        fine = child[s_idx, c_idx]
        times = np.bincount(fine, minlength=n)
        _need((times == 1).all(), L, TAB_CHILD8, lambda: f"fine row {int(np.flatnonzero(times != 1)[0])} is listed "
              f"{int(times[times != 1][0])} times, not exactly once")
        bad = np.flatnonzero(par[fine] != c_idx)
        _need(len(bad) == 0, L, TAB_CHILD8, lambda: f"fine row {int(fine[bad[0]])} is listed under coarse row {int(c_idx[bad[0]])}, "
              f"its parent is {int(par[fine[bad[0]]])}")
        bad = np.flatnonzero(slot[fine] != s_idx)
        _need(len(bad) == 0, L, TAB_CHILD8, lambda: f"fine row {int(fine[bad[0]])} sits at slot {int(s_idx[bad[0]])}, its slot "
              f"(x&1) + 2(y&1) + 4(z&1) is {int(slot[fine[bad[0]]])}")
        _check_masks(T, L, TAB_GMASKDOWN, TAB_PREDOWN, child < n)

        uprows = T[L, TAB_UPROWS]
        _need(uprows.size == npad, L, TAB_UPROWS, f"{uprows.size} entries, expected {npad}")
        _need(_is_permutation(uprows[:n], n), L, TAB_UPROWS, "is not a permutation of the level's rows")
        up = T[L, TAB_UP8]
        _need(up.size == 8 * npad, L, TAB_UP8, f"{up.size} entries, expected 8 x {npad}")
        up = up.reshape(8, npad)
        _need(up.min() >= 0 and up.max() <= nC, L, TAB_UP8, "an entry outside [0, n of the coarse level]")
        _need((up[:, n:] == nC).all(), L, TAB_UP8, "a padding entry is not the coarse level's n")
        hits = up[:, :n] < nC
        bad = np.flatnonzero(hits.sum(0) != 1)
        _need(len(bad) == 0, L, TAB_UP8, lambda: f"virtual row {int(bad[0])} has {int(hits[:, bad[0]].sum())} hits, not exactly one")
        s_of_v = hits.argmax(0)
        fr = uprows[:n]
        bad = np.flatnonzero(s_of_v != slot[fr])
        _need(len(bad) == 0, L, TAB_UP8, lambda: f"virtual row {int(bad[0])} has its hit at slot {int(s_of_v[bad[0]])}, the slot of "
              f"fine row {int(fr[bad[0]])} is {int(slot[fr[bad[0]]])}")
        bad = np.flatnonzero(up[s_of_v, np.arange(n)] != par[fr])
        _need(len(bad) == 0, L, TAB_UP8, lambda: f"virtual row {int(bad[0])} points at coarse row {int(up[s_of_v[bad[0]], bad[0]])}, the "
              f"parent of fine row {int(fr[bad[0]])} is {int(par[fr[bad[0]]])}")
        _check_masks(T, L, TAB_GMASKUP, TAB_PREUP, up < nC)
