"""Seeded inputs of the scene build at the sizes where csrc/scene.hip and csrc/radix.hip switch paths (not collected; numpy
only).  Every case is the smallest input that reaches its branch; ``CASES[name]()`` returns int32 [n0, 4] rows (b, x, y, z),
``SAMPLE`` the ``sample=`` the host-side checker gets for it, ``SMALL`` the names cheap enough for the CPU-only tests."""
import numpy as np

LO, HI = -(1 << 17), (1 << 17) - 1      # the coordinate range's ends


def cloud(n, extent, seed, batches=1, origin=(0, 0, 0)):
    """Exactly ``n`` distinct voxels per batch sample, uniform in an ``extent``^3 box whose low corner is ``origin``, in a
    seeded random row order."""
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(batches):
        if extent ** 3 <= 1 << 26:
            cell = rng.choice(extent ** 3, n, replace=False)
            pts = np.stack([cell % extent, (cell // extent) % extent, cell // (extent * extent)], 1)
        else:
            pts = rng.integers(0, extent, (n + n // 8 + 16, 3))
            _, first = np.unique(pts, axis=0, return_index=True)
            pts = pts[np.sort(first)[:n]]
            assert len(pts) == n
        parts.append(np.concatenate([np.full((n, 1), b), pts + np.asarray(origin)], 1))
    return np.concatenate(parts).astype(np.int32)


def morton(xyz):
    """z y x bit-interleaved key of int [n, 3] coordinates (offset to be non-negative): the order of the build's first sort
    inside one batch sample."""
    v = np.asarray(xyz).astype(np.int64) - LO
    key = np.zeros(len(v), np.int64)
    for bit in range(18):
        for a in range(3):
            key |= ((v[:, a] >> bit) & 1) << (3 * bit + a)
    return key


def compact(n, seed, **kw):
    """About one cell in four occupied: the level-0 grid path, and every 16-row group has neighbours."""
    return cloud(n, int(np.ceil((4 * n) ** (1 / 3))) + 1, seed, **kw)


def far(n, seed):
    """Spread over the whole coordinate range: level 0 takes the hash table, hardly any voxel has a neighbour."""
    return cloud(n, 1 << 18, seed, origin=(LO, LO, LO))


def box12(counts, seed):
    """Voxels inside a 12^3 box whose eight corners are occupied (a padded bounding box of 16^3 = 4096 cells), ``counts[b]``
    of them in sample b: at 64 cells per voxel the build switches between the dense grid and the hash table."""
    rng = np.random.default_rng(seed)
    corners = np.array([[x, y, z] for z in (0, 11) for y in (0, 11) for x in (0, 11)])
    parts = []
    for b, n in enumerate(counts):
        cell = rng.permutation(12 ** 3)
        inner = np.stack([cell % 12, (cell // 12) % 12, cell // 144], 1)
        inner = inner[~((inner == 0) | (inner == 11)).all(1)][:n - 8]
        pts = np.concatenate([corners, inner])[rng.permutation(n)]
        parts.append(np.concatenate([np.full((n, 1), b), pts - 5], 1))
    return np.concatenate(parts).astype(np.int32)


def range_corners():
    """Voxels at both ends of the range on every axis, in the same sample and in the samples a wrapped key would land in.
    The library's keys interleave x, y, z below the batch index; a neighbour one step past 2^17 - 1 that was packed without
    a range check would carry into the batch bits and come out as (b + 1 | 2 | 4, -2^17, ...) for x | y | z.  Neither end may
    see the other, at any level.  Odd negative extremes (-2^17 + 1) share their stride-2 parents with -2^17."""
    rows = []
    for b in range(6):
        for y, z in ((5, 5), (-6, 7), (HI, LO)):
            rows += [[b, HI, y, z], [b, LO, y, z], [b, y, HI, z], [b, y, LO, z], [b, y, z, HI], [b, y, z, LO]]
        rows += [[b, LO + 1, LO + 1, LO + 1], [b, LO + 1, LO, LO], [b, LO, LO + 3, LO], [b, HI, HI, HI], [b, HI - 1, HI, HI],
                 [b, LO, LO, LO], [b, HI, LO, LO], [b, LO, HI, HI], [b, -1, -1, -1], [b, 0, 0, 0], [b, -1, 0, -2]]
    rows = np.unique(np.array(rows), axis=0)                 # sorted by batch first: samples stay contiguous
    rng = np.random.default_rng(17)
    return np.concatenate([rng.permutation(rows[rows[:, 0] == b]) for b in range(6)]).astype(np.int32)


def batches_1023():
    """1023 samples (the largest batch index the keys hold is 1022) of the same three voxels, which sit at the range's ends: a
    neighbour lookup that wrapped would land on the same xyz of another sample (x - 1 of -2^17 carries 73 samples up)."""
    xyz = np.array([[LO, LO, LO], [HI, HI, HI], [HI, LO, LO]])
    return np.concatenate([np.concatenate([np.full((3, 1), b), xyz], 1) for b in range(1023)]).astype(np.int32)


def twin_samples():
    """Two samples with identical coordinate sets."""
    c = compact(700, 41)
    return np.concatenate([c, c + np.array([1, 0, 0, 0], np.int32)])


CASES = {}
for _n in (127, 128, 129, 1023, 1024, 1025, 2049):        # npad / 16-lane group edges; the 1024-voxel blocks of k_heads_*
    CASES[f"compact{_n}"] = lambda n=_n: compact(n, n)
    CASES[f"far{_n}"] = lambda n=_n: far(n, n + 1)
CASES.update({
    "neg_two_samples_1500": lambda: cloud(1500, 18, 5, batches=2, origin=(-9, -11, -7)),
    "box12_one_sample_64": lambda: box12([64], 1),         # 4096 cells = 64 per voxel: grid
    "box12_one_sample_63": lambda: box12([63], 2),         # one above: hash
    "box12_two_samples_128": lambda: box12([64, 64], 3),
    "box12_two_samples_127": lambda: box12([64, 63], 4),
    "range_corners": range_corners,
    "corner_hi_20": lambda: cloud(2000, 20, 6, origin=(HI - 19, HI - 19, HI - 19)),      # grid path against the range's end
    "corner_lo_20": lambda: cloud(2000, 20, 7, origin=(LO, LO, LO)),
    "batches_1023": batches_1023,
    "twin_samples_700": twin_samples,
    "tiles_65536": lambda: compact(65536, 8),              # k_tile_prefix: 1024 tiles, one chunk
    "tiles_65537": lambda: compact(65537, 9),              # ... 1026 tiles, two chunks and a carry
    "one_launch_131072": lambda: compact(131072, 10),      # 128 blocks of 1024: k_heads_all and the one-launch sort
    "chain_131073": lambda: compact(131073, 11),           # 129 blocks: the launch chains
    "super_tile_262144": lambda: compact(262144, 12),      # the whole level is one super tile
    "super_tiles_266000": lambda: compact(266000, 13),     # two super tiles: tile_bits = 1
    "block_sums_1048577": lambda: compact(1048577, 14),    # 1025 block sums: k_heads_scan walks two chunks
})
SAMPLE = {"block_sums_1048577": 100_000}   # the 27 neighbour lookups on a subset; the smaller cases are checked row by row
SMALL = [n for n in CASES if n.startswith(("compact", "far", "box12", "neg_", "range_", "corner_", "twin_")) or n == "batches_1023"]
GRID_VS_HASH = ["neg_two_samples_1500", "compact1025", "tiles_65537"]    # rebuilt under A3D_GRID=0
