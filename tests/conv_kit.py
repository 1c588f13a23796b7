"""Scenes and references shared by the exact sparse-convolution tests (test_gpu_wgrad_edges.py, test_gpu_conv_edges.py) and the
CPU-side plan-class test: named scenes, the World of a scene (oracle levels, row maps both ways, internal-row pair lists
from the CPU oracle's kernel maps) and seeded integer operands.  The coordinate builders need no GPU; a World does."""
import zlib

import numpy as np
import torch

from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from gpu_util import _random_coords, internal_to_oracle_rows, scratch  # noqa: F401  (scratch: the NaN-poisoned workspace)
from oracle import backbone as ob


def _box(n, seed):
    """n distinct random voxels of a 48^3 box, shuffled."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(48 ** 3, n, replace=False)
    xyz = np.stack([cells % 48, (cells // 48) % 48, cells // (48 * 48)], 1)
    return np.concatenate([np.zeros((n, 1), np.int64), xyz], 1).astype(np.int32)


SCENES = {
    "s1500": lambda: make_scene(1500, seed=3)["coords"],           # levels [1493, 302, 40, 6, 2]
    "two_batch": lambda: _random_coords(900, 40, 1, batches=2, negative=True),
    "line37": lambda: np.array([[0, i, 0, 0] for i in range(37)], np.int32),      # 3 groups, 24 of 27 offsets without a pair
    "one": lambda: np.array([[0, 3, 4, 5]], np.int32),
    "outlier": lambda: np.concatenate([_random_coords(700, 24, 4), np.array([[0, 90000, -70000, 5]], np.int32)]),
    "g1024": lambda: _box(16384, 1024),                            # exactly 1024 / 1025 level-0 groups
    "g1025": lambda: _box(16385, 1025),
    "s20000": lambda: make_scene(20000, seed=0)["coords"],         # 20136 rows, 1259 groups
    "w6000": lambda: make_scene(6000, seed=5)["coords"],           # test_gpu_conv.py's world (rounding test)
    "s1500m1": lambda: make_scene(1500, seed=3)["coords"][:-1],    # stem: every n % 4
    "s1500m2": lambda: make_scene(1500, seed=3)["coords"][:-2],
    "s1500m3": lambda: make_scene(1500, seed=3)["coords"][:-3],
    # the forward kernels' edges (test_gpu_conv_edges.py): one 64-row tile less one / exact / plus one, two exact tiles,
    # the 8192-row switch of the 128-column build, 2047 / 2048 level-0 groups
    "box63": lambda: _box(63, 63),
    "box64": lambda: _box(64, 64),
    "box65": lambda: _box(65, 65),
    "box128": lambda: _box(128, 128),
    "box8191": lambda: _box(8191, 8191),
    "box8192": lambda: _box(8192, 8192),
    "g2047": lambda: _box(32752, 2047),
    "g2048": lambda: _box(32768, 2048),
}


class World:
    """One scene with the oracle's levels, the row maps between the two and the internal-row pair lists (cached)."""

    def __init__(self, name):
        self.name = name
        self.coords = np.ascontiguousarray(SCENES[name]())
        self.sc = Scene(torch.from_numpy(self.coords).cuda())
        self.lv = ob.SparseLevels(self.coords)
        self.to_oracle = [internal_to_oracle_rows(self.sc, self.lv, i) for i in range(5)]
        self.to_internal = []
        for m in self.to_oracle:
            inv = np.empty(len(m), np.int64)
            inv[m] = np.arange(len(m))
            self.to_internal.append(inv)
        self._pairs = {}

    def pairs(self, kind, level_in):
        """list over k of (input rows, output rows) of the op, INTERNAL rows, as int64 device tensors"""
        key = (kind, level_in)
        if key not in self._pairs:
            lo = level_in + (1 if kind == "down" else -1 if kind == "up" else 0)
            if kind == "conv3":
                kmap = self.lv.kernel_map(level_in, 3)
            elif kind == "down":
                kmap = self.lv.stride_map(level_in)
            elif kind == "up":
                kmap = [(rc, rf) for (rf, rc) in self.lv.stride_map(level_in - 1)]
            else:
                kmap = [(np.arange(self.lv.n(level_in)), np.arange(self.lv.n(level_in)))]
            self._pairs[key] = _remap(kmap, self.to_internal[level_in], self.to_internal[lo])
        return self._pairs[key]

    def stem_pairs(self, ks):
        """pairs of the input convolution: input rows in the CALLER's order (= the oracle's level 0), output rows internal"""
        key = ("stem", ks)
        if key not in self._pairs:
            n = self.lv.n(0)
            self._pairs[key] = _remap(self.lv.kernel_map(0, ks), np.arange(n), self.to_internal[0])
        return self._pairs[key]


def _remap(kmap, in_rows, out_rows):
    """oracle pairs -> device index tensors through the given row maps"""
    return [(torch.from_numpy(in_rows[np.asarray(ri, np.int64)]).cuda(), torch.from_numpy(out_rows[np.asarray(ro, np.int64)]).cuda())
            for ri, ro in kmap]


_WORLDS = {}


def world(name) -> World:
    """The scenes are built once per process, at first use (a child interpreter builds only what its selection needs)."""
    if name not in _WORLDS:
        _WORLDS[name] = World(name)
    return _WORLDS[name]


def _ints(shape, lo, hi, *seed):
    """integers in [lo, hi] as float32 on the device, from a generator seeded by the case"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))
    return torch.randint(lo, hi + 1, shape, generator=g).float().cuda()
