"""Scenes and references shared by the exact sparse-convolution tests (test_gpu_wgrad_edges.py, test_gpu_conv_edges.py,
test_gpu_conv_train_edges.py) and the CPU-side plan-class test: named scenes, the World of a scene (oracle levels, row maps
both ways, internal-row pair lists from the CPU oracle's kernel maps), seeded integer operands, and what the two forward
modules share (reference, bit equality, profile entries).  The coordinate builders need no GPU; a World does."""
import zlib

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
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
    # the training builds' edges (test_gpu_conv_train_edges.py): 63 / 64 per-tile partials (64-row tiles) and 63 / 64
    # per-group partials (16-row groups of k_conv_wl) -- where bn_sums_from_partials changes its kernel
    "box4032": lambda: _box(4032, 4032),
    "box4096": lambda: _box(4096, 4096),
    "box1008": lambda: _box(1008, 1008),
    "box1024": lambda: _box(1024, 1024),
}


# level sizes by the CPU oracle; both test modules assert them, so that a change of make_scene or of the oracle cannot
# silently move a case off its edge
SCENE_LEVELS = {
    "one": [1, 1, 1, 1, 1],
    "line37": [37, 19, 10, 5, 3],
    "box63": [63, 63, 62, 54, 26],
    "box64": [64, 64, 63, 56, 25],
    "box65": [65, 65, 65, 61, 25],
    "box128": [128, 127, 123, 101, 27],
    "outlier": [701, 582, 208, 28, 9],
    "two_batch": [1800, 1721, 1198, 404, 118],
    "s1500": [1493, 302, 40, 6, 2],
    "box8191": [8191, 6362, 1718, 216, 27],
    "box8192": [8192, 6328, 1714, 216, 27],
    "g1024": [16384, 10009, 1728, 216, 27],
    "g1025": [16385, 10054, 1728, 216, 27],
    "s20000": [20136, 4349, 942, 184, 40],
    "g2047": [32752],                              # level 0 only (32 -> 32 layers)
    "g2048": [32768],
    "box4032": [4032],                             # level 0 only: 63 / 64 tiles of 64 rows, 63 / 64 groups of 16 rows
    "box4096": [4096],                             # (the training builds' per-block partials, TRAIN_BOX_CASES)
    "box1008": [1008],
    "box1024": [1024],
}

KVOL = {"conv3": 27, "down": 8, "up": 8, "linear": 1}      # linear: A3D_OP_LINEAR, the rows of LINEAR_CASES only


def level_out(kind, level_in):
    return level_in + (1 if kind == "down" else -1 if kind == "up" else 0)


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


# ---- shared by the exact forward modules (test_gpu_conv_edges.py: the inference builds, test_gpu_conv_train_edges.py: the
# training builds): the a3d_conv_deep_mode fixture, case-table worlds and operands, the float64 reference, bit equality, the
# profile entry of a launch against its declared plan class.
KINDS = {"conv3": L.OP_CONV3, "down": L.OP_DOWN, "up": L.OP_UP, "linear": L.OP_LINEAR}


@pytest.fixture(params=[1, 0], ids=["deep", "streamk"])
def mode(request):
    """a3d_conv_deep_mode: with the small-level kernel (k_conv_deep takes what its cost model allows) and without."""
    lib = L.load()
    before = lib.a3d_conv_deep_mode(request.param)
    yield request.param
    lib.a3d_conv_deep_mode(before)


def _set_mode(m):
    return L.load().a3d_conv_deep_mode(m)


def _world(name):
    w = world(name)
    want = SCENE_LEVELS[name]
    assert w.sc.n[:len(want)] == want and [w.lv.n(i) for i in range(len(want))] == want, (name, w.sc.n)
    if name == "outlier":
        assert w.sc.grid_dims is None                                 # level 0 on the hash table
    return w


def _rows(w, kind, level_in):
    return w.sc.n[level_in], w.sc.n[level_out(kind, level_in)]


def _conv_ref(pairs, x64, w64, n_out):
    """sum_k index_add(out rows_k, x[in rows_k] @ W[k]) in float64 on the device"""
    ref = torch.zeros(n_out, w64.shape[2], dtype=torch.float64, device="cuda")
    for k, (ri, ro) in enumerate(pairs):
        if len(ri):
            ref.index_add_(0, ro, x64[ri] @ w64[k])
    return ref


def _assert_bits(got, ref64, where):
    """got (fp32) == the float64 reference cast to fp32, element for element"""
    ref = ref64.float()
    assert (ref.double() == ref64).all(), (where, "the reference left the exact range")
    if torch.equal(got, ref):
        return
    bad = got != ref                                # NaN differs from everything
    r, c = (int(v) for v in bad.nonzero()[0])
    rows = bad.any(1).nonzero().flatten()
    pytest.fail(f"{where}: out[{r}, {c}] = {got[r, c].item()!r}, expected {ref[r, c].item()!r}; {int(bad.sum())} elements differ "
                f"in {len(rows)} rows ({rows[:8].tolist()} ...), columns {bad.any(0).nonzero().flatten()[:8].tolist()} ...")


def _with_zero_row(t):
    return torch.cat([t, torch.zeros(1, t.shape[1], device="cuda")])


def _row_id(row):
    name, kind, level_in, cin, cout, cin2, m = row
    return f"{name}-{kind}-L{level_in}-{cin}-{cout}" + (f"+{cin2}" if cin2 else "") + ("-deep" if m else "-streamk")


def _operands(w, kind, level_in, cin, cout, tag, lo=-3, hi=3):
    n_in, n_out = _rows(w, kind, level_in)
    x = _with_zero_row(_ints((n_in, cin), lo, hi, w.name, kind, level_in, cin, tag, "x"))
    W = _ints((KVOL[kind], cin, cout), lo, hi, w.name, kind, level_in, cin, cout, tag, "w")
    ref = _conv_ref(w.pairs(kind, level_in), x.double(), W.double(), n_out)
    return x, W, ref


def _profiled(run):
    """the spconv profile entries of the launches inside run()"""
    lib = L.load()
    lib.a3d_profile_read(None, 0)
    lib.a3d_profile_enable(1)
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        lib.a3d_profile_enable(0)
    buf = (L.ProfEntry * 64)()
    n = lib.a3d_profile_read(buf, 64)
    assert n >= 0, lib.a3d_last_error().decode()
    return out, [(buf[i].bn, buf[i].ksplit, buf[i].kernel_volume & 255, buf[i].cin, buf[i].cout, buf[i].n_out) for i in range(n)
                 if buf[i].id == 0]


def _assert_ran_its_class(entries, cls, K, cin, cout, n_out, where):
    """the profile entry carries the small-level kernel (column field >= 1000) or not, the column width, the stage width"""
    assert len(entries) == 1, (where, entries)
    if cls[0] == "wl":
        want = (cout, 0)                                             # stage width 0: k_conv_wl
    elif cls[0] == "deep":
        want = (1000 + cls[2], cls[3])
    else:
        want = (cls[2], cls[3])
    assert entries[0] == want + (K, cin, cout, n_out), (where, cls, entries[0])
