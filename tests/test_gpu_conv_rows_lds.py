"""-m gpu: k_conv_sk (csrc/spconv.hip) where its neighbour rows come from.

The kernel keeps the K x 64 neighbour rows of a tile in an LDS block behind the weight ring (fetched by LDS-DMA, one round trip
per tile) and reads them with ds_read_b32 in the stage loop; with two blocks the NEXT tile's rows and group masks are requested
beside the first stage of the current tile.  What can go wrong there: a block read before its DMA has landed or rewritten while
a wave still reads it, the wrong tile's block after a tile the workgroup skipped, the first row read of a part that begins
inside a tile (not at offset 0, not at channel chunk 0), the tail piece of a table whose K is no multiple of four (27), the
layers without a table (1x1) and the fused projection's "offset 27", which compute their rows, the builds with one block
(STATS builds of the 96-column kernel) or none (64 x 96).

Everything runs with the small-level kernel switched off (a3d_conv_deep_mode 0), so that small scenes reach k_conv_sk.

Reference: conv_kit's float64 gathered convolution on integer operands (exact in fp32 whatever the partition: every assertion
is bit equality, as in test_gpu_conv_edges.py).  Integers cannot show a changed ORDER of summation; that is what the second
library is for: with A3D_LIB_PATH naming another build of the library (the parent commit's), the package runs on that one, and
test_equal_bits_with_the_other_build runs the same launches on Gaussian operands through the library built in the tree as
well and asks for equal bits."""
import ctypes
import os

import numpy as np
import pytest
import torch

import conv_edge_cases as E
from agile3d_amd import lib as L
from agile3d_amd.engine import Scene
from agile3d_amd.lib import ptr as _ptr, stream as _stream
from conv_kit import (KINDS, KVOL, World, _assert_bits, _box, _conv_ref, _ints, _profiled, _rows, _with_zero_row, _world,
                      internal_to_oracle_rows, scratch)
from gpu_util import pack_weight
from oracle import backbone as ob
from test_gpu_conv_edges import Program
from test_gpu_conv_train_edges import BnOperands, BwOperands, _dgrad_call, _forward_call

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(autouse=True)
def streamk():
    lib = L.load()
    before = lib.a3d_conv_deep_mode(0)
    yield
    lib.a3d_conv_deep_mode(before)


# ---- scenes of this module (conv_kit's named scenes beside them) -------------------------------------------------------
def _apart(n):
    """n voxels four cells apart on a line: no voxel has a neighbour, every tile has ONE present offset (the centre)"""
    return np.array([[0, 4 * i, 0, 0] for i in range(n)], np.int32)


def _cube(e):
    """a dense e^3 cube: the interior voxels have all 27 neighbours"""
    g = np.arange(e)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([np.zeros((len(xyz), 1), np.int64), xyz], 1).astype(np.int32)


_LOCAL = {"box129": lambda: _box(129, 129), "apart70": lambda: _apart(70), "cube8": lambda: _cube(8)}
_LOCAL_WORLDS = {}


class _LocalWorld(World):
    def __init__(self, name):
        self.name = name
        self.coords = np.ascontiguousarray(_LOCAL[name]())
        self.sc = Scene(torch.from_numpy(self.coords).cuda())
        self.lv = ob.SparseLevels(self.coords)
        self.to_oracle = [internal_to_oracle_rows(self.sc, self.lv, i) for i in range(5)]
        self.to_internal = []
        for m in self.to_oracle:
            inv = np.empty(len(m), np.int64)
            inv[m] = np.arange(len(m))
            self.to_internal.append(inv)
        self._pairs = {}


def _w(name):
    if name in _LOCAL:
        if name not in _LOCAL_WORLDS:
            _LOCAL_WORLDS[name] = _LocalWorld(name)
        return _LOCAL_WORLDS[name]
    return _world(name)


def _offsets_per_tile(w, kind, level_in):
    """present offsets of every 64-row output tile (what the kernel takes from the group masks), from the oracle's pairs"""
    _, n_out = _rows(w, kind, level_in)
    cnt = torch.zeros((n_out + 63) // 64, dtype=torch.int64)
    for _, ro in w.pairs(kind, level_in):
        if len(ro):
            cnt[torch.unique(ro.cpu() // 64)] += 1
    return cnt


def _operands(w, kind, level_in, cin, cout, tag):
    n_in, n_out = _rows(w, kind, level_in)
    x = _with_zero_row(_ints((n_in, cin), -3, 3, w.name, kind, level_in, cin, tag, "x"))
    W = _ints((KVOL[kind], cin, cout), -3, 3, w.name, kind, level_in, cin, cout, tag, "w")
    return x, W, _conv_ref(w.pairs(kind, level_in), x.double(), W.double(), n_out)


def _apply(lib, sc, kind, level_in, x, cin, cout, wp, n_out):
    """a3d_conv_apply of `lib` on a NaN-filled y and a 0xFF-filled workspace"""
    nbytes = lib.a3d_conv_apply_workspace_bytes(sc.handle, KINDS[kind], level_in, cin, cout)
    assert nbytes, lib.a3d_last_error().decode()
    ws = scratch(nbytes)
    y = torch.full((n_out + 1, cout), NAN, device="cuda")
    rc = lib.a3d_conv_apply(sc.handle, KINDS[kind], level_in, _ptr(x), x.stride(0), cin, _ptr(wp), cout, _ptr(y), cout, 1, _ptr(ws),
                            nbytes, _stream())
    assert rc == 0, (rc, lib.a3d_last_error().decode())
    return y


def _run_exact(name, kind, level_in, cin, cout, build=None):
    """one launch against the float64 reference, the same launch again for equal bits; build = (bn, ch): what must have run"""
    w = _w(name)
    _, n_out = _rows(w, kind, level_in)
    x, W, ref = _operands(w, kind, level_in, cin, cout, "rows")
    wp = pack_weight(W)
    where = f"scene {name} {kind} level {level_in} {cin}->{cout}"
    y, entries = _profiled(lambda: _apply(L.load(), w.sc, kind, level_in, x, cin, cout, wp, n_out))
    assert len(entries) == 1 and entries[0][0] < 1000 and entries[0][1] > 0, (where, "not k_conv_sk", entries)
    if build is not None:
        assert entries[0][:2] == build, (where, entries)
    _assert_bits(y[:n_out], ref, where)
    assert (y[n_out] == 0).all(), (where, "zero row")
    y2 = _apply(L.load(), w.sc, kind, level_in, x, cin, cout, wp, n_out)
    assert torch.equal(y, y2), (where, "the same launch twice")


# ---- 1. row counts: one row, a partial tile, one tile, a one-row second tile, three tiles (both blocks, in use again) -----
_ROWS = [("one", 1), ("box63", 63), ("box64", 64), ("box65", 65), ("box129", 129)]


@pytest.mark.parametrize("kind,level_in", [("conv3", 0), ("down", 0), ("up", 1)])
@pytest.mark.parametrize("name,n", _ROWS, ids=[s for s, _ in _ROWS])
def test_row_counts_and_table_kinds(name, n, kind, level_in):
    """n_out = 1, 63, 64, 65, 129 (conv3 and up; down: the level below) for the three table kinds at their own K: 27 (seven
    DMA pieces, the last one three offsets and a repeat), 8 and 8; 96 and 128 input channels: 3 and 4 stages per offset"""
    w = _w(name)
    assert w.sc.n[0] == n
    for cin in (96, 128):
        _run_exact(name, kind, level_in, cin, 96, (96, 32))


# ---- 2. one present offset per tile, all 27 ------------------------------------------------------------------------------
def test_one_present_offset_per_tile():
    w = _w("apart70")
    assert _offsets_per_tile(w, "conv3", 0).tolist() == [1, 1]
    _run_exact("apart70", "conv3", 0, 96, 96, (96, 32))
    _run_exact("apart70", "conv3", 0, 128, 128)


def test_all_27_offsets_present():
    w = _w("cube8")
    cnt = _offsets_per_tile(w, "conv3", 0)
    assert len(cnt) == 8 and int((cnt == 27).sum()) >= 2, cnt.tolist()
    _run_exact("cube8", "conv3", 0, 96, 96, (96, 32))
    _run_exact("cube8", "conv3", 0, 128, 96, (96, 32))


# ---- 3. shares that cut a tile inside an offset --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return E.build_planner(str(tmp_path_factory.mktemp("conv_plan")))


def _cuts_inside_an_offset(w, kind, level_in, cin, cout, planner):
    """The share boundaries of the launch that fall inside an offset of a tile (a part whose first stage is channel chunk
    s0 % nchunk != 0), by the kernel's own arithmetic: cost of a tile = present offsets x nchunk + ov, share w begins at
    tot w / G.  96-column build with 32-channel stages: nchunk = cin / 32, ov = 3 (48 MFMAs per stage)."""
    levels = [w.sc.n[i] for i in range(5)]
    plan = E.run_planner(planner, [E.op_query(levels, kind, level_in, cin, cout, 0)])[0]
    assert (plan["family"], plan["bn"], plan["ch"], plan["handoff"], plan["n_cblk"]) == ("sk", 96, 32, 1, 1), plan
    nchunk, ov = cin // 32, 3
    cost = _offsets_per_tile(w, kind, level_in) * nchunk + ov
    assert len(cost) == plan["ntile"]
    pre = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(cost, 0)])
    tot, G = int(pre[-1]), min(plan["G"], int(pre[-1]))
    inside = 0
    for wg in range(1, G):
        lo = tot * wg // G
        t = int(torch.searchsorted(pre, lo, right=True)) - 1
        s0 = lo - int(pre[t]) - ov
        if 0 < s0 < int(cost[t]) - ov and s0 % nchunk:
            inside += 1
    return inside, G


@pytest.mark.parametrize("cin", [96, 128])
@pytest.mark.parametrize("name", ["box129", "two_batch"])
def test_share_cut_inside_an_offset(name, cin, planner):
    """Three tiles on 8+ workgroups and 29 tiles on 100+: parts whose first row read is not offset 0 of their tile and whose
    first stage is not chunk 0 of its offset"""
    w = _w(name)
    inside, G = _cuts_inside_an_offset(w, "conv3", 0, cin, 96, planner)
    assert inside >= 2, (name, cin, inside, G)
    _run_exact(name, "conv3", 0, cin, 96, (96, 32))


# ---- 4. other builds: 128 columns (PAIR 0 and 1), 64 x 64, 64 x 96 (no block), 32 columns --------------------------------
_BUILDS = [("box8191", "conv3", 0, 32, 128, (128, 32)),     # <128, 32, 0>
           ("box8192", "conv3", 0, 32, 128, (128, 32)),     # <128, 32, 1>: the low-register build from 8192 rows on
           ("box8192", "up", 1, 32, 128, (128, 32)),        # ... at K = 8
           ("two_batch", "conv3", 0, 64, 64, (64, 64)),     # <64, 64, 0>
           ("two_batch", "conv3", 0, 96, 64, (64, 96)),     # <64, 96, 0>: the rows stay in global memory
           ("two_batch", "conv3", 0, 32, 64, (64, 32)),     # <64, 32, 0>
           ("two_batch", "conv3", 0, 96, 32, (32, 96)),     # <32, 96, 0>
           ("two_batch", "down", 0, 64, 32, (32, 64))]      # <32, 64, 0> at K = 8


@pytest.mark.parametrize("name,kind,level_in,cin,cout,build", _BUILDS, ids=[f"{r[0]}-{r[1]}-{r[3]}-{r[4]}" for r in _BUILDS])
def test_other_builds(name, kind, level_in, cin, cout, build):
    _run_exact(name, kind, level_in, cin, cout, build)


# ---- 5. a 1x1 layer: no table, rows computed -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box65", "box129"])
def test_linear_layer_without_a_table(name):
    _run_exact(name, "linear", 0, 128, 96, (96, 32))
    _run_exact(name, "linear", 0, 32, 32, (32, 32))


# ---- 6. the fused projection: offset 27 after the tile's own offsets, rows computed --------------------------------------
@pytest.mark.parametrize("cin,cout,cin2", [(96, 96, 32), (96, 96, 128), (128, 128, 64)])
@pytest.mark.parametrize("name", ["box65", "box129"])
def test_fused_projection(name, cin, cout, cin2):
    w = _w(name)
    n = w.sc.n[0]
    x = _with_zero_row(_ints((n, cin), -3, 3, name, cin, "proj x"))
    x2 = _ints((n, cin2), -3, 3, name, cin2, "proj x2")
    W = _ints((27, cin, cout), -3, 3, name, cin, cout, "proj w")
    Wp = _ints((1, cin2, cout), -3, 3, name, cin2, cout, "proj wp")
    shift = _ints((cout,), -3, 3, name, cout, "proj shift")
    ref = torch.relu(_conv_ref(w.pairs("conv3", 0), x.double(), W.double(), n) + x2.double() @ Wp[0].double() + shift.double())
    both = torch.cat([pack_weight(W), pack_weight(Wp)]).contiguous()
    outs = []
    for _ in range(2):
        op = Program(w.sc, L.OP_CONV3, 0, cin, cout, 27, both, None, shift, relu=True, proj_cin=cin2, proj_pad=32)
        op.fill(0, x[:n])
        op.fill(op.proj_buf, x2, 32)
        _, entries = _profiled(op.run)
        assert len(entries) == 1, entries                    # one launch: the projection ran inside the conv
        outs.append(op.buffer(1).clone())
    where = f"scene {name} conv3 level 0 {cin}->{cout} (+{cin2})"
    _assert_bits(outs[0][:n], ref, where)
    assert (outs[0][n] == 0).all(), (where, "zero row")
    assert torch.equal(outs[0], outs[1]), (where, "the same launch twice")


# ---- 7. the training builds: STATS = 1 (one block beside the 96-column ring), STATS = 2 ----------------------------------
@pytest.mark.parametrize("name", ["box129", "two_batch"])
def test_stats_builds(name):
    w = _w(name)
    kind, level_in, cin, cout = "conv3", 0, 96, 96
    _, n_out = _rows(w, kind, level_in)
    x, W, ref = _operands(w, kind, level_in, cin, cout, "stats")
    wp = pack_weight(W)
    where = f"scene {name} {cin}->{cout}"
    bn = BnOperands(n_out, cout, name, "rows bn")
    raw, mean, _, _, _, _ = _forward_call(w, kind, level_in, x, cin, wp, cout, bn, True)
    _assert_bits(raw, ref, where + " STATS 1: raw")
    assert 64 * ref.abs().max().item() < 2 ** 24            # per-tile sums are exact: one rounding, in the division
    assert torch.equal(mean, (ref.sum(0) / n_out).float()), (where, "STATS 1: save_mean")
    raw2, mean2, _, _, _, _ = _forward_call(w, kind, level_in, x, cin, wp, cout, bn, False)
    assert torch.equal(raw, raw2) and torch.equal(mean, mean2), (where, "STATS 1 twice")
    bw = BwOperands(n_out, cout, name, "rows bw")
    g_ref = (ref + bw.prev.double()) * bw.mask
    gbuf, sums = _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, 1, 1, True)
    _assert_bits(gbuf[:n_out, 32:32 + cout].contiguous(), g_ref, where + " STATS 2: g")
    # terms are multiples of 1/2: a 64-row partial is exact in fp32 while 128 x the largest |term| stays below 2^24
    assert 2 * 64 * max(g_ref.abs().max().item(), (g_ref * bw.xhat).abs().max().item()) < 2 ** 24
    assert torch.equal(sums, torch.stack([g_ref.sum(0), (g_ref * bw.xhat).sum(0)])), (where, "STATS 2: sums")
    gbuf2, sums2 = _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, 1, 1, False)
    assert torch.equal(gbuf[:, 32:32 + cout], gbuf2[:, 32:32 + cout]) and torch.equal(sums, sums2), (where, "STATS 2 twice")


# ---- 8. equal bits with another build of the library ---------------------------------------------------------------------
_IN_TREE = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "libagile3d_hip.so")
_BITS = [("box129", "conv3", 0, 96, 96), ("box129", "conv3", 0, 128, 96), ("two_batch", "conv3", 0, 96, 96),
         ("two_batch", "conv3", 0, 128, 96), ("two_batch", "down", 0, 96, 96), ("two_batch", "up", 1, 96, 96),
         ("two_batch", "conv3", 0, 64, 64), ("two_batch", "conv3", 0, 96, 64), ("box8192", "conv3", 0, 32, 128),
         ("s20000", "conv3", 0, 128, 96), ("s20000", "conv3", 0, 96, 96), ("box65", "linear", 0, 128, 96)]


def test_equal_bits_with_the_other_build():
    """Gaussian x and W: a sum taken in another order rounds differently.  The scene handle is the first library's; the two
    builds differ in spconv.hip alone and share the handle's layout."""
    other_path = os.environ.get("A3D_LIB_PATH")
    if not other_path or os.path.realpath(other_path) == os.path.realpath(_IN_TREE):
        pytest.skip("A3D_LIB_PATH names no second build of the library")
    mine = L.load()                                        # the build A3D_LIB_PATH names
    tree = ctypes.CDLL(_IN_TREE)
    for fn in ("a3d_conv_apply_workspace_bytes", "a3d_conv_apply", "a3d_conv_deep_mode", "a3d_last_error"):
        getattr(tree, fn).argtypes, getattr(tree, fn).restype = getattr(mine, fn).argtypes, getattr(mine, fn).restype
    before = tree.a3d_conv_deep_mode(0)
    try:
        for name, kind, level_in, cin, cout in _BITS:
            w = _w(name)
            n_in, n_out = _rows(w, kind, level_in)
            g = torch.Generator().manual_seed(cin * 1000 + cout)
            x = _with_zero_row(torch.randn(n_in, cin, generator=g).cuda())
            wp = pack_weight(torch.randn(KVOL[kind], cin, cout, generator=g).cuda())
            ya = _apply(mine, w.sc, kind, level_in, x, cin, cout, wp, n_out)
            yb = _apply(tree, w.sc, kind, level_in, x, cin, cout, wp, n_out)
            diff = (ya[:n_out] - yb[:n_out]).abs().max().item()
            print(f"   {name} {kind} L{level_in} {cin}->{cout}: max |diff| between the builds {diff!r}")
            assert torch.equal(ya, yb), (name, kind, level_in, cin, cout, diff)
    finally:
        tree.a3d_conv_deep_mode(before)
