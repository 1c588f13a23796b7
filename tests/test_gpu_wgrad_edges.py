"""-m gpu: the weight gradient of the sparse convolutions (csrc/wgrad.hip) at its plan, list and shape edges.

a3d_conv_wgrad with a gather table (K = 27 / 8) adds the neighbour table, out_map, the per-offset group lists and the
segment / XCD plan to what the K = 1 linear entry runs; the network-level gradient tests reach it at one scene, one segment
length per shape and a tolerance of 2e-4 of the largest |dW| of all offsets, which hides a dropped or doubled pair.

Reference: the pairs of offset k come from the CPU oracle's kernel maps (oracle.backbone.SparseLevels), remapped to the
library's internal rows by coordinates; ref[k] = x[in rows]^T dy[out rows] in float64.  EXACT tests draw x and dy as integers
in [-3, 3] (stem colours in {0..3}): every product and every partial sum, in any order, is an integer below 2^24 (the largest
map here has 20136 pairs, 20136 x 9 << 2^24), so fp32 arithmetic is exact and the assertion is bit equality -- one missing,
doubled or misplaced pair changes an integer.  dW starts as NaN and the workspace as 0xFF bytes: a partial slot that no
workgroup wrote, or an offset without pairs that is not written as zeros, shows up.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd.engine import Scene
from agile3d_amd.lib import ptr as _ptr, stream as _stream
from conv_kit import _ints, scratch, world
from gpu_util import ERR_FAMILIES, _adversarial_inputs

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = {"conv3": L.OP_CONV3, "down": L.OP_DOWN, "up": L.OP_UP, "linear": L.OP_LINEAR}
KVOL = {"conv3": 27, "down": 8, "up": 8, "linear": 1}
# (kind, level_in) wherever the kind exists
KIND_LEVELS = [(kind, lvl) for kind in KINDS for lvl in range(5)
               if not (kind == "down" and lvl == 4) and not (kind == "up" and lvl == 0)]
WIDTHS_IN = [32, 64, 96, 128, 192, 256, 384]      # the forward suite's width sets (test_gpu_conv.py)
WIDTHS_OUT = [32, 64, 96, 128, 256]
# the pairs that select the 13 channels-per-lane builds of k_wgrad: {32, 64, 96, 128}^2 without (96, 128), (128, 96), (128, 128),
# which repeat a build with two channel blocks (pinned by test_wgrad_plan_host.py::test_the_build_table_of_the_gpu_modules)
BUILD_PAIRS = [(ci, co) for ci in (32, 64, 96, 128) for co in (32, 64, 96, 128) if (ci, co) not in ((96, 128), (128, 96), (128, 128))]
assert len(BUILD_PAIRS) == 13


def _reference(pairs, x, dy):
    """ref[k] = x[in rows]^T dy[out rows] in float64 (gathers and matmuls on the device, index lists from the CPU oracle)"""
    x64, dy64 = x.double(), dy.double()
    ref = torch.zeros(len(pairs), x.shape[1], dy.shape[1], dtype=torch.float64, device="cuda")
    for k, (ri, ro) in enumerate(pairs):
        if len(ri):
            ref[k] = x64[ri].T @ dy64[ro]
    return ref


def _assert_exact(dw, ref, where):
    got = dw.double()
    if torch.equal(got, ref):
        return
    bad = got != ref                                # NaN differs from everything
    k, ci, co = (int(v) for v in bad.nonzero()[0])
    offsets = sorted(set(bad.nonzero()[:, 0].tolist()))
    pytest.fail(f"{where} k={k}: dW[{k}, {ci}, {co}] = {got[k, ci, co].item()!r}, expected {ref[k, ci, co].item()!r}; "
                f"{int(bad.sum())} elements differ, in offsets {offsets}")


def _conv_wgrad(sc, kind, level_in, x, dy, cin, cout, nbytes=None):
    """a3d_conv_wgrad itself on views with unit channel stride: NaN-filled dW, 0xFF-filled workspace."""
    lib = L.load()
    sc.prepare_wgrad()
    code = KINDS[kind]
    if nbytes is None:
        nbytes = lib.a3d_conv_wgrad_workspace_bytes(sc.handle, code, level_in, cin, cout)
        assert nbytes, lib.a3d_last_error().decode()
    ws = scratch(nbytes)
    dw = torch.full((KVOL[kind], cin, cout), NAN, device="cuda")
    L.check(lib.a3d_conv_wgrad(sc.handle, code, level_in, _ptr(x), x.stride(0), _ptr(dy), dy.stride(0), cin, cout, _ptr(dw),
                               _ptr(ws), nbytes, _stream()), "a3d_conv_wgrad")
    return dw


def _rows(w, kind, level_in):
    lo = level_in + (1 if kind == "down" else -1 if kind == "up" else 0)
    return w.sc.n[level_in], w.sc.n[lo]


def _sweep(w, kind, level_in, pairs_cc):
    """Every (cin, cout) of pairs_cc exact: one x / dy / reference at the widest pair, column slices of them per pair."""
    n_in, n_out = _rows(w, kind, level_in)
    cmax_in, cmax_out = max(ci for ci, _ in pairs_cc), max(co for _, co in pairs_cc)
    X = _ints((n_in, cmax_in), -3, 3, w.name, kind, level_in, "x")
    DY = _ints((n_out, cmax_out), -3, 3, w.name, kind, level_in, "dy")
    ref = _reference(w.pairs(kind, level_in), X, DY)
    empty = [k for k, (ri, _) in enumerate(w.pairs(kind, level_in)) if len(ri) == 0]
    for cin, cout in pairs_cc:
        where = f"scene {w.name} {kind} level {level_in} {cin}->{cout}"
        dw = _conv_wgrad(w.sc, kind, level_in, X[:, :cin].contiguous(), DY[:, :cout].contiguous(), cin, cout)
        _assert_exact(dw, ref[:, :cin, :cout], where)
        for k in empty:
            assert (dw[k] == 0).all(), (where, k, "an offset without pairs must be exact zeros")
    return len(empty)


# ----------------------------------------------------------------------------------------------------------------------
# 1. work lists against the group masks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s1500", "two_batch", "line37", "one", "outlier", "g1024", "g1025", "s20000"])
def test_work_lists_are_the_set_bits_of_the_group_masks(name):
    """k_wgrad_lists: for every map and offset k, lists[k, :counts[k]] are the ascending groups whose mask has bit k and
    counts[k] is the popcount (test_scene_tables ties the masks to coordinates).  g1024 / g1025 / s20000 have 1024, 1025
    and 1259 level-0 groups: the second trip of the kernel's 1024-group loop and its carry."""
    w = world(name)
    sc = w.sc
    lists = sc.wgrad_lists()
    tabs = {L.OP_CONV3: L.TAB_GMASK27, L.OP_DOWN: L.TAB_GMASKDOWN, L.OP_UP: L.TAB_GMASKUP}
    assert sorted(lists) == sorted([(L.OP_CONV3, l) for l in range(5)] + [(k, l) for k in (L.OP_DOWN, L.OP_UP) for l in range(4)])
    if name in ("g1024", "g1025"):
        assert (sc.n[0] + 15) // 16 == int(name[1:]) and sc.grid_dims is not None
    for (kind, level), (lst, cnt) in lists.items():
        npos = sc.n[level + 1] if kind == L.OP_DOWN else sc.n[level]
        ng = (npos + 15) // 16
        gm = sc.table(level, tabs[kind])
        assert len(gm) >= ng and not gm[ng:].any(), (name, kind, level, "mask bits past the last group")
        assert lst.shape == (27 if kind == L.OP_CONV3 else 8, (ng + 63) // 64 * 64)
        for k in range(lst.shape[0]):
            want = np.flatnonzero((gm[:ng] >> np.uint32(k)) & 1)
            assert cnt[k] == len(want), (name, kind, level, k, int(cnt[k]), len(want))
            assert np.array_equal(lst[k, :cnt[k]], want), (name, kind, level, k)


# ----------------------------------------------------------------------------------------------------------------------
# 2. every build, kind and level, exact
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,level_in", KIND_LEVELS, ids=[f"{k}-L{l}" for k, l in KIND_LEVELS])
def test_exact_every_width_pair_s1500(kind, level_in):
    """7 x 5 width pairs (every backbone pairing, all 13 builds with a gather table) on the scene whose level 4 has 2 rows,
    whose levels 2-4 have fewer groups than a workgroup has waves and where offsets are absent from whole levels."""
    w = world("s1500")
    if kind == "conv3" and level_in == 0:
        assert w.sc.n == [1493, 302, 40, 6, 2]
    _sweep(w, kind, level_in, [(ci, co) for ci in WIDTHS_IN for co in WIDTHS_OUT])


_SMALL = [(s, k, l) for s in ("s1500", "two_batch", "line37", "one", "outlier") for k, l in KIND_LEVELS]


@pytest.mark.parametrize("name,kind,level_in", _SMALL, ids=[f"{s}-{k}-L{l}" for s, k, l in _SMALL])
def test_exact_13_builds(name, kind, level_in):
    """The 13 build-selecting pairs on negative coordinates and two samples, a line (24 of 27 offsets without a pair: all but the three along it), one
    voxel (only the centre offset has pairs) and a scene whose level 0 sits on the hash table.  (s1500 is here for the child
    interpreters of test_other_segment_lengths_and_the_pointer_build.)"""
    w = world(name)
    if name == "outlier":
        assert w.sc.grid_dims is None
    n_empty = _sweep(w, kind, level_in, BUILD_PAIRS)
    if name == "line37" and kind == "conv3" and level_in == 0:
        assert n_empty == 24 and (w.sc.n[0] + 15) // 16 == 3
    if name == "one" and kind == "conv3":
        assert n_empty == 26


@pytest.mark.parametrize("name", ["g1025", "s20000"])
def test_exact_many_segments_per_offset(name):
    """Level 0 of the large scenes under the cost model's own plan: many segments per offset, lists from both trips of
    k_wgrad_lists' loop."""
    w = world(name)
    _sweep(w, "conv3", 0, [(32, 32)])
    _sweep(w, "conv3", 0, [(96, 96)])
    _sweep(w, "down", 0, [(32, 32)])


def test_second_call_returns_the_same_bits():
    """The plan of a (scene, shape) is cached.  A twin scene of the same coordinates has the same lists, hence the same plan
    and workspace size, under another serial: its FIRST library call for the shape is a3d_conv_wgrad itself (a plan-cache
    miss inside the launch path), the second a hit; both must equal the reference and each other."""
    w = world("s1500")
    twin = Scene(torch.from_numpy(w.coords).cuda())
    lib = L.load()
    for kind, level_in, cin, cout in [("conv3", 0, 96, 96), ("conv3", 2, 64, 128), ("down", 1, 64, 64), ("up", 4, 256, 128),
                                      ("linear", 0, 128, 32)]:
        n_in, n_out = _rows(w, kind, level_in)
        x, dy = _ints((n_in, cin), -3, 3, "twice", kind, "x"), _ints((n_out, cout), -3, 3, "twice", kind, "dy")
        ref = _reference(w.pairs(kind, level_in), x, dy)
        nbytes = lib.a3d_conv_wgrad_workspace_bytes(w.sc.handle, KINDS[kind], level_in, cin, cout)
        assert nbytes
        where = f"scene s1500 (twin) {kind} level {level_in} {cin}->{cout}"
        first = _conv_wgrad(twin, kind, level_in, x, dy, cin, cout, nbytes=nbytes)
        second = _conv_wgrad(twin, kind, level_in, x, dy, cin, cout, nbytes=nbytes)
        _assert_exact(first, ref, where + " first call")
        _assert_exact(second, ref, where + " second call")
        assert torch.equal(first, second)
        assert lib.a3d_conv_wgrad_workspace_bytes(twin.handle, KINDS[kind], level_in, cin, cout) == nbytes


# ----------------------------------------------------------------------------------------------------------------------
# 3. the plan at other segment lengths, and the pointer build
# ----------------------------------------------------------------------------------------------------------------------
def test_other_segment_lengths_and_the_pointer_build():
    """A3D_WGRAD_SEG / A3D_WGRAD_WIDE are read once per process: fresh interpreters, one at a time, run the 13-build exact
    tests on s1500, line37 and one.  Segment length 1: every group its own segment (three of four waves idle in the LDS fold,
    cnt[k] slots per offset, the XCD remainders of seg_lo differ per offset); 3: the last segment of most offsets is short;
    WIDE: the 64-bit pointer build, on the strided operands too."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    select = "test_exact_13_builds and (s1500 or line37 or one)"
    for var, value, expr in [("A3D_WGRAD_SEG", "1", select), ("A3D_WGRAD_SEG", "3", select),
                             ("A3D_WGRAD_WIDE", "1", f"({select}) or test_strided_and_offset_operands")]:
        env = {k: v for k, v in os.environ.items() if k not in ("A3D_WGRAD_SEG", "A3D_WGRAD_WIDE")}
        env[var] = value
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider",
                              "-k", expr], env=env, capture_output=True, text=True, timeout=600, cwd=root)
        print(f"{var}={value}: {out.stdout.strip().splitlines()[-1] if out.stdout.strip() else out.stderr[-300:]}")
        assert out.returncode == 0, (f"{var}={value}", out.stdout[-3000:], out.stderr[-1000:])
        assert " passed" in out.stdout and "skipped" not in out.stdout and "no tests ran" not in out.stdout, out.stdout[-500:]


# ----------------------------------------------------------------------------------------------------------------------
# 4. strided and offset operands
# ----------------------------------------------------------------------------------------------------------------------
def _column_slice(t, ld, c0):
    """t as columns [c0, c0 + width) of a NaN-filled [rows, ld] buffer"""
    wide = torch.full((t.shape[0], ld), NAN, device="cuda")
    wide[:, c0:c0 + t.shape[1]] = t
    return wide[:, c0:c0 + t.shape[1]]


# the up op at every reading of "levels 0 and 3": level_in 3, and the maps owned by fine levels 0 and 3 (level_in 1 and 4)
_STRIDED = [("conv3", 0), ("conv3", 3), ("up", 1), ("up", 3), ("up", 4)]


@pytest.mark.parametrize("kind,level_in", _STRIDED, ids=[f"{k}-L{l}" for k, l in _STRIDED])
def test_strided_and_offset_operands(kind, level_in):
    """x / dy as column slices of wider NaN-filled buffers, as the backbone's concatenation buffers hand them over: leading
    dimensions width + 32 at column 32, and width + 2 at column 2 -- even, no multiple of 4, the base pointer 8-byte aligned
    only (the pointer build's aligned(8) loads depend on the ABI accepting exactly that).  Same bits as the contiguous call,
    equal to the reference; a read outside the slice meets NaN.  Odd leading dimensions are refused."""
    w = world("s1500")
    lib = L.load()
    n_in, n_out = _rows(w, kind, level_in)
    for cin, cout in [(96, 96), (32, 128), (128, 32)]:
        x, dy = _ints((n_in, cin), -3, 3, "strided", kind, level_in, cin, "x"), _ints((n_out, cout), -3, 3, "strided", kind, level_in, cout, "dy")
        ref = _reference(w.pairs(kind, level_in), x, dy)
        plain = _conv_wgrad(w.sc, kind, level_in, x, dy, cin, cout)
        _assert_exact(plain, ref, f"scene s1500 {kind} level {level_in} {cin}->{cout} contiguous")
        for xpad, xc0 in [(32, 32), (2, 2)]:
            for ypad, yc0 in [(32, 32), (2, 2)]:
                xs, dys = _column_slice(x, cin + xpad, xc0), _column_slice(dy, cout + ypad, yc0)
                assert xs.data_ptr() % 8 == 0 and dys.data_ptr() % 8 == 0
                got = _conv_wgrad(w.sc, kind, level_in, xs, dys, cin, cout)
                _assert_exact(got, ref, f"scene s1500 {kind} level {level_in} {cin}->{cout} ldx {cin + xpad} at {xc0}, ldy {cout + ypad} at {yc0}")
                assert torch.equal(got, plain)
        nbytes = lib.a3d_conv_wgrad_workspace_bytes(w.sc.handle, KINDS[kind], level_in, cin, cout)
        ws, dw = scratch(nbytes), torch.full((KVOL[kind], cin, cout), NAN, device="cuda")
        xw, dyw = torch.zeros(n_in, cin + 2, device="cuda"), torch.zeros(n_out, cout + 2, device="cuda")
        for ldx, ldy in [(cin + 1, cout), (cin, cout + 1), (cin + 1, cout + 1)]:
            rc = lib.a3d_conv_wgrad(w.sc.handle, KINDS[kind], level_in, _ptr(xw), ldx, _ptr(dyw), ldy, cin, cout, _ptr(dw), _ptr(ws),
                                    nbytes, _stream())
            assert rc == L.A3D_ERR_INVALID, (ldx, ldy, rc)
        torch.cuda.synchronize()
        assert torch.isnan(dw).all(), "a refused call wrote dW"


# ----------------------------------------------------------------------------------------------------------------------
# 5. stem weight gradient, all routes, exact
# ----------------------------------------------------------------------------------------------------------------------
def _stem_wgrad(sc, feats3, dy, kvol, nbytes):
    lib = L.load()
    ws = scratch(nbytes)
    dw = torch.full((kvol, 3, 32), NAN, device="cuda")
    L.check(lib.a3d_stem_wgrad(sc.handle, _ptr(feats3), _ptr(dy), dy.stride(0), kvol, _ptr(dw), _ptr(ws), nbytes, _stream()),
            "a3d_stem_wgrad")
    return dw


_STEM_SCENES = ["s1500", "two_batch", "g1025", "line37", "one", "outlier", "s1500m1", "s1500m2", "s1500m3"]


@pytest.mark.parametrize("ks", [5, 3])
@pytest.mark.parametrize("name", _STEM_SCENES)
def test_stem_wgrad_every_route_exact(name, ks):
    """a3d_stem_wgrad through the C ABI, colours in {0..3} in the CALLER's row order, dy integers in internal order.  The
    workspace size picks the route: a3d_stem_wgrad_scene_workspace_bytes lets a dense-grid scene run 5^3 on the matrix cores,
    a3d_stem_wgrad_workspace_bytes forces it onto the thread-per-row kernel (3^3 always runs there); a scene without the
    grid (outlier, one, two_batch) takes the hash lookups.  Both sizes must give the reference, hence each other.  g1025
    and s1500 minus 0-3 rows give every n % 4 of the matrix-core kernel's 4-voxel steps; s1500 and outlier also run with
    lddy = 36."""
    w = world(name)
    sc, lib = w.sc, L.load()
    n, kvol = sc.n[0], ks ** 3
    if name == "g1025":
        assert n % 4 == 1 and sc.grid_dims is not None
    if name.startswith("s1500"):
        assert n % 4 == (1493 - int(name[6:] or 0)) % 4 and sc.grid_dims is not None
    if name == "outlier":
        assert sc.grid_dims is None
    feats3 = _ints((n, 3), 0, 3, name, "colours")
    dy = _ints((n, 32), -3, 3, name, "stem dy")
    ref = _reference(w.stem_pairs(ks), feats3, dy)
    small, scene_sized = lib.a3d_stem_wgrad_workspace_bytes(kvol), lib.a3d_stem_wgrad_scene_workspace_bytes(sc.handle, kvol)
    assert small and scene_sized >= small
    results = []
    for lddy in (32, 36) if name in ("s1500", "outlier") else (32,):
        d = dy if lddy == 32 else _column_slice(dy, lddy, 0)
        for nbytes, label in ((scene_sized, "scene-sized workspace"), (small, "fixed-size workspace")):
            dw = _stem_wgrad(sc, feats3, d, kvol, nbytes)
            _assert_exact(dw, ref, f"scene {name} stem {ks}^3 level 0 3->32, lddy {lddy}, {label}")
            results.append(dw)
    assert all(torch.equal(results[0], r) for r in results[1:])


def test_stem_wgrad_refuses_bad_arguments():
    w = world("line37")
    lib = L.load()
    n = w.sc.n[0]
    f, dy, dw = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 36, device="cuda"), torch.full((125, 3, 32), NAN, device="cuda")
    nbytes = lib.a3d_stem_wgrad_workspace_bytes(125)
    ws = scratch(nbytes)
    for lddy, kvol in [(34, 125), (28, 125), (32, 64)]:
        assert lib.a3d_stem_wgrad(w.sc.handle, _ptr(f), _ptr(dy), lddy, kvol, _ptr(dw), _ptr(ws), nbytes, _stream()) == L.A3D_ERR_INVALID
    assert lib.a3d_stem_wgrad(w.sc.handle, _ptr(f), _ptr(dy), 32, 125, _ptr(dw), _ptr(ws), nbytes - 512, _stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(dw).all()


# ----------------------------------------------------------------------------------------------------------------------
# 6. rounding quality on adversarial inputs
# ----------------------------------------------------------------------------------------------------------------------
ROUND_SHAPES = [("conv3", 0, 96, 96), ("conv3", 2, 192, 128), ("conv3", 4, 256, 256), ("down", 0, 32, 32), ("up", 3, 256, 128)]
# allowed multiple of torch's own float32 error per family (see the test's docstring)
ROUND_FACTOR = {family: 4.0 for family in ERR_FAMILIES}


def _adversarial_rows(family, n_in, n_out, cin, cout, seed):
    """(x [n_in, cin], dy [n_out, cout]) of test_gpu_conv.py's families with dy in the role of w.  A weight gradient sums
    over ROWS, so the families' structure along the contraction axis (channels of x / input channels of w there) lies along
    the rows here: cancel = rows in pairs (x, -x) against (dy, dy (1 + u 2^-12)) -- neighbours in the internal row order,
    which the centre offset and many others pair up."""
    e_in, e_out = n_in + (n_in & 1), n_out + (n_out & 1)
    xt, _ = _adversarial_inputs(family, cin, e_in, 2, 1, seed)
    _, wd = _adversarial_inputs(family, 1, e_out, cout, 1, seed + 1)
    return xt.t()[:n_in].contiguous(), wd[0, :n_out].contiguous()


def test_rounding_error_bounds_on_adversarial_inputs():
    """The weight gradient BOUNDED on the five adversarial families, one shape per kind and level class, on the forward
    suite's 6000-voxel world.  Per offset k with P_k > 0 pairs the error |dW - ref| is normalised by the float64 sum of
    |x|^T |dy| over the same pairs (elements where that is positive).

    Hard bound, per offset: (P_k + 1) 2^-24, the a-priori bound of an fp32 sum of P_k rounded products in any order.
    Measured bound, per (shape, family) over its offsets' worst: factor x the error of torch's float32 CPU evaluation of the
    same per-offset sums against the same reference, + 1e-7; factor 4 covers a different but valid summation order (the
    rule of test_gpu_train_primitives._derived_bound).  The comparison is per shape, not per offset: at P_k of one or two a
    fused multiply-add evaluation is exact where two rounded products are not, and a ratio of such errors means nothing.

    Measured on the MI355X (kernel error / torch float32 error, worst shape per family; the kernel's worst normalised error):
    wide 1.00 (3.9e-07)   cancel 0.99 (1.9e-07)   same_sign 0.98 (3.1e-07)   tiny 1.34 (2.1e-07)   subnormal 0.91 (1.7e-07)
    -- no family needs more than the factor of four; the worst ratios all come from conv3 level 4 256 -> 256 (6 rows, P_k <= 6),
    on the longer sums the kernel's error is 0.3 .. 0.9 of torch's.
    """
    w = world("w6000")
    worst, ratios = {}, {}
    for si, (kind, level_in, cin, cout) in enumerate(ROUND_SHAPES):
        n_in, n_out = _rows(w, kind, level_in)
        pairs = w.pairs(kind, level_in)
        for fi, family in enumerate(ERR_FAMILIES):
            x, dy = _adversarial_rows(family, n_in, n_out, cin, cout, 5000 + 100 * si + fi)
            xd, dyd = x.cuda(), dy.cuda()
            dw = _conv_wgrad(w.sc, kind, level_in, xd, dyd, cin, cout)
            name = f"{kind}_L{level_in}_{cin}_{cout}_{family}"
            assert torch.isfinite(dw).all(), name
            ref = _reference(pairs, xd, dyd)
            mag = _reference(pairs, xd.abs(), dyd.abs())
            ek_all = e32_all = 0.0
            for k, (ri, ro) in enumerate(pairs):
                P = len(ri)
                if P == 0:
                    assert (dw[k] == 0).all(), (name, k)
                    continue
                f32 = (x[ri.cpu()].T @ dy[ro.cpu()]).cuda()
                live = mag[k] > 0
                ek = float(((dw[k].double() - ref[k]).abs()[live] / mag[k][live]).max())
                e32 = float(((f32.double() - ref[k]).abs()[live] / mag[k][live]).max())
                assert ek <= (P + 1) * 2.0 ** -24, (name, k, P, ek)
                ek_all, e32_all = max(ek_all, ek), max(e32_all, e32)
            ratio = ek_all / e32_all if e32_all > 0 else 0.0
            print(f"{name:34s} kernel {ek_all:.3e}  torch float32 {e32_all:.3e}  ratio {ratio:.2f}  (of sum|x||dy|)")
            worst.setdefault(family, []).append((ek_all, name))
            ratios.setdefault(family, []).append((ratio, name))
            assert ek_all <= ROUND_FACTOR[family] * e32_all + 1e-7, (name, ek_all, e32_all, ROUND_FACTOR[family])
    for family in ERR_FAMILIES:
        err, name = max(worst[family])
        r, rname = max(ratios[family])
        print(f"{family}: worst {err:.3e} ({name}); worst ratio to torch float32 {r:.2f} ({rname})")
