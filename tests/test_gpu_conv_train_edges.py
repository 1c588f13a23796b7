"""-m gpu: the TRAINING builds of the sparse-convolution kernels (csrc/spconv.hip: k_conv_sk, k_conv_deep, k_conv_wl with
STATS = 1 and STATS = 2) at their plan and scene edges.

Every kernel family is compiled three times.  STATS = 0 is the inference build (test_gpu_conv_edges.py).  STATS = 1 is the
build behind a3d_conv_bn_train_forward: its epilogue also writes, per 64-row tile (16-row group for k_conv_wl) and column,
the sum of the tile's rows and their squared deviations from the tile mean, which k_bn_combine_tiles (bnorm.hip) merges.
STATS = 2 is the build behind a3d_conv_dgrad_bn: its epilogue adds the gradient already in the buffer, masks by y > 0,
stores g and writes per-tile sums of g and g * xhat, which bn_sums_from_partials folds (k_col_final<16, 1> below 64 blocks,
k_col_final<256, 4> from 64 on).  These are separate code objects, their epilogues compiled from one source: the helpers above
k_conv_sk in spconv.hip, which k_conv_deep and k_conv_wl call for both builds and k_conv_sk for STATS = 2 and for the write of
a tile's partials (its STATS = 1 statistics and its plain epilogue stand spelled out in the kernel); plan_conv picks their class
exactly as it does for the inference build (test_conv_plan_classes.py holds that), so the class tables of conv_edge_cases.py
apply, and the cases here are the ones of the forward module plus 63 / 64-block scenes and 1x1 rows.

The C entry points are called through lib.py on the test's own buffers: every output starts as NaN, every workspace as 0xFF
bytes, the hand-off state is the library's (state_dev = NULL) or a zeroed block of the test's whose failure word must still
be 0 afterwards.

EXACT arithmetic, as in the forward module: all operands are small integers (rstd and the sums' terms: multiples of 1/2), so
`raw`, `g`, every per-block partial sum and the float64 totals are exact whatever the partition, the hand-off order or the
MFMA association.  raw, save_mean, g and the backward sums are asserted BIT FOR BIT against float64 references built from
the CPU oracle's pair lists.  save_rstd, y and the running statistics go through 1 / sqrtf and fp32 products: they are held
to the bounds of test_gpu_backward.py's _check_conv_bn_unit (the running mean to 2e-6 of max(1, max |mean|), not of
max(1, max |raw|) as there: the tighter of the two); dx / dgamma / dbeta of a3d_bn_backward_apply on the sums to
the bounds of test_gpu_train_primitives.py.  The worst observed ratio to each bound is printed per test and, with
A3D_CONV_TRAIN_REPORT=<file>, written with the (mode, class) -> rows table to that file (profiles/conv_train_edge_classes.txt).
"""
import os

import numpy as np
import pytest
import torch

import conv_edge_cases as E
from agile3d_amd import lib as L
from agile3d_amd.lib import ptr as _ptr, stream as _stream
from conv_kit import (KINDS, _assert_bits, _assert_ran_its_class, _conv_ref, _ints, _operands, _profiled, _row_id, _rows, _set_mode,
                      _with_zero_row, _world, mode, scratch)  # noqa: F401  (mode: the a3d_conv_deep_mode fixture)
from gpu_util import pack_weight

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = float(np.float32(1e-5))                      # the fp32 number the library is handed, in the references too
MOMENTUM = 0.5
ERR_INVALID, ERR_WORKSPACE = -1, -5                # include/agile3d_hip.h


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _pick(values, shape, *seed):
    return torch.tensor(values, device="cuda")[_ints(shape, 0, len(values) - 1, *seed).long()].contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# the report: which (stats, mode, class) ran on which rows, the worst ratio to each tolerance-checked bound
# ----------------------------------------------------------------------------------------------------------------------
_RAN = set()                 # (stats, (scene, kind, level_in, cin, cout, 0, mode))
_WORST = {}                  # bound name -> (ratio, where)
_BOUNDS = ["forward rstd 2e-5", "forward y 5e-5 of scale", "forward running_var 2e-5 of scale", "forward running_mean 2e-6 of scale",
           "backward dx 5e-5 of scale", "backward dgamma 2e-4 of scale", "backward dbeta 2e-4 of scale"]


def _ratio(name, err, bound, where, seen):
    r = float(err) / bound
    seen[name] = max(seen.get(name, 0.0), r)
    if r > _WORST.get(name, (-1.0, ""))[0]:
        _WORST[name] = (r, where)
    return r


def _show(seen):
    print("   worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in seen.items()))


def _class_name(cls):
    if cls[0] == "wl":
        return f"k_conv_wl K={cls[1]}"
    if cls[0] == "deep":
        return f"k_conv_deep K={cls[1]} <{cls[2]},{cls[3]}> D={cls[4]} P{'>1' if cls[5] else '=1'} G{'>256' if cls[6] else '<=256'}"
    return (f"k_conv_sk K={cls[1]} <{cls[2]},{cls[3]},{cls[4]}> {'hand-offs' if cls[5] else 'whole tiles'}"
            f"{' G at cap' if cls[6] else ''}{' 64-column second pass' if cls[7] else ''}")


def _build_name(cls):
    if cls[0] == "wl":
        return "k_conv_wl"
    if cls[0] == "deep":
        return f"k_conv_deep<{cls[2]},{cls[3]}> D={cls[4]}"
    return f"k_conv_sk<{cls[2]},{cls[3]},{cls[4]}>"


def _write_report(path, workdir):
    ran = sorted(_RAN)
    exe = E.build_planner(workdir)
    plans = E.run_planner(exe, [E.row_query(row, stats=s) for s, row in ran])
    by_class, by_build = {}, {}
    for (s, row), p in zip(ran, plans):
        cls = E.plan_class(p, E.row_query(row))
        size = "small" if E.SCENE_LEVELS[row[0]][0] < 4096 else "large"
        by_class.setdefault((s, row[6], _class_name(cls)), []).append(row)
        by_build.setdefault((s, _build_name(cls)), {"small": [], "large": []})[size].append(row)
    out = ["# The training builds of the sparse-convolution kernels (STATS = 1: a3d_conv_bn_train_forward, STATS = 2:",
           "# a3d_conv_dgrad_bn) as tests/test_gpu_conv_train_edges.py ran them.  Classes by the planning block of spconv.hip",
           "# compiled as a host program (tests/conv_plan_main.cpp) with ConvShape.stats set; the table rows also assert their",
           "# class from the launch's profile entry.  Written by the module itself:",
           "#   A3D_CONV_TRAIN_REPORT=profiles/conv_train_edge_classes.txt pytest -m gpu tests/test_gpu_conv_train_edges.py",
           "#", "# 1. Builds: rows on scenes below 4096 level-0 voxels (small) and from 4096 on (large), one example each"]
    for (s, b), d in sorted(by_build.items()):
        ex = " | ".join(f"{k} {len(v):5d}" + (f" e.g. {_row_id(v[0])}" if v else "") for k, v in d.items())
        out.append(f"STATS {s} | {b:32s} | {ex}")
    out += ["#", "# 2. Worst observed error as a fraction of each tolerance-checked bound (1.0 = at the bound), and where"]
    for name in _BOUNDS:
        r, where = _WORST.get(name, (float("nan"), "not run"))
        out.append(f"{name:36s} {r:8.4f}   {where}")
    out += ["#", "# 3. (STATS, a3d_conv_deep_mode, class): rows that ran it, the first three"]
    for (s, m, c), rows in sorted(by_class.items()):
        out.append(f"STATS {s} | mode {m} | {c:72s} | {len(rows):5d} rows | " + ", ".join(_row_id(r) for r in rows[:3]))
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


@pytest.fixture(scope="module", autouse=True)
def _report(tmp_path_factory):
    yield
    path = os.environ.get("A3D_CONV_TRAIN_REPORT")
    if path and _RAN:
        _write_report(path, str(tmp_path_factory.mktemp("conv_plan")))


# ----------------------------------------------------------------------------------------------------------------------
# a) a3d_conv_bn_train_forward (STATS = 1)
# ----------------------------------------------------------------------------------------------------------------------
class BnOperands:
    """gamma in {-2, -1, 1, 2}, integer beta, residual and running statistics for `width` columns; narrower ops slice."""

    def __init__(self, n_out, width, *seed):
        self.gamma = _pick([-2.0, -1.0, 1.0, 2.0], (width,), *seed, "gamma")
        self.beta = _ints((width,), -3, 3, *seed, "beta")
        self.res = _ints((n_out, width), -3, 3, *seed, "res")
        self.rm = _ints((width,), -3, 3, *seed, "running mean")
        self.rv = _ints((width,), 0, 3, *seed, "running var")


def _forward_call(w, kind, level_in, x, cin, wp, cout, bn, own_state):
    """one a3d_conv_bn_train_forward on NaN outputs and a 0xFF workspace -> (raw, mean, rstd, ybuf, rm, rv)"""
    lib = L.load()
    _, n_out = _rows(w, kind, level_in)
    nbytes = lib.a3d_conv_bn_train_workspace_bytes(w.sc.handle, KINDS[kind], level_in, cin, cout)
    assert nbytes, lib.a3d_last_error().decode()
    ws = scratch(nbytes)
    raw, mean, rstd = _nan(n_out, cout), _nan(cout), _nan(cout)
    ybuf = _nan(n_out + 1, cout + 64)
    ys = ybuf[:, 64:]
    gamma, beta, res = bn.gamma[:cout].contiguous(), bn.beta[:cout].contiguous(), bn.res[:, :cout]
    rm, rv = bn.rm[:cout].clone(), bn.rv[:cout].clone()
    state = torch.zeros(lib.a3d_conv_state_bytes() // 4, dtype=torch.int32, device="cuda") if own_state else None
    L.check(lib.a3d_conv_bn_train_forward(w.sc.handle, KINDS[kind], level_in, _ptr(x), x.stride(0), cin, _ptr(wp), cout, _ptr(raw),
                                          cout, _ptr(gamma), _ptr(beta), EPS, _ptr(res), res.stride(0), 1, _ptr(ys),
                                          ybuf.stride(0), 1, _ptr(mean), _ptr(rstd), _ptr(rm), _ptr(rv), MOMENTUM, _ptr(state),
                                          _ptr(ws), nbytes, _stream()), "a3d_conv_bn_train_forward")
    if own_state:
        assert int(state[1]) == 0, ("failure word", int(state[1]))
    return raw, mean, rstd, ybuf, rm, rv


def _check_forward(w, kind, level_in, cin, cout, x, wp, raw_ref, bn, where, seen, row=None, cls=None):
    """The assertions of the module docstring for one launch; raw_ref [n_out, cout] float64.  With `cls` the launch's
    profile entry must show the declared class.  The second call owns its hand-off state."""
    _, n_out = _rows(w, kind, level_in)
    if cls is not None:
        got, entries = _profiled(lambda: _forward_call(w, kind, level_in, x, cin, wp, cout, bn, False))
        _assert_ran_its_class(entries, cls, E.KVOL[kind], cin, cout, n_out, where)
    else:
        got = _forward_call(w, kind, level_in, x, cin, wp, cout, bn, False)
    raw, mean, rstd, ybuf, rm, rv = got
    if row is not None:
        _RAN.add((1, row))
    _assert_bits(raw, raw_ref, where + ": raw")
    # a block's sum is an integer of magnitude <= rows x max |raw| < 2^24: exact in fp32 in any order, so the fp64 total is
    # the exact sum and the one division is rounded alike on both sides
    assert 64 * raw_ref.abs().max().item() < 2 ** 24, (where, "a per-block sum could leave the exact range")
    total = raw_ref.sum(0)
    mean_ref = total / n_out
    if not torch.equal(mean, mean_ref.float()):
        c = int((mean != mean_ref.float()).nonzero()[0])
        pytest.fail(f"{where}: save_mean[{c}] = {mean[c].item()!r}, expected {mean_ref[c].item()!r} (column sum {total[c].item()}, "
                    f"{n_out} rows); {int((mean != mean_ref.float()).sum())} columns differ")
    m2 = ((raw_ref - mean_ref) ** 2).sum(0)
    var = m2 / n_out
    unbiased = m2 / (n_out - 1) if n_out > 1 else var            # one row: towards the biased value (bnorm.hip, cnt == 1)
    sd = torch.sqrt(var + EPS)
    assert not torch.isnan(rstd).any(), (where, "rstd NaN")
    _ratio("forward rstd 2e-5", ((rstd.double() - 1 / sd).abs() * sd).max(), 2e-5, where, seen)
    gamma, beta = bn.gamma[:cout].double(), bn.beta[:cout].double()
    y_ref = torch.relu((raw_ref - mean_ref) / sd * gamma + beta + bn.res[:, :cout].double())
    ys = ybuf[:n_out, 64:]
    assert not torch.isnan(ys).any(), (where, "y NaN", torch.isnan(ys).any(1).nonzero().flatten()[:8].tolist())
    _ratio("forward y 5e-5 of scale", (ys.double() - y_ref).abs().max(), 5e-5 * max(1.0, y_ref.abs().max().item()), where, seen)
    assert (ybuf[n_out, 64:] == 0).all(), (where, "zero row")
    assert torch.isnan(ybuf[:, :64]).all(), (where, "wrote outside its column slice")
    rv_ref = (1 - MOMENTUM) * bn.rv[:cout].double() + MOMENTUM * unbiased
    rm_ref = (1 - MOMENTUM) * bn.rm[:cout].double() + MOMENTUM * mean_ref
    assert not torch.isnan(rv).any() and not torch.isnan(rm).any(), (where, "running statistics NaN")
    _ratio("forward running_var 2e-5 of scale", (rv.double() - rv_ref).abs().max(), 2e-5 * max(1.0, rv_ref.abs().max().item()),
           where, seen)
    _ratio("forward running_mean 2e-6 of scale", (rm.double() - rm_ref).abs().max(), 2e-6 * max(1.0, mean_ref.abs().max().item()),
           where, seen)
    raw2, mean2, rstd2, ybuf2, _, _ = _forward_call(w, kind, level_in, x, cin, wp, cout, bn, True)
    assert torch.equal(raw, raw2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2), (where, "second call differs")
    assert torch.equal(ybuf[:, 64:], ybuf2[:, 64:]), (where, "second call: y differs")
    return raw, mean, rstd, ybuf, rm, rv


def _assert_bounds(seen, names, where):
    over = {k: v for k, v in seen.items() if k in names and not v <= 1.0}
    assert not over, (where, "error / bound", over)


_FWD = _BOUNDS[:4]
_BWD = _BOUNDS[4:]


# ----------------------------------------------------------------------------------------------------------------------
# b) a3d_conv_dgrad_bn (STATS = 2) and a3d_bn_backward_apply on its sums
# ----------------------------------------------------------------------------------------------------------------------
class BwOperands:
    """The BatchNorm unit whose output gradient the op completes, `width` columns: prev (the gradient already in g), raw,
    mean in {-1, 0, 1}, rstd in {0.5, 1, 2}, y in [-2, 2] with exact zeros of both signs, gamma in {-2, -1, 1, 2}."""

    def __init__(self, n_out, width, *seed):
        self.n_out = n_out
        self.prev = _ints((n_out, width), -3, 3, *seed, "prev")
        self.raw = _ints((n_out, width), -3, 3, *seed, "raw")
        self.mean = _ints((width,), -1, 1, *seed, "mean")
        self.rstd = _pick([0.5, 1.0, 2.0], (width,), *seed, "rstd")
        self.gamma = _pick([-2.0, -1.0, 1.0, 2.0], (width,), *seed, "bw gamma")
        y = _ints((n_out, width), -2, 2, *seed, "y")
        minus = _ints((n_out, width), 0, 1, *seed, "y sign") > 0
        self.y = torch.where((y == 0) & minus, torch.full_like(y, -0.0), y)
        assert n_out < 8 or ((self.y == 0).any() and torch.signbit(self.y[self.y == 0]).any())
        self.mask = (self.y > 0).double()
        self.xhat = (self.raw.double() - self.mean.double()) * self.rstd.double()
        self._wide = {}

    def wide(self, cout):
        """raw and y as column slices (at 32, at 0) of buffers 32 wider whose other columns are NaN"""
        if cout not in self._wide:
            rw, yw = _nan(self.n_out, cout + 32), _nan(self.n_out, cout + 32)
            rw[:, 32:] = self.raw[:, :cout]
            yw[:, :cout] = self.y[:, :cout]
            self._wide[cout] = (rw, yw)
        return self._wide[cout]


def _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, acc, relu, own_state):
    """one a3d_conv_dgrad_bn: g a column slice at 32 of a NaN buffer 64 wider (holding prev with acc) -> (gbuf, sums)"""
    lib = L.load()
    _, n_out = _rows(w, kind, level_in)
    nbytes = lib.a3d_conv_bn_train_workspace_bytes(w.sc.handle, KINDS[kind], level_in, cin, cout)
    assert nbytes, lib.a3d_last_error().decode()
    ws = scratch(nbytes)
    gbuf = _nan(n_out + 1, cout + 64)
    gs = gbuf[:, 32:32 + cout]
    if acc:
        gs[:n_out] = bw.prev[:, :cout]
        gs[n_out] = 0
    rw, yw = bw.wide(cout)
    if not relu:
        yw = _nan(n_out, cout + 32)                               # not to be read
    mean, rstd = bw.mean[:cout].contiguous(), bw.rstd[:cout].contiguous()
    sums = _nan(2, cout, dtype=torch.float64)
    state = torch.zeros(lib.a3d_conv_state_bytes() // 4, dtype=torch.int32, device="cuda") if own_state else None
    L.check(lib.a3d_conv_dgrad_bn(w.sc.handle, KINDS[kind], level_in, _ptr(x), x.stride(0), cin, _ptr(wp), cout, _ptr(gs),
                                  gbuf.stride(0), int(acc), _ptr(yw), yw.stride(0), _ptr(rw[:, 32:]), rw.stride(0), _ptr(mean),
                                  _ptr(rstd), int(relu), _ptr(sums), _ptr(state), _ptr(ws), nbytes, _stream()), "a3d_conv_dgrad_bn")
    if own_state:
        assert int(state[1]) == 0, ("failure word", int(state[1]))
    return gbuf, sums


def _check_dgrad(w, kind, level_in, cin, cout, x, wp, conv_ref, bw, where, seen, row=None, cls=None):
    """acc x relu over one op (the table row is the backward op as the library launches it: x is dy, the output has cout
    columns); the acc = 1 launches own their hand-off state.  conv_ref [n_out, cout] float64."""
    lib = L.load()
    _, n_out = _rows(w, kind, level_in)
    xhat, gamma = bw.xhat[:, :cout], bw.gamma[:cout].contiguous()
    rw, _ = bw.wide(cout)
    mean, rstd = bw.mean[:cout].contiguous(), bw.rstd[:cout].contiguous()
    first = True
    for acc in (0, 1):
        pre = conv_ref + bw.prev[:, :cout].double() if acc else conv_ref
        for relu in (0, 1):
            here = f"{where} acc {acc} relu {relu}"
            if cls is not None and first:
                (gbuf, sums), entries = _profiled(lambda: _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, acc, relu, False))
                _assert_ran_its_class(entries, cls, E.KVOL[kind], cin, cout, n_out, here)
            else:
                gbuf, sums = _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, acc, relu, bool(acc))
            first = False
            g_ref = pre * bw.mask[:, :cout] if relu else pre
            gs = gbuf[:, 32:32 + cout]
            _assert_bits(gs[:n_out].contiguous(), g_ref, here + ": g")
            assert (gs[n_out] == 0).all(), (here, "zero row")
            assert torch.isnan(gbuf[:, :32]).all() and torch.isnan(gbuf[:, 32 + cout:]).all(), (here, "wrote outside its column slice")
            # every term is a multiple of 1/2; a block (<= 64 rows) sums to below 2^24 half-units in any order if 64 times
            # the column's largest |term| does: then each fp32 partial and the fp64 total are exact
            terms = g_ref * xhat
            assert 2 * 64 * max(g_ref.abs().max().item(), terms.abs().max().item()) < 2 ** 24, (here, "partials leave the exact range")
            sums_ref = torch.stack([g_ref.sum(0), terms.sum(0)])
            if not torch.equal(sums, sums_ref):
                bad = sums != sums_ref
                k, c = (int(v) for v in bad.nonzero()[0])
                pytest.fail(f"{here}: sums[{k}, {c}] = {sums[k, c].item()!r}, expected {sums_ref[k, c].item()!r}; "
                            f"{int(bad.sum())} of {bad.numel()} differ")
            gbuf2, sums2 = _dgrad_call(w, kind, level_in, x, cin, wp, cout, bw, acc, relu, not acc)
            assert torch.equal(gbuf[:, 32:32 + cout], gbuf2[:, 32:32 + cout]) and torch.equal(sums, sums2), (here, "second call differs")
            # the consumer: BatchNorm backward from the sums [2][C] and the stored g
            dx, dgamma, dbeta = _nan(n_out + 1, cout), _nan(cout), _nan(cout)
            L.check(lib.a3d_bn_backward_apply(_ptr(rw[:, 32:]), rw.stride(0), None, 0, _ptr(gs), gbuf.stride(0), n_out, cout, _ptr(gamma),
                                              _ptr(mean), _ptr(rstd), 0, _ptr(sums), n_out, _ptr(sums), _ptr(dx), cout, None, 0,
                                              _ptr(dgamma), _ptr(dbeta), 1, _stream()), "a3d_bn_backward_apply")
            dx_ref = gamma.double() * rstd.double() * (g_ref - sums_ref[0] / n_out - xhat * sums_ref[1] / n_out)
            assert (dx[n_out] == 0).all() and not torch.isnan(dx).any(), (here, "dx")
            _ratio("backward dx 5e-5 of scale", (dx[:n_out].double() - dx_ref).abs().max(), 5e-5 * max(1.0, dx_ref.abs().max().item()),
                   here, seen)
            _ratio("backward dgamma 2e-4 of scale", (dgamma.double() - sums_ref[1]).abs().max(),
                   2e-4 * max(1.0, sums_ref[1].abs().max().item()), here, seen)
            _ratio("backward dbeta 2e-4 of scale", (dbeta.double() - sums_ref[0]).abs().max(),
                   2e-4 * max(1.0, sums_ref[0].abs().max().item()), here, seen)
    if row is not None:
        _RAN.add((2, row))


# ----------------------------------------------------------------------------------------------------------------------
# 1. small scenes: every kind, level and width pair
# ----------------------------------------------------------------------------------------------------------------------
_SMALL = [(s, k, l) for s in E.SMALL_SCENES for k, l in E.KIND_LEVELS]
_SMALL_IDS = [f"{s}-{k}-L{l}" for s, k, l in _SMALL]


def _sweep_refs(w, kind, level_in, lo, hi, tag):
    """one x / W at the widest pair; the references of the seven input widths are running sums over channel ranges"""
    n_in, n_out = _rows(w, kind, level_in)
    K = E.KVOL[kind]
    pairs = w.pairs(kind, level_in)
    assert len(pairs) == K
    X = _with_zero_row(_ints((n_in, E.WIDTHS_IN[-1]), lo, hi, w.name, kind, level_in, tag, "x"))
    W = _ints((K, E.WIDTHS_IN[-1], E.WIDTHS_OUT[-1]), lo, hi, w.name, kind, level_in, tag, "w")
    X64, W64 = X.double(), W.double()
    refs, acc = {}, 0
    for a, b in zip([0] + E.WIDTHS_IN, E.WIDTHS_IN):
        acc = acc + _conv_ref(pairs, X64[:, a:b], W64[:, a:b], n_out)
        refs[b] = acc
    return X, W, refs


@pytest.mark.parametrize("name,kind,level_in", _SMALL, ids=_SMALL_IDS)
def test_small_scenes_train_forward_every_width_pair(mode, name, kind, level_in):
    """a3d_conv_bn_train_forward over the 7 x 5 width pairs on levels of 1 .. 1800 rows: fewer rows than a tile, exactly one
    and two tiles, one row over, a line, two touching samples, the hash path."""
    w = _world(name)
    _, n_out = _rows(w, kind, level_in)
    X, W, refs = _sweep_refs(w, kind, level_in, -3, 3, "train")
    bn = BnOperands(n_out, E.WIDTHS_OUT[-1], name, kind, level_in)
    seen = {}
    for cin in E.WIDTHS_IN:
        x = X[:, :cin].contiguous()
        for cout in E.WIDTHS_OUT:
            where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {mode}"
            _check_forward(w, kind, level_in, cin, cout, x, pack_weight(W[:, :cin, :cout]), refs[cin][:, :cout], bn, where, seen,
                           row=(name, kind, level_in, cin, cout, 0, mode))
    _show(seen)
    _assert_bounds(seen, _FWD, f"scene {name} {kind} level {level_in} mode {mode}")


@pytest.mark.parametrize("name,kind,level_in", _SMALL, ids=_SMALL_IDS)
def test_small_scenes_dgrad_bn_every_width_pair(mode, name, kind, level_in):
    """a3d_conv_dgrad_bn over the same ops and width pairs, acc x relu each, then a3d_bn_backward_apply on its sums."""
    w = _world(name)
    _, n_out = _rows(w, kind, level_in)
    X, W, refs = _sweep_refs(w, kind, level_in, -2, 2, "dgrad")
    bw = BwOperands(n_out, E.WIDTHS_OUT[-1], name, kind, level_in)
    seen = {}
    for cin in E.WIDTHS_IN:
        x = X[:, :cin].contiguous()
        for cout in E.WIDTHS_OUT:
            where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {mode}"
            _check_dgrad(w, kind, level_in, cin, cout, x, pack_weight(W[:, :cin, :cout]), refs[cin][:, :cout], bw, where, seen,
                         row=(name, kind, level_in, cin, cout, 0, mode))
    _show(seen)
    _assert_bounds(seen, _BWD, f"scene {name} {kind} level {level_in} mode {mode}")


# ----------------------------------------------------------------------------------------------------------------------
# 2. the case tables: every build on a small and a large scene, one row per large-scene class, 63 / 64 partials, 1x1 rows
# ----------------------------------------------------------------------------------------------------------------------
_WL_CASES = [((name, kind, 0, 32, 32, 0, m), ("wl", E.KVOL[kind])) for name in E.WL_SCENES for kind in ("conv3", "down") for m in (1, 0)]
_TABLE = E.EPI_CASES + E.LARGE_CASES + E.TRAIN_CASES + _WL_CASES
_TABLE_IDS = [f"{t}-{_row_id(r)}" for t, rows in (("epi", E.EPI_CASES), ("large", E.LARGE_CASES), ("train", E.TRAIN_CASES),
                                                     ("wl", _WL_CASES)) for r, _ in rows]


@pytest.mark.parametrize("row,cls", _TABLE, ids=_TABLE_IDS)
def test_table_rows_train_forward(row, cls):
    """One a3d_conv_bn_train_forward per table row; the launch's profile entry shows the family, column width and stage
    width of the class declared next to the row (test_conv_plan_classes.py holds the declaration against the planner)."""
    name, kind, level_in, cin, cout, cin2, m = row
    assert cin2 == 0
    w = _world(name)
    if name.startswith("g"):
        assert (w.sc.n[0] + 15) // 16 == int(name[1:])
    _, n_out = _rows(w, kind, level_in)
    x, W, ref = _operands(w, kind, level_in, cin, cout, "train")
    bn = BnOperands(n_out, cout, name, kind, level_in, cin, cout)
    where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {m} {cls}"
    seen = {}
    before = _set_mode(m)
    try:
        _check_forward(w, kind, level_in, cin, cout, x, pack_weight(W), ref, bn, where, seen, row=row, cls=cls)
    finally:
        _set_mode(before)
    _show(seen)
    _assert_bounds(seen, _FWD, where)


@pytest.mark.parametrize("row,cls", _TABLE, ids=_TABLE_IDS)
def test_table_rows_dgrad_bn(row, cls):
    """a3d_conv_dgrad_bn on the same rows (each row is the backward op as launched), acc x relu, the first launch profiled."""
    name, kind, level_in, cin, cout, cin2, m = row
    w = _world(name)
    _, n_out = _rows(w, kind, level_in)
    x, W, ref = _operands(w, kind, level_in, cin, cout, "dgrad", -2, 2)
    bw = BwOperands(n_out, cout, name, kind, level_in, cin, cout)
    where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {m} {cls}"
    seen = {}
    before = _set_mode(m)
    try:
        _check_dgrad(w, kind, level_in, cin, cout, x, pack_weight(W), ref, bw, where, seen, row=row, cls=cls)
    finally:
        _set_mode(before)
    _show(seen)
    _assert_bounds(seen, _BWD, where)


# ----------------------------------------------------------------------------------------------------------------------
# 3. deliberate edges of the statistics: a constant column, a mean far from zero, one voxel
# ----------------------------------------------------------------------------------------------------------------------
_EDGE_ROWS = [("two_batch", "conv3", 0, 64, 64, 0, 0),       # k_conv_sk<64, 64, 0> with hand-offs: the last arriver's epilogue
              ("box65", "conv3", 0, 32, 32, 0, 0)]           # k_conv_wl: five 16-row groups, the last of one row
_RSTD_OF_ZERO = np.float32(1.0) / np.sqrt(np.float32(1e-5))      # 1 / sqrtf(0 + eps), both steps correctly rounded
assert _RSTD_OF_ZERO.dtype == np.float32


def _edge_classes(row):
    return ("wl", 27) if row[3] == 32 else ("sk", 27, 64, 64, 0, 1, 0, 0)


@pytest.mark.parametrize("row", _EDGE_ROWS, ids=[_row_id(r) for r in _EDGE_ROWS])
def test_constant_output_column(row):
    """One output column of W is all zero: that column of raw is constant 0, every tile's sum and M2 are exactly 0, the
    merge's m2 < 0 clamp must not matter: mean == 0, rstd == 1 / sqrtf(eps) bit for bit, y == relu(beta + res) exactly."""
    name, kind, level_in, cin, cout, _, m = row
    w = _world(name)
    n_in, n_out = _rows(w, kind, level_in)
    x = _with_zero_row(_ints((n_in, cin), -3, 3, name, "constant x"))
    W = _ints((27, cin, cout), -3, 3, name, "constant w")
    col = 17
    W[:, :, col] = 0
    ref = _conv_ref(w.pairs(kind, level_in), x.double(), W.double(), n_out)
    assert (ref[:, col] == 0).all() and (ref != 0).any(0).sum() == cout - 1
    bn = BnOperands(n_out, cout, name, "constant")
    where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {m}: constant column {col}"
    seen = {}
    before = _set_mode(m)
    try:
        raw, mean, rstd, ybuf, rm, rv = _check_forward(w, kind, level_in, cin, cout, x, pack_weight(W), ref, bn, where, seen,
                                                        cls=_edge_classes(row))
    finally:
        _set_mode(before)
    _show(seen)
    _assert_bounds(seen, _FWD, where)
    assert mean[col].item() == 0.0, (where, mean[col].item())
    assert np.float32(rstd[col].item()) == _RSTD_OF_ZERO, (where, rstd[col].item(), float(_RSTD_OF_ZERO))
    assert torch.equal(ybuf[:n_out, 64 + col], torch.relu(bn.beta[col] + bn.res[:, col])), (where, "y of the constant column")
    assert rm[col].item() == MOMENTUM * bn.rm[col].item() and rv[col].item() == MOMENTUM * bn.rv[col].item(), where


# the last block of partials has a row count that is no power of two (21 of 64, 5 of 16): S_b / n_b is then not a float,
# the fp32 mean the block used differs from it, and the merge's cross term 2 dm (S_b - n_b m_b) is not zero
_BIASED_ROWS = [("s1500", "conv3", 0, 64, 64, 0, 0),         # k_conv_sk<64, 64, 0> with hand-offs, 23 tiles + 21 rows
                ("box63", "conv3", 0, 64, 64, 0, 0),         # the same build, one tile of 63 rows: a tile mean taken over 64
                                                             # would pass the rstd bound on zero-mean data, not on these
                ("line37", "conv3", 0, 32, 32, 0, 0)]        # k_conv_wl, two groups + 5 rows


@pytest.mark.parametrize("row", _BIASED_ROWS, ids=[_row_id(r) for r in _BIASED_ROWS])
def test_sign_biased_input(row):
    """x and W in {0..3}: every column mean lies far from zero (with the symmetric operands of the other tests it is a
    small fraction of the spread) and every block's mean far from the batch mean, so the shift of the per-block M2 to the batch
    mean in k_bn_combine_tiles, n_b dm^2 + 2 dm (S_b - n_b m_b), carries variance; the reference shows both parts non-zero.
    The same assertions as everywhere else."""
    name, kind, level_in, cin, cout, _, m = row
    w = _world(name)
    _, n_out = _rows(w, kind, level_in)
    x, W, ref = _operands(w, kind, level_in, cin, cout, "biased", 0, 3)
    mean_ref, rows = ref.mean(0), 16 if cin == 32 else 64                        # rows per block of partials
    nb = torch.tensor([min(rows, n_out - r) for r in range(0, n_out, rows)], dtype=torch.float64, device="cuda")[:, None]
    S = torch.stack([ref[r:r + rows].sum(0) for r in range(0, n_out, rows)])
    m_used = (S.float() * (1 / nb.float())).double()                            # the fp32 block mean, as the kernels take it
    cross = 2 * (m_used - mean_ref) * (S - nb * m_used)
    print(f"   column means {mean_ref.min().item():.1f} .. {mean_ref.max().item():.1f}, row spread {ref.std(0).max().item():.2f}, "
          f"block means {m_used.min().item():.1f} .. {m_used.max().item():.1f}, largest cross term {cross.abs().max().item():.3e}")
    assert (mean_ref > ref.std(0)).all() and (m_used != mean_ref).any() and (cross != 0).any(), "the shift terms are zero"
    bn = BnOperands(n_out, cout, name, "biased")
    where = f"scene {name} {kind} level {level_in} {cin}->{cout} mode {m}: x, W >= 0"
    seen = {}
    before = _set_mode(m)
    try:
        _check_forward(w, kind, level_in, cin, cout, x, pack_weight(W), ref, bn, where, seen, cls=_edge_classes(row))
    finally:
        _set_mode(before)
    _show(seen)
    _assert_bounds(seen, _FWD, where)


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64), (128, 96), (32, 128)])
def test_one_voxel(mode, cin, cout):
    """n_out = 1 (torch refuses one row in training mode; the reference is the formula): mean = raw, var = 0, rstd =
    1 / sqrtf(eps), y = relu(beta + res), and the running variance moves towards the BIASED value 0 (bnorm.hip, cnt == 1)."""
    w = _world("one")
    x, W, ref = _operands(w, "conv3", 0, cin, cout, "one voxel")
    assert ref.shape[0] == 1
    bn = BnOperands(1, cout, "one", cin, cout)
    where = f"scene one conv3 level 0 {cin}->{cout} mode {mode}"
    seen = {}
    raw, mean, rstd, ybuf, rm, rv = _check_forward(w, "conv3", 0, cin, cout, x, pack_weight(W), ref, bn, where, seen)
    _show(seen)
    _assert_bounds(seen, _FWD, where)
    assert torch.equal(mean, ref[0].float()), where
    assert (rstd.cpu().numpy() == _RSTD_OF_ZERO).all(), (where, rstd[:4].tolist(), float(_RSTD_OF_ZERO))
    assert torch.equal(ybuf[0, 64:], torch.relu(bn.beta + bn.res[0])), where
    assert torch.equal(rv, MOMENTUM * bn.rv) and torch.equal(rm, MOMENTUM * bn.rm + MOMENTUM * ref[0].float()), where


# ----------------------------------------------------------------------------------------------------------------------
# 4. refusals: an error code, a message, nothing written
# ----------------------------------------------------------------------------------------------------------------------
def _refusal_operands():
    w = _world("box65")
    x, W, _ = _operands(w, "conv3", 0, 64, 64, "refusal")
    return w, x, pack_weight(W), L.load().a3d_conv_bn_train_workspace_bytes(w.sc.handle, L.OP_CONV3, 0, 64, 64)


def _refused(rc, outputs, what):
    msg = L.load().a3d_last_error()
    torch.cuda.synchronize()
    assert rc in (ERR_INVALID, ERR_WORKSPACE), (what, rc)
    assert msg and msg.decode().strip(), (what, "no message")
    for name, t in outputs.items():
        assert torch.isnan(t).all(), (what, name, "written by a refused call")


@pytest.mark.parametrize("how", ["one byte short", "not 256-aligned", "no y"])
def test_train_forward_refuses(how):
    """a3d_conv_bn_train_forward with a workspace one byte short of a3d_conv_bn_train_workspace_bytes, one that is not
    256-aligned, or without y.  (A residual can not reach a statistics launch through this entry: it goes to the BatchNorm
    apply pass, never to the conv -- launch_conv_sk's refusal of it has no public path, so it is not tested.)"""
    lib = L.load()
    w, x, wp, nbytes = _refusal_operands()
    n = w.sc.n[0]
    bn = BnOperands(n, 64, "refusal")
    ws = scratch(nbytes + 256)
    ws_ptr, ws_bytes = (_ptr(ws), nbytes - 1) if how == "one byte short" else (_ptr(ws[16:]), nbytes) if how == "not 256-aligned" \
        else (_ptr(ws), nbytes)
    assert ws.data_ptr() % 256 == 0
    out = {"raw": _nan(n, 64), "mean": _nan(64), "rstd": _nan(64), "y": _nan(n + 1, 64), "rm": _nan(64), "rv": _nan(64)}
    rc = lib.a3d_conv_bn_train_forward(w.sc.handle, L.OP_CONV3, 0, _ptr(x), x.stride(0), 64, _ptr(wp), 64, _ptr(out["raw"]), 64,
                                       _ptr(bn.gamma), _ptr(bn.beta), EPS, None, 0, 1, None if how == "no y" else _ptr(out["y"]), 64, 1,
                                       _ptr(out["mean"]), _ptr(out["rstd"]), _ptr(out["rm"]), _ptr(out["rv"]), MOMENTUM, None, ws_ptr,
                                       ws_bytes, _stream())
    _refused(rc, out, f"a3d_conv_bn_train_forward, {how}")


@pytest.mark.parametrize("how", ["one byte short", "not 256-aligned", "relu without y"])
def test_dgrad_bn_refuses(how):
    """a3d_conv_dgrad_bn with relu = 1 and y = NULL, a short workspace, a misaligned one."""
    lib = L.load()
    w, x, wp, nbytes = _refusal_operands()
    n = w.sc.n[0]
    bw = BwOperands(n, 64, "refusal")
    ws = scratch(nbytes + 256)
    ws_ptr, ws_bytes = (_ptr(ws), nbytes - 1) if how == "one byte short" else (_ptr(ws[16:]), nbytes) if how == "not 256-aligned" \
        else (_ptr(ws), nbytes)
    assert ws.data_ptr() % 256 == 0
    out = {"g": _nan(n + 1, 64), "sums": _nan(2, 64, dtype=torch.float64)}
    y = None if how == "relu without y" else _ptr(bw.y)
    rc = lib.a3d_conv_dgrad_bn(w.sc.handle, L.OP_CONV3, 0, _ptr(x), x.stride(0), 64, _ptr(wp), 64, _ptr(out["g"]), 64, 0, y, 64,
                               _ptr(bw.raw), 64, _ptr(bw.mean), _ptr(bw.rstd), 1, _ptr(out["sums"]), None, ws_ptr, ws_bytes, _stream())
    _refused(rc, out, f"a3d_conv_dgrad_bn, {how}")
