"""-m gpu: backward of the sparse convolutions (first part) against torch autograd through
the oracle's gather-GEMM-scatter convolution (oracle/backbone.py: sparse_conv, ME's CPU algorithm) on the same seeded
inputs, rows matched by coordinates.  Tolerance 2e-4 of the gradient's scale (fp32 sums over up to 27 x N pairs)."""
import os

import numpy as np
import pytest
import torch

from agile3d_amd import backward as B
from agile3d_amd import lib as L
from agile3d_amd import SparseTensor
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from gpu_util import internal_to_oracle_rows
from oracle import backbone as ob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    coords = np.concatenate([make_scene(5000, seed=6)["coords"], make_scene(2500, seed=7, batch_index=1)["coords"]])
    sc = Scene(torch.from_numpy(coords).cuda())
    lv = ob.SparseLevels(coords)
    maps = [torch.from_numpy(internal_to_oracle_rows(sc, lv, i)) for i in range(5)]
    return sc, lv, maps


def _kmap(lv, kind, level_in):
    if kind == L.OP_CONV3:
        return lv.kernel_map(level_in, 3)
    if kind == L.OP_DOWN:
        return lv.stride_map(level_in)
    if kind == L.OP_UP:
        return [(rc, rf) for (rf, rc) in lv.stride_map(level_in - 1)]
    n = lv.n(level_in)
    return [(np.arange(n), np.arange(n))]


CASES = [(L.OP_CONV3, 0, 96, 96), (L.OP_CONV3, 0, 128, 96), (L.OP_CONV3, 1, 32, 32), (L.OP_CONV3, 1, 32, 64),
         (L.OP_CONV3, 2, 192, 128), (L.OP_CONV3, 3, 384, 256), (L.OP_CONV3, 4, 256, 256),
         (L.OP_DOWN, 0, 32, 32), (L.OP_DOWN, 2, 64, 64), (L.OP_DOWN, 3, 128, 128),
         (L.OP_UP, 4, 256, 256), (L.OP_UP, 2, 128, 96), (L.OP_UP, 1, 96, 96),
         (L.OP_LINEAR, 0, 96, 128), (L.OP_LINEAR, 3, 384, 256), (L.OP_LINEAR, 1, 128, 96)]


@pytest.mark.parametrize("kind,level_in,cin,cout", CASES)
def test_conv_backward_matches_autograd(world, kind, level_in, cin, cout):
    sc, lv, maps = world
    lo = B.level_out(kind, level_in)
    n_in, n_out = sc.n[level_in], sc.n[lo]
    g = torch.Generator().manual_seed(kind * 100 + level_in * 10 + cin + cout)
    K = {L.OP_CONV3: 27, L.OP_DOWN: 8, L.OP_UP: 8, L.OP_LINEAR: 1}[kind]
    X = torch.randn(n_in, cin, generator=g, requires_grad=True)
    W = (torch.randn(K, cin, cout, generator=g) / (cin * 4) ** 0.5).requires_grad_()
    dY = torch.randn(n_out, cout, generator=g)
    Y = ob.sparse_conv(X, W, _kmap(lv, kind, level_in), n_out)
    Y.backward(dY)
    m_in, m_out = maps[level_in], maps[lo]
    x_dev, dy_dev = X.detach()[m_in].cuda(), dY[m_out].cuda()
    # forward through the same helper (sanity: the maps and the op are what the oracle computes)
    y = B.run_conv(sc, kind, level_in, B.pack_weight(W.detach().cuda()), x_dev, cin, cout).cpu()
    assert (y - Y.detach()[m_out]).abs().max().item() <= 2e-4 * max(1.0, Y.abs().max().item())
    dx = B.conv_input_grad(sc, kind, level_in, W.detach().cuda(), dy_dev).cpu()
    ref_dx = X.grad[m_in]
    err_x = (dx - ref_dx).abs().max().item()
    assert err_x <= 2e-4 * max(1.0, ref_dx.abs().max().item()), ("dx", err_x)
    dw = B.conv_weight_grad(sc, kind, level_in, x_dev, dy_dev).cpu()
    err_w = (dw - W.grad).abs().max().item()
    scale_w = max(1.0, W.grad.abs().max().item())
    print(f"kind {kind} L{level_in} {cin}->{cout}: dx err {err_x:.2e}, dW err {err_w:.2e} (scale {scale_w:.1f})")
    assert dw.shape == W.grad.shape and err_w <= 2e-4 * scale_w, ("dW", err_w, scale_w)


def test_weight_grad_is_deterministic_and_checks_its_arguments(world):
    sc, lv, maps = world
    g = torch.Generator().manual_seed(5)
    x = torch.randn(sc.n[0], 96, generator=g).cuda()
    dy = torch.randn(sc.n[0], 96, generator=g).cuda()
    a = B.conv_weight_grad(sc, L.OP_CONV3, 0, x, dy)
    b = B.conv_weight_grad(sc, L.OP_CONV3, 0, x, dy)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        B.conv_weight_grad(sc, L.OP_CONV3, 0, x[:-1], dy)
    with pytest.raises(L.A3DError):
        B.conv_weight_grad(sc, L.OP_CONV3, 0, x[:, :48].contiguous(), dy)       # channels not a multiple of 32
    with pytest.raises(RuntimeError):
        B.conv_weight_grad(sc, L.OP_CONV3, 0, x.cpu(), dy.cpu())                # no CPU path


def test_weight_grad_needs_the_scene_work_lists_and_balances_over_them():
    """a3d_conv_wgrad walks the scene's per-offset group lists (a3d_scene_build_wgrad_lists): a scene without them is refused
    with a message that names the call, the Python wrapper builds them on first use, and the result on a scene where
    whole offsets are missing from most groups (two far-apart clumps + isolated voxels: long runs of absent groups) still
    matches a float64 evaluation of the pair sums."""
    import ctypes as C
    lib = L.load()
    g = np.random.default_rng(3)
    clump = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    lonely = g.integers(-400, 400, size=(600, 3)) * 3 + 1000               # no two of them adjacent
    xyz = np.unique(np.concatenate([clump, clump + 200, lonely]), axis=0)
    coords = np.concatenate([np.zeros((len(xyz), 1), np.int64), xyz], 1).astype(np.int32)
    sc = Scene(torch.from_numpy(coords).cuda())
    assert lib.a3d_conv_wgrad_workspace_bytes(sc.handle, L.OP_CONV3, 0, 32, 32) == 0
    assert b"a3d_scene_build_wgrad_lists" in lib.a3d_last_error()
    n = sc.n[0]
    x = torch.randn(n, 64, generator=torch.Generator().manual_seed(1)).cuda()
    dy = torch.randn(n, 32, generator=torch.Generator().manual_seed(2)).cuda()
    dw = B.conv_weight_grad(sc, L.OP_CONV3, 0, x, dy)                        # builds the lists
    assert lib.a3d_conv_wgrad_workspace_bytes(sc.handle, L.OP_CONV3, 0, 64, 32) > 0
    npad = (n + 127) // 128 * 128
    nb = torch.from_numpy(sc.table(0, L.TAB_NBR27).reshape(27, npad)[:, :n].astype(np.int64)).cuda()
    x64, dy64 = x.double(), dy.double()
    ref = torch.zeros(27, 64, 32, dtype=torch.float64, device="cuda")
    for k in range(27):
        ok = nb[k] < n
        ref[k] = x64[nb[k][ok]].T @ dy64[ok]
    err = (dw.double() - ref).abs().max().item()
    assert err <= 1e-4 * max(1.0, ref.abs().max().item()), err
    assert torch.equal(dw, B.conv_weight_grad(sc, L.OP_CONV3, 0, x, dy))


def test_weight_grad_pointer_build_for_operands_beyond_a_buffer_descriptor():
    """Operands of 4 GB and more cannot sit behind a buffer descriptor: k_wgrad<..., WIDE> gathers through 64-bit pointers
    instead.  A3D_WGRAD_WIDE=1 forces that build on the small test operands (read once per process: own interpreter)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, A3D_WGRAD_WIDE="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_backward.py"), "-x", "-q", "-p",
                          "no:cacheprovider", "-k", "conv_backward_matches or linear_weight_grad or work_lists"], env=env,
                         capture_output=True, text=True, timeout=1200, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:]


def test_finite_difference_of_a_small_loss(world):
    """An oracle-free property: for loss = sum(conv(x; W) * R), dW from the kernels predicts the loss change of a
    weight perturbation (first order, fp64 accumulation of the loss on the host)."""
    sc, lv, maps = world
    g = torch.Generator().manual_seed(9)
    n = sc.n[2]
    x = torch.randn(n, 64, generator=g).cuda()
    W = (torch.randn(27, 64, 64, generator=g) / 16).cuda()
    R = torch.randn(n, 64, generator=g).cuda()
    dW = B.conv_weight_grad(sc, L.OP_CONV3, 2, x, R)
    V = torch.randn(27, 64, 64, generator=g).cuda()
    eps = 1e-2
    lp = (B.run_conv(sc, L.OP_CONV3, 2, B.pack_weight(W + eps * V), x, 64, 64).double() * R.double()).sum()
    lm = (B.run_conv(sc, L.OP_CONV3, 2, B.pack_weight(W - eps * V), x, 64, 64).double() * R.double()).sum()
    fd = ((lp - lm) / (2 * eps)).item()
    an = (dW.double() * V.double()).sum().item()
    assert abs(fd - an) <= 1e-3 * max(1.0, abs(an)), (fd, an)


@pytest.mark.parametrize("n,C,relu,with_res", [(5000, 96, True, True), (777, 32, True, False), (1300, 256, False, False),
                                                (16, 128, True, True), (40000, 64, True, True)])
def test_batchnorm_training_forward_backward_vs_torch(n, C, relu, with_res):
    """nn.BatchNorm1d(training) (+ residual, + ReLU) and its autograd on the CPU in float64 as the reference."""
    g = torch.Generator().manual_seed(n + C)
    x = (torch.randn(n, C, generator=g) * 2 + 0.5)
    res = torch.randn(n, C, generator=g) if with_res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    dy = torch.randn(n, C, generator=g)
    xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    rd = res.double().requires_grad_() if with_res else None
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    y_ref = torch.nn.functional.batch_norm(xd, rm_ref, rv_ref, gd, bd, training=True, momentum=0.02, eps=1e-5)
    if with_res:
        y_ref = y_ref + rd
    if relu:
        y_ref = torch.relu(y_ref)
    y_ref.backward(dy.double())
    rm_d, rv_d = rm.cuda(), rv.cuda()
    y, mean, rstd = B.bn_train_forward(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, res.cuda() if with_res else None, relu,
                                       rm_d, rv_d, 0.02)
    assert (y.cpu().double() - y_ref.detach()).abs().max().item() <= 2e-5
    assert (rm_d.cpu().double() - rm_ref).abs().max().item() <= 1e-6 and (rv_d.cpu().double() - rv_ref).abs().max().item() <= 1e-5
    dx, dgamma, dbeta, dres = B.bn_train_backward(x.cuda(), y, dy.cuda(), gamma.cuda(), mean, rstd, relu, with_res)
    sx = max(1.0, xd.grad.abs().max().item())
    assert (dx.cpu().double() - xd.grad).abs().max().item() <= 5e-5 * sx
    assert (dgamma.cpu().double() - gd.grad).abs().max().item() <= 2e-4 * max(1.0, gd.grad.abs().max().item())
    assert (dbeta.cpu().double() - bd.grad).abs().max().item() <= 2e-4 * max(1.0, bd.grad.abs().max().item())
    if with_res:
        assert (dres.cpu().double() - rd.grad).abs().max().item() <= 1e-6
    s = B.column_sums(dy.cuda())
    assert (s.cpu().double() - dy.double().sum(0)).abs().max().item() <= 1e-3
    assert torch.equal(B.column_sums(dy.cuda()), s)      # deterministic


FUSED = [(L.OP_CONV3, 0, 96, 96), (L.OP_CONV3, 0, 128, 96), (L.OP_CONV3, 1, 32, 32), (L.OP_CONV3, 2, 64, 64),
         (L.OP_CONV3, 3, 128, 128), (L.OP_CONV3, 4, 256, 256), (L.OP_DOWN, 0, 32, 32), (L.OP_DOWN, 2, 64, 64),
         (L.OP_UP, 1, 96, 96), (L.OP_UP, 4, 256, 256), (L.OP_LINEAR, 0, 128, 96), (L.OP_LINEAR, 3, 384, 256),
         (L.OP_LINEAR, 2, 32, 64)]


@pytest.mark.parametrize("kind,level_in,cin,cout", FUSED)
def test_conv_bn_unit_with_statistics_from_the_conv_epilogue(world, kind, level_in, cin, cout):
    """a3d_conv_bn_train_forward (round 5: conv -> BatchNorm(train) (+ res)(ReLU) in one call, the batch statistics taken
    per tile in the conv kernel's epilogue) against float64: raw output, mean / rstd, running statistics, y written into a
    column slice of a wider buffer, for every kernel family the training convs run on (k_conv_sk with and without
    hand-offs, the LDS-resident 32-channel kernel, 1x1)."""
    _check_conv_bn_unit(world, kind, level_in, cin, cout)


@pytest.fixture(scope="module")
def world_9000():
    """One scene whose level 0 has at least 8192 rows: from there on a 128-column layer with 32-channel stages runs the
    low-register build of the stream-K kernel, which the 7500 voxels of `world` do not reach."""
    coords = make_scene(9000, seed=8)["coords"]
    sc = Scene(torch.from_numpy(coords).cuda())
    assert sc.n[0] >= 8192
    lv = ob.SparseLevels(coords)
    return sc, lv, [torch.from_numpy(internal_to_oracle_rows(sc, lv, 0))]


@pytest.fixture
def streamk_only():
    lib = L.load()
    before = lib.a3d_conv_deep_mode(0)
    yield
    lib.a3d_conv_deep_mode(before)


def test_conv_bn_unit_low_register_128_column_build_from_8192_rows(world_9000, streamk_only):
    """The same check where the conv is 3^3, 32 -> 128 on 9000 rows (its statistics build)."""
    _check_conv_bn_unit(world_9000, L.OP_CONV3, 0, 32, 128)


def test_input_gradient_conv_low_register_128_column_build_from_8192_rows(world_9000, streamk_only):
    """The same check where the input-gradient conv is 3^3, 32 -> 128 on 9000 rows (its backward-sums build)."""
    _check_input_gradient_conv_bn(world_9000, L.OP_CONV3, 0, 128, 32, True, True)


def _check_conv_bn_unit(world, kind, level_in, cin, cout):
    sc, lv, maps = world
    lo = B.level_out(kind, level_in)
    n_in, n_out = sc.n[level_in], sc.n[lo]
    g = torch.Generator().manual_seed(kind * 1000 + level_in * 100 + cin + cout)
    K = {L.OP_CONV3: 27, L.OP_DOWN: 8, L.OP_UP: 8, L.OP_LINEAR: 1}[kind]
    X = torch.randn(n_in, cin, generator=g)
    W = torch.randn(K, cin, cout, generator=g) / (cin * 4) ** 0.5
    R = torch.randn(n_out, cout, generator=g)
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    rm, rv = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5
    m_in, m_out = maps[level_in], maps[lo]
    raw_ref = ob.sparse_conv(X.double(), W.double(), _kmap(lv, kind, level_in), n_out)
    rm_ref, rv_ref = rm.double().clone(), rv.double().clone()
    y_ref = torch.relu(torch.nn.functional.batch_norm(raw_ref, rm_ref, rv_ref, gamma.double(), beta.double(), training=True,
                                                      momentum=0.02, eps=1e-5) + R.double())
    x = torch.zeros(n_in + 1, cin + 32, device="cuda")
    x[:n_in, 32:] = X[m_in].cuda()
    ybuf = torch.full((n_out + 1, cout + 64), float("nan"), device="cuda")
    rm_d, rv_d = rm.cuda(), rv.cuda()
    state = B.StateArena(torch.device("cuda"), 4)
    raw, mean, rstd = B.conv_bn_train_forward(sc, kind, level_in, B.pack_weight(W.cuda()), x[:, 32:], cin, cout, gamma.cuda(),
                                              beta.cuda(), 1e-5, R[m_out].cuda(), True, ybuf[:, 64:], rm_d, rv_d, 0.02, state=state)
    scale = max(1.0, raw_ref.abs().max().item())
    assert (raw.cpu().double() - raw_ref[m_out]).abs().max().item() <= 2e-5 * scale
    assert (mean.cpu().double() - raw_ref.mean(0)).abs().max().item() <= 2e-6 * scale
    var = raw_ref.var(0, unbiased=False)
    assert ((rstd.cpu().double() - 1 / torch.sqrt(var + 1e-5)).abs() * torch.sqrt(var + 1e-5)).max().item() <= 2e-5
    assert (ybuf[:n_out, 64:].cpu().double() - y_ref[m_out]).abs().max().item() <= 5e-5 * scale
    assert (ybuf[n_out, 64:] == 0).all() and torch.isnan(ybuf[:, :64]).all()          # zero row written, nothing outside the slice
    assert (rm_d.cpu().double() - rm_ref).abs().max().item() <= 2e-6 * scale
    assert (rv_d.cpu().double() - rv_ref).abs().max().item() <= 2e-5 * max(1.0, rv_ref.abs().max().item())
    # bit-determinism of the statistics (fixed summation orders, hand-offs included)
    ybuf2 = torch.empty_like(ybuf)
    raw2, mean2, rstd2 = B.conv_bn_train_forward(sc, kind, level_in, B.pack_weight(W.cuda()), x[:, 32:], cin, cout, gamma.cuda(),
                                                 beta.cuda(), 1e-5, R[m_out].cuda(), True, ybuf2[:, 64:], rm.cuda(), rv.cuda(), 0.02,
                                                 state=state)
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2) and torch.equal(raw, raw2)
    # accumulation in the epilogue: y += conv(x) on a column slice
    acc = torch.randn(n_out + 1, cout + 32, generator=g).cuda()
    want = acc[:n_out, 32:].double().cpu() + raw_ref[m_out]
    B.conv_apply_acc(sc, kind, level_in, B.pack_weight(W.cuda()), x[:, 32:], cin, cout, acc[:, 32:], acc=True, state=state)
    assert (acc[:n_out, 32:].cpu().double() - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("kind,level_in,cin,cout", [(L.OP_CONV3, 0, 96, 96), (L.OP_CONV3, 1, 32, 32), (L.OP_CONV3, 2, 64, 128),
                                                    (L.OP_CONV3, 4, 256, 256), (L.OP_DOWN, 1, 32, 32), (L.OP_UP, 3, 256, 128),
                                                    (L.OP_LINEAR, 0, 96, 128), (L.OP_LINEAR, 3, 128, 256)])
@pytest.mark.parametrize("acc,relu", [(False, True), (True, True), (True, False)])
def test_input_gradient_conv_with_batchnorm_backward_sums(world, kind, level_in, cin, cout, acc, relu):
    """a3d_conv_dgrad_bn (round 5): the input-gradient conv that completes dL/dx of a conv + BatchNorm(+ReLU) unit's output x
    masks it and sums g, g xhat in its epilogue.  Against the plain input-gradient conv (checked against autograd above)
    followed by the mask and float64 sums; then a3d_bn_backward_apply on those sums against the layer-at-a-time
    a3d_bn_train_backward."""
    _check_input_gradient_conv_bn(world, kind, level_in, cin, cout, acc, relu)


def _check_input_gradient_conv_bn(world, kind, level_in, cin, cout, acc, relu):
    sc, lv, maps = world
    lo = B.level_out(kind, level_in)
    n_in, n_out = sc.n[level_in], sc.n[lo]
    g = torch.Generator().manual_seed(kind * 131 + level_in * 17 + cin + 3 * cout + acc + 2 * relu)
    K = {L.OP_CONV3: 27, L.OP_DOWN: 8, L.OP_UP: 8, L.OP_LINEAR: 1}[kind]
    W = (torch.randn(K, cin, cout, generator=g) / (cin * 4) ** 0.5).cuda()
    dy = torch.zeros(n_out + 1, cout, device="cuda")
    dy[:n_out] = torch.randn(n_out, cout, generator=g).cuda()
    raw = (torch.randn(n_in, cin, generator=g) * 1.5 + 0.2).cuda()
    gamma, beta = (torch.rand(cin, generator=g) + 0.5).cuda(), torch.randn(cin, generator=g).cuda()
    y, mean, rstd = B.bn_train_forward(raw, gamma, beta, 1e-5, None, relu, None, None, 0.1, zero_row=True)
    prev = torch.randn(n_in + 1, cin, generator=g).cuda()
    parts = B.packed_input_grad_weights(kind, W)
    assert len(parts) == 1
    state = B.StateArena(torch.device("cuda"), 8)
    plain = prev.clone()
    B.conv_input_grad_into(sc, kind, level_in, parts, dy, cin, cout, plain, acc=acc, state=state)
    want_g = plain[:n_in].double()
    if relu:
        want_g = want_g * (y[:n_in] > 0)
    xhat = (raw.double() - mean.double()) * rstd.double()
    want_sums = torch.stack([want_g.sum(0), (want_g * xhat).sum(0)])
    out = prev.clone()
    sums = B.conv_dgrad_bn(sc, kind, level_in, parts[0], dy, cout, out, acc, y, raw, mean, rstd, relu, state=state)
    # (the plain conv of a small level may run on k_conv_deep, the one with the sums on the stream-K kernel: the same terms in
    # another partition of the sum -- rounding, not bit-identity)
    assert torch.equal(out[:n_in], want_g.float()) or (out[:n_in].double() - want_g).abs().max().item() <= 2e-5 * max(1.0, want_g.abs().max().item())
    assert (out[n_in] == 0).all()
    scale = max(1.0, want_sums.abs().max().item())
    assert (sums - want_sums).abs().max().item() <= 2e-5 * scale, (sums - want_sums).abs().max().item()
    # deterministic
    out2 = prev.clone()
    sums2 = B.conv_dgrad_bn(sc, kind, level_in, parts[0], dy, cout, out2, acc, y, raw, mean, rstd, relu, state=state)
    assert torch.equal(sums, sums2) and torch.equal(out, out2)
    # BatchNorm backward from those sums == the layer-at-a-time backward on the unmasked gradient
    dx = torch.empty(n_in + 1, cin, device="cuda")
    dg, db = B.bn_backward_from_sums(raw, out, gamma, mean, rstd, sums, dx)
    dx_ref, dg_ref, db_ref, _ = B.bn_train_backward(raw, y[:n_in], plain[:n_in].contiguous(), gamma, mean, rstd, relu, False,
                                                    zero_row=True)
    sx = max(1.0, dx_ref.abs().max().item())
    assert (dx - dx_ref).abs().max().item() <= 2e-5 * sx and (dx[n_in] == 0).all()
    assert (dg - dg_ref).abs().max().item() <= 2e-4 * max(1.0, dg_ref.abs().max().item())
    assert (db - db_ref).abs().max().item() <= 2e-4 * max(1.0, db_ref.abs().max().item())


@pytest.mark.parametrize("ks", [5, 3])
def test_stem_weight_grad_matches_autograd(world, ks):
    sc, lv, maps = world
    n = sc.n[0]
    g = torch.Generator().manual_seed(31 + ks)
    F3 = torch.rand(n, 3, generator=g)                                   # caller row order = the oracle's
    W = (torch.randn(ks ** 3, 3, 32, generator=g) / 6.0).requires_grad_()
    dY = torch.randn(n, 32, generator=g)
    ob.sparse_conv(F3, W, lv.kernel_map(0, ks), n).backward(dY)
    dw = B.stem_weight_grad(sc, F3.cuda(), dY[maps[0]].cuda(), ks ** 3).cpu()
    err = (dw - W.grad).abs().max().item()
    assert err <= 2e-4 * max(1.0, W.grad.abs().max().item()), err
    assert torch.equal(B.stem_weight_grad(sc, F3.cuda(), dY[maps[0]].cuda(), ks ** 3).cpu(), dw)


def test_backbone_training_step_matches_autograd():
    """Training-mode forward (BatchNorm on batch statistics) and backward of the whole Res16UNet34C + lin_squeeze_head
    on the HIP kernels against torch autograd (float64) through the oracle backbone: the output, the updated running
    statistics and the gradient of EVERY backbone parameter (63 conv kernels, 62 x 2 BatchNorm parameters, the bias)."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_backbone import BackboneTape
    torch.manual_seed(3)
    model = build_model(default_args()).cuda().train()
    with torch.no_grad():                                   # non-trivial BatchNorm parameters
        for n_, p in model.named_parameters():
            if n_.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            elif n_.endswith("bn.bias"):
                p.normal_(0, 0.2)
    DT = torch.float32 if os.environ.get('A3D_ORACLE_F32') else torch.float64   # ground truth in float64
    sd0 = {k: v.detach().cpu().to(DT).clone() if v.is_floating_point() else v.detach().cpu().clone() for k, v in model.state_dict().items()}
    # (6000 voxels: the coarsest level then has ~25 rows -- with 2500 voxels it has ~10, and BatchNorm over ten rows turns a
    # last-bit difference in the first layers into 1-2e-3 on the level-4 kernel gradients: the comparison then sits on the
    # tolerance and moves across it with the summation order of an early layer)
    scn = make_scene(int(os.environ.get("A3D_TRAIN_VOX", "6000")), seed=12)
    coords, n = scn["coords"], len(scn["coords"])
    g = torch.Generator().manual_seed(4)
    feats = torch.rand(n, 3, generator=g)
    R = torch.randn(n, 128, generator=g) / 16
    # ---- HIP kernels: forward
    sc = Scene(torch.from_numpy(coords).cuda())
    tape = BackboneTape(model, sc, feats.cuda())
    # ---- oracle: autograd through the training-mode forward.  ReLU's derivative jumps at 0 and the sums behind the
    # gradients cancel heavily (a single flipped element moves a BatchNorm bias gradient by a percent), so the oracle
    # applies the 0/1 masks of the forward pass under test, in the same order: both sides then differentiate the SAME
    # piecewise-linear function, and the forward outputs are still compared on their own.
    lv = ob.SparseLevels(coords)
    maps = [torch.from_numpy(internal_to_oracle_rows(sc, lv, i)) for i in range(5)]
    masks = []
    for level, node in tape.relu_levels:
        m = torch.empty(node.v.shape, dtype=DT)
        m[maps[level]] = (node.v > 0).cpu().to(DT)          # internal row order -> oracle row order
        masks.append(m)
    assert len(masks) == 1 + 8 + 2 * sum(ob.LAYERS)             # stem, 4 down + 4 up, two per BasicBlock
    it = iter(masks)
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k else v.clone()) for k, v in sd0.items()}
    ob.RELU = lambda z: z * next(it)
    try:
        out, _ = ob.res16unet34c_forward(sd, lv, feats.to(DT), bn=ob.batch_norm_train)
    finally:
        ob.RELU = torch.relu
    Wh = sd["lin_squeeze_head.kernel"]
    pcd_ref = out @ (Wh if Wh.dim() == 2 else Wh[0]) + sd["lin_squeeze_head.bias"].reshape(1, -1)
    (pcd_ref * R.to(DT)).sum().backward()
    err_out = (tape.output.cpu().double() - pcd_ref.detach()).abs().max().item()
    assert err_out <= 2e-4 * max(1.0, pcd_ref.abs().max().item()), err_out
    grads = tape.backward(R.cuda())
    names = [k for k in sd if k.startswith(("backbone.", "lin_squeeze_head.")) and sd[k].requires_grad and
             sd[k].grad is not None]                        # (the backbone's unused `final` layer has no gradient)
    assert len(names) == 63 + 62 * 2 + 1                   # 63 conv kernels (62 + the head), BatchNorm pairs, the head bias
    assert set(grads) == set(names), set(names) ^ set(grads)
    worst = ("", 0.0)
    for k in names:
        ref = sd[k].grad
        got = grads[k].cpu().double()
        assert got.shape == ref.shape, k
        rel = (got - ref).abs().max().item() / max(1e-3, ref.abs().max().item())
        worst = max(worst, (k, rel), key=lambda t: t[1])
        if os.environ.get("A3D_SHOW_GRADS"):
            print(f"   {k:48s} rel {rel:.2e}  scale {ref.abs().max().item():.3e}")
    print(f"backbone training step: output err {err_out:.2e}, {len(names)} parameter gradients, worst relative error "
          f"{worst[1]:.2e} ({worst[0]})")
    assert worst[1] <= 2e-3, worst
    for k, v in model.state_dict().items():                 # running statistics moved like torch's (momentum 0.02)
        if "running_" in k and k.startswith("backbone."):
            assert (v.cpu().double() - sd[k]).abs().max().item() <= 1e-4 * max(1.0, sd[k].abs().max().item()), k


def test_adamw_and_grad_clip_match_torch():
    """Three steps of clip_grad_norm_(0.1) + AdamW(lr 1e-4, weight_decay 1e-4) (main.py:125-127, engine.py:145-150)
    against torch.optim.AdamW / torch.nn.utils.clip_grad_norm_ on the CPU."""
    from agile3d_amd.optim import AdamW, clip_grad_norm_
    g = torch.Generator().manual_seed(8)
    shapes = {"a.kernel": (27, 96, 96), "b.bn.weight": (96,), "c.kernel": (128, 96), "d.bias": (1, 128)}
    ref_p = {k: torch.nn.Parameter(torch.randn(s, generator=g)) for k, s in shapes.items()}
    dev_p = {k: v.detach().clone().cuda() for k, v in ref_p.items()}
    ref_opt = torch.optim.AdamW(ref_p.values(), lr=1e-4, weight_decay=1e-4)
    opt = AdamW(dev_p.items(), lr=1e-4, weight_decay=1e-4)
    for step in range(3):
        grads = {k: torch.randn(s, generator=g) * (0.02 if step == 1 else 1.0) for k, s in shapes.items()}
        for k, p in ref_p.items():
            p.grad = grads[k].clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_p.values(), 0.1)
        ref_opt.step()
        dgr = {k: v.cuda() for k, v in grads.items()}
        norm, coef = clip_grad_norm_(dgr, 0.1)
        assert abs(norm - ref_norm.item()) <= 1e-5 * ref_norm.item()
        opt.step(dgr, coef)
        for k in shapes:
            assert (dev_p[k].cpu() - ref_p[k].detach()).abs().max().item() <= 1e-6, (step, k)   # a couple of ulps at |p| ~ 4
    st = ref_opt.state[ref_p["a.kernel"]]
    assert (opt.state["a.kernel"][0].cpu() - st["exp_avg"]).abs().max().item() <= 1e-9
    assert (opt.state["a.kernel"][1].cpu() - st["exp_avg_sq"]).abs().max().item() <= 1e-12


@pytest.mark.parametrize("n", [20, 1000, 40001])
def test_layernorm_and_linear_weight_grad_vs_torch(n):
    """The decoder's row-wise pieces: nn.LayerNorm(128) forward / backward and dW = x^T dy of its nn.Linear layers."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 128, generator=g) * 1.7 + 0.3
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    dy = torch.randn(n, 128, generator=g)
    xd, gd, bd = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    y_ref = torch.nn.functional.layer_norm(xd, (128,), gd, bd, 1e-5)
    y_ref.backward(dy.double())
    y = B.layernorm_forward(x.cuda(), gamma.cuda(), beta.cuda())
    assert (y.cpu().double() - y_ref.detach()).abs().max().item() <= 1e-5
    dx, dg, db = B.layernorm_backward(x.cuda(), dy.cuda(), gamma.cuda())
    assert (dx.cpu().double() - xd.grad).abs().max().item() <= 2e-5 * max(1.0, xd.grad.abs().max().item())
    assert (dg.cpu().double() - gd.grad).abs().max().item() <= 1e-4 * max(1.0, gd.grad.abs().max().item())
    assert (db.cpu().double() - bd.grad).abs().max().item() <= 1e-4 * max(1.0, bd.grad.abs().max().item())
    x2 = torch.randn(n, 128, generator=g)
    for cout in (128, 1024) if n >= 32 else (128,):
        d2 = torch.randn(n, cout, generator=g)
        dw = B.linear_weight_grad(x2.cuda(), d2.cuda()).cpu().double()
        ref = x2.double().t() @ d2.double()
        assert (dw - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item())


def test_backbone_trains_with_clip_and_adamw():
    """The training pieces together: BackboneTape gradients -> clip_grad_norm_(0.1) -> AdamW, eight steps on one scene
    with a least-squares target on pcd_features.  The loss must fall; nothing here touches torch autograd."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.optim import AdamW, clip_grad_norm_
    from agile3d_amd.train_backbone import BackboneTape
    torch.manual_seed(5)
    model = build_model(default_args()).cuda().train()
    scn = make_scene(4000, seed=20)
    sc = Scene(torch.from_numpy(scn["coords"]).cuda())
    feats = torch.from_numpy(scn["feats"]).cuda()
    target = torch.randn(len(scn["coords"]), 128, generator=torch.Generator().manual_seed(6)).cuda() * 0.5
    params = {k: p for k, p in model.named_parameters() if k.startswith(("backbone.", "lin_squeeze_head."))}
    opt = AdamW(params.items(), lr=2e-3, weight_decay=1e-4)
    losses = []
    for step in range(8):
        tape = BackboneTape(model, sc, feats)
        diff = tape.output - target
        losses.append(float((diff * diff).mean()))
        grads = tape.backward(diff * (2.0 / diff.numel()))
        norm, coef = clip_grad_norm_(grads, 0.1)
        assert np.isfinite(norm) and 0.0 < coef <= 1.0
        opt.step(grads, coef)
        if step == 2:
            # after an optimiser step every packed weight is stale: the next tape repacks all of them with ONE launch
            # (a3d_pack_conv_weights_multi) into the buffers they already own -- the same bits as packing weight by weight
            from agile3d_amd import backward as B
            from agile3d_amd.train_backbone import packed_weights_of
            pw = packed_weights_of(model)
            ptrs = {k: e.forward.data_ptr() for k, e in pw._c.items()}
            pw.refresh_all()
            assert pw._table is not None and pw._table[1] > len(pw._c) and len(pw._c) >= 40
            for k, e in pw._c.items():
                wf, parts, conv, kind = e.forward, e.parts, e.conv, e.kind
                w = conv.kernel3().detach().contiguous()
                assert wf.data_ptr() == ptrs[k] and e.version == pw._version(conv)
                assert torch.equal(wf, B.pack_weight(w)), k
                fresh = B.packed_input_grad_weights(kind, w)
                assert [(a, b) for a, b, _ in fresh] == [(a, b) for a, b, _ in parts]
                assert all(torch.equal(x[2], y[2]) for x, y in zip(fresh, parts)), k
    print("losses", [round(v, 4) for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0], losses


def test_decoder_training_step_matches_autograd():
    """Forward and backward of the click decoder (three layers of click-to-scene / click-to-click / FFN / scene-to-click
    + mask head, aux outputs included) on the HIP library against float64 autograd through oracle/decoder.py: the three
    logits tensors, the gradient of every decoder parameter and dL/d(pcd_features).  Like in the backbone test the
    oracle follows the branch of the forward pass under test (ReLU masks, label-derived attention masks)."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_decoder import DecoderTape
    from oracle import decoder as od
    torch.manual_seed(11)
    model = build_model(default_args()).cuda().train()
    g = torch.Generator().manual_seed(12)
    N = 1500
    pcd = torch.randn(N, 128, generator=g) * 0.7
    xyz = torch.rand(N, 3, generator=g) * 4.0
    sd = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items() if v.is_floating_point()}
    pos = od.fourier_pos_enc(xyz.double(), sd["pos_enc.gauss_B"], xyz.double().min(0)[0], xyz.double().max(0)[0])
    ci = {"0": [7], "1": [10, 400], "2": [33], "3": [900, 1200, 77]}
    ct = {"0": [6], "1": [0, 3], "2": [1], "3": [2, 4, 5]}
    R = [torch.randn(N, 4, generator=g) / 8 for _ in range(3)]
    tape = DecoderTape(model, pcd.cuda(), pos.float().cuda(), ci, ct)
    # ---- oracle with the tape's branch decisions
    n_fg = 6
    relu_seq = []
    for l in range(3):
        ffn, mlp = tape.relu_masks[2 * l].cpu().double(), tape.relu_masks[2 * l + 1].cpu().double()
        relu_seq += [ffn, mlp[:n_fg], mlp[n_fg:]]
    it = iter(relu_seq)
    for k in sd:
        if not k.startswith(("backbone.", "pos_enc.")):
            sd[k].requires_grad_()
    pcd_o = pcd.double().requires_grad_()
    od.RELU = lambda z: z * next(it)
    try:
        outs = od.forward_mask(sd, pcd_o, xyz.double(), pos, ci, ct, grad=True,
                               force_masks=[m.cpu().bool() for m in tape.attn_masks])
    finally:
        od.RELU = torch.relu
    for l in range(3):
        err = (tape.logits[l].cpu().double() - outs[l].detach()).abs().max().item()
        assert err <= 2e-4 * max(1.0, outs[l].abs().max().item()), (l, err)
    sum((o * r.double()).sum() for o, r in zip(outs, R)).backward()
    grads, d_pcd = tape.backward([r.cuda() for r in R])
    names = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
    assert set(grads) == set(names), set(names) ^ set(grads)
    worst = ("", 0.0)
    for k in names:
        ref, got = sd[k].grad, grads[k].cpu().double()
        assert got.shape == ref.shape, k
        rel = (got - ref).abs().max().item() / max(1e-3, ref.abs().max().item())
        worst = max(worst, (k, rel), key=lambda t: t[1])
        if os.environ.get("A3D_SHOW_GRADS"):
            print(f"   {k:56s} rel {rel:.2e}  scale {ref.abs().max().item():.3e}")
    rel_pcd = (d_pcd.cpu().double() - pcd_o.grad).abs().max().item() / pcd_o.grad.abs().max().item()
    print(f"decoder training step: {len(names)} parameter gradients, worst relative error {worst[1]:.2e} ({worst[0]}), "
          f"d_pcd {rel_pcd:.2e}")
    assert worst[1] <= 2e-3 and rel_pcd <= 2e-3, (worst, rel_pcd)


def test_full_training_step_reduces_the_loss():
    """engine.py:38-150 on the HIP library: backbone (training mode) -> object sampling + simulated clicks with no-grad
    decoder passes -> decoder (training mode) -> weighted BCE + dice on all three levels -> backward through decoder and
    backbone -> clip 0.1 -> AdamW.  Six iterations on one 2-scene batch with the same random draws every time: the
    total loss falls.  No torch autograd anywhere."""
    import random
    import types

    from agile3d_amd import batched_coordinates, build_model, default_args
    from agile3d_amd.criterion import build_mask_criterion
    from agile3d_amd.optim import AdamW
    from agile3d_amd.train_step import train_one_step
    torch.manual_seed(21)
    args = default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"])
    model = build_model(args).cuda()
    criterion = build_mask_criterion(args)
    scenes = [make_scene(3000, seed=30), make_scene(2500, seed=31)]
    batch = (batched_coordinates([s["coords"][:, 1:] for s in scenes]),
             torch.from_numpy(np.concatenate([s["raw_xyz"] for s in scenes])),
             torch.from_numpy(np.concatenate([s["feats"] for s in scenes])),
             [torch.from_numpy(s["labels"].astype(np.int64)) for s in scenes], None, None, [{}, {}],
             ("scene0030_00", "scene0031_00"), (0, 0))
    opt = AdamW(model.named_parameters(), lr=1e-3, weight_decay=1e-4)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    hist = []
    for step in range(6):
        np.random.seed(3), torch.manual_seed(3), random.seed(3)          # same objects and clicks every iteration
        st = train_one_step(model, criterion, opt, batch, torch.device("cuda"), max_norm=0.1)
        hist.append(st)
    losses = [h["loss"] for h in hist]
    print("losses", [round(v, 4) for v in losses], "grad norms", [round(h["grad_norm"], 3) for h in hist], "clicks", hist[0]["clicks"])
    # lr 1e-3 on a random-weight network: the trajectory is sensitive to rounding (another summation order moves
    # individual iterations), so the check is that training brings the loss down, not where the last iteration lands
    assert all(np.isfinite(losses)) and min(losses[2:]) < 0.8 * losses[0], losses
    assert set(hist[0]["loss_dict"]) == {"loss_bce", "loss_dice", "loss_bce_0", "loss_dice_0", "loss_bce_1", "loss_dice_1"}
    moved = [k for k, v in model.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) >= 268                       # every trained tensor of backbone, head and decoder
    model.eval()                                   # and the inference path sees the new weights
    x = SparseTensor(features=batch[2], coordinates=batch[0], device="cuda")
    assert torch.isfinite(model.forward_backbone(x, raw_coordinates=batch[1].cuda())[0].F).all()


def test_whole_network_gradients_match_autograd():
    """Backbone and decoder chained (the hand-off is dL/d(pcd_features)): all 268 trained tensors of the model against
    float64 autograd through oracle backbone (training-mode BatchNorm) + oracle decoder, same branch on both sides."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_backbone import BackboneTape
    from agile3d_amd.train_decoder import DecoderTape
    from oracle import decoder as od
    torch.manual_seed(13)
    model = build_model(default_args()).cuda().train()
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("bn.weight"):
                p.uniform_(0.5, 1.5)
            elif n_.endswith("bn.bias"):
                p.normal_(0, 0.2)
    DT = torch.float64
    sd0 = {k: v.detach().cpu().to(DT).clone() if v.is_floating_point() else v.detach().cpu().clone()
           for k, v in model.state_dict().items()}
    scn = make_scene(3000, seed=14)
    coords, n = scn["coords"], len(scn["coords"])
    g = torch.Generator().manual_seed(15)
    feats = torch.rand(n, 3, generator=g)
    xyz = torch.from_numpy(scn["raw_xyz"])
    lab = scn["labels"]
    ids = [i for i in np.unique(lab) if i > 0 and (lab == i).sum() >= 3][:2]
    ci = {"0": [int(np.flatnonzero(lab == 0)[5])], "1": [int(r) for r in np.flatnonzero(lab == ids[0])[:2]],
          "2": [int(np.flatnonzero(lab == ids[1])[0])]}
    ct = {"0": [3], "1": [0, 2], "2": [1]}
    R = [torch.randn(n, 3, generator=g) / 8 for _ in range(3)]
    # ---- HIP: backbone tape -> decoder tape -> backward through both
    sc = Scene(torch.from_numpy(coords).cuda())
    bt = BackboneTape(model, sc, feats.cuda())
    pos = od.fourier_pos_enc(xyz.to(DT), sd0["pos_enc.gauss_B"], xyz.to(DT).min(0)[0], xyz.to(DT).max(0)[0])
    dtp = DecoderTape(model, bt.output, pos.float().cuda(), ci, ct)
    gd, d_pcd = dtp.backward([r.cuda() for r in R])
    grads = dict(gd)
    grads.update(bt.backward(d_pcd))
    # ---- oracle on the same branch (the 0/1 ReLU masks and the attention masks of the HIP run)
    lv = ob.SparseLevels(coords)
    maps = [torch.from_numpy(internal_to_oracle_rows(sc, lv, i)) for i in range(5)]
    bmasks = []
    for level, node in bt.relu_levels:
        m = torch.empty(node.v.shape, dtype=DT)
        m[maps[level]] = (node.v > 0).cpu().to(DT)
        bmasks.append(m)
    n_fg = 3
    dmasks = []
    for l in range(3):
        ffn, mlp = dtp.relu_masks[2 * l].cpu().to(DT), dtp.relu_masks[2 * l + 1].cpu().to(DT)
        dmasks += [ffn, mlp[:n_fg], mlp[n_fg:]]
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and "running" not in k and k != "pos_enc.gauss_B" else v.clone())
          for k, v in sd0.items()}
    itb, itd = iter(bmasks), iter(dmasks)
    ob.RELU, od.RELU = (lambda z: z * next(itb)), (lambda z: z * next(itd))
    # The decoder of this random-weight network is ill-conditioned in its INPUT: moving pcd_features by 1e-5 (what two
    # summation orders of the conv kernel differ by) moves its parameter gradients by up to 1.4e-2 (measured with
    # two share partitions of the conv kernel (round 2); near-ties in the sharp attention softmaxes).  So the float64 decoder is evaluated AT the HIP
    # backbone's features (checked against the float64 backbone's to 1e-4 first) and the float64 backbone is driven by
    # the float64 decoder's dL/d(pcd_features): the chain rule end to end, each half at a well-conditioned point.
    try:
        out, _ = ob.res16unet34c_forward(sd, lv, feats.to(DT), bn=ob.batch_norm_train)
        Wh = sd["lin_squeeze_head.kernel"]
        pcd_o = out @ (Wh if Wh.dim() == 2 else Wh[0]) + sd["lin_squeeze_head.bias"].reshape(1, -1)
        fwd_err = (bt.output.cpu().to(DT) - pcd_o.detach()).abs().max().item() / pcd_o.detach().abs().max().item()
        print(f"whole network: forward pcd_features relative error {fwd_err:.2e}")
        assert fwd_err <= 1e-4, fwd_err
        pcd_leaf = bt.output.cpu().to(DT).clone().requires_grad_()
        outs = od.forward_mask(sd, pcd_leaf, xyz.to(DT), pos, ci, ct, grad=True, force_masks=[m.cpu().bool() for m in dtp.attn_masks])
    finally:
        ob.RELU = od.RELU = torch.relu
    sum((o * r.to(DT)).sum() for o, r in zip(outs, R)).backward()
    e_hand = (d_pcd.cpu().to(DT) - pcd_leaf.grad).abs().max().item() / pcd_leaf.grad.abs().max().item()
    (pcd_o * pcd_leaf.grad).sum().backward()
    names = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
    assert len(names) == 268 and set(grads) == set(names), set(names) ^ set(grads)

    def rel(keys):
        errs = sorted(((grads[k].cpu().to(DT) - sd[k].grad).abs().max().item() / max(1e-3, sd[k].grad.abs().max().item()), k) for k in keys)
        return errs[len(errs) // 2][0], errs[-1]
    dec_med, dec_worst = rel([k for k in names if k in dict(gd)])
    bb_med, bb_worst = rel([k for k in names if k not in dict(gd)])
    print(f"whole network: 268 gradients; decoder median {dec_med:.2e} worst {dec_worst[0]:.2e} ({dec_worst[1]}); "
          f"dL/d(pcd_features) {e_hand:.2e}; backbone median {bb_med:.2e} worst {bb_worst[0]:.2e} ({bb_worst[1]})")
    assert dec_worst[0] <= 1e-4 and e_hand <= 1e-4, (dec_worst, e_hand)
    # the backbone's worst tensors are the level-4 kernels: BatchNorm over the ~10 rows this scene has there
    assert bb_med <= 1e-3 and bb_worst[0] <= 5e-3, (bb_med, bb_worst)


def test_checkpoint_resume_continues_bit_identically(tmp_path):
    """main.py:131-152,190-201: train two iterations, save, load into a fresh model + optimiser, and the third iteration
    equals the third iteration of the uninterrupted run bit for bit (weights, Adam moments, step count, BatchNorm
    running statistics all travel); the optimiser entry is readable by torch.optim.AdamW."""
    import random

    from agile3d_amd import batched_coordinates, build_model, default_args
    from agile3d_amd.criterion import build_mask_criterion
    from agile3d_amd.optim import AdamW
    from agile3d_amd.train_step import MultiStepLR, load_checkpoint, save_checkpoint, train_one_step
    args = default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"])
    sc_ = make_scene(2500, seed=40)
    batch = (batched_coordinates([sc_["coords"][:, 1:]]), torch.from_numpy(sc_["raw_xyz"]), torch.from_numpy(sc_["feats"]),
             [torch.from_numpy(sc_["labels"].astype(np.int64))], None, None, [{}], ("scene0040_00",), (0,))
    crit = build_mask_criterion(args)
    dev = torch.device("cuda")

    def seeds(i):
        np.random.seed(i), torch.manual_seed(i), random.seed(i)
    torch.manual_seed(1)
    model = build_model(args).cuda()
    opt = AdamW(model.named_parameters(), lr=5e-4, weight_decay=1e-4)
    sched = MultiStepLR(opt, [1000])
    for i in range(2):
        seeds(10 + i)
        train_one_step(model, crit, opt, batch, dev, 0.1)
    save_checkpoint(str(tmp_path / "checkpoint.pth"), model, opt, sched, 0, args)
    seeds(12)
    ref = train_one_step(model, crit, opt, batch, dev, 0.1)
    ref_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    torch.manual_seed(99)
    model2 = build_model(args).cuda()                                   # different initial weights, overwritten by the file
    opt2 = AdamW(model2.named_parameters(), lr=5e-4, weight_decay=1e-4)
    assert load_checkpoint(str(tmp_path / "checkpoint.pth"), model2, opt2, MultiStepLR(opt2, [1000])) == 1
    assert opt2.step_count == 2
    seeds(12)
    got = train_one_step(model2, crit, opt2, batch, dev, 0.1)
    assert got["loss"] == ref["loss"] and got["grad_norm"] == ref["grad_norm"]
    for k, v in model2.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k
    ck = torch.load(str(tmp_path / "checkpoint.pth"), map_location="cpu", weights_only=False)
    topt = torch.optim.AdamW([torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()], lr=5e-4)
    topt.load_state_dict(ck["optimizer"])                               # same layout as the reference's files
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "epoch", "args"}


@pytest.mark.parametrize("Lq,Lk,Hh,dh,tr", [(20, 50000, 8, 16, 0), (37, 70001, 8, 16, 0), (20, 50000, 8, 16, 1),
                                             (50000, 20, 8, 16, 1), (40000, 30, 1, 128, 1), (40000, 30, 1, 128, 0)])
def test_attention_primitives_long_dimensions(Lq, Lk, Hh, dh, tr):
    """a3d_attn_scores / a3d_attn_apply at the sizes of the training path (tens of thousands of points on one side): the
    split / per-head / matrix-core variants against float64 einsum."""
    from agile3d_amd import decoder_ops as ops
    g = torch.Generator().manual_seed(Lq + Lk + dh)
    C_ = Hh * dh
    q = torch.randn(Lq, C_, generator=g).cuda()
    k = torch.randn(Lk, C_, generator=g).cuda()
    S = ops.attn_scores(q, k, 0.25, heads=Hh)
    ref_S = 0.25 * torch.einsum("ihd,jhd->hij", q.cpu().double().view(Lq, Hh, dh), k.cpu().double().view(Lk, Hh, dh))
    assert (S.cpu().double() - ref_S).abs().max().item() <= 1e-4
    P = torch.softmax(S, -1).contiguous()
    if tr:      # O[j, h, :] = sum_i P[h, i, j] X[i, h, :]
        out = torch.empty((Lk, C_), dtype=torch.float32, device="cuda")
        ops.attn_apply(P, q, True, 0.5, out)
        ref = 0.5 * torch.einsum("hij,ihd->jhd", P.cpu().double(), q.cpu().double().view(Lq, Hh, dh)).reshape(Lk, C_)
    else:       # O[i, h, :] = sum_j P[h, i, j] V[j, h, :]
        out = torch.empty((Lq, C_), dtype=torch.float32, device="cuda")
        ops.attn_apply(P, k, False, 0.5, out)
        ref = 0.5 * torch.einsum("hij,jhd->ihd", P.cpu().double(), k.cpu().double().view(Lk, Hh, dh)).reshape(Lq, C_)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), err


def test_reference_training_sequence_through_the_model_api():
    """The literal sequence of the reference's training loop (engine.py:38-150) on the public interface only:
    ``model.train(); forward_backbone; (eval + no_grad click rounds); forward_mask; criterion; losses.backward();
    torch.nn.utils.clip_grad_norm_; optimizer.step()`` with a torch.optim optimiser.  The HIP tapes sit behind
    torch.autograd (agile3d_amd/autograd.py).  Checked against ``train_one_step`` (the same arithmetic driven by hand)
    from identical weights and random draws: same clicks, same loss, same gradient norm, and -- with plain SGD on both
    sides, so that the update is linear in the gradient -- the same parameters after every step (Adam turns the 1e-9
    rounding noise of mathematically-zero gradients, e.g. the key bias of an attention layer, into +-lr steps, which
    says nothing about the gradients).  A third step then runs with torch.optim.AdamW as the reference does."""
    import copy
    import random

    from agile3d_amd import batched_coordinates, build_model, default_args
    from agile3d_amd.criterion import build_mask_criterion
    from agile3d_amd.train_step import train_one_step, train_one_step_api
    args = default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"])
    scenes = [make_scene(3000, seed=50), make_scene(2600, seed=51)]
    batch = (batched_coordinates([s["coords"][:, 1:] for s in scenes]),
             torch.from_numpy(np.concatenate([s["raw_xyz"] for s in scenes])),
             torch.from_numpy(np.concatenate([s["feats"] for s in scenes])),
             [torch.from_numpy(s["labels"].astype(np.int64)) for s in scenes], None, None, [{}, {}],
             ("scene0050_00", "scene0051_00"), (0, 0))
    dev = torch.device("cuda")
    torch.manual_seed(5)
    model_a = build_model(args).cuda()
    model_b = copy.deepcopy(model_a)
    crit = build_mask_criterion(args)
    lr = 1e-2

    class HandSGD:            # train_one_step's optimiser interface: step(gradients by name, clip coefficient)
        def __init__(self, model):
            self.params, self.lr = dict(model.named_parameters()), lr

        def step(self, grads, coef):
            with torch.no_grad():
                for k, g in grads.items():
                    self.params[k].add_(g.reshape(self.params[k].shape), alpha=-self.lr * coef)
    opt_a = torch.optim.SGD(model_a.parameters(), lr=lr)
    opt_b = HandSGD(model_b)
    pb = dict(model_b.named_parameters())
    sd_keys_bn = [k for k in model_a.state_dict() if k.endswith("running_mean") or k.endswith("running_var")]
    for step in range(2):
        np.random.seed(7 + step), torch.manual_seed(7 + step), random.seed(7 + step)
        sa = train_one_step_api(model_a, crit, opt_a, batch, dev, max_norm=0.1)
        np.random.seed(7 + step), torch.manual_seed(7 + step), random.seed(7 + step)
        sb = train_one_step(model_b, crit, opt_b, batch, dev, max_norm=0.1)
        print(f"step {step}: api loss {sa['loss']:.6f} norm {sa['grad_norm']:.5f} | hand-driven loss {sb['loss']:.6f} "
              f"norm {sb['grad_norm']:.5f} clicks {sa['clicks']}")
        assert sa["clicks"] == sb["clicks"]
        assert abs(sa["loss"] - sb["loss"]) <= 1e-5 * max(1.0, abs(sb["loss"]))
        assert abs(sa["grad_norm"] - sb["grad_norm"]) <= 1e-4 * sb["grad_norm"]
        for k in sb["loss_dict"]:
            assert abs(sa["loss_dict"][k] - sb["loss_dict"][k]) <= 1e-5 * max(1.0, abs(sb["loss_dict"][k])), k
        worst = 0.0
        for k, p in model_a.named_parameters():
            d = (p.detach() - pb[k].detach()).abs().max().item()
            worst = max(worst, d / max(1e-2, pb[k].detach().abs().max().item()))
        print(f"parameters after step {step}: worst difference relative to the tensor's scale {worst:.2e}")
        assert worst <= 1e-5
        for k in sd_keys_bn:
            assert torch.allclose(model_a.state_dict()[k], model_b.state_dict()[k], rtol=1e-5, atol=1e-6), k
        # every step starts from bit-identical weights: the click simulator takes discrete decisions (arg-max labels,
        # largest error cluster), so a 1e-7 difference in a parameter can move a click and with it the next loss
        model_b.load_state_dict(model_a.state_dict())
    n_grad = sum(1 for p in model_a.parameters() if p.grad is not None)
    assert n_grad >= 268, n_grad                       # every trained tensor received a gradient through autograd
    # the reference's optimiser (main.py:125): one more iteration with torch.optim.AdamW
    before = {k: v.detach().clone() for k, v in model_a.named_parameters()}
    opt = torch.optim.AdamW(model_a.parameters(), lr=1e-4, weight_decay=1e-4)
    np.random.seed(9), torch.manual_seed(9), random.seed(9)
    sc = train_one_step_api(model_a, crit, opt, batch, dev, max_norm=0.1)
    assert np.isfinite(sc["loss"]) and sc["grad_norm"] > 0
    assert sum(1 for k, v in model_a.named_parameters() if not torch.equal(v.detach(), before[k])) >= 268
    # eval after training through the API: the inference path picks the new weights up by itself
    model_a.eval()
    x = SparseTensor(features=batch[2], coordinates=batch[0], device="cuda")
    r = model_a.forward_backbone(x, raw_coordinates=batch[1].cuda())
    assert torch.isfinite(r[0].F).all()


@pytest.mark.parametrize("Lq,Lk,masked", [(37, 5003, True), (20, 3000, False), (130, 1700, True)])
def test_flash_click_to_scene_attention_vs_float64_autograd(Lq, Lk, masked):
    """a3d_flash_c2s_forward / _backward (no [8, Lq, Lk] matrix; softmax statistics kept, probabilities recomputed in the
    backward pass) against float64 autograd of the plain formula: output, dq, dk, dv; ragged sizes (Lq, Lk not multiples
    of 16 / 64), a mask that blocks 60 % of the entries and whole 64-key chunks of some queries."""
    from agile3d_amd import decoder_ops as ops
    from attn_kit import check, mha_ref
    g = torch.Generator().manual_seed(Lq * 7 + Lk)
    q, k, v = (torch.randn(n, 128, generator=g) for n in (Lq, Lk, Lk))
    w = torch.randn(Lq, 128, generator=g)
    mask = None
    if masked:
        mask = (torch.rand(Lq, Lk, generator=g) < 0.6)
        mask[:, 5] = False                                  # no row fully blocked (the reference's mask_module guarantees it)
        mask[3, 64:640] = True                              # whole chunks blocked for one query
        mask = mask.to(torch.uint8)
    want = mha_ref(q, k, v, w, mask)
    dev = torch.device("cuda")
    qs, kd, vd, md, wd = (q * 0.25).to(dev), k.to(dev), v.to(dev), (mask.to(dev).contiguous() if masked else None), w.to(dev)
    o, stats = ops.flash_c2s_forward(qs, kd, vd, md)
    dq, dk, dv = ops.flash_c2s_backward(qs, kd, vd, md, o, stats, wd)
    dq2, dk2, dv2 = ops.flash_c2s_backward(qs, kd, vd, md, o, stats, wd)
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)      # deterministic
    check(f"flash c2s {Lq}x{Lk}", (o, dq * 0.25, dk, dv), want)


@pytest.mark.parametrize("Lq,Lk", [(5003, 37), (3000, 20), (1700, 130)])
def test_flash_scene_to_click_attention_vs_float64_autograd(Lq, Lk):
    """a3d_flash_s2c_forward / _backward (the N points as queries over few keys) against float64 autograd."""
    from agile3d_amd import decoder_ops as ops
    from attn_kit import check, mha_ref
    g = torch.Generator().manual_seed(Lq * 3 + Lk)
    q, k, v = (torch.randn(n, 128, generator=g) for n in (Lq, Lk, Lk))
    w = torch.randn(Lq, 128, generator=g)
    want = mha_ref(q, k, v, w, None)
    dev = torch.device("cuda")
    qs, kd, vd, wd = (q * 0.25).to(dev), k.to(dev), v.to(dev), w.to(dev)
    o, stats = ops.flash_s2c_forward(qs, kd, vd)
    dq, dk, dv = ops.flash_s2c_backward(qs, kd, vd, o, stats, wd)
    check(f"flash s2c {Lq}x{Lk}", (o, dq * 0.25, dk, dv), want)


def test_batched_decoder_tape_equals_one_tape_per_sample():
    """DecoderTape over a batch (row-wise layers once over all samples' rows, attention and mask head per sample on row
    ranges -- what train_one_step runs) against one single-sample tape per batch sample: the same logits (bit for bit: every
    output row is computed by the same arithmetic) and the same gradients up to the order of the sums over rows (parameter
    gradients are sums over all samples' rows in one reduction instead of one per sample)."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_decoder import DecoderTape
    from oracle import decoder as od
    torch.manual_seed(21)
    model = build_model(default_args()).cuda().train()
    g = torch.Generator().manual_seed(22)
    sizes = [1700, 2300, 1100]
    cis = [{"0": [7], "1": [10, 400], "2": [33], "3": [900, 1200, 77]},
           {"0": [], "1": [5, 2000, 14, 15, 16, 90], "2": [1000]},
           {"0": [3, 4], "1": [600]}]
    cts = [{"0": [6], "1": [0, 3], "2": [1], "3": [2, 4, 5]},
           {"0": [], "1": [0, 1, 2, 3, 4, 6], "2": [5]},
           {"0": [1, 2], "1": [0]}]
    pcds, poss, Rs = [], [], []
    for n, ci in zip(sizes, cis):
        pcd = torch.randn(n, 128, generator=g) * 0.7
        xyz = (torch.rand(n, 3, generator=g) * 4.0).double()
        B_ = model.state_dict()["pos_enc.gauss_B"].detach().cpu().double()
        poss.append(od.fourier_pos_enc(xyz, B_, xyz.min(0)[0], xyz.max(0)[0]).float().cuda())
        pcds.append(pcd.cuda())
        Rs.append([(torch.randn(n, len(ci), generator=g) / 8).cuda() for _ in range(3)])
    batched = DecoderTape(model, pcds, poss, cis, cts)
    singles = [DecoderTape(model, p, q, ci, ct) for p, q, ci, ct in zip(pcds, poss, cis, cts)]
    for l in range(3):
        for b, t in enumerate(singles):
            assert torch.equal(batched.logits[l][b], t.logits[l]), (l, b)
    gb, dpb = batched.backward([[Rs[b][l] for b in range(3)] for l in range(3)])
    gs, dps = {}, []
    for b, t in enumerate(singles):
        g_, dp = t.backward(Rs[b])
        dps.append(dp)
        for k, v in g_.items():
            gs[k] = v if k not in gs else gs[k] + v
    assert set(gb) == set(gs)
    worst = ("", 0.0)
    for k in gs:
        rel = (gb[k] - gs[k]).abs().max().item() / max(1e-3, gs[k].abs().max().item())
        worst = max(worst, (k, rel), key=lambda t: t[1])
    rel_p = (dpb - torch.cat(dps)).abs().max().item() / torch.cat(dps).abs().max().item()
    print(f"batched tape vs per-sample tapes: {len(gs)} parameter gradients, worst relative difference {worst[1]:.2e} "
          f"({worst[0]}), d_pcd {rel_p:.2e}")
    assert worst[1] <= 2e-5 and rel_p <= 2e-5, (worst, rel_p)
    batched.release()
    assert batched.steps == [] and batched.pcd is None


@pytest.mark.parametrize("N,G,Q", [(1, 2, 11), (255, 3, 12), (4097, 6, 40), (80_000, 11, 200), (3000, 256, 256)])
def test_next_layer_mask_matches_the_torch_expression(N, G, Q):
    """a3d_next_layer_mask (the training tape's attention mask of the next decoder layer, agile3d.py:362-383) against the torch
    expression it replaces: label = first arg-max over the 1 + K logits, mask[q][n] = label[n] != group(q) and some point
    carries group(q).  Ties (equal logits), groups that own no point and groups no query belongs to are in the data."""
    from agile3d_amd.decoder_ops import next_layer_mask
    g = torch.Generator().manual_seed(N + 7 * G + Q)
    logits = torch.randn(N, G, generator=g)
    logits[:, G - 1] = -50.0                                   # a group that never wins: "nothing blocked" for its queries
    if N > 4:
        logits[1::3] = torch.round(logits[1::3])               # ties: the FIRST maximum counts
        logits[2] = 1.0
    gq = torch.randint(0, G, (Q,), generator=g, dtype=torch.int32)
    gq[0] = G - 1
    lg, gqd = logits.cuda(), gq.cuda()
    got = next_layer_mask(lg, gqd)
    labels = lg.argmax(1)
    counts = torch.bincount(labels, minlength=G)
    want = ((labels[None, :] != gqd.long()[:, None]) & (counts[gqd.long()] > 0)[:, None]).to(torch.uint8)
    assert got.shape == (Q, N) and got.dtype == torch.uint8
    assert torch.equal(got, want)
    assert not got[0].any()
