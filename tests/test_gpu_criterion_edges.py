"""-m gpu: a3d_mask_losses (csrc/criterion.hip) at its shape edges -- n around the 64-lane wave and the 256-thread block,
C from 1 to the kernel's 64, a null weights pointer, logits far from zero, non-unit upstream gradients -- against
oracle.criterion's loss_bce_sample / loss_dice_sample on float64 copies of the same fp32 logits, autograd for the gradient.

Bounds (tests/test_criterion.py's): a loss <= 2e-6 * max(1, |ref|) (a batch with confidently wrong rows has a loss near
16, where one fp32 ulp is 1.9e-6); the gradient <= 1e-8 + 1e-5 * max|ref|.

The dice term switches on num = 2 p[t] / C > 1e-6; a row near the threshold may flip legitimately and move the loss by
about w / n, so every input is asserted (in float64) to have NO row with num in [0.5e-6, 2e-6]."""
import ctypes as C

import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd.criterion import SetCriterion, _losses_one
from oracle import criterion as oc

pytestmark = pytest.mark.gpu

LOSS_REL = 2e-6     # worst on the MI355X over this module: 5.79e-8 (of max(1, |ref|))
GRAD_ABS, GRAD_REL = 1e-8, 1e-5     # worst on the MI355X: 4.65e-7 of max|ref|
WORST = {"loss": 0.0, "grad": 0.0}


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print(f"\nworst over test_gpu_criterion_edges: loss {WORST['loss']:.2e} of max(1, |ref|) (<= {LOSS_REL:g}), "
          f"gradient {WORST['grad']:.2e} of max|ref| (<= {GRAD_REL:g} + {GRAD_ABS:g} absolute)")


def make_case(n, c, seed=None, t=None):
    """Seeded logits [n, c], targets and click weights: randn with +1.5 on the target column; the first max(1, n // 8)
    rows confidently wrong (-40 everywhere, +40 on the column after the target: the dice switch is off, only bce pulls);
    every row shifted by its own constant of scale 50 (softmax is shift invariant; without the max subtraction expf
    would overflow); weights in [0.8, 2) with every 7th exactly 0."""
    gen = torch.Generator().manual_seed(n * 100 + c if seed is None else seed)
    if t is None:
        t = torch.randint(0, c, (n,), generator=gen)
    z = torch.randn(n, c, generator=gen)
    rows = torch.arange(n)
    z[rows, t] += 1.5
    if c > 1 and n > 1:
        k = max(1, n // 8)
        z[:k] = -40.0
        z[rows[:k], (t[:k] + 1) % c] = 40.0
    z = z + 50.0 * torch.randn(n, 1, generator=gen)
    w = 0.8 + 1.2 * torch.rand(n, generator=gen)
    w[::7] = 0.0
    p = z.double().softmax(1)
    num = 2.0 * p[rows, t] / c
    assert int(((num >= 0.5e-6) & (num <= 2e-6)).sum()) == 0, "a row sits at the dice switch: the comparison is not defined"
    return z, t, w


def reference(z, t, w, coef_bce, coef_dice):
    """-> (float64 [bce, dice], d(coef_bce * bce + coef_dice * dice) / dz as float64 numpy)."""
    z64 = z.double().requires_grad_(True)
    w64 = torch.ones(len(z), dtype=torch.float64) if w is None else w.double()
    bce, dice = oc.loss_bce_sample(z64, t, w64), oc.loss_dice_sample(z64, t, w64)
    (coef_bce * bce + coef_dice * dice).backward()
    return np.array([float(bce.detach()), float(dice.detach())]), z64.grad.numpy()


def check_losses(out, ref, what):
    got = out.cpu().double().numpy()
    for j, name in enumerate(("bce", "dice")):
        err = abs(got[j] - ref[j]) / max(1.0, abs(ref[j]))
        WORST["loss"] = max(WORST["loss"], err)
        assert err <= LOSS_REL, (what, name, got[j], ref[j], err)


def check_grad(grad, ref, what):
    err = float(np.abs(grad.cpu().double().numpy() - ref).max())
    scale = float(np.abs(ref).max())
    if scale > 0:
        WORST["grad"] = max(WORST["grad"], err / scale)
    assert err <= GRAD_ABS + GRAD_REL * scale, (what, err, scale)


@pytest.mark.parametrize("c", [1, 2, 3, 11, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_grid(n, c):
    z, t, w = make_case(n, c)
    ref, gref = reference(z, t, w, 1.0, 2.0)
    out, grad = _losses_one(z.cuda(), t, w, 1.0, 2.0, True)
    check_losses(out, ref, (n, c))
    check_grad(grad, gref, (n, c))
    g = grad.cpu()
    assert (g[w == 0] == 0).all(), "rows of weight 0 carry a gradient"
    assert (w == 0).sum() == (n + 6) // 7 and np.abs(gref[(w == 0).numpy()]).max() == 0.0
    if c == 1:
        assert (out.cpu() == 0).all() and (g == 0).all()


@pytest.mark.parametrize("n,c", [(257, 11), (64, 64)])
def test_coefficients_and_null_pointers(n, c):
    z, t, w = make_case(n, c)
    zd = z.cuda()
    # weights None = explicit ones, bit for bit
    out_none, grad_none = _losses_one(zd, t, None, 1.0, 2.0, True)
    out_ones, grad_ones = _losses_one(zd, t, torch.ones(n), 1.0, 2.0, True)
    assert torch.equal(out_none.view(torch.int32), out_ones.view(torch.int32))
    assert torch.equal(grad_none.view(torch.int32), grad_ones.view(torch.int32))
    ref, gref = reference(z, t, None, 1.0, 2.0)
    check_losses(out_none, ref, (n, c, "no weights"))
    check_grad(grad_none, gref, (n, c, "no weights"))
    # the coefficients scale the gradient's two parts, never the loss values
    base, _ = _losses_one(zd, t, w, 1.0, 2.0, True)
    for cb, cd in ((1.0, 0.0), (0.0, 2.0), (0.0, 0.0)):
        ref, gref = reference(z, t, w, cb, cd)
        out, grad = _losses_one(zd, t, w, cb, cd, True)
        assert torch.equal(out.view(torch.int32), base.view(torch.int32)), (cb, cd)
        check_losses(out, ref, (n, c, cb, cd))
        check_grad(grad, gref, (n, c, cb, cd))
        if cb == cd == 0.0:
            assert (grad == 0).all()
    # a null gradient pointer: the same loss bits
    out_nograd, none = _losses_one(zd, t, w, 1.0, 2.0, False)
    assert none is None and torch.equal(out_nograd.view(torch.int32), base.view(torch.int32))


def test_bad_targets_and_refusals():
    lib = L.load()
    n, c = 300, 5
    z, t, w = make_case(n, c)
    zd = z.cuda()
    ref, gref = reference(z, t, w, 1.0, 2.0)
    for bad in (-1, c):
        tb = t.clone()
        tb[137] = bad
        out, _ = _losses_one(zd, tb, w, 1.0, 2.0, True)
        assert torch.isnan(out).all(), (bad, out)
        out, grad = _losses_one(zd, t, w, 1.0, 2.0, True)       # the error word does not survive the call
        check_losses(out, ref, ("after a bad target", bad))
        check_grad(grad, gref, ("after a bad target", bad))
    with pytest.raises(L.A3DError, match="a3d_mask_losses"):
        _losses_one(torch.zeros(0, 3, device="cuda"), torch.zeros(0, dtype=torch.long), None, 1.0, 2.0, True)
    with pytest.raises(L.A3DError, match="a3d_mask_losses"):
        _losses_one(torch.zeros(8, 65, device="cuda"), torch.zeros(8, dtype=torch.long), None, 1.0, 2.0, True)
    td = t.to(device="cuda", dtype=torch.int32)
    out = torch.full((2,), 7.0, device="cuda")
    ws = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rc = lib.a3d_mask_losses(zd.data_ptr(), td.data_ptr(), None, n, c, 1.0, 2.0, out.data_ptr(), None, ws.data_ptr(), 63,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -5 and lib.a3d_last_error().decode().startswith("a3d_mask_losses:")      # A3D_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0]


@pytest.fixture(scope="module")
def two_levels():
    """Two samples, (300, 4) and (129, 7), a final and one aux level; the oracle's losses and nothing else shared."""
    shapes = [(300, 4), (129, 7)]
    main = [make_case(n, c, seed=n * 100 + c) for n, c in shapes]
    aux = [make_case(n, c, seed=n * 100 + c + 50000, t=m[1])[0] for (n, c), m in zip(shapes, main)]
    return dict(z=[m[0] for m in main], aux=aux, t=[m[1] for m in main], w=[m[2] for m in main],
                weight_dict={"loss_bce": 1.0, "loss_dice": 2.0, "loss_bce_0": 1.0, "loss_dice_0": 2.0})


def _outputs(zs, auxs):
    return {"pred_masks": zs, "aux_outputs": [{"pred_masks": auxs}]}


def test_set_criterion_one_pass_equals_two(two_levels):
    """forward_and_grad = forward + grad_logits, bit for bit, and both agree with the oracle."""
    s = two_levels
    crit = SetCriterion(s["weight_dict"], ["bce", "dice"])
    outputs = _outputs([z.cuda() for z in s["z"]], [z.cuda() for z in s["aux"]])
    d1, g1 = crit.forward_and_grad(outputs, s["t"], s["w"])
    d2 = crit.forward(outputs, s["t"], s["w"])
    g2 = crit.grad_logits(outputs, s["t"], s["w"])
    assert set(d1) == set(d2) == set(s["weight_dict"])
    for k in d1:
        assert torch.equal(d1[k].view(torch.int32), d2[k].view(torch.int32)), k
    for a, b in zip(g1["pred_masks"] + g1["aux_outputs"][0], g2["pred_masks"] + g2["aux_outputs"][0]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    dref, _, gm, ga = oc.total_and_grads(_outputs([z.double() for z in s["z"]], [z.double() for z in s["aux"]]), s["t"],
                                         [w.double() for w in s["w"]], s["weight_dict"])
    for k in d1:
        want = float(dref[k].detach())
        err = abs(float(d1[k]) - want) / max(1.0, abs(want))
        WORST["loss"] = max(WORST["loss"], err)
        assert err <= LOSS_REL, (k, float(d1[k]), want)
    for got, ref in zip(g1["pred_masks"] + g1["aux_outputs"][0], gm + ga[0]):
        check_grad(got, ref.numpy(), "forward_and_grad")


def test_set_criterion_backward_with_upstream_gradients(two_levels):
    """CriterionFn.backward with non-unit upstream gradients: d(3 loss_bce + 0.5 loss_dice_0) / d(logits) of both levels;
    a level whose losses do not enter the expression gets a zero gradient."""
    s = two_levels
    crit = SetCriterion(s["weight_dict"], ["bce", "dice"])

    def leaves(dtype, device):
        return ([z.to(device=device, dtype=dtype).requires_grad_(True) for z in s["z"]],
                [z.to(device=device, dtype=dtype).requires_grad_(True) for z in s["aux"]])

    zs, auxs = leaves(torch.float32, "cuda")
    d = crit(_outputs(zs, auxs), s["t"], s["w"])
    (3.0 * d["loss_bce"] + 0.5 * d["loss_dice_0"]).backward()
    rz, raux = leaves(torch.float64, "cpu")
    dref = oc.criterion(_outputs(rz, raux), s["t"], [w.double() for w in s["w"]])
    (3.0 * dref["loss_bce"] + 0.5 * dref["loss_dice_0"]).backward()
    for got, ref in zip(zs + auxs, rz + raux):
        assert float(ref.grad.abs().max()) > 0
        check_grad(got.grad, ref.grad.numpy(), "3 bce + 0.5 dice_0")

    zs, auxs = leaves(torch.float32, "cuda")
    d = crit(_outputs(zs, auxs), s["t"], s["w"])
    (0.5 * d["loss_dice_0"] + 0.25 * d["loss_bce_0"]).backward()
    for z in zs:
        assert z.grad is not None and (z.grad == 0).all(), "the final level is not in the expression"
    rz, raux = leaves(torch.float64, "cpu")
    dref = oc.criterion(_outputs(rz, raux), s["t"], [w.double() for w in s["w"]])
    (0.5 * dref["loss_dice_0"] + 0.25 * dref["loss_bce_0"]).backward()
    for got, ref in zip(auxs, raux):
        check_grad(got.grad, ref.grad.numpy(), "aux level alone")
