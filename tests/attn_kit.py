"""What the attention tests of the training decoder share (not collected, like ``session_kit.py``): the float64 reference of
softmax(q k^T / 4 + mask) v with its gradients, the keep matrix of a dropout site, the comparison of (o, dq, dk, dv) at the
flash tests' bar, and outputs / workspaces that start out as NaN, so that an element nothing wrote fails a comparison
instead of passing on zeros.  The kernels are reached through ``agile3d_amd.decoder_ops`` only."""
import torch

from agile3d_amd import decoder_ops as ops
from dropout_ref import scale as drop_scale

DEV = torch.device("cuda")
TOL = 2e-5


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def poisoned(nbytes):
    return torch.full((int(nbytes),), 255, dtype=torch.uint8, device=DEV)        # 0xff bytes: NaN as floats


def zmat(seed, sample, site, p, heads, rows, cols):
    """Z = keep / (1 - p) in float64, from the library's mask (pinned on the numpy restatement in test_gpu_dropout.py)."""
    return ops.dropout_mask(seed, sample, site, p, heads, rows, cols).cpu().double() * drop_scale(p)


def mha_ref(q, k, v, w, mask, Z=None, per_head=False, dtype=torch.float64):
    """softmax(q k^T / 4 + mask) (o Z) v per head (8 x 16) in float64 on the CPU, autograd for the loss sum(o * w):
    (o, dq, dk, dv).  ``per_head``: one head at a time (16-channel slices, written back), for the cases whose [8, Lq, Lk]
    float64 matrices would take gigabytes.  ``dtype=torch.float32``: the same formula in plain float32, whose distance from
    the float64 result is what the rounding of the scores alone costs (check_measured)."""
    Lq, Lk = q.shape[0], k.shape[0]
    q64, k64, v64, w64 = (t.to(dtype) for t in (q, k, v, w))
    blocked = mask.bool()[None] if mask is not None else None
    o, dq = torch.empty(Lq, 128, dtype=dtype), torch.empty(Lq, 128, dtype=dtype)
    dk, dv = torch.empty(Lk, 128, dtype=dtype), torch.empty(Lk, 128, dtype=dtype)
    nh = 1 if per_head else 8
    for h0 in range(0, 8, nh):
        sl = slice(16 * h0, 16 * (h0 + nh))
        qh, kh, vh = (t[:, sl].clone().requires_grad_(True) for t in (q64, k64, v64))
        s = torch.einsum("ihd,jhd->hij", qh.view(Lq, nh, 16), kh.view(Lk, nh, 16)) / 4.0
        if blocked is not None:
            s = s.masked_fill(blocked, float("-inf"))
        p = torch.softmax(s, -1)
        if Z is not None:
            p = p * Z[h0:h0 + nh].to(dtype)
        oh = torch.einsum("hij,jhd->ihd", p, vh.view(Lk, nh, 16)).reshape(Lq, 16 * nh)
        (oh * w64[:, sl]).sum().backward()
        o[:, sl], dq[:, sl], dk[:, sl], dv[:, sl] = oh.detach(), qh.grad, kh.grad, vh.grad
    return o, dq, dk, dv


def check(tag, got, want, tol=TOL, names=("o", "dq", "dk", "dv")):
    """max|got - want| <= tol * max|want| per pair, every figure printed before the first assertion."""
    errs = []
    for name, g, r in zip(names, got, want):
        err = (g.double().cpu() - r.detach()).abs().max().item()
        sc = max(1e-6, r.detach().abs().max().item())
        print(f"{tag} {name}: max|diff| {err:.2e} (scale {sc:.2e}) -> {err / sc:.2e}")
        errs.append((name, err, sc))
    for name, err, sc in errs:
        assert err <= tol * sc, (tag, name, err, sc)          # (a NaN fails: the comparison is False)


def check_measured(tag, got, want, ref32, floor=TOL, factor=4.0, names=("o", "dq", "dk", "dv")):
    """Scores far from zero: the float32 rounding of a score of 60 alone moves its weight by about 1e-5 relative, so the bar
    is measured -- max|got - want| <= max(floor, factor * e32) * max|want| per output, e32 the distance of the plain float32
    formula (``ref32``) from float64 (``want``); the factor is for another summation order and v_exp_f32 against expf.  Every
    figure is printed before the first assertion; returns [(name, e32, kernel's figure)]."""
    rows = []
    for name, g, r, r32 in zip(names, got, want, ref32):
        r = r.detach()
        sc = max(1e-6, r.abs().max().item())
        e32 = (r32.detach().double() - r).abs().max().item() / sc
        err = (g.double().cpu() - r).abs().max().item() / sc
        print(f"{tag} {name}: e32 {e32:.2e}, kernel {err:.2e} (scale {sc:.2e}), bar {max(floor, factor * e32):.2e}")
        rows.append((name, e32, err))
    for name, e32, err in rows:
        assert factor * e32 <= 1e-3, (tag, name, e32, "too extreme an input for float32")
        assert err <= max(floor, factor * e32), (tag, name, err, e32)      # (a NaN fails: the comparison is False)
    return rows
