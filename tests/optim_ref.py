"""float64 restatement of the optimiser step (agile3d_amd/optim.py, csrc/optim.hip): torch.optim.AdamW's single-tensor
update with torch's scalar semantics (every hyper-parameter a Python double, every derived scalar formed in double), the
sum of squares of clip_grad_norm_ and its clip coefficient.  tests/test_optim_ref.py pins it on torch.optim.AdamW."""
import math

import numpy as np


def adamw_step64(p, g, m, v, t, lr, betas, eps, wd, grad_scale=1.0):
    """One AdamW update of step number ``t`` (counts from 1) on float64 copies of the arrays: -> (p, m, v, delta) with
    delta the update term lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) that was subtracted from p."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    g = g * float(grad_scale)
    p = p * (1.0 - float(lr) * float(wd))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * (g * g)
    step_size = float(lr) / (1.0 - b1 ** t)
    denom = np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + float(eps)
    delta = step_size * (m / denom)
    return p - delta, m, v, delta


def sum_squares64(*arrays):
    """sum over all arrays of sum x^2, every element squared and added in float64."""
    tot = 0.0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        tot += float(np.dot(a, a))
    return tot


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s factor: max_norm / (norm + 1e-6) clamped to 1; no clipping for max_norm <= 0."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6)) if max_norm > 0 else 1.0


def ulp32(x):
    """The spacing of fp32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
