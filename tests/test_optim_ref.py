"""CPU: tests/optim_ref.py (the float64 reference the GPU optimiser tests compare with) against torch.optim.AdamW on
float64 parameters, including parameters that skip steps."""
import numpy as np
import torch

from optim_ref import adamw_step64, clip_coef, sum_squares64


def test_adamw_step64_matches_torch_adamw_float64():
    """5 steps on 3 tensors, tensor 1 without a gradient at steps 2 and 4: parameters, both moments and the step counts
    equal torch's to 1e-14 relative.  exp_avg is measured against b1 |m| + (1 - b1) |g|, the size of its two terms: where
    they cancel, torch's lerp_ (m + (1 - b1) (g - m), fused) and the plain formula round differently by an ulp of the
    TERMS, which is not small against a result near zero.  p and exp_avg_sq against themselves."""
    gen = torch.Generator().manual_seed(41)
    hp = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    shapes = [(7,), (5, 13), (257,)]
    ref = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=torch.float64)) for s in shapes]
    opt = torch.optim.AdamW(ref, **hp)
    p = [r.detach().numpy().copy() for r in ref]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    t = [0, 0, 0]
    terms = [None, None, None]           # b1 |m| + (1 - b1) |g| of every tensor's latest update
    for step in range(1, 6):
        for i, r in enumerate(ref):
            skip = i == 1 and step in (2, 4)
            r.grad = None if skip else torch.randn(shapes[i], generator=gen, dtype=torch.float64) * 10.0 ** (i - 1)
            if not skip:
                t[i] += 1
                terms[i] = hp["betas"][0] * np.abs(m[i]) + (1.0 - hp["betas"][0]) * np.abs(r.grad.numpy())
                p[i], m[i], v[i], _ = adamw_step64(p[i], r.grad.numpy(), m[i], v[i], t[i], hp["lr"], hp["betas"],
                                                   hp["eps"], hp["weight_decay"], 1.0)
        opt.step()
        for i, r in enumerate(ref):
            st = opt.state[r]
            assert float(st["step"]) == t[i], (step, i)
            for name, ours, theirs, size in (("p", p[i], r.detach().numpy(), None),
                                             ("exp_avg", m[i], st["exp_avg"].numpy(), terms[i]),
                                             ("exp_avg_sq", v[i], st["exp_avg_sq"].numpy(), None)):
                err = np.abs(ours - theirs)
                if size is None:
                    size = np.abs(theirs)
                assert (err <= 1e-14 * size).all(), (step, i, name, float((err / size).max()))
    assert t == [5, 3, 5]


def test_grad_scale_sum_squares_and_clip_coef():
    rng = np.random.default_rng(3)
    p, g, m, v = rng.standard_normal((4, 50))
    v = v * v
    a = adamw_step64(p, g, m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.25)
    b = adamw_step64(p, g * 0.25, m, v, 3, 1e-3, (0.9, 0.999), 1e-8, 1e-2, 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    x = rng.standard_normal(1000).astype(np.float32)
    y = np.array([1e25, -1e25, 3.0], np.float32)
    want = float((torch.from_numpy(x).double() ** 2).sum() + (torch.from_numpy(y).double() ** 2).sum())
    assert abs(sum_squares64(x, y) - want) <= 1e-14 * want
    norm = want ** 0.5
    ref = torch.nn.Parameter(torch.from_numpy(np.concatenate([x, y])).double())
    ref.grad = ref.detach().clone()
    tn = torch.nn.utils.clip_grad_norm_([ref], 0.1)
    assert abs(float(tn) - norm) <= 1e-14 * norm
    assert abs(clip_coef(norm, 0.1) - 0.1 / (norm + 1e-6)) == 0.0
    assert clip_coef(0.0, 0.1) == 1.0 and clip_coef(0.05, 0.1) == 1.0
    assert clip_coef(5.0, 0.0) == 1.0 and clip_coef(5.0, -1.0) == 1.0
