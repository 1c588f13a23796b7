"""-m gpu: the HIP backbone against fixtures made by running the REFERENCE's own ``Agile3d.forward_backbone``
(tests/golden/backbone_case_*.npz; generator tests/golden/make_backbone_goldens.py, which needs the reference and so
never runs here).  The weights come from the formula in tests/backbone_fixture.py, checked against the sums stored in
each fixture before use.
  * eval mode: pcd_features, the five aux feature maps (rows matched by coordinates) and the position encoding;
  * train mode: pcd_features, every BatchNorm's updated running statistics and the stored parameter gradients of
    L = sum(pcd_features * R), the latter corrected for ReLU decisions at a kink (see the train test)."""
import numpy as np
import pytest
import torch

import backbone_fixture as bf
from agile3d_amd import SparseTensor, build_model, default_args
from oracle import backbone as ob

pytestmark = pytest.mark.gpu
TOL = 1e-3              # forward: absolute, and so also relative to max(1, max |ref|)
GRAD_TOL = 2e-3         # gradients: relative to the tensor's own max (test_gpu_backward.py's bar)
STATS_TOL = 1e-4        # running statistics: relative to max(1, max |ref|) (test_gpu_backward.py's bar)


def _model(c, decoder_weights):
    args = default_args(conv1_kernel_size=int(c["conv1_kernel_size"]))
    model = build_model(args)
    model.load_state_dict(bf.fixture_state_dict(model.state_dict(), decoder_weights, c), strict=True)
    return model.cuda()


def _inputs(c):
    x = SparseTensor(features=torch.from_numpy(c["feats"]), coordinates=torch.from_numpy(c["coords"]), device="cuda")
    return x, torch.from_numpy(c["raw_xyz"]).cuda()


def _compare(label, got, ref, report):
    got = got.detach().double().cpu()
    ref = torch.from_numpy(np.asarray(ref)).double()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    report.append((label, err, scale))
    return err, scale


def _print(name, mode, report):
    for label, err, scale in report:
        print(f"   {name} {mode} {label:52s} max|diff| {err:.3e}  scale {scale:.3e}")


@pytest.mark.parametrize("name", bf.backbone_cases())
def test_eval_backbone_matches_the_reference_run(name, decoder_weights):
    c = bf.load_backbone_case(name)
    model = _model(c, decoder_weights).eval()
    x, raw = _inputs(c)
    with torch.no_grad():
        pcd, aux, _, pos = model.forward_backbone(x, raw_coordinates=raw)
    assert torch.equal(pcd.C.cpu(), torch.from_numpy(c["coords"]))
    keep = torch.from_numpy(c["level0_rows"])
    report = []
    err, scale = _compare("pcd_features", pcd.F.cpu()[keep], c["pcd_features"], report)
    assert err <= TOL and err <= TOL * max(1.0, scale), (err, scale)
    enc = torch.cat([p.cpu() for p in pos[4][0]], 0)                  # one encoding per sample, in sample order
    perr, _ = _compare("pos_enc", enc[keep], c["pos_enc"], report)
    assert perr <= 1e-4, perr
    assert len(aux) == 5
    for i, fm in enumerate(aux):
        level = 4 - i
        Cg = fm.C.cpu().numpy()
        assert (Cg[:, 1:] % (1 << level) == 0).all(), i
        pos_of = {tuple(r): j for j, r in enumerate(Cg.tolist())}
        if level >= 2:                                               # every row stored: the coordinate SETS agree
            assert len(pos_of) == len(c[f"aux{i}_coords"]), (i, len(pos_of), len(c[f"aux{i}_coords"]))
        rows = [pos_of[tuple(r)] for r in c[f"aux{i}_coords"].tolist()]
        err, scale = _compare(f"aux{i} (stride {1 << level})", fm.F.cpu()[rows], c[f"aux{i}"], report)
        assert err <= TOL and err <= TOL * max(1.0, scale), (i, err, scale)
    _print(name, "eval", report)
    worst = max(report, key=lambda r: r[1])
    print(f"case {name} eval: worst max|diff| {worst[1]:.3e} ({worst[0]}, scale {worst[2]:.3e})")


def _oracle_train(sd0, c, R, masks=None):
    """float64 autograd through oracle/backbone.py in training mode.  With ``masks`` (0/1 per ReLU, forward order) every
    ReLU applies the given decisions instead of its own; returns (sd with .grad, [(pre-activation, mask)])."""
    sd = {k: (v.double().requires_grad_() if bf.is_fixture_weight(k) and v.is_floating_point() and "running" not in k
              else v.double() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    seen = []
    it = iter(masks) if masks is not None else None

    def relu(z):
        m = next(it) if it is not None else (z > 0).to(z.dtype)
        seen.append((z.detach(), m))
        return z * m

    ob.RELU = relu
    try:
        out, _ = ob.res16unet34c_forward(sd, ob.SparseLevels(c["coords"]), torch.from_numpy(c["feats"]).double(),
                                         bn=ob.batch_norm_train)
    finally:
        ob.RELU = torch.relu
    pcd = out @ sd["lin_squeeze_head.kernel"] + sd["lin_squeeze_head.bias"].reshape(1, -1)
    (pcd * R.double()).sum().backward()
    return sd, seen


@pytest.mark.parametrize("name", bf.train_cases())
def test_train_backbone_matches_the_reference_run(name, decoder_weights):
    """One training-mode forward_backbone + backward through the public API.  The output and the running statistics are
    compared with the fixture as they are.  The gradients are, too, once corrected for the ReLUs whose input lies within
    rounding of 0: there the fp32 forward may take the other branch than the float64 run of the fixture, and one such
    decision moves a BatchNorm bias gradient by percents (a kink of the function, not an error of either side).  The
    correction is the difference of two float64 oracle runs, one with the fixture's own decisions and one with the HIP
    forward's; every differing decision must sit at a pre-activation within 1e-4 of 0 relative to its layer."""
    from gpu_util import internal_to_oracle_rows
    c = bf.load_backbone_case(name, train=True)
    model = _model(c, decoder_weights).train()
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    x, raw = _inputs(c)
    pcd, _, _, _ = model.forward_backbone(x, raw_coordinates=raw)
    # the HIP forward's ReLU decisions, in the oracle's row order (read before the backward frees the activations)
    fn = pcd.F.grad_fn                                               # BackboneFn's node holds the tape
    while not hasattr(fn, "holder"):
        fn = fn.next_functions[0][0]
    tape = fn.holder.tape
    lv = ob.SparseLevels(c["coords"])
    maps = [torch.from_numpy(internal_to_oracle_rows(pcd._a3d.scene, lv, i)) for i in range(5)]
    masks = []
    for level, node in tape.relu_levels:
        m = torch.empty(node.v.shape, dtype=torch.float64)
        m[maps[level]] = (node.v > 0).cpu().double()
        masks.append(m)
    R = bf.grad_probe(name, len(c["coords"])).cuda()
    (pcd.F * R).sum().backward()
    keep = torch.from_numpy(c["level0_rows"])
    report = []
    err, scale = _compare("pcd_features", pcd.F.detach().cpu()[keep], c["pcd_features"], report)
    assert err <= TOL and err <= TOL * max(1.0, scale), (err, scale)
    state = model.state_dict()
    n_state = 0
    worst_stats = ("", 0.0)
    for k in c:
        if k.startswith("state::"):
            n = k[len("state::"):]
            err, scale = _compare(n, state[n], c[k], report)
            worst_stats = max(worst_stats, (n, err / max(1.0, scale)), key=lambda t: t[1])
            n_state += 1
    # the kink correction
    sd_own, _ = _oracle_train(sd0, c, R.cpu())
    sd_hip, seen = _oracle_train(sd0, c, R.cpu(), masks)
    assert len(seen) == 1 + 8 + 2 * sum(ob.LAYERS)
    n_flip, flip_max = 0, 0.0
    for z, m in seen:
        flip = (z > 0) != (m > 0)
        if flip.any():
            n_flip += int(flip.sum())
            rel = z[flip].abs().max().item() / max(1.0, z.abs().max().item())
            flip_max = max(flip_max, rel)
    params = dict(model.named_parameters())
    n_grad = 0
    worst_grad = worst_raw = ("", 0.0)
    for k in c:
        if not k.startswith("grad::"):
            continue
        n = k[len("grad::"):]
        g, g_own, g_hip = params[n].grad, sd_own[n].grad, sd_hip[n].grad
        assert g is not None, n
        if "grad_cin::" + n in c:
            cin = torch.from_numpy(c["grad_cin::" + n])
            g, g_own, g_hip = g[:, cin.cuda()], g_own[:, cin], g_hip[:, cin]
        ref = torch.from_numpy(c[k]).double()
        denom = max(1e-3, ref.abs().max().item())
        err, scale = _compare(f"d {n}", g.double().cpu() - (g_hip - g_own), c[k], report)
        worst_grad = max(worst_grad, (n, err / denom), key=lambda t: t[1])
        raw_err = (g.double().cpu() - ref).abs().max().item()
        worst_raw = max(worst_raw, (n, raw_err / denom), key=lambda t: t[1])
        n_grad += 1
    _print(name, "train", report)
    print(f"case {name} train: pcd_features max|diff| {report[0][1]:.3e} (scale {report[0][2]:.3e}); {n_state} running "
          f"statistics, worst relative {worst_stats[1]:.3e} ({worst_stats[0]}); {n_grad} gradients, worst relative "
          f"{worst_grad[1]:.3e} ({worst_grad[0]}); {n_flip} ReLU decisions at a kink (|x| <= {flip_max:.1e} of the "
          f"layer's max), uncorrected worst relative {worst_raw[1]:.3e} ({worst_raw[0]})")
    assert n_state == 2 * 62 and n_grad == 2 * 62 + 11, (n_state, n_grad)
    assert worst_stats[1] <= STATS_TOL, worst_stats
    assert flip_max <= 1e-4, flip_max
    assert worst_grad[1] <= GRAD_TOL, worst_grad
