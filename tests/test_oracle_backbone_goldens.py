"""The CPU oracle of the backbone (oracle/backbone.py) against fixtures made by running the REFERENCE's own
``Agile3d.forward_backbone`` (tests/golden/make_backbone_goldens.py over the MinkowskiEngine stand-in
tests/golden/me_functional.py): topology, cat order, BatchNorm momenta and running-statistics rule, coarse and fine
coordinate sets.  The oracle runs in float64; the fixtures are float64 results rounded to fp32.  Negative controls show
that the fixtures tell the kernel-offset enumeration and the blocks' BatchNorm momentum apart."""
import numpy as np
import pytest
import torch

import backbone_fixture as bf
from oracle import backbone as ob
from oracle.decoder import fourier_pos_enc

TOL = 2e-6          # relative to max(1, max |ref|): the fixture is fp32-rounded float64


@pytest.fixture(scope="module")
def weights(decoder_weights):
    """{conv1_kernel_size: float64 state dict} built by the formula (weight sums checked against each fixture)."""
    from agile3d_amd.model import build_model, default_args
    out = {}
    for name in bf.backbone_cases():
        c = bf.load_backbone_case(name)
        k = int(c["conv1_kernel_size"])
        shapes = build_model(default_args(conv1_kernel_size=k)).state_dict()
        sd = bf.fixture_state_dict(shapes, decoder_weights, c)
        out[k] = {n: (v.double() if v.is_floating_point() and bf.is_fixture_weight(n) else v) for n, v in sd.items()}
    return out


def _err(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    got = got.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item()) if ref.numel() else 1.0
    return (got - ref).abs().max().item() / scale if ref.numel() else 0.0


def _rows_by_coords(oracle_coords, fixture_coords):
    pos = {tuple(r): i for i, r in enumerate(oracle_coords.tolist())}
    assert len(pos) == len(oracle_coords)
    return [pos[tuple(r)] for r in fixture_coords.tolist()]


def _eval_errors(sd, c):
    coords = c["coords"]
    lv = ob.SparseLevels(coords)
    feats = torch.from_numpy(c["feats"]).double()
    with torch.no_grad():
        out, fm = ob.res16unet34c_forward(sd, lv, feats)
        Wh = sd["lin_squeeze_head.kernel"]
        pcd = out @ Wh + sd["lin_squeeze_head.bias"].reshape(1, -1)
    keep = c["level0_rows"]
    errs = {"pcd_features": _err(pcd[keep], c["pcd_features"])}
    for i, f in enumerate(fm):
        level = 4 - i
        assert int(c[f"aux{i}_stride"]) == 1 << level
        oc = lv.levels[level].copy()
        oc[:, 1:] *= 1 << level
        if level >= 2:      # all rows stored: the coordinate SETS are equal
            assert len(oc) == len(c[f"aux{i}_coords"]), (i, len(oc), len(c[f"aux{i}_coords"]))
        rows = _rows_by_coords(oc, c[f"aux{i}_coords"])
        errs[f"aux{i}"] = _err(f[rows], c[f"aux{i}"])
    return errs


def _pos_enc(sd, c):
    raw = torch.from_numpy(c["raw_xyz"])
    parts, off = [], 0
    for n in c["sample_sizes"].tolist():       # one range per sample
        r = raw[off:off + n]
        parts.append(fourier_pos_enc(r, sd["pos_enc.gauss_B"], r.min(0)[0], r.max(0)[0]))
        off += n
    return torch.cat(parts)[c["level0_rows"]]


@pytest.mark.parametrize("name", bf.backbone_cases())
def test_eval_forward_matches_the_reference_run(weights, name):
    c = bf.load_backbone_case(name)
    sd = weights[int(c["conv1_kernel_size"])]
    errs = _eval_errors(sd, c)
    perr = (_pos_enc(sd, c).double() - torch.from_numpy(c["pos_enc"]).double()).abs().max().item()
    print(f"case {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f", pos_enc {perr:.2e}")
    assert max(errs.values()) <= TOL, errs
    assert perr <= 2e-6


def _train_run(sd0, c, name, bn=ob.batch_norm_train):
    sd = {k: (v.clone().requires_grad_() if v.is_floating_point() and bf.is_fixture_weight(k) and "running" not in k
              else v.clone()) for k, v in sd0.items()}
    lv = ob.SparseLevels(c["coords"])
    out, _ = ob.res16unet34c_forward(sd, lv, torch.from_numpy(c["feats"]).double(), bn=bn)
    pcd = out @ sd["lin_squeeze_head.kernel"] + sd["lin_squeeze_head.bias"].reshape(1, -1)
    (pcd * bf.grad_probe(name, len(pcd)).double()).sum().backward()
    return sd, pcd.detach()


def _train_errors(sd, pcd, c):
    errs = {"pcd_features": _err(pcd[c["level0_rows"]], c["pcd_features"])}
    for k in c:
        if k.startswith("state::"):
            errs[k] = _err(sd[k[len("state::"):]], c[k])
        elif k.startswith("grad::"):
            n = k[len("grad::"):]
            g = sd[n].grad
            if "grad_cin::" + n in c:
                g = g[:, torch.from_numpy(c["grad_cin::" + n])]
            ref = torch.from_numpy(c[k]).double()
            errs[k] = (g.double() - ref).abs().max().item() / max(1e-3, ref.abs().max().item())
    return errs


@pytest.mark.parametrize("name", bf.train_cases())
def test_train_forward_running_stats_and_gradients_match_the_reference_run(weights, name):
    c = bf.load_backbone_case(name, train=True)
    sd, pcd = _train_run(weights[int(c["conv1_kernel_size"])], c, name)
    errs = _train_errors(sd, pcd, c)
    n_state = sum(k.startswith("state::") for k in errs)
    n_grad = sum(k.startswith("grad::") for k in errs)
    assert n_state == 2 * 62 and n_grad == 2 * 62 + 11, (n_state, n_grad)
    worst = max(errs, key=errs.get)
    print(f"case {name} (train): pcd_features {errs['pcd_features']:.2e}, {n_state} running statistics, {n_grad} "
          f"gradients, worst {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= TOL, (worst, errs[worst])


def test_negative_control_kernel_order(weights):
    """The same weights read in the other (z fastest) kernel-offset enumeration miss the fixture by far more than the
    tolerance: the fixture pins the enumeration the stand-in uses, and a kernel-order slip in the oracle would show."""
    from agile3d_amd.model import convert_kernel_order
    c = bf.load_backbone_case("a")
    sd = convert_kernel_order(weights[int(c["conv1_kernel_size"])], "z_fastest")
    errs = _eval_errors(sd, c)
    print("z-fastest weights:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["pcd_features"] > 100 * TOL and min(errs.values()) > 100 * TOL, errs


def test_negative_control_block_bn_momentum(weights):
    """BasicBlock norms with bn_momentum 0.02 (instead of the class default 0.1 the reference's _make_layer leaves
    them) miss the fixture's running statistics by far more than the tolerance."""
    c = bf.load_backbone_case("a", train=True)

    def bn_002(x, sd, prefix):
        return ob.batch_norm_train(x, sd, prefix, momentum=0.02)

    sd, pcd = _train_run(weights[int(c["conv1_kernel_size"])], c, "a", bn=bn_002)
    errs = _train_errors(sd, pcd, c)
    block = [v for k, v in errs.items() if k.startswith("state::") and k.endswith(("norm1.bn.running_var",
                                                                                  "norm2.bn.running_var"))]
    print(f"block momentum 0.02: worst running-statistics error {max(block):.2e}, smallest {min(block):.2e}")
    assert min(block) > 100 * TOL
    assert errs["pcd_features"] <= TOL            # (batch statistics: the forward itself does not change)
