#!/usr/bin/env python3
"""Generate the backbone fixtures by RUNNING THE REFERENCE's own ``Agile3d.forward_backbone``.

Runs only in the build container (needs /root/reference, which never travels to the GPU box).  The reference's
``models`` package is imported over ``me_functional`` (a working MinkowskiEngine stand-in built from torch's dense
operators), the reference ``Agile3d`` is built and loaded with ``strict=True`` from
  * backbone + lin_squeeze_head: the formula of ``tests/backbone_fixture.py`` (37.9 M parameters, not committed);
  * everything else: the committed ``decoder_weights.npz`` (its ``pos_enc.gauss_B`` feeds the position encoding),
and run in float64 (the position encoding in float32, as ``get_pos_encs`` casts) on three synthetic scenes:
  a    2 k voxels of room-like surfaces in [-24, 23]^3 plus isolated voxels, conv1_kernel_size 5
  b    a batch of two such scenes of different sizes, conv1_kernel_size 5
  c    one scene, conv1_kernel_size 3
Eval mode (every case), ``backbone_case_<name>.npz``: inputs, ``pcd_features`` after ``lin_squeeze_head``, the five
``aux`` feature maps with their coordinates (stride multiples, as MinkowskiEngine stores them) and the finest-level
position encoding.  The reference's CPU branch (agile3d.py:146-150) encodes a whole batch as one range; the project
follows the GPU branch (one range per sample), so the encoding stored for a batch is ``get_pos_encs`` run on each
sample alone.
Train mode (a and b), ``backbone_case_<name>_train.npz``: one ``model.train()`` forward from the formula's running
statistics: ``pcd_features``, every BatchNorm's updated running statistics, and for L = sum(pcd_features * R) (R from
``backbone_fixture.grad_probe``) the float64 autograd gradients of every BatchNorm weight and bias, the stem kernel,
``lin_squeeze_head``, one 3^3 kernel per level, a stride-2 kernel, a transposed kernel and a 1x1 projection.
Every committed file stays below 1 MiB: level-0 rows (and the level-1 rows of the aux map) are stored for a fixed
subset of rows (``level0_rows``, every 6th / 8th row of the input order; every 2nd row at level 1), large kernel
gradients for a fixed subset of input channels (``grad_cin::<name>``).

  python tests/golden/make_backbone_goldens.py            write the fixtures
  python tests/golden/make_backbone_goldens.py --check    regenerate and compare with the committed files (1 fp32 ulp)
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

import me_functional  # noqa: E402
import backbone_fixture as bf  # noqa: E402

MAX_FILE_BYTES = 1 << 20
LEVEL0_ROW_STEP = 6           # level-0 rows kept: every 6th row of the input order
LEVEL1_ROW_STEP = 2
LEVEL0_ROW_STEP_TRAIN = 8     # (the train-mode output is pinned through the gradients as well)
GRAD_CIN_KEEP = 4             # kernel gradients of more than GRAD_FULL_MAX elements: 4 input channels kept
GRAD_FULL_MAX = 20000
GRAD_KERNELS = [
    "backbone.conv0p1s1.kernel",            # the stem
    "lin_squeeze_head.kernel", "lin_squeeze_head.bias",
    "backbone.block8.1.conv2.kernel",       # 3^3, level 0
    "backbone.block1.1.conv1.kernel",       # 3^3, level 1
    "backbone.block6.0.conv2.kernel",       # 3^3, level 2
    "backbone.block3.2.conv1.kernel",       # 3^3, level 3
    "backbone.block4.5.conv2.kernel",       # 3^3, level 4
    "backbone.conv2p2s2.kernel",            # stride 2, level 1 -> 2
    "backbone.convtr7p2s2.kernel",          # transposed, level 1 -> 0
    "backbone.block8.0.downsample.0.kernel",   # 1x1 projection, level 0
]


# ----------------------------------------------------------------------------- scenes
def _shell(lo, hi):
    g = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3)
    on = np.zeros(len(g), bool)
    for ax in range(3):
        on |= (g[:, ax] == lo[ax]) | (g[:, ax] == hi[ax])
    return g[on]


def make_surfaces(seed, n_target, lo=-24, hi=23, n_isolated=6):
    """Room-like surfaces: a floor, two walls and box shells in [lo, hi]^3, plus isolated voxels (no neighbour
    within 2 cells: alone under every kernel of the stem)."""
    rng = np.random.default_rng(seed)
    w = hi - lo
    f = [int(lo + rng.integers(0, 4))]
    parts = [np.stack(np.meshgrid(np.arange(lo, hi + 1), np.arange(lo, hi + 1), f, indexing="ij"), -1).reshape(-1, 3)]
    parts[0] = parts[0][rng.random(len(parts[0])) < 0.15 * n_target / 1000]  # a ragged floor
    wall_h = max(3, round(w * n_target / 8000))
    for ax in (0, 1):
        wall = _shell([lo, lo, lo], [hi, hi, hi])
        parts.append(wall[(wall[:, ax] == lo) & (wall[:, 2] < f[0] + wall_h)])
    pts = np.unique(np.concatenate(parts), axis=0)
    while len(pts) < n_target:
        size = rng.integers(3, 11, 3)
        a = rng.integers(lo, hi - size + 1)
        box = _shell(a, a + size)
        new = np.unique(np.concatenate([pts, box]), axis=0)
        if len(new) > n_target * 1.02:
            continue
        pts = new
    occupied = {tuple(p) for p in pts.tolist()}
    iso = []
    while len(iso) < n_isolated:
        p = rng.integers(lo, hi + 1, 3)
        near = [(p[0] + dx, p[1] + dy, p[2] + dz) for dx in range(-2, 3) for dy in range(-2, 3) for dz in range(-2, 3)]
        if not any(q in occupied for q in near):
            iso.append(p)
            occupied.add(tuple(p.tolist()))
    pts = np.concatenate([pts, np.array(iso)])
    return pts[rng.permutation(len(pts))].astype(np.int32)


def make_input(specs, seed):
    """specs: list of (n_target, seed) per batch sample -> coords [N,4], feats [N,3], raw xyz [N,3], sample sizes."""
    cs, fs, rs = [], [], []
    for b, (n, s) in enumerate(specs):
        p = make_surfaces(s, n)
        rng = np.random.default_rng(seed * 100 + b)
        cs.append(np.concatenate([np.full((len(p), 1), b, np.int32), p], 1))
        fs.append(rng.random((len(p), 3), dtype=np.float32))
        raw = (p.astype(np.float32) + rng.random((len(p), 3), dtype=np.float32)) * np.float32(0.02)
        rs.append((raw - raw.min(0, keepdims=True)).astype(np.float32))
    return np.concatenate(cs), np.concatenate(fs), np.concatenate(rs), [len(c) for c in cs]


CASES = {
    "a": dict(specs=[(2200, 11)], seed=1, conv1=5, train=True),
    "b": dict(specs=[(1300, 12), (800, 13)], seed=2, conv1=5, train=True),
    "c": dict(specs=[(1800, 14)], seed=3, conv1=3, train=False),
}


# ----------------------------------------------------------------------------- the reference
def build_reference(conv1, decoder_weights):
    me_functional.install()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    if REPO not in sys.path:
        sys.path.insert(1, REPO)
    import models as ref_models
    from agile3d_amd.model import default_args
    ref = ref_models.build_model(default_args(conv1_kernel_size=conv1))
    shapes = ref.state_dict()
    w = bf.backbone_weights(shapes)
    sd = {}
    for k, v in shapes.items():
        sd[k] = w[k] if bf.is_fixture_weight(k) else torch.from_numpy(decoder_weights[k])
    print("strict load into the reference:", ref.load_state_dict(sd, strict=True))
    ref.backbone.double()
    ref.lin_squeeze_head.double()
    return ref, w


def _rows(n, step):
    return np.arange(0, n, step, dtype=np.int64)


def run_case(name, spec, decoder_weights):
    me = me_functional
    coords, feats, raw, sizes = make_input(spec["specs"], spec["seed"])
    ref, w = build_reference(spec["conv1"], decoder_weights)
    names, sums = bf.weight_sums(w)
    n = len(coords)
    keep0 = _rows(n, LEVEL0_ROW_STEP)
    base = dict(coords=coords, feats=feats, raw_xyz=raw, sample_sizes=np.array(sizes, np.int64),
                conv1_kernel_size=np.int64(spec["conv1"]), weight_names=np.array(names), weight_sums=sums,
                level0_rows=keep0)

    def inputs():
        x = me.SparseTensor(torch.from_numpy(feats).double(), coordinates=torch.from_numpy(coords))
        return x, torch.from_numpy(raw)

    # ---- eval mode
    ref.eval()
    with torch.no_grad():
        x, r = inputs()
        pcd, aux, coordinates, _ = ref.forward_backbone(x, raw_coordinates=r)
        assert torch.equal(pcd.C, torch.from_numpy(coords)), "stride-1 set must keep the input row order"
        pos, off = [], 0
        for s in sizes:     # one range per sample (the GPU branch), see the module docstring
            st = me.SparseTensor(r[off:off + s], coordinates=torch.from_numpy(coords[off:off + s]))
            pos.append(ref.get_pos_encs([st])[0][0][0])
            off += s
        pos = torch.cat(pos, 0)
    ev = dict(base, pcd_features=pcd.F[keep0].float().numpy(), pos_enc=pos[keep0].float().numpy())
    stats = {"pcd_features": pcd.F.abs().max().item()}
    for i, fm in enumerate(aux):
        level = 4 - i
        Fm, Cm = fm.F.float().numpy(), fm.C.numpy()
        if level <= 1:
            keep = keep0 if level == 0 else _rows(len(Fm), LEVEL1_ROW_STEP)
            Fm, Cm = Fm[keep], Cm[keep]
        ev[f"aux{i}"], ev[f"aux{i}_coords"] = Fm, Cm
        ev[f"aux{i}_stride"] = np.int64(fm.tensor_stride[0])
        zero = float((fm.F == 0).double().mean())
        stats[f"aux{i} (stride {fm.tensor_stride[0]}, {len(fm)} rows, zero {zero:.2f})"] = fm.F.abs().max().item()
        assert zero <= 0.9, (name, i, zero)
    assert 0.3 <= stats["pcd_features"] <= 30, stats
    out = {f"backbone_case_{name}.npz": ev}
    print(f"case {name}: {n} voxels, samples {sizes}, eval scales", {k: round(v, 3) for k, v in stats.items()})

    # ---- train mode
    if spec["train"]:
        ref.train()
        for k, p in ref.named_parameters():
            p.grad = None
        x, r = inputs()
        pcd, aux, _, _ = ref.forward_backbone(x, raw_coordinates=r)
        R = bf.grad_probe(name, n).double()
        (pcd.F * R).sum().backward()
        scale = pcd.F.abs().max().item()
        assert 0.3 <= scale <= 30, scale
        for i, fm in enumerate(aux):
            assert float((fm.F == 0).double().mean()) <= 0.9, (name, "train", i)
        keep_t = _rows(n, LEVEL0_ROW_STEP_TRAIN)
        tr = dict(base, level0_rows=keep_t, pcd_features=pcd.F.detach()[keep_t].float().numpy())
        params = dict(ref.named_parameters())
        bufs = dict(ref.named_buffers())
        for k, v in bufs.items():
            if "running_" in k and bf.is_fixture_weight(k):
                tr[f"state::{k}"] = v.float().numpy()
        gnames = [k for k in params if k.endswith(("bn.weight", "bn.bias"))] + GRAD_KERNELS
        for k in gnames:
            g = params[k].grad
            assert g is not None, k
            if g.dim() == 3 and g.numel() > GRAD_FULL_MAX:
                cin = np.linspace(0, g.shape[1] - 1, GRAD_CIN_KEEP).round().astype(np.int64)
                g = g[:, torch.from_numpy(cin)]
                tr[f"grad_cin::{k}"] = cin
            tr[f"grad::{k}"] = g.float().numpy()
        out[f"backbone_case_{name}_train.npz"] = tr
        print(f"case {name}: train pcd scale {scale:.3f}, {len(gnames)} gradients")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixtures")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    torch.set_num_threads(os.cpu_count() or 1)
    z = np.load(os.path.join(HERE, "decoder_weights.npz"))
    decoder_weights = {k: z[k] for k in z.files}
    worst = 0.0
    for name in a.cases.split(","):
        files = run_case(name, CASES[name], decoder_weights)
        for fname, arrays in files.items():
            path = os.path.join(a.out, fname)
            if a.check:
                old = np.load(path)
                assert sorted(old.files) == sorted(arrays), (fname, set(old.files) ^ set(arrays))
                for k, v in arrays.items():
                    o = old[k]
                    assert o.shape == v.shape and o.dtype == v.dtype, (fname, k)
                    if v.dtype == np.float32:
                        mag = np.maximum(np.abs(o), np.float32(1e-6) * np.abs(o).max(initial=0.0))
                        ulp = np.spacing(mag.astype(np.float32))
                        d = float((np.abs(v.astype(np.float64) - o) / ulp).max()) if v.size else 0.0
                        worst = max(worst, d)
                        assert d <= 1.0, (fname, k, d)
                    else:
                        assert np.array_equal(o, v), (fname, k)
                print(f"{fname}: reproduces")
            else:
                with tempfile.NamedTemporaryFile(dir=a.out, suffix=".npz", delete=False) as f:
                    np.savez_compressed(f, **arrays)
                os.replace(f.name, path)
                os.chmod(path, 0o644)
                size = os.path.getsize(path)
                print(f"{fname}: {size / 1024:.0f} KiB")
                assert size < MAX_FILE_BYTES, (fname, size)
    if a.check:
        print(f"all fixtures reproduce (worst {worst:.2f} fp32 ulp)")


if __name__ == "__main__":
    main()
