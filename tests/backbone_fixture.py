"""Backbone weights for the reference-run backbone fixtures (tests/golden/backbone_case_*.npz), made by formula.

The backbone has 37.9 M parameters: too many to commit.  Every element is instead a counter-based hash of (tensor
name, element index) -- splitmix64 -- mapped onto the tensor's range, so that the generator and every test, on any
machine, build bit-identical fp32 weights without a random-number stream.  The fixtures store each tensor's float64
sum and sum of squares; ``check_weight_sums`` compares them before a test uses the weights.

  kernels        U(-a, a), a = sqrt(3 / fan_in) * KERNEL_GAIN, fan_in = kernel volume * Cin
  conv biases    U(-0.1, 0.1)
  BN weight      U(0.8, 1.2)        BN bias       U(-0.1, 0.1)
  running_mean   U(-0.1, 0.1)       running_var   U(0.5, 1.5)
"""
from __future__ import annotations

import os

import numpy as np
import torch

KERNEL_GAIN = 1.5
_GAMMA = np.uint64(0x9E3779B97F4A7C15)


def _fnv1a(name: str) -> np.uint64:
    h = 0xCBF29CE484222325
    for b in name.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(h)


def hash_uniform(name: str, n: int) -> np.ndarray:
    """n float64 values in [0, 1): splitmix64 of (fnv1a(name) + (i + 1) * gamma), top 53 bits."""
    with np.errstate(over="ignore"):
        z = _fnv1a(name) + (np.arange(1, n + 1, dtype=np.uint64) * _GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53))


def hash_tensor(name: str, shape, lo: float, hi: float) -> torch.Tensor:
    """fp32 tensor of ``shape`` with elements lo + (hi - lo) * hash_uniform(name)."""
    n = int(np.prod(shape)) if len(shape) else 1
    v = lo + (hi - lo) * hash_uniform(name, n)
    return torch.from_numpy(v.astype(np.float32).reshape(tuple(shape)))


def is_fixture_weight(name: str) -> bool:
    return name.startswith(("backbone.", "lin_squeeze_head."))


def weight_value(name: str, shape) -> torch.Tensor:
    if name.endswith("num_batches_tracked"):
        return torch.zeros((), dtype=torch.int64)
    if name.endswith(".kernel"):
        fan_in = shape[0] * shape[1] if len(shape) == 3 else shape[0]
        a = (3.0 / fan_in) ** 0.5 * KERNEL_GAIN
        return hash_tensor(name, shape, -a, a)
    if name.endswith("bn.weight"):
        return hash_tensor(name, shape, 0.8, 1.2)
    if name.endswith("bn.running_var"):
        return hash_tensor(name, shape, 0.5, 1.5)
    if name.endswith(("bn.bias", "bn.running_mean", ".bias")):
        return hash_tensor(name, shape, -0.1, 0.1)
    raise KeyError(f"no formula for {name}")


def backbone_weights(shapes: dict) -> dict:
    """{name: tensor} for every backbone / lin_squeeze_head entry of ``shapes`` (name -> shape, e.g. a state_dict)."""
    out = {}
    for k, v in shapes.items():
        if is_fixture_weight(k):
            out[k] = weight_value(k, tuple(v.shape) if torch.is_tensor(v) else tuple(v))
    return out


def weight_sums(weights: dict):
    """(sorted names, float64 [n, 2] of sum and sum of squares) over the floating-point entries."""
    names = sorted(k for k, v in weights.items() if v.is_floating_point())
    sums = np.array([[weights[k].double().sum().item(), weights[k].double().square().sum().item()] for k in names])
    return names, sums


def check_weight_sums(weights: dict, fixture) -> None:
    """Fail loudly if the formula no longer makes the weights the fixture was generated with."""
    names, sums = weight_sums(weights)
    assert names == [str(s) for s in fixture["weight_names"]], "the fixture's weight names differ"
    ref = fixture["weight_sums"]
    bad = [n for n, a, b in zip(names, sums, ref) if not np.allclose(a, b, rtol=1e-12, atol=1e-9)]
    assert not bad, f"weights drifted from the fixture: {bad[:5]}"


def grad_probe(name: str, n: int) -> torch.Tensor:
    """The seeded R of L = sum(pcd_features * R) for fixture ``name``: fp32 [n, 128] in [-1, 1)."""
    return hash_tensor(f"R:{name}", (n, 128), -1.0, 1.0)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def backbone_cases():
    return sorted(f[len("backbone_case_"):-4] for f in os.listdir(GOLDEN)
                  if f.startswith("backbone_case_") and f.endswith(".npz") and not f.endswith("_train.npz"))


def train_cases():
    return sorted(f[len("backbone_case_"):-len("_train.npz")] for f in os.listdir(GOLDEN)
                  if f.startswith("backbone_case_") and f.endswith("_train.npz"))


def load_backbone_case(name: str, train: bool = False) -> dict:
    z = np.load(os.path.join(GOLDEN, f"backbone_case_{name}{'_train' if train else ''}.npz"))
    return {k: z[k] for k in z.files}


def fixture_state_dict(shapes: dict, decoder_weights: dict, fixture) -> dict:
    """The full state dict a fixture was generated with: the formula's backbone + lin_squeeze_head (checked against
    the fixture's sums) and the committed decoder weights for everything else."""
    w = backbone_weights(shapes)
    check_weight_sums(w, fixture)
    sd = {}
    for k in shapes:
        v = w[k] if k in w else decoder_weights[k]
        sd[k] = v if torch.is_tensor(v) else torch.from_numpy(v)
    return sd
