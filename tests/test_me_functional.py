"""Known-answer cases for the MinkowskiEngine stand-in that runs the reference's backbone for the fixtures
(tests/golden/me_functional.py).  CPU only; independent of the project's oracle and library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import me_functional as mef  # noqa: E402


def _st(coords, feats):
    return mef.SparseTensor(torch.as_tensor(feats, dtype=torch.float64),
                            coordinates=torch.as_tensor(coords, dtype=torch.int32))


def _conv(cin, cout, k, stride=1, transpose=False, bias=False):
    cls = mef.MinkowskiConvolutionTranspose if transpose else mef.MinkowskiConvolution
    m = cls(cin, cout, kernel_size=k, stride=stride, bias=bias,
            kernel_generator=mef.KernelGenerator(k, stride, 1, region_type=mef.RegionType.HYPER_CUBE))
    return m.double()


def _rows_by_coord(t):
    return {tuple(c[1:]): i for i, c in enumerate(t.C.tolist())}


def test_two_voxels_one_hot_kernels_pin_the_offset_index():
    """Voxel B = A + (1, 0, 0): the one-hot kernel at k moves B's feature onto A iff k is the offset (+1, 0, 0), which
    x fastest is k = 2 + 3 * 1 + 9 * 1 = 14 (and the centre 13 is the identity)."""
    x = _st([[0, 0, 0, 0], [0, 1, 0, 0]], [[1.0], [10.0]])
    conv = _conv(1, 1, 3)
    for k, expect in {13: [1.0, 10.0], 14: [10.0, 0.0], 12: [0.0, 1.0], 16: [0.0, 0.0], 22: [0.0, 0.0]}.items():
        with torch.no_grad():
            conv.kernel.zero_()
            conv.kernel[k] = 1.0
        assert conv(x).F.reshape(-1).tolist() == expect, k
    # the other axes: B = A + (0, 1, 0) sits at k = 1 + 3 * 2 + 9 = 16, B = A + (0, 0, 1) at k = 1 + 3 + 18 = 22
    for c_b, k in (((0, 1, 0), 16), ((0, 0, 1), 22), ((-1, -1, -1), 0), ((1, 1, 1), 26)):
        x = _st([[0, 0, 0, 0], [0, *c_b]], [[1.0], [10.0]])
        with torch.no_grad():
            conv.kernel.zero_()
            conv.kernel[k] = 1.0
        assert conv(x).F.reshape(-1).tolist() == [10.0, 0.0], (c_b, k)


def test_5x5x5_offset_and_bias():
    x = _st([[0, 4, 4, 4], [0, 6, 3, 4]], [[1.0, 2.0], [3.0, -1.0]])
    conv = _conv(2, 1, 5, bias=True)
    with torch.no_grad():
        conv.kernel.zero_()
        conv.kernel[4 + 5 * 1 + 25 * 2] = torch.tensor([[1.0], [100.0]])   # offset (+2, -1, 0)
        conv.bias.fill_(0.5)
    assert conv(x).F.reshape(-1).tolist() == [3.0 - 100.0 + 0.5, 0.5]


def test_full_block_collapses_to_one_coarse_voxel():
    blk = [[0, x, y, z] for z in (2, 3) for y in (4, 5) for x in (0, 1)]
    feats = torch.arange(8.0).reshape(8, 1)
    x = _st(blk, feats)
    conv = _conv(1, 1, 2, stride=2)
    with torch.no_grad():
        conv.kernel.copy_(torch.arange(8.0).reshape(8, 1, 1))            # W[k] = k, slot k = x + 2y + 4z
    y = conv(x)
    assert y.C.tolist() == [[0, 0, 4, 2]] and y.tensor_stride == [2, 2, 2]
    # row i of blk is child slot i, so out = sum_k k * x_k = sum_k k^2
    assert y.F.item() == float(sum(k * k for k in range(8)))
    pool = mef.MinkowskiAvgPooling(kernel_size=2, stride=2, dimension=3)
    p = pool(x)
    assert p.coordinate_map_key == y.coordinate_map_key and float(p.F) == 3.5


def test_transposed_conv_writes_the_cached_fine_set():
    fine = [[0, 1, 0, 0], [0, 0, 0, 0], [0, 3, 2, 1], [0, 2, 3, 0]]      # two coarse parents, in a scrambled order
    x = _st(fine, torch.zeros(4, 1))
    down = _conv(1, 3, 2, stride=2)
    coarse = down(x)
    assert sorted(coarse.C.tolist()) == [[0, 0, 0, 0], [0, 2, 2, 0]]
    coarse = coarse._like(torch.tensor([[1.0, 2.0, 3.0], [10.0, 20.0, 30.0]], dtype=torch.float64)
                          if coarse.C[0, 1] == 0 else torch.tensor([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0]],
                                                                   dtype=torch.float64))
    up = _conv(3, 1, 2, stride=2, transpose=True)
    with torch.no_grad():
        up.kernel.copy_(torch.arange(8.0).reshape(8, 1, 1).expand(8, 3, 1))   # W[k] = k for every input channel
    y = up(coarse)
    assert y.coordinate_map_key == x.coordinate_map_key and torch.equal(y.C, x.C)   # the fine set, its row order
    # out_fine[c + bits(k)] = in[c] @ W[k]: slot of (1,0,0) is 1, of (0,0,0) 0, of (3,2,1)-(2,2,0) = (1,0,1) 5,
    # of (2,3,0)-(2,2,0) = (0,1,0) 2
    assert y.F.reshape(-1).tolist() == [6.0 * 1, 0.0, 60.0 * 5, 60.0 * 2]
    assert mef.cat(y, x).F.shape == (4, 2)
    with pytest.raises(AssertionError):
        mef.cat(y, coarse)


def test_negative_coordinates_floor():
    x = _st([[0, -1, -2, -3], [0, 0, 0, 0], [0, -2, -1, -4]], torch.ones(3, 1))
    conv = _conv(1, 1, 2, stride=2)
    with torch.no_grad():
        conv.kernel.fill_(1.0)
    y = conv(x)
    got = {tuple(c): float(f) for c, f in zip(y.C.tolist(), y.F.reshape(-1).tolist())}
    assert got == {(0, -2, -2, -4): 2.0, (0, 0, 0, 0): 1.0}
    # one more level down, from stride 2 to stride 4
    z = _conv(1, 1, 2, stride=2)
    with torch.no_grad():
        z.kernel.fill_(1.0)
    assert sorted(z(y).C.tolist()) == [[0, -4, -4, -4], [0, 0, 0, 0]]


def test_batch_norm_ignores_empty_cells():
    """BatchNorm over the occupied rows only, in both modes; a following conv sees zeros in the empty cells even though
    BN moved every occupied row."""
    g = torch.Generator().manual_seed(0)
    coords = [[0, i, 2 * i % 5, 0] for i in range(6)]
    feats = torch.randn(6, 3, generator=g, dtype=torch.float64)
    bn = mef.MinkowskiBatchNorm(3, momentum=0.02).double()
    bn.train()
    y = bn(_st(coords, feats))
    ref = torch.nn.functional.batch_norm(feats, None, None, training=True, eps=1e-5)
    assert torch.allclose(y.F, ref, atol=1e-12)
    assert torch.allclose(bn.bn.running_mean, 0.02 * feats.mean(0), atol=1e-15)
    assert torch.allclose(bn.bn.running_var, 0.98 + 0.02 * feats.var(0, unbiased=True), atol=1e-15)
    bn.eval()
    assert torch.allclose(bn(_st(coords, feats)).F,
                          (feats - bn.bn.running_mean) / torch.sqrt(bn.bn.running_var + 1e-5), atol=1e-12)
    shifted = _st(coords, feats)._like(feats + 5.0)           # every occupied row non-zero: empty cells stay zero
    conv = _conv(3, 1, 3)
    with torch.no_grad():
        conv.kernel.fill_(1.0)
    rows = _rows_by_coord(shifted)
    a = rows[(0, 0, 0)]
    # (0,0,0)'s only occupied neighbour under a 3^3 kernel is itself ((1,2,0) is 2 cells away in y)
    assert torch.allclose(conv(shifted).F[a], (feats[a] + 5.0).sum().reshape(1))


def test_two_batch_entries_never_mix():
    c = [[0, 0, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 1, 1]]
    x = _st(c, torch.tensor([[1.0], [2.0], [4.0], [8.0]]))
    conv = _conv(1, 1, 3)
    with torch.no_grad():
        conv.kernel.fill_(1.0)
    # sample 0: (0,0,0) and (1,1,1) are neighbours; sample 1: (1,0,0) and (0,0,0) are neighbours
    assert conv(x).F.reshape(-1).tolist() == [9.0, 6.0, 6.0, 9.0]
    down = _conv(1, 1, 2, stride=2)
    with torch.no_grad():
        down.kernel.fill_(1.0)
    y = down(x)
    got = {tuple(cc): float(f) for cc, f in zip(y.C.tolist(), y.F.reshape(-1).tolist())}
    assert got == {(0, 0, 0, 0): 9.0, (1, 0, 0, 0): 6.0}


def test_matches_a_direct_sum_on_a_random_scene():
    """A 3^3 conv of the stand-in against the definition, out[u] = sum_k in[u + d_k] @ W[k], summed in Python."""
    g = torch.Generator().manual_seed(1)
    pts = torch.unique(torch.randint(-6, 6, (120, 3), generator=g), dim=0)
    coords = torch.cat([torch.zeros(len(pts), 1, dtype=torch.int64), pts], 1)
    feats = torch.randn(len(pts), 2, generator=g, dtype=torch.float64)
    x = _st(coords, feats)
    conv = _conv(2, 3, 3)
    with torch.no_grad():
        conv.kernel.copy_(torch.randn(27, 2, 3, generator=g, dtype=torch.float64))
    y = conv(x)
    rows = _rows_by_coord(x)
    for i, c in enumerate(x.C.tolist()):
        acc = torch.zeros(3, dtype=torch.float64)
        for k in range(27):
            d = (k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1)
            j = rows.get((c[1] + d[0], c[2] + d[1], c[3] + d[2]))
            if j is not None:
                acc += feats[j] @ conv.kernel[k]
        assert torch.allclose(y.F[i], acc, atol=1e-12), i
