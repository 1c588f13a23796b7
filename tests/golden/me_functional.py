"""A working stand-in for the parts of MinkowskiEngine that the reference's backbone executes (TEST INFRASTRUCTURE).

``install()`` registers it as ``MinkowskiEngine`` (plus ``.MinkowskiOps`` / ``.MinkowskiPooling``) so that the
reference's ``models`` package can be imported AND run on a CPU.  Every sparse operation is computed from torch's
dense operators: the rows of a tensor are scattered onto a zero grid ``[B, C, Z, Y, X]``, ``F.conv3d`` /
``F.conv_transpose3d`` / ``F.avg_pool3d`` run on it, and the result is gathered back at the output coordinates.  The
grid is rebuilt from the occupied rows for every operation, so every unoccupied cell is zero in front of each
convolution (after a BatchNorm an empty cell would no longer be zero).  Nothing here is shared with the project's
oracle or library: this file is the independent side of the comparison.  Autograd runs through all of it.

Conventions, as MinkowskiEngine v0.5 documents them:
  * coordinates int32 ``[N, 4]`` = (batch, x, y, z) in units of the finest voxel; a tensor of stride ``s`` holds
    multiples of ``s``;
  * odd kernel ``K``, stride 1: output set = input set, ``out[u] = sum_k in[u + d_k] @ W[k]`` (cross-correlation);
  * kernel 2, stride 2: output set = the unique ``floor(c / 2s) * 2s`` of the input set (floor also for negative
    coordinates), ``out[c] = sum_k in[c + s * bits(k)] @ W[k]``;
  * transposed kernel 2, stride 2: output set = the coordinate set the manager has cached for the target stride, in
    that set's row order (so that ``MinkowskiOps.cat`` with the encoder's tensor of that stride lines up);
  * kernel tensors ``[K, Cin, Cout]`` (``[Cin, Cout]`` for 1x1), bias ``[1, Cout]``.

The one convention taken on trust: the enumeration of the kernel offsets, ``k = ix + K * iy + K^2 * iz`` (x fastest),
written once in ``_dense_weight``.  MinkowskiEngine's source is not available offline; the project's load-time switch
for the other enumeration is ``agile3d_amd.model.kernel_order_permutation``.
"""
from __future__ import annotations

import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as tnf

GRID_ALIGN = 16   # the grid origin is a multiple of the coarsest stride: floor(c / 2s) * 2s is a cell boundary


# ----------------------------------------------------------------------------- coordinates
class CoordinateMapKey:
    def __init__(self, tensor_stride: int):
        self.tensor_stride = int(tensor_stride)

    def get_tensor_stride(self):
        return [self.tensor_stride] * 3

    def __eq__(self, other):
        return isinstance(other, CoordinateMapKey) and other.tensor_stride == self.tensor_stride

    def __hash__(self):
        return hash(self.tensor_stride)

    def __repr__(self):
        return f"CoordinateMapKey(stride={self.tensor_stride})"


class CoordinateManager:
    """Caches one coordinate set (and with it one row order) per tensor stride."""

    def __init__(self):
        self.sets = {}

    def insert(self, stride: int, coords: torch.Tensor) -> CoordinateMapKey:
        coords = coords.to(torch.int32).contiguous()
        assert coords.dim() == 2 and coords.shape[1] == 4
        assert len(torch.unique(coords, dim=0)) == len(coords), "duplicate coordinates"
        assert bool((coords[:, 1:] % stride == 0).all()), "coordinates are not multiples of the stride"
        if stride in self.sets:
            old = self.sets[stride]
            assert torch.equal(old, coords), f"stride {stride} is already cached with another row order"
        self.sets[stride] = coords
        return CoordinateMapKey(stride)

    def coordinates(self, key: CoordinateMapKey) -> torch.Tensor:
        return self.sets[key.tensor_stride]

    def strided(self, key: CoordinateMapKey) -> CoordinateMapKey:
        """The stride-2 coarsening of ``key``'s set: cached if present, otherwise the sorted unique floor."""
        s = key.tensor_stride
        if 2 * s in self.sets:
            return CoordinateMapKey(2 * s)
        c = self.sets[s].to(torch.int64)
        down = torch.cat([c[:, :1], torch.div(c[:, 1:], 2 * s, rounding_mode="floor") * (2 * s)], 1)
        return self.insert(2 * s, torch.unique(down, dim=0))


class SparseTensor:
    """Features ``F`` [N, C] on the coordinate set ``C`` [N, 4] of one (manager, stride)."""

    def __init__(self, features, coordinates=None, tensor_stride=1, coordinate_map_key=None,
                 coordinate_manager=None, device=None, **_ignored):
        if coordinates is not None:
            if coordinate_manager is None:
                coordinate_manager = CoordinateManager()
            s = tensor_stride if isinstance(tensor_stride, int) else int(tensor_stride[0])
            coordinate_map_key = coordinate_manager.insert(s, torch.as_tensor(coordinates))
        assert coordinate_manager is not None and coordinate_map_key is not None
        self.coordinate_manager = coordinate_manager
        self.coordinate_map_key = coordinate_map_key
        self.F = features
        assert len(self.F) == len(self.C), (len(self.F), len(self.C))

    @property
    def C(self):
        return self.coordinate_manager.coordinates(self.coordinate_map_key)

    @property
    def tensor_stride(self):
        return self.coordinate_map_key.get_tensor_stride()

    @property
    def device(self):
        return self.F.device

    def __len__(self):
        return len(self.F)

    def _same_set(self, other):
        assert other.coordinate_manager is self.coordinate_manager, "different coordinate managers"
        assert other.coordinate_map_key == self.coordinate_map_key, "different coordinate sets"

    def __iadd__(self, other):
        self._same_set(other)
        self.F = self.F + other.F
        return self

    def __add__(self, other):
        self._same_set(other)
        return self._like(self.F + other.F)

    def _like(self, feats):
        return SparseTensor(feats, coordinate_map_key=self.coordinate_map_key,
                            coordinate_manager=self.coordinate_manager)


# ----------------------------------------------------------------------------- dense grids
class _Grid:
    """The cells of stride ``s`` covering ``coords``: origin a multiple of GRID_ALIGN, an even number of cells."""

    def __init__(self, coords: torch.Tensor, s: int, n_batch: int):
        c = coords[:, 1:].to(torch.int64)
        lo = torch.div(c.min(0).values, GRID_ALIGN, rounding_mode="floor") * GRID_ALIGN
        ext = torch.div(c.max(0).values - lo, s, rounding_mode="floor") + 1
        ext = ext + (ext % 2)
        self.s, self.origin, self.B = s, lo, n_batch
        self.ext = [int(v) for v in ext]           # (x, y, z)

    def index(self, coords: torch.Tensor, s: int | None = None):
        """(b, z, y, x) cell indices of ``coords`` on this grid, or on its 2x finer / coarser version (``s``)."""
        s = self.s if s is None else s
        c = coords.to(torch.int64)
        u = c[:, 1:] - self.origin
        assert bool((u % s == 0).all())
        u = torch.div(u, s, rounding_mode="floor")
        return c[:, 0], u[:, 2], u[:, 1], u[:, 0]

    def scatter(self, coords, feats):
        b, z, y, x = self.index(coords)
        grid = feats.new_zeros((self.B, self.ext[2], self.ext[1], self.ext[0], feats.shape[1]))
        grid = grid.index_put((b, z, y, x), feats)
        return grid.permute(0, 4, 1, 2, 3)         # [B, C, Z, Y, X]

    @staticmethod
    def gather(dense, idx):
        b, z, y, x = idx
        assert bool((z >= 0).all() and (z < dense.shape[2]).all() and (y >= 0).all() and (y < dense.shape[3]).all()
                    and (x >= 0).all() and (x < dense.shape[4]).all()), "output coordinate off the grid"
        return dense.permute(0, 2, 3, 4, 1)[b, z, y, x]


def _n_batch(*coord_sets):
    return int(max(int(c[:, 0].max()) for c in coord_sets)) + 1


def _dense_weight(W: torch.Tensor, K: int, transpose: bool):
    """[K^3, Cin, Cout] -> conv3d's [Cout, Cin, kz, ky, kx] (conv_transpose3d's [Cin, Cout, ...]).

    THE kernel-offset enumeration: k = ix + K * iy + K^2 * iz, x fastest (taken on trust, see the module docstring)."""
    Wv = W.view(K, K, K, W.shape[1], W.shape[2])   # [iz, iy, ix, Cin, Cout]
    return Wv.permute(3, 4, 0, 1, 2) if transpose else Wv.permute(4, 3, 0, 1, 2)


def _as_int(v):
    if isinstance(v, (list, tuple)):
        assert len(set(v[:3])) == 1, v
        return int(v[0])
    return int(v)


# ----------------------------------------------------------------------------- layers
class RegionType:
    HYPER_CUBE, HYPER_CROSS, CUSTOM = 0, 1, 2

    def __init__(self, v):
        self.v = v


class KernelGenerator:
    def __init__(self, kernel_size=-1, stride=1, dilation=1, region_type=None, axis_types=None, dimension=3):
        self.kernel_size = _as_int(kernel_size)
        self.stride = _as_int(stride)
        assert _as_int(dilation) == 1, "dilation is not supported"
        assert region_type in (None, RegionType.HYPER_CUBE) or getattr(region_type, "v", None) == 0, region_type
        self.kernel_volume = self.kernel_size ** 3


class MinkowskiNetwork(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.D = D


class _Conv(nn.Module):
    TRANSPOSE = False

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, dimension=3, **_ignored):
        super().__init__()
        if kernel_generator is None:
            kernel_generator = KernelGenerator(kernel_size, stride, dilation, dimension=dimension)
        self.K, self.stride = kernel_generator.kernel_size, kernel_generator.stride
        vol = kernel_generator.kernel_volume
        shape = (in_channels, out_channels) if vol == 1 else (vol, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.zeros(*shape))
        self.bias = nn.Parameter(torch.zeros(1, out_channels)) if bias else None
        if self.TRANSPOSE:
            assert self.K == 2 and self.stride == 2, "only the kernel-2 stride-2 transposed convolution is modelled"
        elif self.stride != 1:
            assert self.K == 2 and self.stride == 2, "only kernel-2 stride-2 strided convolutions are modelled"
        else:
            assert self.K % 2 == 1, "stride-1 kernels are odd"

    def _finish(self, y, x, key):
        if self.bias is not None:
            y = y + self.bias
        return SparseTensor(y, coordinate_map_key=key, coordinate_manager=x.coordinate_manager)

    def forward(self, x: SparseTensor) -> SparseTensor:
        s = x.coordinate_map_key.tensor_stride
        C = x.C
        if self.K == 1:                                            # 1x1: a plain matrix product on the same set
            return self._finish(x.F @ self.kernel, x, x.coordinate_map_key)
        g = _Grid(C, s, _n_batch(C))
        dense = g.scatter(C, x.F)
        if self.stride == 1:
            y = tnf.conv3d(dense, _dense_weight(self.kernel, self.K, False), padding=self.K // 2)
            return self._finish(g.gather(y, g.index(C)), x, x.coordinate_map_key)
        y = tnf.conv3d(dense, _dense_weight(self.kernel, 2, False), stride=2)
        key = x.coordinate_manager.strided(x.coordinate_map_key)
        out_c = x.coordinate_manager.coordinates(key)
        return self._finish(g.gather(y, g.index(out_c, 2 * s)), x, key)


class MinkowskiConvolution(_Conv):
    pass


class MinkowskiConvolutionTranspose(_Conv):
    TRANSPOSE = True

    def forward(self, x: SparseTensor) -> SparseTensor:
        s = x.coordinate_map_key.tensor_stride
        assert s % 2 == 0, "nothing finer than stride 1"
        key = CoordinateMapKey(s // 2)
        out_c = x.coordinate_manager.coordinates(key)              # the cached fine set, in its row order
        g = _Grid(x.C, s, _n_batch(x.C, out_c))
        y = tnf.conv_transpose3d(g.scatter(x.C, x.F), _dense_weight(self.kernel, 2, True), stride=2)
        return self._finish(g.gather(y, g.index(out_c, s // 2)), x, key)


class MinkowskiBatchNorm(nn.Module):
    """nn.BatchNorm1d over the occupied rows (train and eval mode alike)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    def forward(self, x: SparseTensor) -> SparseTensor:
        return x._like(self.bn(x.F))


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()

    def forward(self, x: SparseTensor) -> SparseTensor:
        return x._like(torch.relu(x.F))


class MinkowskiAvgPooling(nn.Module):
    """Kernel 2, stride 2: the mean over the occupied children of every coarse voxel."""

    def __init__(self, kernel_size=2, stride=2, dilation=1, kernel_generator=None, dimension=3):
        super().__init__()
        assert _as_int(kernel_size) == 2 and _as_int(stride) == 2, "only kernel 2, stride 2 is modelled"

    def forward(self, x: SparseTensor) -> SparseTensor:
        s = x.coordinate_map_key.tensor_stride
        C = x.C
        g = _Grid(C, s, _n_batch(C))
        total = tnf.avg_pool3d(g.scatter(C, x.F), 2, stride=2)
        count = tnf.avg_pool3d(g.scatter(C, x.F.new_ones((len(C), 1))), 2, stride=2)
        key = x.coordinate_manager.strided(x.coordinate_map_key)
        idx = g.index(x.coordinate_manager.coordinates(key), 2 * s)
        return SparseTensor(g.gather(total, idx) / g.gather(count, idx), coordinate_map_key=key,
                            coordinate_manager=x.coordinate_manager)


def cat(*tensors):
    """MinkowskiOps.cat: the features of tensors on ONE coordinate set, side by side in argument order."""
    for t in tensors[1:]:
        tensors[0]._same_set(t)
    return tensors[0]._like(torch.cat([t.F for t in tensors], 1))


class _ConstructionOnly(nn.Module):
    """Names the reference constructs somewhere but the backbone's forward never runs."""

    def __init__(self, *a, **k):
        super().__init__()

    def forward(self, *a, **k):
        raise NotImplementedError(f"{type(self).__name__} is not modelled by the stand-in")


class MinkowskiInstanceNorm(_ConstructionOnly):
    pass


class MinkowskiAvgUnpooling(_ConstructionOnly):
    pass


class MinkowskiSumPooling(_ConstructionOnly):
    pass


def install():
    """Register the stand-in as ``MinkowskiEngine`` in ``sys.modules``; returns the module."""
    me = types.ModuleType("MinkowskiEngine")
    names = dict(SparseTensor=SparseTensor, CoordinateManager=CoordinateManager, CoordinateMapKey=CoordinateMapKey,
                 MinkowskiNetwork=MinkowskiNetwork, RegionType=RegionType, KernelGenerator=KernelGenerator,
                 MinkowskiConvolution=MinkowskiConvolution, MinkowskiConvolutionTranspose=MinkowskiConvolutionTranspose,
                 MinkowskiBatchNorm=MinkowskiBatchNorm, MinkowskiReLU=MinkowskiReLU,
                 MinkowskiAvgPooling=MinkowskiAvgPooling, MinkowskiInstanceNorm=MinkowskiInstanceNorm,
                 MinkowskiAvgUnpooling=MinkowskiAvgUnpooling, MinkowskiSumPooling=MinkowskiSumPooling, cat=cat)
    for k, v in names.items():
        setattr(me, k, v)
    ops = types.ModuleType("MinkowskiEngine.MinkowskiOps")
    ops.SparseTensor, ops.cat = SparseTensor, cat
    pool = types.ModuleType("MinkowskiEngine.MinkowskiPooling")
    pool.MinkowskiAvgPooling = MinkowskiAvgPooling
    me.MinkowskiOps, me.MinkowskiPooling = ops, pool
    sys.modules["MinkowskiEngine"] = me
    sys.modules["MinkowskiEngine.MinkowskiOps"] = ops
    sys.modules["MinkowskiEngine.MinkowskiPooling"] = pool
    return me
