"""-m gpu: ``a3d_sparse_quantize`` (csrc/quantize.hip) at the block edges of its scans (``scan2_incl_excl``, csrc/radix.hip:
4096-element blocks, 1024 block sums per chunk), at the ends of its 21-bit key fields (voxel indices in [-2^20, 2^20)) and
around zero.  Bit-exact integers against the plain-Python oracle; above a million points against closed-form expectations."""
import numpy as np
import pytest
import torch

from agile3d_amd import sparse_quantize
from agile3d_amd.lib import A3DError
from oracle import quantize as oq

pytestmark = pytest.mark.gpu
Q = 1 << 20
DTYPES = [np.float32, np.float64]


def device(xyz, qs):
    q, umap, inv = sparse_quantize(torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), quantization_size=qs, return_index=True,
                                   return_inverse=True)
    assert q.dtype == torch.int32 and umap.dtype == torch.int64 and inv.dtype == torch.int64
    return q.cpu().numpy(), umap.cpu().numpy(), inv.cpu().numpy()


def same_as_oracle(xyz, qs):
    q, umap, inv = device(xyz, qs)
    wq, wu, wi = oq.sparse_quantize(xyz, qs)
    assert np.array_equal(q, wq) and np.array_equal(umap, wu) and np.array_equal(inv, wi)
    return q, umap, inv


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["distinct", "three_voxels"])
@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8192, 8193])
def test_scan_block_edges(n, kind, dtype):
    """One element below, at and above one and two 4096-element scan blocks; all points in voxels of their own (every flag of
    both scans set) and all points in three voxels (three flags set in each)."""
    rng = np.random.default_rng(n)
    if kind == "distinct":
        i = rng.permutation(n)
        vox = np.stack([i % 29 - 14, (i // 29) % 23 - 11, i // (29 * 23) - 6], 1)
    else:
        vox = np.array([[3, -2, 1], [-40, 7, 0], [3, -2, 2]])[rng.integers(0, 3, n)]
    xyz = ((vox + rng.random((n, 3)) * 0.875 + 0.0625) * 0.25).astype(dtype)      # well inside the voxel: exact in fp32
    q, umap, inv = same_as_oracle(xyz, 0.25)
    assert np.array_equal(q[inv], vox)
    assert len(q) == (n if kind == "distinct" else len(np.unique(vox, axis=0)))


def test_scan_block_sum_chunks_mostly_distinct():
    """4096 * 1024 + 1 points: 1025 block sums, so k_scan2_blocks walks a second chunk on top of a carry.  Four points in five
    open a voxel (every block sum of both scans is non-zero), the fifth repeats its predecessor's; the voxel ids are
    scrambled so that the sorted order is not the input order.  unique_map and inverse_map have closed forms."""
    n = 4096 * 1024 + 1
    i = np.arange(n, dtype=np.int64)
    rep = i - (i % 5 == 4)                                     # the point that opened i's voxel
    scr = (rep * 2654435761) & ((1 << 23) - 1)                 # odd multiplier: a bijection of 23-bit ids
    vox = np.stack([(scr & 255) - 128, ((scr >> 8) & 255) - 128, (scr >> 16) - 64], 1).astype(np.int32)
    xyz = ((vox + 0.5) * 0.25).astype(np.float32)
    q, umap, inv = sparse_quantize(torch.from_numpy(xyz).cuda(), quantization_size=0.25, return_index=True, return_inverse=True)
    want_umap = torch.from_numpy(i[i % 5 != 4])
    assert len(q) == len(want_umap) and torch.equal(umap.cpu(), want_umap)
    assert torch.equal(inv.cpu(), torch.from_numpy(rep - rep // 5))
    assert torch.equal(q.cpu(), torch.from_numpy(vox)[want_umap])


def test_scan_block_sum_chunks_one_late_voxel():
    """The same size with every point but the last in one voxel: all block sums but the first and the last are zero, and the
    last block holds the one element past 1024 blocks."""
    n = 4096 * 1024 + 1
    xyz = np.full((n, 3), 0.3, np.float32)
    xyz[-1] = [0.3, 1.3, 0.3]
    q, umap, inv = device(xyz, 1.0)
    assert q.tolist() == [[0, 0, 0], [0, 1, 0]] and umap.tolist() == [0, n - 1]
    assert not inv[:-1].any() and inv[-1] == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_voxel_index_limits(axis, dtype):
    """floor(x / qs) = -2^20 and 2^20 - 1 are accepted and come back exactly; 2^20, -2^20 - 1 and the infinities are refused.
    qs = 0.5 and multiples of 1/8: every quotient is exact in fp32."""
    base = np.array([[0.1, 0.2, 0.3], [-7.3, 2.2, 9.9], [0.1, 0.2, 0.3]], dtype)
    for value, index in ((-Q * 0.5, -Q), ((Q - 1) * 0.5, Q - 1), ((Q - 1) * 0.5 + 0.375, Q - 1), (-Q * 0.5 + 0.125, -Q)):
        xyz = np.concatenate([base, base[:1]])
        xyz[3, axis] = value
        q, umap, inv = same_as_oracle(xyz, 0.5)
        want = np.floor(base[0] / dtype(0.5)).astype(np.int32)
        want[axis] = index
        assert q[inv[3]].tolist() == want.tolist() and umap.tolist() == [0, 1, 3] and inv.tolist() == [0, 1, 0, 2]
    for value in (Q * 0.5, (-Q - 1) * 0.5, -Q * 0.5 - 0.125, Q * 0.5 + 0.125, np.inf, -np.inf):
        xyz = np.concatenate([base, base[:1]])
        xyz[3, axis] = value
        with pytest.raises(A3DError, match="outside"):
            device(xyz, 0.5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_key_fields_do_not_bleed(axis, dtype):
    """Points that differ only in one axis while the other two sit at opposite extremes: a 21-bit field that carried into its
    neighbour would change the decoded triple or merge two voxels."""
    values = [-Q, -Q + 1, -1, 0, 1, Q - 2, Q - 1]
    rows = []
    for others in ((Q - 1, -Q), (-Q, Q - 1), (-Q, -Q), (Q - 1, Q - 1)):
        for v in values:
            r = list(others)
            r.insert(axis, v)
            rows.append(r)
    vox = np.array(rows, np.int64)[np.random.default_rng(axis).permutation(len(rows))]
    xyz = ((vox + 0.5) * 0.5).astype(dtype)       # 2^20 + 0.5 has 22 significant bits: exact in fp32
    q, umap, inv = same_as_oracle(xyz, 0.5)
    assert np.array_equal(q, vox) and umap.tolist() == list(range(len(vox))) and inv.tolist() == list(range(len(vox)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("qs", [1.0, 0.05])
def test_around_zero(dtype, qs):
    """-0.0 is voxel 0, anything below zero is voxel -1 however small: -1e-30 and the subnormals of the dtype (floor of a
    negative subnormal quotient is -1; a flush to zero would move the point to voxel 0)."""
    tiny = np.finfo(dtype).tiny                   # the smallest normal number
    sub = [tiny / 4, np.nextafter(dtype(0), dtype(1))]     # subnormals: a quarter of it, and the smallest of all
    col = np.array([0.0, -0.0, 1e-30, -1e-30, tiny, -tiny, sub[0], -sub[0], sub[1], -sub[1]], dtype)
    want = np.array([0, 0, 0, -1, 0, -1, 0, -1, 0, -1])
    assert (col[6:] != 0).all()                   # the host kept them
    for axis in range(3):
        xyz = np.full((len(col), 3), 0.5 * qs, dtype)
        xyz[:, axis] = col
        q, umap, inv = same_as_oracle(xyz, qs)
        assert np.array_equal(q[inv][:, axis], want), (axis, q[inv][:, axis])
        assert len(q) == 2 and umap.tolist() == [0, 3]
