"""-m gpu: the HIP coordinate manager against the CPU oracle's SparseLevels."""
import numpy as np
import pytest
import torch

from agile3d_amd import lib as L
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene
from gpu_util import _random_coords, internal_to_oracle_rows, key4
from oracle import backbone as ob

pytestmark = pytest.mark.gpu


CASES = {
    "dense24": lambda: _random_coords(700, 24, 0),
    "neg_batch2": lambda: _random_coords(900, 40, 1, batches=2, negative=True),
    "synthetic5k": lambda: make_scene(5000, seed=2)["coords"],
    "single_voxel": lambda: np.array([[0, 3, 4, 5]], np.int32),
    "tiny_line": lambda: np.array([[0, i, 0, 0] for i in range(37)], np.int32),
    "sparse_far": lambda: _random_coords(800, 60000, 3, negative=True),
    "compact_plus_outlier": lambda: np.concatenate([_random_coords(700, 24, 4), np.array([[0, 90000, -70000, 5]], np.int32)]),
}
# level 0 uses a dense voxel grid when the padded bounding box has <= 64 cells per voxel, the hash table otherwise
GRID = {"dense24": True, "neg_batch2": False, "synthetic5k": True, "single_voxel": False, "tiny_line": True,
        "sparse_far": False, "compact_plus_outlier": False}


@pytest.mark.parametrize("name", list(CASES))
def test_scene_tables(name):
    coords = CASES[name]()
    sc = Scene(torch.from_numpy(coords).cuda())
    lv = ob.SparseLevels(coords)
    assert sc.n == [lv.n(i) for i in range(5)]
    assert (sc.grid_dims is not None) == GRID[name], (name, sc.grid_dims)
    if sc.grid_dims:
        ext = coords[:, 1:].max(0) - coords[:, 1:].min(0) + 1
        assert sc.grid_dims == tuple(int(e) + 4 for e in ext)
    maps = [internal_to_oracle_rows(sc, lv, i) for i in range(5)]   # also checks coordinate sets
    for level in range(5):
        n = sc.n[level]
        npad = (max(n, 1) + 127) // 128 * 128
        xyzb = sc.table(level, L.TAB_XYZB).reshape(-1, 4).astype(np.int64)
        nbr = sc.table(level, L.TAB_NBR27).reshape(27, npad)
        gm = sc.table(level, L.TAB_GMASK27)
        assert nbr.min() >= 0 and nbr.max() <= n
        assert (nbr[:, n:] == n).all()
        present = np.zeros((27, npad), bool)
        bxyz = np.stack([xyzb[:, 3], xyzb[:, 0], xyzb[:, 1], xyzb[:, 2]], 1)
        keys = set(key4(bxyz).tolist())
        for k in range(27):
            d = np.array([0, k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])
            tgt = bxyz + d
            r = nbr[k, :n]
            hit = r < n
            present[k, :n] = hit
            assert np.array_equal(bxyz[r[hit]], tgt[hit]), (level, k)
            miss_keys = key4(tgt[~hit]).tolist()
            assert not any(mk in keys for mk in miss_keys), (level, k, "existing neighbour reported missing")
        exp_gm = np.zeros(npad // 16, np.uint32)
        for k in range(27):
            exp_gm |= (present[k].reshape(-1, 16).any(1).astype(np.uint32) << np.uint32(k))
        assert np.array_equal(gm, exp_gm), level
        if level == 4:
            continue
        nC = sc.n[level + 1]
        npadC = (max(nC, 1) + 127) // 128 * 128
        xyzbC = sc.table(level + 1, L.TAB_XYZB).reshape(-1, 4).astype(np.int64)
        child = sc.table(level, L.TAB_CHILD8).reshape(8, npadC)
        gmd = sc.table(level, L.TAB_GMASKDOWN)
        seen = np.zeros(n, int)
        exp = np.zeros(npadC // 16, np.uint32)
        for s in range(8):
            r = child[s, :nC]
            hit = r < n
            assert (r[~hit] == n).all() and (child[s, nC:] == n).all()
            f = xyzb[r[hit]]
            assert np.array_equal(f[:, :3] >> 1, xyzbC[:nC][hit][:, :3]) and np.array_equal(f[:, 3], xyzbC[:nC][hit][:, 3])
            slot = (f[:, 0] & 1) + 2 * (f[:, 1] & 1) + 4 * (f[:, 2] & 1)
            assert (slot == s).all()
            np.add.at(seen, r[hit], 1)
            full = np.zeros(npadC, bool)
            full[:nC] = hit
            exp |= (full.reshape(-1, 16).any(1).astype(np.uint32) << np.uint32(s))
        assert (seen == 1).all()
        assert np.array_equal(gmd, exp)
        up = sc.table(level, L.TAB_UP8).reshape(8, npad)
        uprows = sc.table(level, L.TAB_UPROWS)
        gmu = sc.table(level, L.TAB_GMASKUP)
        assert sorted(uprows[:n].tolist()) == list(range(n))
        hitm = up[:, :n] < nC
        assert (hitm.sum(0) == 1).all() and (up[:, n:] == nC).all() and (up[:, :n][~hitm] == nC).all()
        s_of_v = hitm.argmax(0)
        f = xyzb[uprows[:n]]
        slot = (f[:, 0] & 1) + 2 * (f[:, 1] & 1) + 4 * (f[:, 2] & 1)
        assert np.array_equal(slot, s_of_v)
        par = up[s_of_v, np.arange(n)]
        assert np.array_equal(xyzbC[par][:, :3], f[:, :3] >> 1) and np.array_equal(xyzbC[par][:, 3], f[:, 3])
        exp = np.zeros(npad // 16, np.uint32)
        for s in range(8):
            full = np.zeros(npad, bool)
            full[:n] = s_of_v == s
            exp |= (full.reshape(-1, 16).any(1).astype(np.uint32) << np.uint32(s))
        assert np.array_equal(gmu, exp)
    orig = sc.table(0, L.TAB_ORIGROW)
    assert sorted(orig.tolist()) == list(range(len(coords)))
    x0 = sc.table(0, L.TAB_XYZB).reshape(-1, 4)
    assert np.array_equal(coords[orig][:, 1:], x0[:, :3]) and np.array_equal(coords[orig][:, 0], x0[:, 3])


def test_scene_errors():
    dup = np.array([[0, 1, 2, 3], [0, 4, 5, 6], [0, 1, 2, 3]], np.int32)
    with pytest.raises(L.A3DError, match="duplicate"):
        Scene(torch.from_numpy(dup).cuda())
    far = np.array([[0, 1, 2, 3], [0, 1 << 17, 0, 0]], np.int32)
    with pytest.raises(L.A3DError, match="range"):
        Scene(torch.from_numpy(far).cuda())


def test_group_skip_efficiency_reported():
    """Not a pass/fail on a threshold tuned to one scene: documents the useful-MFMA fraction the
    row clustering achieves and guards against regressions to the dense 27-offset rate."""
    coords = make_scene(20000, seed=0)["coords"]
    sc = Scene(torch.from_numpy(coords).cuda())
    n = sc.n[0]
    npad = (n + 127) // 128 * 128
    nbr = sc.table(0, L.TAB_NBR27).reshape(27, npad)
    gm = sc.table(0, L.TAB_GMASK27)
    pairs = int((nbr[:, :n] < n).sum())
    active = sum(bin(int(m)).count("1") for m in gm) * 16
    dense = 27 * npad
    print(f"pairs={pairs} group-active slots={active} dense slots={dense} "
          f"useful={pairs / active:.3f} (dense would be {pairs / dense:.3f})")
    assert pairs / active > 1.3 * pairs / dense


def test_batch_ranges_and_malformed_batches():
    """Batch samples are contiguous ascending row ranges (ME.utils.batched_coordinates); the scene build
    reports them from its single read-back and rejects anything else."""
    from agile3d_amd.engine import Scene
    from agile3d_amd.lib import A3DError
    parts = [make_scene(n, seed=s, batch_index=b)["coords"] for b, (n, s) in enumerate([(700, 1), (1500, 2), (300, 3)])]
    c = np.concatenate(parts)
    sc = Scene(torch.from_numpy(c).cuda())
    lens = [len(p) for p in parts]
    assert sc.batch_ranges == [(0, lens[0]), (lens[0], lens[0] + lens[1]), (lens[0] + lens[1], sum(lens))]
    assert Scene(torch.from_numpy(parts[0]).cuda()).batch_ranges == [(0, lens[0])]
    swapped = np.concatenate([parts[1], parts[0], parts[2]])                  # not ascending
    interleaved = c.copy()
    interleaved[[5, lens[0] + 5]] = interleaved[[lens[0] + 5, 5]]             # sample 0 no longer contiguous
    gap = np.concatenate([parts[0], parts[2]])                                # batch index 1 missing
    for bad in (swapped, interleaved, gap):
        with pytest.raises(A3DError):
            Scene(torch.from_numpy(np.ascontiguousarray(bad)).cuda())


def _sort_pairs(keys, vals, b0, b1):
    import ctypes as C
    lib = L.load()
    n = keys.numel()
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    ws = torch.empty(max(256, lib.a3d_sort_pairs_workspace_bytes(max(n, 1))), dtype=torch.uint8, device="cuda")
    L.check(lib.a3d_sort_pairs_u64(C.c_void_p(keys.data_ptr()), C.c_void_p(vals.data_ptr()), n, b0, b1, C.c_void_p(ko.data_ptr()),
                                   C.c_void_p(vo.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "a3d_sort_pairs_u64")
    return ko, vo


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 100_003, 131_072, 131_073, 393_217, 1_300_000])   # <= 128 blocks of 1024 keys: the one-launch sort; above: the launch chain
@pytest.mark.parametrize("kind", ["random63", "few_bits", "constant", "descending", "morton_like"])
def test_radix_sort_pairs_is_a_stable_sort(n, kind):
    """csrc/radix.hip against torch.sort(stable=True): every workgroup-boundary size, keys with constant digits (skipped
    on the device), all-equal keys (the order of the values must survive), a partial bit range."""
    g = torch.Generator().manual_seed(n * 7 + len(kind))
    if kind == "random63":
        keys = torch.randint(0, 2 ** 62, (n,), generator=g, dtype=torch.int64)
    elif kind == "few_bits":       # 5 distinct values far apart: most digits constant, long runs of ties
        keys = torch.randint(0, 5, (n,), generator=g, dtype=torch.int64) << 37
    elif kind == "constant":
        keys = torch.full((n,), 0x0123456789ABCDE, dtype=torch.int64)
    elif kind == "descending":
        keys = torch.arange(n, 0, -1, dtype=torch.int64) * 977
    else:                           # batch index on top, ~30 varying bits below, an offset bit pattern in between
        keys = (torch.randint(0, 4, (n,), generator=g, dtype=torch.int64) << 54) | (0x2492 << 38) | \
            torch.randint(0, 2 ** 30, (n,), generator=g, dtype=torch.int64)
    vals = torch.randperm(n, generator=g, dtype=torch.int64).to(torch.int32)
    b0, b1 = (0, 64) if kind != "descending" else (0, 40)
    ko, vo = _sort_pairs(keys.cuda(), vals.cuda(), b0, b1)
    field = (keys >> b0) & ((1 << (b1 - b0)) - 1) if b1 - b0 < 64 else keys
    order = torch.sort(field, stable=True)[1]
    assert torch.equal(ko.cpu(), keys[order]), kind
    assert torch.equal(vo.cpu(), vals[order]), kind
