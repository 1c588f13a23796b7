"""-m gpu: ``a3d_scene_create`` (csrc/scene.hip, with the sort and scans of csrc/radix.hip) at the sizes where it switches
paths, held to the tables' contract by tests/scene_rule.py.  Integer equality throughout.

The cases (tests/scene_cases.py) are the smallest inputs that reach a branch: row counts around the 128-row padding and the
1024-voxel blocks of the level compaction; 65 536 / 65 537 rows (one chunk of k_tile_prefix / two and a carry); 131 072 /
131 073 voxels (one launch with grid barriers / launch chains); one and two super tiles; 1 048 577 voxels (two chunks of
block sums in k_heads_scan); the dense grid against the hash table at exactly 64 cells per voxel; both ends of the
coordinate range; 1023 batch samples; concurrent builds.

What cannot be observed from outside: WHICH form of phase 1 ran.  A build that is alone takes the one-launch forms up to
131 072 voxels only if ``barrier_grid_fits`` says the device as this process sees it holds the grid (a partitioned device
may not), and falls back to the chains when a barrier gives up; nothing in the ABI reports the choice.  The tests therefore
pin what the tables must be on either path, and the one switch that can be set from outside (A3D_SORT_ONE_LAUNCH=0, read once
per process) is compared bit for bit in a second interpreter."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import scene_cases as cases
import scene_rule as R
from agile3d_amd import lib as L
from agile3d_amd.engine import Scene
from agile3d_amd.synthetic import make_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables_of(scene):
    return {key: scene.table(*key) for key in R.table_keys()}


def build_and_check(coords, sample=None):
    scene = Scene(torch.from_numpy(coords).cuda())
    want = R.grid_expected(coords)
    assert scene.grid_dims == want, (scene.grid_dims, want)
    T = tables_of(scene)
    assert scene.n == [T[lv, L.TAB_XYZB].size // 4 for lv in range(5)]
    R.check_tables(coords, T, sample=sample)
    return scene, T


MID = ["tiles_65536", "tiles_65537", "one_launch_131072", "chain_131073", "super_tile_262144", "super_tiles_266000"]


@pytest.mark.parametrize("name", cases.SMALL + MID)
def test_tables_hold_the_contract(name):
    build_and_check(cases.CASES[name](), cases.SAMPLE.get(name))


def test_block_sum_chunks_of_the_level_compaction():
    """1 048 577 voxels: 1025 blocks of 1024, so k_heads_scan adds up a second chunk of block sums on top of a carry."""
    coords = cases.CASES["block_sums_1048577"]()
    need = L.load().a3d_scene_workspace_bytes(len(coords))
    free = torch.cuda.mem_get_info()[0]
    if need + (1 << 30) > free:
        pytest.skip(f"the scene workspace takes {need >> 20} MiB, {free >> 20} MiB are free")
    build_and_check(coords, cases.SAMPLE["block_sums_1048577"])


def test_range_ends_do_not_see_each_other():
    """(2^17 - 1, y, z) and (-2^17, y, z) in every sample a wrapped key could land in: the hit lists of the rows at either end
    hold only rows one step away in the same sample (check_tables proves it row by row; this states it for the two ends)."""
    coords = cases.CASES["range_corners"]()
    scene, T = build_and_check(coords)
    for level in range(5):
        x = T[level, L.TAB_XYZB].reshape(-1, 4).astype(np.int64)
        n = len(x)
        nbr = T[level, L.TAB_NBR27].reshape(27, -1)[:, :n]
        lo, hi = cases.LO >> level, cases.HI >> level
        for axis in range(3):
            at_hi, at_lo = x[:, axis] == hi, x[:, axis] == lo
            assert at_hi.any() and at_lo.any()
            for k in range(27):
                d = R.offset27(k)[axis]
                if d == 1:
                    assert (nbr[k][at_hi] == n).all(), (level, axis, k)
                if d == -1:
                    assert (nbr[k][at_lo] == n).all(), (level, axis, k)


def test_1023_samples_and_the_refusal_of_the_1024th():
    coords = cases.CASES["batches_1023"]()
    scene, T = build_and_check(coords)
    assert scene.batch_ranges == [(3 * b, 3 * b + 3) for b in range(1023)]
    assert scene.n == [3 * 1023] * 5              # the three voxels stay apart at every level
    n = scene.n[0]
    nbr = T[0, L.TAB_NBR27].reshape(27, -1)[:, :n]
    assert ((nbr < n).sum(0) == 1).all()          # no voxel has a neighbour but itself, in its own sample or another
    more = np.concatenate([coords, np.array([[1023, 0, 0, 0]], np.int32)])
    with pytest.raises(L.A3DError, match="range"):
        Scene(torch.from_numpy(more).cuda())


def test_refused_rows_are_not_reported_as_duplicates():
    """A row outside the range has no key of its own.  Two such rows, or one next to the voxel whose key is 0 -- sample 0,
    (-2^17, -2^17, -2^17) -- are out of range, not duplicates of each other (what the 1024th sample above found)."""
    lo = cases.LO
    for rows in ([[0, 1, 2, 3], [0, 1 << 17, 0, 0], [0, 0, -(1 << 17) - 1, 0]],
                 [[0, lo, lo, lo], [0, 4, 5, 6], [0, 0, 0, 1 << 17]],
                 [[0, lo, lo, lo], [1, 4, 5, 6], [1023, 0, 0, 0]],
                 [[0, 1, 2, 3], [-1, 0, 0, 0], [-1, 0, 0, 0]]):
        with pytest.raises(L.A3DError, match="range"):
            Scene(torch.tensor(rows, dtype=torch.int32).cuda())


def test_refusals_on_the_chain_path():
    """131 073 voxels (129 blocks: the launch chains) are refused for the same reasons, with the same errors, as three."""
    good = cases.CASES["chain_131073"]()
    dup = good.copy()
    dup[100_000] = dup[7]
    with pytest.raises(L.A3DError, match="duplicate"):
        Scene(torch.from_numpy(dup).cuda())
    far = good.copy()
    far[131_072, 2] = 1 << 17
    with pytest.raises(L.A3DError, match="range"):
        Scene(torch.from_numpy(far).cuda())
    two = good.copy()
    two[70_000:, 0] = 1
    Scene(torch.from_numpy(two).cuda())           # two contiguous samples build
    two[[5, 131_000]] = two[[131_000, 5]]         # sample 0 no longer contiguous
    with pytest.raises(L.A3DError, match="contiguous"):
        Scene(torch.from_numpy(two).cuda())


@pytest.fixture(scope="module")
def small_scene():
    return Scene(torch.from_numpy(cases.CASES["compact129"]()).cuda())


@pytest.mark.parametrize("level,table", [(1, L.TAB_ORIGROW), (4, L.TAB_CHILD8), (4, L.TAB_PREDOWN), (4, L.TAB_PREUP),
                                         (4, L.TAB_GMASKDOWN), (4, L.TAB_UP8), (4, L.TAB_GMASKUP), (4, L.TAB_UPROWS),
                                         (0, L.TAB_ORDER27), (0, 13), (0, -1), (5, L.TAB_XYZB), (-1, L.TAB_XYZB)])
def test_tables_that_do_not_exist_are_refused(small_scene, level, table):
    """Among them id 9, which ``lib.TAB_ORDER27`` still names and the library no longer serves."""
    with pytest.raises(L.A3DError):
        small_scene.table(level, table)
    assert small_scene.table(0, L.TAB_ORIGROW).size == 129      # the scene still answers


CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import scene_cases, scene_rule
from agile3d_amd.engine import Scene
for name in sys.argv[3:]:
    sc = Scene(torch.from_numpy(scene_cases.CASES[name]()).cuda())
    np.savez(sys.argv[2] + "/" + name + ".npz", grid=np.array(sc.grid_dims or (0, 0, 0)), sizes=np.array(sc.n),
             **{f"t{lv}_{t}": sc.table(lv, t) for lv, t in scene_rule.table_keys()})
'''


def _rebuilt_with(switch, names, tmp_path):
    """The named cases built in a second interpreter (the switches are read once per process), one child at a time."""
    env = dict(os.environ, **dict([switch.split("=")]))
    subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path)] + names, check=True, env=env, timeout=300)
    return {name: np.load(str(tmp_path / f"{name}.npz")) for name in names}


def _same_tables(z, T, sizes):
    assert z["sizes"].tolist() == sizes
    for lv, t in R.table_keys():
        other = z[f"t{lv}_{t}"]
        assert other.dtype == T[lv, t].dtype and np.array_equal(other, T[lv, t]), (R.NAMES[t], lv)


def test_launch_chains_build_the_tables_of_the_one_launch_forms(tmp_path):
    """A3D_SORT_ONE_LAUNCH=0 keeps the launch chains at 131 072 voxels, where the default build may take the one-launch sort and
    k_heads_all: same sorts, same scans, so every table is the same bit for bit."""
    name = "one_launch_131072"
    scene, T = build_and_check(cases.CASES[name]())
    z = _rebuilt_with("A3D_SORT_ONE_LAUNCH=0", [name], tmp_path)[name]
    _same_tables(z, T, scene.n)


def test_hash_table_builds_the_tables_of_the_dense_grid(tmp_path):
    """A3D_GRID=0 forces the hash table at level 0.  The row order comes from the Morton sort and the sort by neighbour mask,
    the lookup structure only answers "which row holds this voxel", so all tables are bit-identical."""
    here = {name: build_and_check(cases.CASES[name]()) for name in cases.GRID_VS_HASH}
    assert all(scene.grid_dims is not None for scene, _ in here.values())
    there = _rebuilt_with("A3D_GRID=0", cases.GRID_VS_HASH, tmp_path)
    for name, (scene, T) in here.items():
        assert there[name]["grid"].tolist() == [0, 0, 0], name
        _same_tables(there[name], T, scene.n)


def test_concurrent_builds_equal_solo_builds():
    """Two host threads, each on its own stream, build eight 5 000-voxel scenes each (in opposite orders): a build that is not
    alone between its first launch and its synchronisation takes the launch chains (SoloPhase1), and every result equals
    the solo build's tables bit for bit.  Whether the two threads' builds really overlapped cannot be asserted -- the
    library's call counter is not visible from outside -- so this pins the results, not the interleaving."""
    coords = [torch.from_numpy(make_scene(5000, seed=30 + i)["coords"]).cuda() for i in range(8)]
    solo = [tables_of(Scene(c)) for c in coords]
    torch.cuda.synchronize()
    results, errors = {}, []
    gate = threading.Barrier(2)

    def worker(tid, order):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                gate.wait(timeout=30)
                scenes = [(i, Scene(coords[i])) for i in order]
                results[tid] = {i: tables_of(s) for i, s in scenes}
                stream.synchronize()
        except Exception as e:      # noqa: BLE001 -- reported by the main thread
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(0, list(range(8)))), threading.Thread(target=worker, args=(1, list(range(7, -1, -1))))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a concurrent build did not finish"
    assert not errors, errors
    for tid in (0, 1):
        for i in range(8):
            for key in R.table_keys():
                assert np.array_equal(results[tid][i][key], solo[i][key]), (tid, i, key)
