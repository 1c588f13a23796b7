"""The cases the tests of ``a3d_orient_normals`` share (not collected; numpy only): voxel sets with one vertex per voxel centre,
rows shuffled, as int32 [n, 4] (b, x, y, z), and synthetic normals where the case needs them."""
import numpy as np

F32 = np.float32


def _rows(xyz, b=0, seed=0):
    xyz = np.unique(np.asarray(xyz, np.int64).reshape(-1, 3), axis=0)
    c = np.concatenate([np.full((len(xyz), 1), b, np.int64), xyz], 1).astype(np.int32)
    return c[np.random.default_rng(seed).permutation(len(c))]


def _box_shell(lo, hi):
    """The voxels of the box lo .. hi (inclusive) with a coordinate at its border."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    return g[((g == lo) | (g == hi)).any(1)]


def shell(k, seed=0):
    """The shell of a k^3 cube: 728 voxels at k = 12, 3176 at k = 24."""
    return _rows(_box_shell((0, 0, 0), (k - 1,) * 3), seed=seed)


CABINET_LO, CABINET_HI = np.array([18, 4, 1]), np.array([25, 11, 8])


def room_with_cabinet(seed=0):
    """``(coords4, cabinet bool [n])``: the shell of a 30^3 room and on its floor the shell of an 8^3 cabinet at x 18..25,
    y 4..11, z 1..8 without a bottom (the 6 x 6 inside of its lowest layer is left out): 5048 + 260 voxels."""
    cab = _box_shell(CABINET_LO, CABINET_HI)
    inner = (cab[:, 2] == 1) & (cab[:, 0] > 18) & (cab[:, 0] < 25) & (cab[:, 1] > 4) & (cab[:, 1] < 11)
    cab = cab[~inner]
    c = _rows(np.concatenate([_box_shell((0, 0, 0), (29, 29, 29)), cab]), seed=seed)
    is_cab = ((c[:, 1:] >= CABINET_LO) & (c[:, 1:] <= CABINET_HI)).all(1)
    assert len(c) == 5308 and is_cab.sum() == 260
    return c, is_cab


def line(m, seed=0):
    """``(coords4, at)``: m voxels along x, rows shuffled; row ``at[x]`` holds the voxel at x."""
    xyz = np.stack([np.arange(m), np.full(m, 3), np.full(m, -2)], 1)
    perm = np.random.default_rng(seed).permutation(m)
    c = np.concatenate([np.zeros((m, 1), np.int64), xyz], 1).astype(np.int32)[perm]
    at = np.empty(m, np.int64)
    at[perm] = np.arange(m)
    return c, at


def plates(k=7, joined=False, seed=0):
    """Two k x k plates an empty layer apart (z = 0 and z = 2); ``joined``: one voxel at z = 1 between their corners."""
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    xyz = [np.concatenate([g, np.full((len(g), 1), z)], 1) for z in (0, 2)]
    if joined:
        xyz.append(np.array([[0, 0, 1]]))
    return _rows(np.concatenate(xyz), seed=seed)


def touching_samples(k=5, seed=0):
    """Two k x k plates side by side in x, the first in batch sample 0 and the second in 1: neighbours in space only."""
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k), indexing="ij"), -1).reshape(-1, 2)
    a = np.concatenate([np.zeros((len(g), 1)), g, np.zeros((len(g), 1))], 1)
    b = np.concatenate([np.ones((len(g), 1)), g + [k, 0], np.zeros((len(g), 1))], 1)
    rng = np.random.default_rng(seed)                                  # (the rows of a batch sample stay together)
    return np.concatenate([a[rng.permutation(len(a))], b[rng.permutation(len(b))]]).astype(np.int32)


def ring(seed=0):
    """``(coords4, normals, at)``: the 40 voxels on the border of an 11 x 11 square in the plane z = 0, and normals
    (cos t, sin t, 0) with t = pi i / 40 at the i-th voxel around: neighbours differ by 4.5 degrees, but the last and the first
    by 175.5 -- the field turns by 180 degrees once around and cannot be oriented.  Row ``at[i]`` holds the i-th voxel."""
    path = [(x, 0) for x in range(10)] + [(10, y) for y in range(10)] + [(x, 10) for x in range(10, 0, -1)] + \
           [(0, y) for y in range(10, 0, -1)]
    assert len(path) == 40 and len(set(path)) == 40
    t = np.pi * np.arange(40) / 40
    nrm = np.stack([np.cos(t), np.sin(t), np.zeros(40)], 1).astype(F32)
    perm = np.random.default_rng(seed).permutation(40)
    c = np.array([(0, x, y, 0) for x, y in path], np.int32)[perm]
    at = np.empty(40, np.int64)
    at[perm] = np.arange(40)
    return c, nrm[perm], at


def random_signs(n, axis=2, seed=0, tilt=0.2):
    """Unit normals near +-axis with random signs and a random tilt: what a surface looks like before it is oriented."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, tilt, (n, 3))
    v[:, axis] = 1.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * rng.choice([-1.0, 1.0], (n, 1))).astype(F32)


def centres(coords4):
    """fp32 [n, 3]: the voxel centres in voxel units (a voxel is centred on its integer coordinates)."""
    return np.asarray(coords4)[:, 1:].astype(F32)
