"""Scenes for the tests of ``a3d_find_planes`` (not collected; numpy only): hand-made planes with exact normals, and the room
of DESIGN 4.9 -- floor, ceiling, four walls, a table top and a sphere, voxelised to one row per voxel."""
import numpy as np

import planes_rule as PR

VOXEL = 0.05
BITS = 20


def frame(positions, bits=BITS):
    """``(origin float64 [3], quantum, bits)`` as the session makes it: the centre of the finite points' box, and the power of
    two that brings the largest half extent to 2^bits quanta."""
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    lo, hi = (p.min(0), p.max(0)) if len(p) else (np.zeros(3), np.zeros(3))
    origin = 0.5 * (lo + hi)
    half = float(np.maximum(hi - origin, origin - lo).max())
    e = int(np.ceil(np.log2(half))) if half > 0 else 0
    while 2.0 ** e < half:
        e += 1
    return origin, 2.0 ** (e - bits), bits


def settings(quantum, normal_deg=20.0, offset_bin=VOXEL, dist_tol=1.5 * VOXEL, min_voxels=200, max_planes=16):
    """The keyword arguments of ``planes_rule.find_planes`` after the frame, from world units."""
    w, tol, cos_min = PR.settings(quantum, offset_bin, normal_deg, dist_tol)
    return dict(bin_width=w, dist_tol=tol, cos_min=cos_min, min_voxels=min_voxels, max_planes=max_planes)


def rectangle(normal, offset, side, count, rng=None, jitter=0.0, centre=(0.0, 0.0, 0.0)):
    """``count`` points (fp32 [count, 3]) of the plane ``normal . p = offset`` on a square grid of ``side`` around the foot of
    ``centre``, and that many copies of the unit normal (fp32)."""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    m = int(np.ceil(np.sqrt(count)))
    g = (np.arange(m) + 0.5) / m - 0.5
    uv = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)[:count] * side
    c = np.asarray(centre, np.float64)
    foot = c + (offset - n @ c) * n
    p = foot + uv[:, :1] * a + uv[:, 1:] * b
    if rng is not None and jitter:
        p = p + rng.uniform(-jitter, jitter, p.shape)
    return p.astype(np.float32), np.tile(n.astype(np.float32), (count, 1))


# ---- hand-made planes: a cell centre's unit vector as the normal, the centre of an offset bin of that cell, in a fixed frame ----
ORIGIN, QUANTUM = (0.0, 0.0, 0.0), 2.0 ** -18
BIN = 0.05
G, D = PR.G, PR.D


def cell_of(a, iu, iv):
    return (a * G + iu) * G + iv


def cell_normal(cell):
    c = PR.direction_table()[cell].astype(np.float64)
    return c / np.linalg.norm(c)


def plate(cell, k, count, side=1.0, frac=0.5):
    """``count`` rows of the plane whose normal is cell ``cell``'s centre, at ``frac`` of the way through offset bin k."""
    return rectangle(cell_normal(cell), (k - D // 2 + frac) * BIN, side, count)


A, B, Cc = cell_of(2, 8, 8), cell_of(0, 5, 11), cell_of(1, 3, 3)


def spent_then_found():
    """199 rows in one bin, then a plane of 300 whose normals straddle a cell border (150 votes a cell)."""
    n = np.array([0.25, 0.0, 1.0]) / np.linalg.norm([0.25, 0.0, 1.0])
    p, _ = rectangle(n, 0.4, 0.6, 300)
    v = np.tile(np.float32([0.25, 0.0, 1.0]), (300, 1))
    v[::2, 0] = 0.26
    v[1::2, 0] = 0.24
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return [plate(B, 450, 199), (p, v.astype(np.float32))]


def seventeen():
    """Seventeen planes in seventeen cells, of 60 .. 76 rows."""
    return [plate(cell_of(i % 3, 2 + (5 * i) % 12, 1 + (7 * i) % 13), 480 + 3 * i, 60 + i, side=0.5) for i in range(17)]


def all_spent():
    """Five planes of 30 .. 26 rows: too small to record at min_voxels = 40, large enough to be a peak."""
    return [plate(cell_of(i % 3, 3 + i, 4), 500 + i, 30 - i, side=0.4) for i in range(5)]


def rotation(deg_x, deg_z):
    ax, az = np.radians(deg_x), np.radians(deg_z)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return rz @ rx


ROOM_SURFACES = ("floor", "ceiling", "wall_x0", "wall_x1", "wall_y0", "wall_y1", "table", "sphere")
SPHERE = ROOM_SURFACES.index("sphere")


def room(yaw_deg, sigma_deg=3.0, seed=0, size=(4.0, 3.0, 2.5), voxel=VOXEL, tilt_deg=3.0, scale=1.0):
    """The room: ``(positions fp32 [n, 3], normals fp32 [n, 3], surface int64 [n] (an index into ROOM_SURFACES), planted
    float64 [7, 3] (the unit normals of the seven planes, rotated), R)``.  A 4 x 3 x 2.5 m box (``scale`` shrinks it), a 1.2 x
    0.8 m table top 0.75 m up, a sphere of radius 0.4 m centred 1.5 m up (its caps -- the rows whose normals pass the cosine
    test of a planted plane -- lie 0.35 m or more from every planted plane: nearer than two offset bins a cap shares the seeds
    of a small plane and tilts its fit); rotated by ``tilt_deg`` about x and ``yaw_deg`` about z;
    sampled at half a voxel, positions jittered by a quarter voxel, then VOXELISED: the first sample of a voxel stays.  Every
    component of a normal gets Gaussian noise of ``sigma_deg`` (in radians) before it is normalised again."""
    rng = np.random.default_rng(seed)
    sx, sy, sz = [s * scale for s in size]
    h = voxel / 2

    def grid(u, v):
        return np.stack(np.meshgrid(np.arange(h / 2, u, h), np.arange(h / 2, v, h), indexing="ij"), -1).reshape(-1, 2)

    parts = []

    def plane(axis, value, u, v, origin_uv=(0.0, 0.0)):
        uv = grid(u, v) + origin_uv
        p = np.zeros((len(uv), 3))
        p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = value, uv[:, 0], uv[:, 1]
        n = np.zeros(3)
        n[axis] = 1.0
        parts.append((p, np.tile(n, (len(p), 1))))

    plane(2, 0.0, sx, sy), plane(2, sz, sx, sy)
    plane(0, 0.0, sy, sz), plane(0, sx, sy, sz)
    plane(1, 0.0, sz, sx), plane(1, sy, sz, sx)
    plane(2, 0.75 * scale, 1.2 * scale, 0.8 * scale, (0.5 * scale, 0.4 * scale))
    r = 0.4 * scale
    centre = np.array([sx - 1.0 * scale, sy - 1.0 * scale, 1.5 * scale])
    k = int(4 * np.pi * r * r / (h * h))
    i = np.arange(k) + 0.5
    phi, theta = np.arccos(1 - 2 * i / k), np.pi * (1 + 5 ** 0.5) * i
    d = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], -1)
    parts.append((centre + r * d, d))
    surface = np.concatenate([np.full(len(p), s) for s, (p, _) in enumerate(parts)])
    R = rotation(tilt_deg, yaw_deg)
    p = np.concatenate([p for p, _ in parts]) @ R.T + rng.uniform(-voxel / 4, voxel / 4, (len(surface), 3))
    nrm = np.concatenate([n for _, n in parts]) @ R.T
    _, first = np.unique(np.floor(p / voxel).astype(np.int64), axis=0, return_index=True)
    first.sort()
    p, nrm, surface = p[first], nrm[first], surface[first]
    nrm = nrm + rng.normal(0.0, np.radians(sigma_deg), nrm.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    planted = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 1]], np.float64) @ R.T
    return p.astype(np.float32), nrm.astype(np.float32), surface, planted, R


def room_report(out, surface, planted):
    """Per planted plane ``(id, share of its rows under that id, angle in degrees between the fit and the planted normal)``,
    and per recorded plane the share of sphere rows among its rows."""
    qv = out["plane_qv"]
    rows = []
    for s in range(len(planted)):
        ids = qv[surface == s]
        ids = ids[ids >= 0]
        if not len(ids):
            rows.append((-1, 0.0, 180.0))
            continue
        k = int(np.bincount(ids).argmax())
        share = float((qv[surface == s] == k).mean())
        rows.append((k, share, float(np.degrees(PR.NR.angle(out["records"]["normal"][k], planted[s])))))
    sphere = [float((surface[qv == k] == SPHERE).mean()) for k in range(len(out["records"]))]
    return rows, sphere
