"""The rule of ``a3d_grow_voxels`` (include/agile3d_hip.h) restated on the host, independently of the package (not collected;
numpy and ``heapq`` only, no import of ``agile3d_amd``): Dijkstra over (dist, owner) pairs on a dict from coordinates to rows,
the lift to the vertices, the summary, and the session's shrink rule.  Everything is integer, so the kernels are held to
these exactly."""
import heapq

import numpy as np

from pieces_rule import neighbours, offsets, serpentine  # noqa: F401  (the constructions the tests share)

BAD_INDEX = 1
METRIC_COST = (1024, 1448, 1774)
MAX_STEPS = 1024


def edges(coords4, connectivity, cost):
    """Per row the list of (row at an admitted offset in the same batch sample, the step's cost = cost[|d|1 - 1])."""
    c = np.asarray(coords4, np.int64).reshape(-1, 4).tolist()
    where = {tuple(p): i for i, p in enumerate(c)}
    offs = offsets(connectivity)
    out = []
    for b, x, y, z in c:
        row = []
        for dx, dy, dz in offs:
            j = where.get((b, x + dx, y + dy, z + dz))
            if j is not None:
                row.append((j, int(cost[abs(dx) + abs(dy) + abs(dz) - 1])))
        out.append(row)
    return out


def seed_rows(n, keys, seed_qv=None, seed_full=None, inverse_map=None):
    """The sorted seed rows: key >= 0 and (seed_qv[row] != 0 or a vertex i with seed_full[i] != 0 and inverse_map[i] == row);
    a seed vertex whose index lies outside the rows is ignored."""
    rows = set()
    if seed_qv is not None:
        rows |= set(np.flatnonzero(np.asarray(seed_qv)).tolist())
    if seed_full is not None:
        marked = np.flatnonzero(np.asarray(seed_full))
        at = marked if inverse_map is None else np.asarray(inverse_map, np.int64)[marked]
        rows |= {int(r) for r in at.tolist() if 0 <= r < n}
    return sorted(r for r in rows if keys[r] >= 0)


def grow_numpy(coords4, keys, cost, limit, connectivity, seed_qv=None, seed_full=None, inverse_map=None):
    """``(dist int32 [n], owner int32 [n])``: per voxel the lexicographic minimum of (d, s) over the seeds s with a walkable
    path of cost d <= limit (walkable: both ends hold the same key >= 0); -1, -1 where there is none.  ``keys`` ``None``: all 0."""
    n = len(coords4)
    keys = np.zeros(n, np.int64) if keys is None else np.asarray(keys, np.int64)
    adj = edges(coords4, connectivity, cost)
    best = [None] * n
    heap = []
    for s in seed_rows(n, keys, seed_qv, seed_full, inverse_map):
        best[s] = (0, s)
        heap.append((0, s, s))
    heapq.heapify(heap)
    while heap:
        d, s, v = heapq.heappop(heap)
        if best[v] != (d, s):
            continue
        for j, c in adj[v]:
            if keys[j] != keys[v] or d + c > limit:
                continue
            if best[j] is None or (d + c, s) < best[j]:
                best[j] = (d + c, s)
                heapq.heappush(heap, (d + c, s, j))
    dist = np.array([-1 if b is None else b[0] for b in best], np.int32).reshape(n)
    owner = np.array([-1 if b is None else b[1] for b in best], np.int32).reshape(n)
    return dist, owner


def lift_numpy(dist, n_full, inverse_map=None):
    """``(selected uint8 [n_full], dist_full int32 [n_full], err)``: an index outside the rows gives 0 / -1 and ``BAD_INDEX``."""
    inv = np.arange(n_full, dtype=np.int64) if inverse_map is None else np.asarray(inverse_map, np.int64)
    assert len(inv) == n_full
    valid = (inv >= 0) & (inv < len(dist))
    dist_full = np.full(n_full, -1, np.int32)
    dist_full[valid] = dist[inv[valid]]
    return (dist_full >= 0).astype(np.uint8), dist_full, (0 if valid.all() else BAD_INDEX)


def summary_numpy(dist, selected, err):
    """The a3d_grow_summary as a dict: a voxel with dist 0 is a seed (every step costs at least 1)."""
    reached = dist >= 0
    return dict(seeds=int((dist == 0).sum()), reached=int(reached.sum()), selected=int(np.asarray(selected).sum()),
                max_dist=int(dist[reached].max()) if reached.any() else 0, err=int(err))


def grow_all(coords4, keys, cost, limit, connectivity, seed_qv=None, seed_full=None, inverse_map=None, n_full=0):
    """Everything the entry point writes: dict(dist_qv, owner_qv, selected_full, dist_full, summary)."""
    dist, owner = grow_numpy(coords4, keys, cost, limit, connectivity, seed_qv, seed_full, inverse_map)
    selected, dist_full, err = lift_numpy(dist, n_full, inverse_map)
    return dict(dist_qv=dist, owner_qv=owner, selected_full=selected, dist_full=dist_full,
                summary=summary_numpy(dist, selected, err))


def shrink_numpy(coords4, inverse_map, selected, cost, limit, connectivity):
    """The session's shrink: the voxels that hold no selected vertex are the outside; a selected vertex stays when its voxel is
    not reached from the outside within ``limit`` (keys all 0).  uint8 [n_full]."""
    n = len(coords4)
    inv = np.asarray(inverse_map, np.int64)
    sel = np.asarray(selected) != 0
    held = np.zeros(n, bool)
    held[inv[sel]] = True
    dist, _ = grow_numpy(coords4, None, cost, limit, connectivity, seed_qv=(~held).astype(np.uint8))
    return (sel & (dist[inv] < 0)).astype(np.uint8)
