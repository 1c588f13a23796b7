"""The rule of ``a3d_orient_normals`` (include/agile3d_hip.h) restated on the host, independently of the package and of the
kernels' method (not collected; numpy and ``heapq`` only): the edge function in ``np.float32`` scalars, Dijkstra on (d, s)
with a heap, the parent by the lowest slot, the parity by walking the voxels in ascending dist, the nearest seeds by a sort.
Everything but the edge function is an integer, so the kernels are held to these exactly."""
import heapq

import numpy as np

F32 = np.float32
BAD_INDEX, BAD_COMPONENT = 1, 2
MAX_ROWS, MAX_SWEEPS = 1 << 21, 4096


def slots(connectivity):
    """``[(k, dx, dy, dz)]`` in ascending slot k = (dx + 1) + 3 (dy + 1) + 9 (dz + 1), for the offsets a connectivity admits."""
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for k in range(27):
        d = (k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1)
        if 1 <= sum(abs(c) for c in d) <= limit:
            out.append((k, *d))
    return out


def edge(a, b):
    """``(w, flip, dot)``: fp32, one rounding per operation, in the order the header writes."""
    a = [F32(x) for x in a]
    b = [F32(x) for x in b]
    with np.errstate(all="ignore"):
        dot = F32(F32(F32(a[0] * b[0]) + F32(a[1] * b[1])) + F32(a[2] * b[2]))
        room = F32(F32(1.0) - np.abs(dot))
        room = F32(0.0) if (np.isnan(room) or room < 0) else room          # fmaxf(x, 0): a NaN gives 0
        w = 1 + int(np.floor(F32(F32(1023.0) * room)))
    return w, bool(dot < 0), dot


def admitted(normals):
    n = np.asarray(normals, F32).reshape(-1, 3)
    return np.isfinite(n).all(1) & (n != 0).any(1)


def edges(coords4, normals, connectivity):
    """Per row the list of ``(slot, row of the neighbour, w, flip, dot)`` in ascending slot: both ends admitted, in the same
    batch sample."""
    c = np.asarray(coords4, np.int64).reshape(-1, 4).tolist()
    where = {tuple(p): i for i, p in enumerate(c)}
    ok = admitted(normals)
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    sl = slots(connectivity)
    out = []
    for i, (b, x, y, z) in enumerate(c):
        row = []
        if ok[i]:
            for k, dx, dy, dz in sl:
                j = where.get((b, x + dx, y + dy, z + dz))
                if j is not None and ok[j]:
                    row.append((k, j, *edge(nrm[i], nrm[j])))
        out.append(row)
    return out


def nearest_seeds(normals, components, positions, viewpoint):
    """``(seed uint8 [n], flip uint8 [n], err)`` of the NEAREST mode: per component the candidate with the least (d2, row)."""
    nrm = np.asarray(normals, F32).reshape(-1, 3)
    n = len(nrm)
    comp = np.asarray(components, np.int64)
    pos = np.asarray(positions, F32).reshape(-1, 3)
    vp = np.asarray(viewpoint, np.float64)
    err = BAD_COMPONENT if (comp >= n).any() else 0
    cand = admitted(nrm) & (comp >= 0) & (comp < n) & np.isfinite(pos).all(1)
    best = {}
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(cand).tolist():
            d = [np.float64(pos[i, a]) - vp[a] for a in range(3)]
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            key = (float(d2), i)
            if comp[i] not in best or key < best[comp[i]]:
                best[comp[i]] = key
        seed, flip = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for _, i in best.values():
            t = [vp[a] - np.float64(pos[i, a]) for a in range(3)]
            g = (np.float64(nrm[i, 0]) * t[0] + np.float64(nrm[i, 1]) * t[1]) + np.float64(nrm[i, 2]) * t[2]
            seed[i], flip[i] = 1, int(g < 0)
    return seed, flip, err


def orient_numpy(coords4, normals, connectivity=26, seed_qv=None, seed_flip=None, components=None, positions=None, viewpoint=None,
                 adj=None):
    """dict(normal_out, flipped, dist, owner, parent, summary-without-the-lift): the rule at its fixed point."""
    nrm = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    n = len(nrm)
    ok = admitted(nrm)
    err = 0
    if seed_qv is None:
        seed_qv, seed_flip, err = nearest_seeds(nrm, components, positions, viewpoint)
    seed = ok & (np.asarray(seed_qv) != 0)
    sflip = seed & (np.asarray(seed_flip) != 0) if seed_flip is not None else np.zeros(n, bool)
    adj = edges(coords4, nrm, connectivity) if adj is None else adj
    best = [None] * n
    heap = []
    for s in np.flatnonzero(seed).tolist():
        best[s] = (0, s)
        heap.append((0, s, s))
    heapq.heapify(heap)
    while heap:
        d, s, v = heapq.heappop(heap)
        if best[v] != (d, s):
            continue
        for _, j, w, _, _ in adj[v]:
            if best[j] is None or (d + w, s) < best[j]:
                best[j] = (d + w, s)
                heapq.heappush(heap, (d + w, s, j))
    dist = np.array([-1 if b is None else b[0] for b in best], np.int32).reshape(n)
    owner = np.array([-1 if b is None else b[1] for b in best], np.int32).reshape(n)
    parent = np.full(n, -1, np.int64)
    eflip = np.zeros(n, np.uint8)
    for v in np.flatnonzero(dist > 0).tolist():
        for _, u, w, flip, _ in adj[v]:                                 # ascending slot: the first that qualifies
            if owner[u] == owner[v] and dist[u] + w == dist[v]:
                parent[v], eflip[v] = u, flip
                break
        else:
            raise AssertionError("a reached voxel without a parent: not a fixed point")
    parity = np.zeros(n, np.uint8)
    for v in np.argsort(dist, kind="stable").tolist():                  # ascending dist: the parent is done first
        if dist[v] == 0:
            parity[v] = sflip[v]
        elif dist[v] > 0:
            parity[v] = parity[parent[v]] ^ eflip[v]
    bits = nrm.view(np.uint32).copy()
    bits[parity == 1] ^= np.uint32(0x80000000)
    conflicts = 0
    for i in range(n):
        for k, j, _, _, dot in adj[i]:
            if k > 13:
                conflicts += bool((-dot if parity[i] ^ parity[j] else dot) < 0)
    reached = dist >= 0
    summary = dict(admitted=int(ok.sum()), seeds=int(seed.sum()), reached=int(reached.sum()), unreached=int((ok & ~reached).sum()),
                   flipped=int(parity.sum()), conflicts=conflicts, max_dist=int(dist[reached].max()) if reached.any() else 0,
                   converged=1, err=err)
    return dict(normal_out=bits.view(F32), flipped=parity, dist=dist, owner=owner, parent=parent, summary=summary)


def lift_numpy(normal_out, n_full, inverse_map=None):
    """``(normal_full fp32 [n_full, 3], err)``: a row outside gives zeros and ``BAD_INDEX``."""
    inv = np.arange(n_full, dtype=np.int64) if inverse_map is None else np.asarray(inverse_map, np.int64)
    valid = (inv >= 0) & (inv < len(normal_out))
    out = np.zeros((n_full, 3), F32)
    out[valid] = normal_out[inv[valid]]
    return out, (0 if valid.all() else BAD_INDEX)


def orient_all(coords4, normals, n_full=0, inverse_map=None, **kw):
    """Everything the entry point writes at its fixed point."""
    r = orient_numpy(coords4, normals, **kw)
    r["normal_full"], err = lift_numpy(r["normal_out"], n_full, inverse_map)
    r["summary"]["err"] |= err
    return r


def brute_force(adj, seed, n):
    """(dist, owner) by relaxing every edge until nothing changes: no heap, no order to get right."""
    none = (1 << 62, 1 << 62)
    val = [(0, s) if seed[s] else none for s in range(n)]
    changed = True
    while changed:
        changed = False
        for v in range(n):
            if val[v] == none:
                continue
            for _, j, w, _, _ in adj[v]:
                c = (val[v][0] + w, val[v][1])
                if c < val[j]:
                    val[j], changed = c, True
    dist = np.array([-1 if v == none else v[0] for v in val], np.int32)
    owner = np.array([-1 if v == none else v[1] for v in val], np.int32)
    return dist, owner


def pca_normals(coords4, viewpoint=None):
    """``(normals fp32 [n, 3], planar bool [n])``: the eigenvector of the smallest eigenvalue of the covariance of the voxel
    centres of the 27-neighbourhood (float64 ``eigh``), towards ``viewpoint`` when given, else with its largest component
    positive; zeros below 3 points.  ``planar``: the neighbourhood lies exactly in a plane (integer test: every centre has
    the same offset along one integer normal found by a cross product)."""
    c = np.asarray(coords4, np.int64).reshape(-1, 4)
    where = {tuple(p): i for i, p in enumerate(c.tolist())}
    n = len(c)
    out = np.zeros((n, 3), F32)
    planar = np.zeros(n, bool)
    for i, (b, x, y, z) in enumerate(c.tolist()):
        pts = np.array([(x + dx, y + dy, z + dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                        if (b, x + dx, y + dy, z + dz) in where], np.int64)
        if len(pts) < 3:
            continue
        q = pts - pts.mean(0)
        val, vec = np.linalg.eigh(q.T @ q)
        v = vec[:, 0]
        if viewpoint is not None:
            if np.dot(v, np.asarray(viewpoint, np.float64) - pts.mean(0)) < 0:
                v = -v
        elif v[np.argmax(np.abs(v))] < 0:
            v = -v
        out[i] = v.astype(F32)
        d = pts - pts[0]
        normal = None
        for a in range(1, len(d)):
            for e in range(a + 1, len(d)):
                cr = np.cross(d[a], d[e])
                if cr.any():
                    normal = cr
                    break
            if normal is not None:
                break
        planar[i] = normal is not None and not (d @ normal).any()
    return out, planar
