"""The rules of ``a3d_label_pieces`` and ``a3d_absorb_pieces`` (include/agile3d_hip.h) restated on the host, independently
of the package (not collected; numpy only, no import of ``agile3d_amd``): a dict from coordinates to rows, union-find, then
the absorb vote.  Everything is integer, so the kernels are held to these exactly."""
import numpy as np

PIECE = np.dtype([("root", "<i4"), ("key", "<i4"), ("voxels", "<i4"), ("clicked", "<i4"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,))])
OVERFLOW, BAD_LABEL, BAD_INDEX = 1, 2, 1


def offsets(connectivity):
    """The (dx, dy, dz) a connectivity admits: 6 means |d|1 = 1, 18 means |d|1 <= 2, 26 means all of the 3^3 table."""
    limit = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= abs(dx) + abs(dy) + abs(dz) <= limit]


def _lookup(coords4):
    return {tuple(c): i for i, c in enumerate(np.asarray(coords4, np.int64).tolist())}


def neighbours(coords4, connectivity):
    """Per row the list of the rows at an admitted offset, in the same batch sample.  ``coords4``: int [n, 4] (b, x, y, z)."""
    where = _lookup(coords4)
    offs = offsets(connectivity)
    out = []
    for b, x, y, z in np.asarray(coords4, np.int64).tolist():
        out.append([j for j in (where.get((b, x + dx, y + dy, z + dz)) for dx, dy, dz in offs) if j is not None])
    return out


def pieces_numpy(coords4, keys, connectivity, click_rows=()):
    """``(piece int32 [n], records PIECE [pieces])``: ``piece[i]`` = the smallest row of i's piece, -1 where ``keys[i] < 0``;
    the records in ascending root."""
    keys = np.asarray(keys, np.int64)
    n = len(keys)
    nbr = neighbours(coords4, connectivity)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        if keys[i] < 0:
            continue
        for j in nbr[i]:
            if keys[j] == keys[i]:
                a, b = find(i), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    piece = np.array([find(i) if keys[i] >= 0 else -1 for i in range(n)], np.int32).reshape(n)
    xyz = np.asarray(coords4, np.int64).reshape(n, 4)[:, 1:]
    clicked = {int(piece[r]) for r in click_rows if 0 <= r < n and piece[r] >= 0}
    roots = np.unique(piece[piece >= 0])
    rec = np.zeros(len(roots), PIECE)
    for k, r in enumerate(roots.tolist()):
        member = piece == r
        rec[k] = (r, keys[r], member.sum(), int(r in clicked), xyz[member].min(0), xyz[member].max(0))
    return piece, rec


def lift_numpy(piece, inverse_map, sentinel):
    """``(piece[inverse_map], err)``: an entry outside the rows keeps ``sentinel`` and sets ``BAD_INDEX``; ``None`` = identity."""
    inv = np.arange(len(piece)) if inverse_map is None else np.asarray(inverse_map, np.int64)
    valid = (inv >= 0) & (inv < len(piece))
    out = np.full(len(inv), sentinel, np.int32)
    out[valid] = piece[inv[valid]]
    return out, (0 if valid.all() else BAD_INDEX)


def absorb_numpy(coords4, labels, min_voxels, connectivity, click_rows=(), n_classes=256, capacity=None):
    """ONE simultaneous step on the input labels: ``(labels_out int32 [n] or None, summary dict)``.  ``None``: more small
    pieces than ``capacity`` -- nothing is written."""
    labels = np.asarray(labels, np.int64)
    piece, rec = pieces_numpy(coords4, labels, connectivity, click_rows)
    nbr = neighbours(coords4, connectivity)
    small = [r for r in rec if r["voxels"] < min_voxels and not r["clicked"]]
    summary = dict(small_pieces=len(small), relabelled_pieces=0, relabelled_voxels=0, kept_isolated=0, err=0)
    if capacity is not None and len(small) > capacity:
        summary["err"] = OVERFLOW
        return None, summary
    out = labels.copy()
    for r in small:
        votes = np.zeros(n_classes, np.int64)
        for i in np.flatnonzero(piece == r["root"]).tolist():
            for j in nbr[i]:
                if labels[j] != labels[i]:
                    votes[labels[j]] += 1
        if votes.max() == 0:
            summary["kept_isolated"] += 1
            continue
        out[piece == r["root"]] = int(votes.argmax())              # (the first maximum: ties go to the lowest label)
        summary["relabelled_pieces"] += 1
        summary["relabelled_voxels"] += int(r["voxels"])
    return out.astype(np.int32), summary


# ---- constructions the host and the GPU tests share ---------------------------------------------------------------------------
def noisy(labels, seed, fraction=0.05):
    """``labels`` with ``fraction`` of the rows relabelled at random (values drawn from the labels present)."""
    rng = np.random.default_rng(seed)
    out = np.asarray(labels).copy()
    rows = rng.choice(len(out), int(round(fraction * len(out))), replace=False)
    out[rows] = rng.choice(np.unique(out), len(rows))
    return out


def serpentine(rows=40, length=64, seed=0):
    """int32 [rows * length + rows - 1, 4]: ``rows`` lines of ``length`` voxels along x, 2 apart in y, joined alternately at
    the ends by one voxel -- ONE piece under every connectivity, of graph diameter rows * (length + 1) - 2 under 6 (2 598 for
    40 x 64) -- with the rows shuffled."""
    pts = []
    for r in range(rows):
        pts += [(0, x, 2 * r, 0) for x in range(length)]
        if r + 1 < rows:
            pts.append((0, length - 1 if r % 2 == 0 else 0, 2 * r + 1, 0))
    pts = np.array(pts, np.int32)
    return pts[np.random.default_rng(seed).permutation(len(pts))]
