"""The rules of ``a3d_similar_pieces`` and ``a3d_vote_pieces`` (include/agile3d_hip.h) restated on the host, independently of
the package (not collected; numpy only, no import of ``agile3d_amd``): the two predicates in ``np.float32`` scalar operations
in the order the header writes them, the edges from ``pieces_rule.neighbours``, components by plain breadth-first search,
records as ``pieces_numpy`` builds them; then the vote, all integers.  The predicates round every operation on its own and
the rest is integer, so the kernels are held to these exactly."""
from collections import deque

import numpy as np

from pieces_rule import PIECE, neighbours

F = np.float32
REF_NORMAL, REF_FEAT = 1, 2
OVERFLOW, BAD_LABEL = 1, 2
VOTE_FIELDS = ("eligible_pieces", "uniform_pieces", "relabelled_pieces", "relabelled_voxels", "blocked_pieces",
               "below_share_pieces", "err")


def nsim(a, b, c, oriented):
    """``dot = (a0*b0 + a1*b1) + a2*b2``; passes iff ``(oriented ? dot : |dot|) >= c``; a NaN fails."""
    with np.errstate(all="ignore"):
        dot = (F(a[0]) * F(b[0]) + F(a[1]) * F(b[1])) + F(a[2]) * F(b[2])
        return bool((dot if oriented else np.abs(dot)) >= F(c))


def fsim(a, b, t):
    """``d_k = a_k - b_k``; ``q = (d0*d0 + d1*d1) + d2*d2``; passes iff ``q <= t``; a NaN fails."""
    with np.errstate(all="ignore"):
        d0, d1, d2 = F(a[0]) - F(b[0]), F(a[1]) - F(b[1]), F(a[2]) - F(b[2])
        return bool((d0 * d0 + d1 * d1) + d2 * d2 <= F(t))


def pair_numpy(normal_a=None, normal_b=None, feat_a=None, feat_b=None, cos_min=1.0, tol2=0.0, oriented=False):
    """The pair predicate: each test only when its pair of values is given."""
    return (normal_a is None or nsim(normal_a, normal_b, cos_min, oriented)) and (feat_a is None or fsim(feat_a, feat_b, tol2))


def similar_numpy(coords4, keys=None, normals=None, feats=None, connectivity=26, cos_min=1.0, tol2=0.0, oriented=False,
                  ref_normal=None, ref_cos_min=1.0, ref_feat=None, ref_tol2=0.0, click_rows=()):
    """``(piece int32 [n], records PIECE [pieces])``: ``piece[i]`` = the smallest row of i's piece, -1 for a row that is not
    admissible; the records in ascending root.  ``keys`` ``None``: all 0."""
    n = len(coords4)
    keys = np.zeros(n, np.int64) if keys is None else np.asarray(keys, np.int64)
    nbr = neighbours(coords4, connectivity)
    ok = [bool(keys[i] >= 0 and (ref_normal is None or nsim(normals[i], ref_normal, ref_cos_min, oriented))
               and (ref_feat is None or fsim(feats[i], ref_feat, ref_tol2))) for i in range(n)]

    def joined(i, j):
        return ok[j] and keys[j] == keys[i] and (normals is None or nsim(normals[i], normals[j], cos_min, oriented)) and \
            (feats is None or fsim(feats[i], feats[j], tol2))

    piece = np.full(n, -1, np.int32)
    for start in range(n):                       # ascending: the first row that reaches a component is its smallest
        if not ok[start] or piece[start] >= 0:
            continue
        piece[start] = start
        queue = deque([start])
        while queue:
            i = queue.popleft()
            for j in nbr[i]:
                if piece[j] < 0 and joined(i, j):
                    piece[j] = start
                    queue.append(j)
    return piece, records_numpy(coords4, piece, keys, click_rows)


def records_numpy(coords4, piece, keys, click_rows=()):
    n = len(piece)
    xyz = np.asarray(coords4, np.int64).reshape(n, 4)[:, 1:]
    clicked = {int(piece[r]) for r in click_rows if 0 <= r < n and piece[r] >= 0}
    roots = np.unique(piece[piece >= 0])
    rec = np.zeros(len(roots), PIECE)
    for k, r in enumerate(roots.tolist()):
        member = piece == r
        rec[k] = (r, keys[r], member.sum(), int(r in clicked), xyz[member].min(0), xyz[member].max(0))
    return rec


def closure_numpy(n, edges, admissible):
    """Brute force: the transitive closure of a symmetric edge list by repeated squaring of the boolean reachability matrix
    (shares nothing with the search above).  ``piece[i]`` = the smallest row i reaches, -1 where not admissible."""
    reach = np.eye(n, dtype=bool)
    for i, j in edges:
        reach[i, j] = reach[j, i] = True
    while True:
        more = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if (more == reach).all():
            break
        reach = more
    return np.array([int(np.flatnonzero(reach[i])[0]) if admissible[i] else -1 for i in range(n)], np.int32).reshape(n)


def vote_numpy(piece, labels, min_voxels=8, share=(2, 3), click_rows=(), n_classes=256, capacity=None):
    """ONE simultaneous step on the input labels: ``(labels_out int32 [n] or None, summary dict)``.  ``None``: more eligible
    pieces than ``capacity`` -- nothing is written."""
    piece, labels = np.asarray(piece, np.int64), np.asarray(labels, np.int64)
    n, (num, den) = len(labels), share
    summary = dict.fromkeys(VOTE_FIELDS, 0)
    in_range = (labels >= 0) & (labels < n_classes)
    roots = [int(r) for r in np.unique(piece[piece >= 0]) if (piece == r).sum() >= min_voxels]
    summary["eligible_pieces"] = len(roots)
    if capacity is not None and len(roots) > capacity:
        summary["err"] = OVERFLOW
        return None, summary
    if not in_range.all():
        summary["err"] |= BAD_LABEL
    out = labels.copy()
    for r in roots:
        member = piece == r
        voxels = int(member.sum())
        votes = np.bincount(labels[member & in_range], minlength=n_classes)
        winner = int(votes.argmax())                                 # the first maximum: ties go to the lowest label
        most, cast = int(votes[winner]), int(votes.sum())
        if most == voxels:
            summary["uniform_pieces"] += 1
        elif most * den < voxels * num:                              # Python integers
            summary["below_share_pieces"] += 1
        elif any(0 <= c < n and piece[c] == r and labels[c] != winner for c in click_rows):
            summary["blocked_pieces"] += 1
        else:
            out[member & in_range] = winner
            if cast > most:
                summary["relabelled_pieces"] += 1
                summary["relabelled_voxels"] += cast - most
    return out.astype(np.int32), summary
