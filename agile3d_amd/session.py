"""A headless interactive session: pick, click, paint full-resolution labels.

The third caller of the model API in the reference is its interactive tool (``interactive_tool/
interactive_segmentation_user.py`` + ``gui.py``).  ``InteractiveSession`` is that tool without a window: the same
sequence of model calls (``forward_backbone`` once per scene, ``forward_mask`` per inference), the same click
dictionaries, relabelled ground truth, record line and ``.npy`` files -- and no Open3D.  What surrounds the two model
calls runs in ``libagile3d_hip.so`` (``csrc/session.hip``, ``csrc/clicks.hip``), reached through ``view.py`` and ``clicks.py``:

    pointer ray -> clicked point        a3d_pick_ray       (the GUI renders a depth image and unprojects, gui.py:247-271)
                                        a3d_pick_mesh      (the same for a triangle mesh: the first SURFACE under the pointer)
    the view of the labelled scan       a3d_render_mesh / a3d_render_points / a3d_render_shade  (Open3D's renderer in the
                                        GUI): id, depth and colour images, pixel by pixel what the two picks return
    vertex normals, the lit material    a3d_vertex_normals / a3d_render_shade_lit / a3d_render_shade_depth  (gui.py:556-557,
                                        135): render(lit=True); rules of ours, Open3D's lit material is not reproduced
    the camera that frames the scene    default_view       (gui.py:561-565; host code)
    the object under a pixel, object    a3d_render_labels / a3d_render_annotate  (label_image, object_at, annotate: the
    borders, the clicks in the view     GUI's user reads them off the window; rules of ours)
    find_nearest, twice per click       a3d_nearest_rows   (utils.py:27-29: two full torch.cdist calls; here exact)
    argmax + clicked rows               a3d_argmax_labels  (interactive_segmentation_user.py:78-81)
    pred[inverse_map], colours, cubes   a3d_session_paint  (:83-84,125-140; gui.py:276-298,327)
    IoU against the relabelled truth    a3d_iou_counts     (:86-88)
    looking into the scan               a3d_pick_ray_section / a3d_pick_mesh_section / a3d_render_mesh_section /
                                        a3d_render_points_section  (Section, set_section: section planes and back-face
                                        culling; in the GUI the camera's near plane cuts a wall away; a rule of ours)
    taking a click back, resuming       a3d_session_edit   (undo, redo, remove_click, restore_clicks / restore_file: the
                                        GUI's "unselect point" is a TODO, gui.py:283-287; a rule of ours)
    where the labels are unsure, the    a3d_session_guide + a3d_click_clusters  (guide, confidence_at: the tool drops the
    next click                          logits after the arg-max, :78-81; a rule of ours)
    where in space a label lies         a3d_label_pieces / a3d_absorb_pieces  (pieces, piece_at, despeckle, guide(regions=
                                        "connected"): connected pieces of a labelling on the voxel lattice; a rule of ours)
    how big an object is, its boxes     a3d_measure_objects / a3d_object_extents  (measure, MeasureResult.section, frame: size,
                                        centroid, axis-aligned and oriented box, covered surface per object; a rule of ours)
    circling what is still wrong and    a3d_region_mask / a3d_select_vertices / a3d_session_overlay  (region_mask, select, paint,
    saying what it is                   erase, corrected: a manual label layer over the model's labels; Open3D gives the
                                        GUI no lasso; a rule of ours)
    which way a cloud's surface faces   a3d_estimate_normals / a3d_render_shade_lit_points / a3d_cull_points  (estimate_normals,
                                        normal_at: one normal per voxel from its 27-voxel neighbourhood; after it a cloud is
                                        lit and culled as a mesh is; the GUI shows clouds unlit; a rule of ours)
    which voxels belong to one surface  a3d_similar_pieces / a3d_vote_pieces  (patches, wand_at, snap: connected components
                                        under a similarity of normals and colours, the patch under a pixel as a selection,
                                        labels snapped to patches by a vote that never contradicts a click; a rule of ours)
    labels on another point set         a3d_point_index_create / a3d_point_index_nearest  (nearest_vertices, transfer,
                                        import_labels: an index over any point set and the bulk exact nearest row within a
                                        reach -- labels to a high-resolution mesh, ground truth from one; a rule of ours)
    more objects like this one          a3d_feature_prototypes / a3d_feature_match  (lookalikes, lookalike_at: one prototype per
                                        example object from the backbone's features, the voxels within a cosine threshold of
                                        one, their connected regions and a suggested click in each; a rule of ours)

There is no CPU path: the model and the scene live on the GPU.

Departures from the reference, on purpose:
  * nearest rows are EXACT (fp32 distances from the coordinate differences); ``torch.cdist`` for one query row uses
    |a|^2 + |b|^2 - 2ab and misses the nearest row on scenes far from the origin;
  * object ids beyond the palette wrap around it (the reference's colour table raises ``KeyError`` above 10 objects);
  * ``infer()`` without a click raises (the reference returns early at ``num_clicks == 0``): a caller that asks for a
    segmentation with nothing to segment has a bug worth hearing about;
  * ``click`` refuses what the model would refuse later (an object id that leaves a gap, too many queries);
  * a click is kept even when no vertex lies inside its cube (the GUI drops it, gui.py:281-282);
  * clicks can be taken back and a saved click file resumed (the reference does neither).  The session's state is a function
    of ONE ordered click list (``click_state``, ``remove_from_clicks``, ``instance_rows``): entry i is the click with time
    index i; removing one lowers the time indices behind it, and removing an object's only click renumbers the objects above
    it, so ids stay 1..K and times 0..m-1.  The relabelled ground truth of a list gives a vertex the HIGHEST object whose
    instance (the original label under the object's EARLIEST click in the list) it carries -- in a session grown by clicks
    alone that is the reference's "last created wins" (gui.py:318-319).  After an edit the labels shown are the last
    inference's with the ids renumbered, not an earlier inference restored.
"""
from __future__ import annotations

import colorsys
import os
from datetime import datetime

import numpy as np
import torch

from . import clicks as K
from . import lib as L
from . import ply
from . import view as V
from .sparse import SparseTensor, sparse_quantize

RECORD_FILE, MASK_DIR, CLICK_DIR = "iou_record.csv", "masks", "clicks"
BACKGROUND_CLICK_COLOR = (0.85, 0.15, 0.15)     # colour of a background click's cube (this project's choice)
_N_IDS = 256                                    # object ids the IoU kernel counts (labels are 0..255)


def default_palette(n_objects: int = 20) -> np.ndarray:
    """[n_objects + 1, 3] fp32 colours in [0, 1], entry k = object k (entry 0, background, is never used: background
    vertices keep their own colour).  Hues walk the circle by the golden angle, so neighbouring ids stay apart."""
    pal = np.zeros((n_objects + 1, 3), np.float32)
    for k in range(1, n_objects + 1):
        pal[k] = colorsys.hsv_to_rgb((0.11 + 0.618033988749895 * (k - 1)) % 1.0, 0.85 if k % 2 else 0.6, 0.95)
    return pal


# ---- the strings the reference writes (interactive_segmentation_user.py:86-108), pure host code ------------------------
def format_iou(miou) -> str:
    """``'NA'`` without ground truth, else the mean IoU (a float32 value) in per cent, rounded to one decimal."""
    if miou is None:
        return "NA"
    return str(round(float(miou) * 100, 1))


def format_avg_clicks(num_clicks: int, num_obj: int) -> str:
    return str(round(num_clicks / num_obj, 1))


def record_line(now: datetime, scene_name: str, num_obj: int, num_clicks: int, iou: str) -> str:
    return (now.strftime("%Y-%m-%d-%H-%M-%S") + "  " + scene_name + "  NumObjects:" + str(num_obj) + "  AvgNumClicks:"
            + format_avg_clicks(num_clicks, num_obj) + "  mIoU:" + iou + "\n")


def mask_file_name(num_clicks: int, num_obj: int, iou: str) -> str:
    return "mask_" + format_avg_clicks(num_clicks, num_obj) + "_" + iou + ".npy"


def click_file_name(num_clicks: int, num_obj: int, iou: str) -> str:
    return "click_" + format_avg_clicks(num_clicks, num_obj) + "_" + iou + ".npy"


# ---- the click list and what derives from it: pure Python / numpy, no library ----------------------------------------------
# A click is a mapping with ``obj`` (0 = background), ``point`` (the picked point, three fp32 values), ``row_qv`` (voxel row),
# ``row_full`` (full-resolution vertex row) and ``position`` (that vertex's coordinates, a list).  A click LIST is a sequence
# of clicks in time order: entry i is the click with time index i.  The functions below never modify their arguments.
def click_state(clicks):
    """``(click_idx, click_time_idx, click_positions)`` of a click list, the dictionaries ``forward_mask`` and the click
    files take: under ``str(k)`` object k's voxel rows in time order, their indices in the list, their vertex positions.
    ``"0"`` is always there and comes first; an object's key appears where its first click does.  The object ids present
    must be exactly 1..K (``ValueError`` otherwise): ``forward_mask`` serves no gap."""
    idx, time_idx, positions = {"0": []}, {"0": []}, {"0": []}
    for i, c in enumerate(clicks):
        obj = int(c["obj"])
        if not 0 <= obj <= 255:
            raise ValueError(f"click {i}: object ids are 0 (background) .. 255, not {obj}")
        key = str(obj)
        if key not in idx:
            idx[key], time_idx[key], positions[key] = [], [], []
        idx[key].append(int(c["row_qv"]))
        time_idx[key].append(i)
        positions[key].append(list(c["position"]))
    n_obj = len(idx) - 1
    missing = [k for k in range(1, n_obj + 1) if str(k) not in idx]
    if missing:
        raise ValueError(f"the objects of a click list must be 1..K without a gap: {n_obj} objects, but no click on {missing}")
    return idx, time_idx, positions


def remove_from_clicks(clicks, index):
    """``(new_clicks, lut)``: the click list without entry ``index`` (``IndexError`` outside ``[0, len)``; no wrap-around).
    The entries behind it move up, which lowers their time index by one.  If the click was its object's only one the
    object ceases to exist and every id above it drops by one.  ``lut`` uint8 [256] maps old to new ids: the identity when
    no object disappeared; else removed id k -> 0 and j -> j - 1 for j > k."""
    clicks = list(clicks)
    if int(index) != index or not 0 <= index < len(clicks):
        raise IndexError(f"click {index} of {len(clicks)}")
    gone = clicks.pop(int(index))
    lut = np.arange(256, dtype=np.uint8)
    k = int(gone["obj"])
    if k > 0 and all(int(c["obj"]) != k for c in clicks):
        lut[k] = 0
        lut[k + 1:] = np.arange(k, 255, dtype=np.uint8)
        clicks = [dict(c, obj=int(lut[int(c["obj"])])) if int(c["obj"]) > k else c for c in clicks]
    return clicks, lut


def restore_lut(lut):
    """The table that takes ``remove_from_clicks``' renumbering back: ids at or above the removed one move up again.  The
    removed object's own labels became background and stay so -- a renumbering keeps no memory of them."""
    lut = np.asarray(lut, dtype=np.uint8)
    back = np.arange(256, dtype=np.uint8)
    gone = np.flatnonzero(lut[1:] == 0)
    if len(gone):
        k = int(gone[0]) + 1
        back[k:255] = np.arange(k + 1, 256, dtype=np.uint8)
        back[255] = 0                                  # (no label: 255 objects before the removal left at most 254)
    return back


def instance_rows(clicks):
    """The voxel rows that name the objects' instances: entry k - 1 is ``row_qv`` of the EARLIEST click of object k in the
    list, k = 1..K.  The relabelled ground truth of the list: a vertex gets the HIGHEST k with
    ``labels_qv_ori[rows[k - 1]] == labels_full_ori[vertex]``, else 0 (``a3d_session_edit``)."""
    first = {}
    for c in clicks:
        first.setdefault(int(c["obj"]), int(c["row_qv"]))
    n_obj = max(first, default=0)
    if any(k not in first for k in range(1, n_obj + 1)):
        raise ValueError("the objects of a click list must be 1..K without a gap")
    return [first[k] for k in range(1, n_obj + 1)]


def clicks_from_dicts(click_idx, click_time_idx, n_rows, max_clicks):
    """``[(obj, voxel row), ...]`` in time order from the two dictionaries of a click file (``click_idx``, ``click_time``)
    -- what ``restore_clicks`` rebuilds its list from.  ``ValueError`` unless: both have the keys ``"0".."K"`` exactly, an
    object k >= 1 has at least one click, rows and times pair up, the times are a permutation of 0..m-1, every row lies in
    ``[0, n_rows)`` and m <= ``max_clicks``."""
    if not isinstance(click_idx, dict) or not isinstance(click_time_idx, dict):
        raise ValueError("click_idx and click_time_idx must be dictionaries")
    keys = [str(k) for k in range(len(click_idx))]
    if sorted(map(str, click_idx)) != sorted(keys) or sorted(map(str, click_time_idx)) != sorted(keys) or not keys:
        raise ValueError(f'click_idx and click_time_idx must both have the keys "0" .. "K" exactly, not {list(click_idx)} '
                         f"and {list(click_time_idx)}")
    if any(not isinstance(k, str) for k in list(click_idx) + list(click_time_idx)):
        raise ValueError("the keys of click_idx and click_time_idx are strings")
    by_time = {}
    for key in keys:
        rows, times = list(click_idx[key]), list(click_time_idx[key])
        if len(rows) != len(times):
            raise ValueError(f"object {key}: {len(rows)} rows but {len(times)} time indices")
        if key != "0" and not rows:
            raise ValueError(f"object {key} has no click")
        for r, t in zip(rows, times):
            if int(r) != r or int(t) != t:
                raise ValueError(f"object {key}: rows and time indices must be integers")
            if not 0 <= r < n_rows:
                raise ValueError(f"object {key}: row {r} outside the {n_rows} voxels")
            if t in by_time:
                raise ValueError(f"time index {t} appears twice")
            by_time[int(t)] = (int(key), int(r))
    m = len(by_time)
    if sorted(by_time) != list(range(m)):
        raise ValueError(f"the time indices must be a permutation of 0 .. {m - 1}")
    if m > max_clicks:
        raise ValueError(f"{m} clicks, but at most {max_clicks} fit beside the background queries")
    return [by_time[t] for t in range(m)]


def marker_hit(markers, u, v, t_pixel, marker_px, depth_slack):
    """The row of ``markers`` (fp32 [k, 6], ``view.marker_table``) that ``a3d_render_annotate`` draws on top at pixel
    ``(u, v)`` (column, row) whose ``t`` image holds ``t_pixel``, or ``None``: the LAST row with ``d2 <= marker_px^2`` and
    ``t_k - t_pixel <= depth_slack``, ``d2 = dx dx + dy dy`` from ``dx = u - x_k``, ``dy = v - y_k`` -- each a single fp32
    operation, as the kernel does them; a row with a NaN covers nothing."""
    f32 = np.float32
    m = np.asarray(markers, dtype=f32).reshape(-1, 6)
    if not len(m):
        return None
    with np.errstate(all="ignore"):
        dx, dy = f32(u) - m[:, 0], f32(v) - m[:, 1]
        d2 = dx * dx + dy * dy
        cover = (d2 <= f32(marker_px) * f32(marker_px)) & (m[:, 2] - f32(t_pixel) <= f32(depth_slack))
    cover &= ~np.isnan(m).any(1)
    hits = np.flatnonzero(cover)
    return int(hits[-1]) if len(hits) else None


def rank_suggestions(clusters, coords_row_lookup, max_suggestions):
    """The suggested clicks of ``guide()``, best first, from the records of the cluster search (dicts with ``cluster_id``,
    ``row``, ``label``, ``pred``, ``error_size``; any order): ranked by ``error_size``, largest first; equal sizes keep
    ascending cluster id -- the stable order ``clicks._pick_clicks`` ranks by, without its shuffle.  At most
    ``max_suggestions`` entries ``{row, point, object, current, size}``: the voxel row, its coordinates (``coords_row_lookup``:
    a callable ``row -> xyz`` or anything indexed by the row), the object the click would go to (the record's ``label``: the
    region's runner-up), the object the row has now (its ``pred``), the distance from the row to the region's border in
    metres.  Pure Python."""
    if int(max_suggestions) != max_suggestions or max_suggestions < 0:
        raise ValueError("max_suggestions must be an integer >= 0")
    lookup = coords_row_lookup if callable(coords_row_lookup) else coords_row_lookup.__getitem__
    ranked = sorted(sorted(clusters, key=lambda c: c["cluster_id"]), key=lambda c: c["error_size"], reverse=True)
    return [{"row": int(c["row"]), "point": [float(x) for x in lookup(int(c["row"]))], "object": int(c["label"]),
             "current": int(c["pred"]), "size": float(c["error_size"])} for c in ranked[:int(max_suggestions)]]


def suggest_clicks(clusters, least_confident, coords_row_lookup, max_suggestions):
    """``rank_suggestions`` -- unless a record's ``error_size`` is not finite: the search found a region that has nothing
    outside it, so it covers every voxel (and is the only record) and no voxel is deeper in it than another.  The
    suggestion is then the least confident voxel alone (``least_confident`` = ``(row, margin)``), for the region's runner-up,
    with ``size = inf``; none when there is no such voxel.  Pure Python."""
    if all(np.isfinite(c["error_size"]) for c in clusters):
        return rank_suggestions(clusters, coords_row_lookup, max_suggestions)
    if least_confident is None:
        return []
    whole = next(c for c in clusters if not np.isfinite(c["error_size"]))
    return rank_suggestions([dict(whole, row=int(least_confident[0]), error_size=float("inf"))], coords_row_lookup,
                            min(1, max_suggestions))


MAX_SPOTS = 255                                 # the pseudo ids 1..255 the cluster search tells apart


def rank_spots(records, max_spots=MAX_SPOTS):
    """The spots ``guide(regions="connected")`` searches, from the records of ``a3d_label_pieces`` (anything with ``root`` and
    ``voxels`` per entry; any order): ranked by size, largest first, ties to the lower root; at most ``max_spots``.  Returns
    the indices into ``records``; the spot at position k gets pseudo id k + 1.  Pure Python."""
    if int(max_spots) != max_spots or max_spots < 0:
        raise ValueError("max_spots must be an integer >= 0")
    order = sorted(range(len(records)), key=lambda k: (-int(records[k]["voxels"]), int(records[k]["root"])))
    return order[:int(max_spots)]


def rank_candidates(clusters, spots, coords_row_lookup, max_candidates):
    """The candidates of ``lookalikes()``, best first, from the records of the cluster search over the searched regions
    (dicts with ``cluster_id``, ``row``, ``label`` = the region's pseudo id, ``error_size``; any order) and ``spots``, the
    regions' ``a3d_label_pieces`` records in pseudo-id order (``spots[label - 1]``; ``key`` = the matched object): ranked by
    ``error_size`` -- the depth of the region's deepest voxel -- largest first, equal depths in ascending cluster id, as
    ``rank_suggestions`` ranks.  At most ``max_candidates`` entries ``{point, row, object, voxels, root, depth}``.  Pure
    Python."""
    if int(max_candidates) != max_candidates or max_candidates < 0:
        raise ValueError("max_candidates must be an integer >= 0")
    lookup = coords_row_lookup if callable(coords_row_lookup) else coords_row_lookup.__getitem__
    ranked = sorted(sorted(clusters, key=lambda c: c["cluster_id"]), key=lambda c: c["error_size"], reverse=True)
    out = []
    for c in ranked[:int(max_candidates)]:
        spot = spots[int(c["label"]) - 1]
        out.append({"point": [float(x) for x in lookup(int(c["row"]))], "row": int(c["row"]), "object": int(spot["key"]),
                    "voxels": int(spot["voxels"]), "root": int(spot["root"]), "depth": float(c["error_size"])})
    return out


class _Result:
    """What the ``*Result`` classes share: keyword arguments become the fields their ``__slots__`` name, ``None`` for what
    was not given."""

    __slots__ = ()

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class PiecesResult(_Result):
    """What ``pieces()`` returns.  Device tensors: ``piece_qv`` int32 [n_voxels] (the smallest voxel row of the voxel's piece)
    and ``piece_full`` int32 [n_full] (the same lifted to the vertices).  Host: ``records``, a numpy structured array
    (``view.PIECE``: root, key = the object id, voxels, clicked, lo, hi) in ascending root; ``object_pieces`` int64 (pieces per
    object id); ``n_pieces``; ``connectivity`` as used."""

    __slots__ = ("piece_qv", "piece_full", "records", "object_pieces", "n_pieces", "connectivity")


class DespeckleResult(_Result):
    """What ``despeckle()`` returns: ``labels_full``, ``colors``, ``miou`` and ``iou_per_object`` as a ``SessionResult`` holds
    them, ``labels_qv`` int32 [n_voxels] on the device, and the counts of ``a3d_absorb_pieces``' summary: ``small_pieces``,
    ``relabelled_pieces``, ``relabelled_voxels``, ``kept_isolated``; ``min_voxels`` and ``connectivity`` as used."""

    __slots__ = ("labels_full", "colors", "miou", "iou_per_object", "labels_qv", "small_pieces", "relabelled_pieces",
                 "relabelled_voxels", "kept_isolated", "min_voxels", "connectivity")


class PatchesResult(_Result):
    """What ``patches()`` returns: the fields of a ``PiecesResult`` -- ``piece_qv`` int32 [n_voxels] (the smallest voxel row of
    the voxel's patch, -1: none; ``grow(within=r.piece_qv)`` walks inside one patch), ``piece_full`` int32 [n_full], ``records``
    (``view.PIECE``; key = the key of ``within``, 0 with ``"all"``) in ascending root, ``n_pieces``, ``connectivity``,
    ``object_pieces`` (patches per object id with ``within="label"``, else ``None``) -- and the thresholds as used:
    ``normal_deg`` and ``cos_min`` (fp32; ``None``: no normal test), ``color_tol`` and ``tol2`` (fp32; ``None``: no colour
    test), ``oriented``, ``within``; and ``workspace``, the call's scratch on the device, which holds the patches' sizes for ``snap``."""

    __slots__ = PiecesResult.__slots__ + ("normal_deg", "cos_min", "color_tol", "tol2", "oriented", "within", "workspace")


class WandResult(_Result):
    """What ``wand_at()`` returns: ``selected`` uint8 [n_full] on the device (1 = the vertex lies in the patch under the pixel;
    ``paint``, ``erase``, ``grow`` and ``shrink`` take the result as it is), ``piece_qv`` int32 [n_voxels] (the partition the
    call computed), and on the host ``count`` (selected vertices), ``record`` (the patch's ``view.PIECE`` row, ``None`` when
    the voxel under the pixel belongs to no patch), ``mode``, ``normal_deg``, ``color_tol``, ``connectivity``, ``within``."""

    __slots__ = ("selected", "count", "record", "piece_qv", "mode", "normal_deg", "color_tol", "connectivity", "within")


class SnapResult(_Result):
    """What ``snap()`` returns: ``labels_full``, ``colors``, ``miou`` and ``iou_per_object`` as a ``SessionResult`` holds them,
    ``labels_qv`` int32 [n_voxels] on the device, and the counts of ``a3d_vote_pieces``' summary: ``eligible_pieces``,
    ``uniform_pieces``, ``relabelled_pieces``, ``relabelled_voxels``, ``blocked_pieces``, ``below_share_pieces``;
    ``min_voxels`` and ``min_share`` as used."""

    __slots__ = ("labels_full", "colors", "miou", "iou_per_object", "labels_qv", "eligible_pieces", "uniform_pieces",
                 "relabelled_pieces", "relabelled_voxels", "blocked_pieces", "below_share_pieces", "min_voxels", "min_share")


def patch_thresholds(normal_deg, color_tol):
    """``(cos_min, tol2)`` of ``patches(normal_deg=, color_tol=)``, pure numpy: ``cos_min = float32(cos(radians(normal_deg)))``
    for an angle in 0 .. 180 degrees, ``tol2 = float32(color_tol) ** 2`` (an fp32 product) for a tolerance >= 0 whose square
    is finite; ``None`` for a test that is switched off (``None``).  ``ValueError`` for anything else."""
    cos_min = tol2 = None
    if normal_deg is not None:
        deg = np.float64(normal_deg)
        if not (np.isfinite(deg) and 0.0 <= deg <= 180.0):
            raise ValueError("normal_deg must be an angle in 0 .. 180 degrees, or None (no normal test)")
        cos_min = np.float32(np.cos(np.radians(deg)))
    if color_tol is not None:
        tol = np.float32(color_tol)
        with np.errstate(over="ignore"):
            tol2 = tol * tol
        if not (np.isfinite(tol2) and tol >= 0.0):
            raise ValueError("color_tol must be finite and >= 0, or None (no colour test)")
    return cos_min, tol2


WAND_MODES = ("chain", "seed", "both")


class SelectResult(_Result):
    """What ``select()`` returns: ``selected`` uint8 [n_full] on the device (1 = the vertex is selected), and on the host
    ``count`` (how many are), ``in_view`` (the vertices the camera sees at all: in front of it, inside the image, on the
    kept side of the section), ``through`` and ``slack`` as used."""

    __slots__ = ("selected", "count", "in_view", "through", "slack")


class GrowResult(_Result):
    """What ``grow()``, ``grow_at()`` and ``shrink()`` return.  Device tensors: ``selected`` uint8 [n_full] (1 = the vertex is
    selected; ``paint`` / ``erase`` take it as it is), ``dist_full`` int32 [n_full] and ``dist_qv`` int32 [n_voxels] (the path
    cost from the nearest seed in the units of ``cost``, -1: not reached), ``owner_qv`` int32 [n_voxels] (the voxel row of that
    seed; of seeds equally near the smallest row; -1: not reached).  Host: ``count`` (selected vertices), ``reached_voxels``,
    ``seeds`` (seed voxels), ``max_distance`` (the largest distance reached, in world units: cost units / 1024 voxels with
    ``radius``, hops x the voxel size with ``steps``), and ``limit``, ``cost``, ``connectivity``, ``within`` as used.  After
    ``shrink()`` the distances and owners are those FROM THE OUTSIDE of the selection and ``selected`` is the eroded set."""

    __slots__ = ("selected", "dist_full", "dist_qv", "owner_qv", "count", "reached_voxels", "seeds", "max_distance", "limit",
                 "cost", "connectivity", "within")


def grow_limit(radius, steps, voxel_size):
    """``(cost, limit)`` of ``grow(radius=, steps=)``, pure Python.  Exactly one of the two: ``radius`` >= 0 in world units
    walks with the metric costs ``view.GROW_METRIC_COST`` = round(1024 (1, sqrt 2, sqrt 3)) up to ``limit = floor(radius /
    voxel_size * 1024)``, computed in float64; ``steps``, an int >= 0, counts hops (costs 1, 1, 1, ``limit = steps``).
    ``ValueError`` for anything else, and for a limit of more than ``view.GROW_MAX_STEPS`` steps: ``pieces()`` answers what
    is connected at all."""
    if (radius is None) == (steps is None):
        raise ValueError("give a radius (world units) or steps (hops), one of them")
    if steps is not None:
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < 0:
            raise ValueError("steps must be an int >= 0")
        cost, limit = (1, 1, 1), int(steps)
    else:
        r = np.float64(radius)
        if not (np.isfinite(r) and r >= 0.0):
            raise ValueError("radius must be finite and >= 0")
        cost, q = V.GROW_METRIC_COST, np.floor(r / np.float64(voxel_size) * np.float64(1024.0))
        limit = int(min(q, np.float64(2.0 ** 40)))
    if limit // min(cost) > V.GROW_MAX_STEPS:
        raise ValueError(f"that is more than {V.GROW_MAX_STEPS} voxel steps: pieces() answers what is connected at all")
    return cost, limit


class NormalsResult(_Result):
    """What ``estimate_normals()`` returns.  Device tensors: ``normals_full`` fp32 [n_full, 3] (unit vectors; zero where the
    vertex's voxel has no valid normal), ``normals_qv`` fp32 [n_voxels, 3], ``variation_qv`` fp32 [n_voxels] (the surface
    variation, smallest eigenvalue over the sum: 0 on a plane, 1/3 for a blob), ``count_qv`` int32 [n_voxels] (the vertices of
    the voxel's 27-voxel neighbourhood).  Host: ``counted`` (vertices that took part), ``valid`` / ``invalid`` (voxels with /
    without a normal), ``err`` (``view.NORMALS_RANGE``: some coordinate is not finite) and ``viewpoint`` (float64 [3] the
    normals are turned towards, or ``None``: the canonical sign)."""

    __slots__ = ("normals_full", "normals_qv", "variation_qv", "count_qv", "counted", "valid", "invalid", "err", "viewpoint")


class OrientResult(_Result):
    """What ``orient_normals()`` and ``orient_at()`` return.  Device tensors: ``normals_full`` fp32 [n_full, 3] and ``normals_qv``
    fp32 [n_voxels, 3] (the input normals with the sign turned where ``flipped_qv`` is 1; every other byte as it was),
    ``flipped_qv`` uint8 [n_voxels], ``dist_qv`` int32 [n_voxels] (the cost of the path from the seed, 1 .. 1024 an edge; -1: not
    reached) and ``owner_qv`` int32 [n_voxels] (the voxel row of that seed).  Host, from ``a3d_orient_normals``' summary:
    ``admitted`` (voxels with a normal), ``seeds``, ``reached``, ``unreached``, ``flipped``, ``conflicts`` (edges whose two
    normals still disagree: where the regions of two seeds meet, or on a loop that cannot be oriented), ``max_dist``, ``err``;
    ``launched``: the relaxation sweeps issued in all; ``connectivity`` as used; ``result``: the ``NormalsResult`` that now
    holds these normals (what ``normal_at``, ``patches`` and ``planes`` take)."""

    __slots__ = ("normals_full", "normals_qv", "flipped_qv", "dist_qv", "owner_qv", "admitted", "seeds", "reached", "unreached",
                 "flipped", "conflicts", "max_dist", "err", "launched", "connectivity", "result")


PLANE_KINDS = ("floor", "ceiling", "wall", "horizontal", "other")


def _unit3(values, what):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0.0:
        raise ValueError(f"{what} must be three finite numbers, not all zero")
    return v / np.linalg.norm(v)


def plane_kinds(normals, offsets, up=(0.0, 0.0, 1.0), normal_deg=20.0):
    """The ``kind`` of every plane ``normal . p = offset`` (``normals`` [k, 3] unit vectors of either sign, ``offsets`` [k]),
    pure numpy in float64: with ``c = normal . up`` (``up`` normalised here), a plane is a ``"wall"`` when its normal lies
    within ``normal_deg`` of perpendicular to ``up`` (``|c| <= sin(normal_deg)``); it is LEVEL when its normal lies within
    ``normal_deg`` of ``up`` or of ``-up`` (``|c| >= cos(normal_deg)``), and its height along ``up`` is ``offset / c``.  Of the
    level planes the lowest is the ``"floor"``, the highest the ``"ceiling"`` (of equal heights the earlier plane), the rest are
    ``"horizontal"``; a single level plane is the ``"floor"``.  Everything else is ``"other"``.  ``normal_deg`` in 0 .. 45
    degrees (beyond, a plane could be both).  Returns a list of k strings."""
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    c0 = np.asarray(offsets, dtype=np.float64).reshape(-1)
    deg = np.float64(normal_deg)
    if len(c0) != len(n) or not (np.isfinite(deg) and 0.0 <= deg <= 45.0):
        raise ValueError("one offset per normal, and normal_deg in 0 .. 45 degrees")
    c = n @ _unit3(up, "up")
    kinds = ["other"] * len(n)
    level = np.flatnonzero(np.abs(c) >= np.cos(np.radians(deg)))
    for k in np.flatnonzero(np.abs(c) <= np.sin(np.radians(deg))):
        kinds[k] = "wall"
    if len(level):
        height = c0[level] / c[level]
        for k in level:
            kinds[k] = "horizontal"
        lowest, highest = level[int(np.argmin(height))], level[int(np.argmax(height))]
        if len(level) > 1 and highest != lowest:
            kinds[highest] = "ceiling"
        kinds[lowest] = "floor"
    return kinds


def upright_rotation(normal, up=(0.0, 0.0, 1.0)):
    """The float64 3 x 3 rotation about ``normal x up`` that takes the direction of ``normal`` (either sign: the one nearer to
    ``up``) to ``up`` -- Rodrigues' formula; the identity when they agree already."""
    u, n = _unit3(up, "up"), _unit3(normal, "normal")
    if n @ u < 0.0:
        n = -n
    axis, c = np.cross(n, u), float(n @ u)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


class PlanesResult(_Result):
    """What ``planes()`` returns.  Device tensors: ``plane_qv`` int32 [n_voxels] (the id of the voxel's plane, -1: none;
    ``grow(..., within=r.plane_qv)`` stays on one plane) and ``plane_full`` int32 [n_full] (the same lifted to the vertices).
    Host: ``records``, a numpy structured array (``view.PLANE``: normal with the canonical sign, offset -- ``normal . p =
    offset`` in scene coordinates --, inliers, score, round, bin, the integer sums, N, off, rms) in the order found;
    ``n_planes``; ``kinds``, one of ``PLANE_KINDS`` per plane (``plane_kinds``); ``floor`` and ``ceiling`` (plane ids or
    ``None``) and ``walls`` (a list of ids); ``rounds``, ``spent``, ``admitted`` and ``left_out`` (a dict: the rows left out
    per reason) from the call's summary; ``up`` (float64 [3], a unit vector) and ``normal_deg``, ``dist_tol``, ``min_voxels``,
    ``max_planes``, ``within`` as used."""

    __slots__ = ("plane_qv", "plane_full", "records", "n_planes", "kinds", "floor", "ceiling", "walls", "rounds", "spent",
                 "admitted", "left_out", "up", "normal_deg", "dist_tol", "min_voxels", "max_planes", "within")

    def _plane(self, k):
        if isinstance(k, bool) or k is None or int(k) != k or not 0 <= k < self.n_planes:
            raise ValueError(f"plane {k!r}: the result holds the planes 0 .. {self.n_planes - 1}")
        return int(k)

    def selection(self, k):
        """uint8 [n_full] on the device: 1 = the vertex lies on plane ``k`` (``paint``, ``erase``, ``grow`` and ``shrink`` take
        it as it is)."""
        return (self.plane_full == self._plane(k)).to(torch.uint8)

    def section(self, k, keep="above", margin=0.0, cull="none"):
        """The ``Section`` of one plane along plane ``k``.  ``keep="above"`` keeps the side ``up`` points to -- of a wall, whose
        normal is about perpendicular to ``up``, the side its recorded normal points to --, ``"below"`` the other.  ``margin``
        (world units, finite) moves the cut INTO the kept side, so that the plane's own voxels go with what is cut away:
        ``set_section(r.section(r.ceiling, "below", margin=0.05))`` cuts the ceiling off."""
        if keep not in ("above", "below"):
            raise ValueError('keep must be "above" or "below"')
        m = float(margin)
        if not np.isfinite(m):
            raise ValueError("margin must be finite")
        rec = self.records[self._plane(k)]
        n, c = rec["normal"].astype(np.float64), float(rec["offset"])
        if n @ self.up < 0.0 and self.kinds[int(k)] != "wall":
            n, c = -n, -c
        if keep == "below":
            n, c = -n, -c
        return Section([(n, c + m)], cull)

    def upright(self):
        """The float64 3 x 3 rotation that takes the floor's normal to ``up`` (``upright_rotation``): ``p @ R.T`` turns a tilted
        scan upright.  The identity when there is no floor."""
        return np.eye(3) if self.floor is None else upright_rotation(self.records["normal"][self.floor], self.up)


_MAX_CULLED = 4                                 # culled copies of a cloud kept at a time (one per eye and mode)


class TransferResult(_Result):
    """What ``nearest_vertices()``, ``transfer()`` and ``import_labels()`` return, one entry per QUERY point (for
    ``import_labels`` the queries are the scene's vertices).  Device tensors: ``nearest`` int32 [m] (the row of the nearest
    source point within ``max_distance``, -1 without one), ``distance2`` fp32 [m] (its squared fp32 distance, +inf without
    one), and where labels were carried ``labels`` int32 [m] (``fill`` without a match) and ``colors`` fp32 [m, 3] (the
    palette's); ``None`` otherwise.  Host: ``matched``, ``unmatched`` (finite points with nothing in reach), ``nonfinite``
    (points with a NaN or an infinity: also -1), ``source_left_out`` (source points that are not finite) and the
    ``max_distance`` of the call."""

    __slots__ = ("nearest", "distance2", "labels", "colors", "matched", "unmatched", "nonfinite", "source_left_out", "max_distance")


_MAX_POINT_INDICES = 4                          # indices over a scene's vertices kept at a time (one per cell size)


class CorrectedResult(_Result):
    """What ``corrected()`` returns: ``labels_full`` int32 [n_full] and ``colors`` fp32 [n_full, 3] on the device -- the model's
    labels with the manual layer laid over them -- ``miou`` and ``iou_per_object`` as a ``SessionResult`` holds them (``None``
    without ground truth), ``overridden`` (vertices the layer holds) and ``differing`` (those of them whose manual label is
    not the model's)."""

    __slots__ = ("labels_full", "colors", "miou", "iou_per_object", "overridden", "differing")


_RENDERED = object()                            # select(section=): "the section the view was rendered under"


def object_table(moments, origin, quantum, area_quantum=None, voxel_size=None):
    """What the records of ``a3d_measure_objects`` (``view.OBJECT_MOMENTS``, one per object id) say in world units -- float64
    from the exact integers, pure numpy.  ``origin``, ``quantum``: the fixed-point frame the call was given; ``area_quantum``
    (``None``: a cloud, no area) and ``voxel_size`` (``None``: no volume).  Returns a dict of arrays over the object ids:

    * ``vertices``, ``voxels`` int64;
    * ``centroid`` [K, 3] = origin + quantum * sum / vertices (NaN for an object without a vertex);
    * ``cov`` [K, 3, 3] = quantum^2 * (mom / vertices - mean mean^T), the population covariance of the quantised
      coordinates; the difference is taken in exact integers (vertices * mom - sum sum^T) and divided once, so nothing
      cancels in floating point (NaN without a vertex);
    * ``area`` [K] = area_thirds * area_quantum / 6: a face's area goes in thirds to the objects of its corners;
    * ``volume`` [K] = voxels * voxel_size^3 -- the volume of the OCCUPIED VOXELS (a scan's surface, one voxel thick), not of
      the solid the surface encloses."""
    m = np.asarray(moments)
    o, q = np.asarray(origin, dtype=np.float64).reshape(3), float(quantum)
    k = len(m)
    vertices, voxels = m["vertices"].astype(np.int64), m["voxels"].astype(np.int64)
    centroid, cov = np.full((k, 3), np.nan), np.full((k, 3, 3), np.nan)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for i in np.flatnonzero(vertices > 0):
        n, s = int(vertices[i]), [int(v) for v in m["sum"][i]]
        centroid[i] = o + q * (np.array(s, dtype=np.float64) / n)
        for (a, b), mom in zip(pairs, m["mom"][i]):
            cov[i, a, b] = cov[i, b, a] = q * q * ((n * int(mom) - s[a] * s[b]) / (n * n))      # Python integers: exact
    table = {"vertices": vertices, "voxels": voxels, "centroid": centroid, "cov": cov, "area": None, "volume": None}
    if area_quantum is not None:
        table["area"] = m["area_thirds"].astype(np.float64) * (float(area_quantum) / 6.0)
    if voxel_size is not None:
        table["volume"] = voxels.astype(np.float64) * float(voxel_size) ** 3
    return table


def principal_axes(cov, vertices=None):
    """The axes of an oriented box from a covariance ``cov`` [3, 3] (or [K, 3, 3], with ``vertices`` [K]): ``(axes, variances)``
    with ``axes`` [.., 3, 3], row j = axis j, and ``variances`` [.., 3] descending.  THE CONVENTION: ``numpy.linalg.eigh``,
    eigenvalues in descending order; axes 0 and 1 are each signed so that their component of largest magnitude is positive (a
    tie goes to the lowest index); axis 2 = axis 0 x axis 1, so the frame is right-handed.  An object with fewer than 3
    vertices, or a covariance that is zero or not finite, gets the identity axes (variances: the diagonal, 0 where not
    finite).  float64, pure numpy."""
    c = np.asarray(cov, dtype=np.float64)
    single = c.ndim == 2
    c = c.reshape(-1, 3, 3)
    count = np.full(len(c), 3) if vertices is None else np.asarray(vertices).reshape(-1)
    axes, variances = np.tile(np.eye(3), (len(c), 1, 1)), np.zeros((len(c), 3))
    for i in range(len(c)):
        if not np.isfinite(c[i]).all():
            continue
        variances[i] = np.diag(c[i])
        if count[i] < 3 or not c[i].any():
            continue
        w, v = np.linalg.eigh(c[i])
        a = v[:, ::-1].T.copy()                      # rows, largest eigenvalue first
        for j in (0, 1):
            if a[j, np.argmax(np.abs(a[j]))] < 0:
                a[j] = -a[j]
        a[2] = np.cross(a[0], a[1])
        axes[i], variances[i] = a, w[::-1]
    return (axes[0], variances[0]) if single else (axes, variances)


class MeasureResult(_Result):
    """What ``measure()`` returns: arrays over the object ids 0..K (host, float64 unless noted).  ``vertices``, ``voxels``
    int64; ``centroid`` [K + 1, 3]; ``lo``, ``hi`` fp32 [K + 1, 3], the exact axis-aligned box (+inf / -inf for an object without
    a vertex); ``cov`` [K + 1, 3, 3]; ``area`` (``None`` on a cloud) and ``volume`` (of the occupied voxels) [K + 1].  With
    ``oriented=True`` the oriented box: ``axes`` [K + 1, 3, 3] (``principal_axes``, rounded to fp32: what the second pass
    projected on), ``centre`` [K + 1, 3] and ``extents`` [K + 1, 3] (its full size along each axis); ``None`` otherwise.
    ``origin``, ``quantum``, ``bits``, ``area_quantum``: the fixed-point frame used; ``moments``: the records as they came."""

    __slots__ = ("vertices", "voxels", "centroid", "lo", "hi", "cov", "area", "volume", "axes", "centre", "extents", "origin",
                 "quantum", "bits", "area_quantum", "moments")

    def section(self, obj, margin=0.0, cull="none"):
        """The ``Section`` that isolates object ``obj`` in ``render`` / ``pick``: ``Section.box(lo - margin, hi + margin)``
        of its axis-aligned box.  With ``margin = 0`` the planes are the box's own fp32 values: every vertex of the object is
        kept.  ``ValueError`` for an object without a vertex."""
        obj = int(obj)
        if not 0 <= obj < len(self.vertices) or self.vertices[obj] == 0:
            raise ValueError(f"object {obj} has no vertex")
        if not (np.isfinite(margin) and margin >= 0):
            raise ValueError("margin must be finite and >= 0")
        return Section.box(self.lo[obj].astype(np.float64) - float(margin), self.hi[obj].astype(np.float64) + float(margin), cull)


class GuideResult(_Result):
    """What ``guide()`` returns.  Device tensors: ``labels_qv`` int32 [n_voxels] (what ``infer()`` computed), ``runner_qv``
    int32 (the second choice), ``margin_qv`` fp32 (winner's logit minus runner-up's; +inf on a clicked voxel), ``margin_full``
    fp32 [n_full], ``colors`` fp32 [n_full, 3] (the confidence view, for ``render(colors=)``).  Host: ``object_voxels`` and
    ``object_contested`` int64 [1 + K] (voxels and contested voxels per object id), ``least_confident`` = ``(row, margin)``
    or ``None``, ``n_contested``, ``suggestions`` (``rank_suggestions``), ``threshold`` and ``full_margin`` as used.  With
    ``regions="connected"``: ``n_spots`` (connected contested spots) and ``n_spots_searched`` (those among them, at most
    ``MAX_SPOTS``, whose deepest voxel was searched); ``None`` otherwise."""

    __slots__ = ("labels_qv", "runner_qv", "margin_qv", "margin_full", "colors", "object_voxels", "object_contested",
                 "least_confident", "n_contested", "suggestions", "threshold", "full_margin", "n_spots", "n_spots_searched")


class LookalikeResult(_Result):
    """What ``lookalikes()`` returns.  Device tensors: ``match_qv`` int32 [n_voxels] (the object a voxel looks like, -1: none),
    ``score_qv`` fp32 [n_voxels] and ``score_full`` fp32 [n_full] (the cosine to the most similar prototype, passing or not; 0
    where a voxel was no candidate), ``colors`` fp32 [n_full, 3] (the similarity view, for ``render(colors=)``).  Host:
    ``candidates`` (``rank_candidates``: dicts ``{point, row, object, voxels, root, depth}``, best first), ``n_regions``
    (matched regions of at least ``min_voxels``), ``n_regions_searched`` (those among them, at most ``MAX_SPOTS``, whose
    deepest voxel was searched), ``prototypes`` (``{object: example voxels}``), ``examples_left_out``, ``rows_nonfinite``,
    and ``cos_min``, ``min_voxels``, ``within``, ``connectivity`` as used."""

    __slots__ = ("match_qv", "score_qv", "score_full", "colors", "candidates", "n_regions", "n_regions_searched", "prototypes",
                 "examples_left_out", "rows_nonfinite", "cos_min", "min_voxels", "within", "connectivity")


class SessionResult(_Result):
    """What one ``infer()`` returns.  ``labels_full`` int32 [n_full] and ``colors`` fp32 [n_full, 3] stay on the device;
    ``miou`` is a Python float (the float32 mean IoU) or ``None`` without ground truth; ``record``, ``mask_path`` and
    ``click_path`` are set when the scene has an ``out_dir``."""

    __slots__ = ("labels_full", "colors", "miou", "iou_per_object", "num_obj", "avg_clicks", "record", "mask_path",
                 "click_path")


def _f3(values, what):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{what} must be three finite numbers")
    return a


def ray_from_pixel(u, v, intrinsic, extrinsic):
    """The pointer ray of pixel ``(u, v)`` (column, row), sampled at its centre ``(u + 0.5, v + 0.5)``, for callers that
    have a pixel and a camera rather than a ray -- the inverse of the GUI's unprojection (gui.py:268-270).  ``intrinsic``:
    3 x 3 pinhole matrix (fx, fy, cx, cy); ``extrinsic``: 4 x 4 world-to-camera, the camera looking along +z.  Returns
    ``(origin, direction)`` in world space, float64: the camera centre and a unit vector.  Pure numpy."""
    k = np.asarray(intrinsic, dtype=np.float64)
    e = np.asarray(extrinsic, dtype=np.float64)
    if k.shape != (3, 3) or e.shape != (4, 4):
        raise ValueError("intrinsic must be 3 x 3 and extrinsic 4 x 4 (world to camera)")
    rot, trans = e[:3, :3], e[:3, 3]
    d_cam = np.array([(float(u) + 0.5 - k[0, 2]) / k[0, 0], (float(v) + 0.5 - k[1, 2]) / k[1, 1], 1.0])
    d = np.linalg.solve(rot, d_cam)                 # camera -> world (no assumption that the rotation is exactly orthogonal)
    return -np.linalg.solve(rot, trans), d / np.linalg.norm(d)


def camera_from_matrices(intrinsic, extrinsic, width, height):
    """The ``lib.Camera`` (``a3d_camera``) of a pinhole camera in the conventions of ``ray_from_pixel``: ``intrinsic`` 3 x 3
    (fx, fy, cx, cy), ``extrinsic`` 4 x 4 world-to-camera looking along +z, pixels sampled at their centres.  ``o`` = the
    camera centre, ``d00`` = the unnormalised world direction of pixel (0, 0)'s centre (its camera-space z is 1), ``du`` /
    ``dv`` = its change per column / row.  Computed in float64, rounded to the fp32 fields once.  Pure numpy."""
    k = np.asarray(intrinsic, dtype=np.float64)
    e = np.asarray(extrinsic, dtype=np.float64)
    if k.shape != (3, 3) or e.shape != (4, 4):
        raise ValueError("intrinsic must be 3 x 3 and extrinsic 4 x 4 (world to camera)")
    if int(width) != width or int(height) != height or not (1 <= width <= L.A3D_RENDER_MAX_SIZE
                                                             and 1 <= height <= L.A3D_RENDER_MAX_SIZE):
        raise ValueError(f"width and height must be integers in 1 .. {L.A3D_RENDER_MAX_SIZE}")
    if not (np.isfinite(k).all() and np.isfinite(e).all()) or k[0, 0] == 0 or k[1, 1] == 0:
        raise ValueError("intrinsic and extrinsic must be finite, fx and fy not zero")
    rot, trans = e[:3, :3], e[:3, 3]
    cols = np.array([[1.0 / k[0, 0], 0.0, (0.5 - k[0, 2]) / k[0, 0]],
                     [0.0, 1.0 / k[1, 1], (0.5 - k[1, 2]) / k[1, 1]],
                     [0.0, 0.0, 1.0]])                 # camera-space du, dv, d00 as columns
    world = np.linalg.solve(rot, cols)
    cam = L.Camera()
    cam.o[:] = [float(x) for x in (-np.linalg.solve(rot, trans)).astype(np.float32)]
    cam.du[:] = [float(x) for x in world[:, 0].astype(np.float32)]
    cam.dv[:] = [float(x) for x in world[:, 1].astype(np.float32)]
    cam.d00[:] = [float(x) for x in world[:, 2].astype(np.float32)]
    cam.width, cam.height = int(width), int(height)
    return cam


def vertex_corner_lists(faces, n):
    """The incidence lists ``a3d_vertex_normals`` walks, in CSR form: ``(offsets int64 [n + 1], corners int32 [3 m])``.
    Vertex ``v`` owns ``corners[offsets[v]:offsets[v + 1]]``, each entry ``3 * face + corner``, ascending -- that is, by
    face and then by corner; a vertex listed twice in one face appears twice, an isolated vertex has an empty range.
    Corners whose index lies outside ``[0, n)`` belong to no vertex: they sit behind ``offsets[n]``.  One stable sort of
    the ``3 m`` vertex indices.  Pure numpy."""
    f = np.asarray(faces).reshape(-1).astype(np.int64)
    n = int(n)
    if 3 * (f.size // 3) != f.size or f.size >= 1 << 31:
        raise ValueError("faces must be [m, 3] with 3 m < 2^31")
    key = np.where((f >= 0) & (f < n), f, n)
    corners = np.argsort(key, kind="stable").astype(np.int32)
    offsets = np.searchsorted(key[corners], np.arange(n + 1), side="left").astype(np.int64)
    return offsets, corners


def framing_view(coords, width, height, fov_deg=35.0):
    """``(intrinsic 3 x 3, extrinsic 4 x 4)`` of a pinhole camera that frames the points ``coords`` [n, 3], in the
    conventions of ``camera_from_matrices``; float64, pure numpy.  The camera looks at the centre of the bounding box from
    ``centre + (0, -dist, 0)`` with +z up: rotation rows right (1, 0, 0), down (0, 0, -1), forward (0, 1, 0).
    ``fov_deg`` is the vertical field of view: ``fx = fy = (height / 2) / tan(fov / 2)``, ``cx = width / 2``,
    ``cy = height / 2``.  ``dist = R / sin(min(fov_v, fov_h) / 2)`` with ``R`` the largest distance of a point from the
    centre: the bounding sphere fits the narrower of the two fields of view, so every point has camera-space z > 0 and
    projects inside the image.  Rows with a non-finite coordinate are ignored; a single point is framed from 1 away."""
    p = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    if int(width) != width or int(height) != height or width < 1 or height < 1:
        raise ValueError("width and height must be positive integers")
    if not (np.isfinite(fov_deg) and 0.0 < fov_deg < 180.0):
        raise ValueError("fov_deg must lie in (0, 180)")
    if len(p) == 0:
        raise ValueError("no finite point to frame")
    centre = 0.5 * (p.min(0) + p.max(0))
    radius = float(np.sqrt(((p - centre) ** 2).sum(1).max()))
    fov_v = np.radians(float(fov_deg))
    f = 0.5 * height / np.tan(0.5 * fov_v)
    fov_h = 2.0 * np.arctan(0.5 * width / f)
    dist = radius / np.sin(0.5 * min(fov_v, fov_h)) if radius > 0 else 1.0
    rot = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    ext = np.eye(4)
    ext[:3, :3] = rot
    ext[:3, 3] = -rot @ (centre + np.array([0.0, -dist, 0.0]))
    return np.array([[f, 0.0, 0.5 * width], [0.0, f, 0.5 * height], [0.0, 0.0, 1.0]]), ext


_CULL = {"none": L.A3D_CULL_NONE, "back": L.A3D_CULL_BACK, "front": L.A3D_CULL_FRONT}


class Section:
    """What of a scene the picks and the view leave out (include/agile3d_hip.h, ``a3d_section``): up to 8 section planes and,
    on a mesh, the culling of faces by the side they turn to the ray.  Host data, immutable, pure numpy.

    ``planes``: a sequence of ``(normal, offset)`` -- the kept side is ``normal . p >= offset`` -- or ``(normal,
    point_on_plane)``, the kept side the one the normal points to.  A normal is normalised in float64 (an offset divided by
    its length, a point projected on the unit normal) and each value rounded to fp32 once; a value that is not finite or a
    zero normal raises ``ValueError``.  ``cull``: ``"none"``, ``"back"`` (drop the faces seen from behind: the near walls
    of a room seen from outside, the "dollhouse" view) or ``"front"``.

    ``normals`` fp32 [k, 3], ``offsets`` fp32 [k], ``cull``.  On a mesh the planes cut the RAY: a crossing counts when its
    ``t`` lies in the ray's interval.  On a cloud they select vertices: ``keeps``."""

    __slots__ = ("normals", "offsets", "cull")

    def __init__(self, planes=(), cull="none"):
        if cull not in _CULL:
            raise ValueError(f"cull must be one of {sorted(_CULL)}, not {cull!r}")
        planes = list(planes)
        if len(planes) > L.A3D_SECTION_MAX_PLANES:
            raise ValueError(f"at most {L.A3D_SECTION_MAX_PLANES} planes, not {len(planes)}")
        normals, offsets = np.zeros((len(planes), 3), np.float32), np.zeros(len(planes), np.float32)
        for k, plane in enumerate(planes):
            try:
                normal, where = plane
                n = np.asarray(normal, dtype=np.float64).reshape(-1)
                w = np.asarray(where, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError(f"plane {k} must be (normal, offset) or (normal, point_on_plane)") from None
            if n.shape != (3,) or w.shape not in ((1,), (3,)) or not (np.isfinite(n).all() and np.isfinite(w).all()):
                raise ValueError(f"plane {k}: a normal of three and an offset or a point of three, all finite")
            length = float(np.linalg.norm(n))
            if not length > 0.0:
                raise ValueError(f"plane {k}: the normal is zero")
            unit = n / length
            c = float(w[0]) / length if w.shape == (1,) else float(unit @ w)
            with np.errstate(over="ignore"):
                normals[k], offsets[k] = unit.astype(np.float32), np.float32(c)
            if not (np.isfinite(normals[k]).all() and np.isfinite(offsets[k])):
                raise ValueError(f"plane {k}: not finite in fp32")
        normals.setflags(write=False)
        offsets.setflags(write=False)
        object.__setattr__(self, "normals", normals)
        object.__setattr__(self, "offsets", offsets)
        object.__setattr__(self, "cull", cull)

    def __setattr__(self, name, value):
        raise AttributeError("a Section is immutable (with_cull, or a new one)")

    def __repr__(self):
        planes = ", ".join(f"({n.tolist()}, {float(c)})" for n, c in zip(self.normals, self.offsets))
        return f"Section(planes=[{planes}], cull={self.cull!r})"

    @property
    def n_planes(self):
        return len(self.offsets)

    @classmethod
    def box(cls, lo, hi, cull="none"):
        """Six planes that keep the axis-aligned box ``lo <= p <= hi``."""
        lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("lo and hi must be three numbers each")
        eye = np.eye(3)
        return cls([(eye[k], float(lo[k])) for k in range(3)] + [(-eye[k], -float(hi[k])) for k in range(3)], cull)

    @classmethod
    def below(cls, z, cull="none"):
        """One plane that keeps ``z' <= z``: it cuts a ceiling off."""
        return cls([((0.0, 0.0, -1.0), -float(z))], cull)

    def with_cull(self, cull):
        """The same planes, bit for bit, with another culling mode (the stored fp32 values are shared, not normalised again:
        a view under one and a pick under the other cut at the same planes)."""
        if cull not in _CULL:
            raise ValueError(f"cull must be one of {sorted(_CULL)}, not {cull!r}")
        other = object.__new__(Section)
        object.__setattr__(other, "normals", self.normals)
        object.__setattr__(other, "offsets", self.offsets)
        object.__setattr__(other, "cull", cull)
        return other

    def keeps(self, points):
        """bool [k]: which of ``points`` [k, 3] lie on the kept side of every plane -- the vertex rule of the header in
        fp32, one operation at a time: ``(nx*x + ny*y) + nz*z >= c``; a NaN fails.  Culling plays no part."""
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        keep = np.ones(len(p), bool)
        with np.errstate(all="ignore"):
            for n, c in zip(self.normals, self.offsets):
                keep &= (n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2] >= c
        return keep

    def struct(self):
        """The ``lib.Section`` (``a3d_section``) the library takes."""
        s = L.Section()
        s.n_planes, s.cull = self.n_planes, _CULL[self.cull]
        for k in range(self.n_planes):
            s.planes[k][:] = [float(x) for x in self.normals[k]] + [float(self.offsets[k])]
        return s


def visible_clicks(section, points):
    """int64 [k']: the indices of the click ``points`` [k, 3] whose marker a view under ``section`` shows -- all of them
    without a section (``None``), else those that ``section.keeps``.  A marker of a click inside the cut-away part would
    float over whatever lies behind it.  Pure numpy."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    return np.arange(len(p)) if section is None else np.flatnonzero(section.keeps(p))


class RenderResult(_Result):
    """What ``render()`` returns.  Device tensors: ``ids`` int32 [h, w] (face of a mesh, vertex of a cloud, -1 = nothing),
    ``t`` fp32 [h, w] (+inf = nothing), ``rgb`` uint8 [h, w, 3], on a mesh ``u`` and ``v`` fp32 [h, w] (else ``None``).
    ``camera``: the ``lib.Camera`` rendered.  ``mesh``: whether ids are faces.  ``lit``: whether ``rgb`` is shaded.
    ``pairs`` and ``n_everywhere``: the (tile, primitive) pairs of the call and the primitives every pixel tested.
    ``section``: the ``Section`` the view was rendered under, or ``None``."""

    __slots__ = ("ids", "t", "rgb", "u", "v", "camera", "mesh", "lit", "pairs", "n_everywhere", "section")


class InteractiveSession:
    """The headless counterpart of ``UserInteractiveSegmentationModel`` plus the GUI's click state.

    ``model``: an ``eval()`` model on the GPU.  ``voxel_size``: the quantisation size (default ``model.voxel_size``).
    ``cube_size``: half edge of the cube a click paints.  ``palette``: [K + 1, 3] colours in [0, 1] per object id (default
    ``default_palette()``; ids above the table wrap over entries 1..K, which departs from the reference -- its table
    raises ``KeyError`` above 10 objects).  ``clock``: a callable returning a ``datetime`` for the record line (default
    ``datetime.now``)."""

    def __init__(self, model, voxel_size=None, cube_size=0.1, palette=None, clock=None,
                 background_click_color=BACKGROUND_CLICK_COLOR):
        self.lib = L.load()
        if model.training:
            raise ValueError("InteractiveSession needs an eval() model")
        self.model = model
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("InteractiveSession runs on the GPU only (model.to('cuda')); there is no CPU path")
        self.voxel_size = float(model.voxel_size if voxel_size is None else voxel_size)
        self.cube_size = float(cube_size)
        pal = default_palette() if palette is None else np.asarray(palette, dtype=np.float32)
        if pal.ndim != 2 or pal.shape[1] != 3 or not 2 <= pal.shape[0] <= 256:
            raise ValueError("palette must be [K + 1, 3] with 1 <= K <= 255")
        self.palette = np.ascontiguousarray(pal)
        self._palette_dev = torch.from_numpy(self.palette).to(self.device)
        self.background_click_color = tuple(float(c) for c in background_click_color)
        self.clock = clock or datetime.now
        self._ws = V.session_workspace(self.device)
        self._small = torch.empty(64, dtype=torch.int32, device=self.device)     # pick result / nearest rows
        self._counts = torch.empty(3 * _N_IDS + 2, dtype=torch.int64, device=self.device)   # IoU counts + its flag + paint's flag
        self._counts_host = torch.empty(3 * _N_IDS + 2, dtype=torch.int64).pin_memory()
        # the click cubes (centre, colour): a pinned host table and its device copy; click() appends one row to both
        self._cubes_host = torch.zeros((L.A3D_MAX_CLICKS, 6), dtype=torch.float32).pin_memory()
        self._cubes = self._cubes_host.numpy()
        self._cubes_dev = torch.zeros((L.A3D_MAX_CLICKS, 6), dtype=torch.float32, device=self.device)
        self._mask_host = None                      # pinned staging of a scene's full-resolution labels (scenes with an out_dir)
        self._edit_err = torch.zeros(1, dtype=torch.int32, device=self.device)   # a3d_session_edit's flag
        self._guide_sum = torch.empty(V.GUIDE_SUMMARY.itemsize, dtype=torch.uint8, device=self.device)   # a3d_session_guide's summary
        self._guide_sum_host = torch.empty(V.GUIDE_SUMMARY.itemsize, dtype=torch.uint8).pin_memory()
        self._manual_err = torch.zeros(1, dtype=torch.int32, device=self.device)   # the flag of the manual layer's own a3d_session_edit
        self._region_sum = torch.empty(V.OVERLAY_SUMMARY.itemsize, dtype=torch.uint8, device=self.device)   # select's / overlay's summary
        self._transfer_sum = torch.empty(V.TRANSFER_SUMMARY.itemsize, dtype=torch.uint8, device=self.device)   # a3d_point_index_nearest's
        self._point_indices = {}
        self._drop_scene()

    # ------------------------------------------------------------------ scene
    def _drop_scene(self):
        self.scene_name = None
        self.out_dir = None
        self.coords_full = self.colors_full = self.labels_full_ori = self.labels_qv_ori = None
        self.inverse_map = self.raw_coords_qv = None
        self.faces = None                           # int32 [m, 3] on the device: a triangle-mesh scene (pick meets its surface)
        self._corner_lists = None                   # (offsets int64 [n + 1], corners int32 [3 m]) on the device: a mesh's incidence lists
        self.normals = None                         # fp32 [n, 3] on the device: a mesh's vertex normals, computed by the first lit
        #                                             render; a cloud's estimated ones, there after estimate_normals() only
        self._normals_last = None                   # a cloud's NormalsResult (normal_at's default)
        self._culled = {}                           # (eye bytes, mode) -> a cloud's culled coordinates; dropped with the normals
        self._coords_host = None
        self._coords_qv_host = None                 # host copy of raw_coords_qv: the points of guide()'s suggestions
        self._vertex_ids = None                     # int32 [n] 0..n-1 on the device, built by the first confidence_at()
        self._backbone = None
        self._mask_host = None
        self._render_ws = None                      # scratch of render(): kept per scene, grown when a view needs more pairs
        self._unique_map = None                     # int64 [n_voxels]: the vertex each voxel was made from (measure(labels=))
        self._measure_frame = None                  # (origin, quantum, bits) of measure(): once per scene, on first use
        self._grow_ws = None                        # scratch of grow(): once per scene, on first use
        self._colors_qv = None                      # fp32 [n_voxels, 3]: the colours the backbone was fed (patches(color_tol=))
        for index in self._point_indices.values():  # cell size (fp32) -> view.PointIndex over coords_full (nearest_vertices, transfer)
            index.close()
        self._point_indices = {}
        self.section = None                         # the Section pick, click_ray and render apply by default (set_section)
        self._reset_clicks()

    def _reset_clicks(self):
        self._colors_last = None                    # colours of the last infer / preview: what render() shows by default
        self._labels_last = None                    # its full-resolution labels: what label_image() shows by default
        self._guide_logits = None                   # (logits, click_idx) of the last infer(): what guide() describes; dropped by
        self._guide_last = None                     # whatever changes the clicks or the scene.  The last guide()'s result.
        self._clicks = []                           # THE state: the ordered click list (entry i = time index i)
        self._redo = []                             # (click list before an undo, the table that renumbers the labels back)
        self._manual = None                         # the manual layer (on uint8 [n], obj int32 [n]) on the device; None = empty
        self.click_idx = {"0": []}
        self.click_time_idx = {"0": []}
        self.click_positions = {"0": []}
        self.num_clicks = 0
        self.new_labels = None if self.labels_full_ori is None else torch.zeros_like(self.labels_full_ori)
        self._labels_qv = None if self.raw_coords_qv is None else torch.zeros(self.raw_coords_qv.shape[0], dtype=torch.int32,
                                                                               device=self.device)

    def load_scene(self, coords_full, colors_full, labels_full=None, name="scene", out_dir=None, faces=None):
        """Voxelise on the GPU, run the backbone once and keep what the clicks need
        (interactive_segmentation_user.py:161-196).  ``coords_full`` [n, 3] float32 / float64 (quantised in its own
        precision, like ``ME.utils.sparse_quantize``), ``colors_full`` [n, 3] in [0, 1], ``labels_full`` [n] instance ids
        or ``None``.  With ``out_dir`` every ``infer()`` appends to ``out_dir/iou_record.csv`` and writes
        ``out_dir/masks/mask_*.npy`` and ``out_dir/clicks/click_*.npy``.  ``faces`` [m, 3] integer indices into
        ``coords_full`` make the scene a triangle mesh: ``pick`` then meets its surface (``ses.faces``, int32 on the
        device; indices outside ``[0, n)`` raise ``ValueError``), and the vertices' incidence lists for the normals of a
        lit ``render`` are built here, on the host (``vertex_corner_lists``).  Everything of a previous scene is dropped,
        its section (``set_section``) included."""
        self._drop_scene()
        dev = self.device
        xyz = torch.as_tensor(np.asarray(coords_full) if not torch.is_tensor(coords_full) else coords_full)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
            raise ValueError("coords_full must be [n, 3] with n > 0")
        if xyz.dtype not in (torch.float32, torch.float64):
            xyz = xyz.to(torch.float64)
        n = xyz.shape[0]
        col = torch.as_tensor(np.asarray(colors_full) if not torch.is_tensor(colors_full) else colors_full)
        if tuple(col.shape) != (n, 3):
            raise ValueError("colors_full must be [n, 3]")
        faces_dev = corner_lists = None
        if faces is not None:
            fa = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces)
            if fa.ndim != 2 or fa.shape[1] != 3 or fa.dtype.kind not in "iu":
                raise ValueError("faces must be [m, 3] integer indices into coords_full")
            if fa.size and (int(fa.min()) < 0 or int(fa.max()) >= n):     # checked once, here: the kernel only skips such faces
                raise ValueError(f"faces: vertex indices outside [0, {n})")
            faces_dev = torch.from_numpy(np.ascontiguousarray(fa, dtype=np.int32)).to(dev)
            corner_lists = tuple(torch.from_numpy(a).to(dev) for a in vertex_corner_lists(fa, n))   # once per scene, on the host
        xyz = xyz.to(dev).contiguous()
        col32 = col.to(dev).to(torch.float32).contiguous()
        coords_qv, unique_map, inverse_map = sparse_quantize(xyz, quantization_size=self.voxel_size, return_index=True,
                                                             return_inverse=True)
        self.coords_full = xyz.to(torch.float32).contiguous()          # what find_nearest and the cubes see (gui.py:559)
        self._coords_host = self.coords_full.cpu().numpy()
        self.colors_full = col32
        self.inverse_map = inverse_map.contiguous()
        self._unique_map = unique_map
        self.raw_coords_qv = xyz[unique_map].to(torch.float32).contiguous()
        self._coords_qv_host = self.raw_coords_qv.cpu().numpy()
        if labels_full is not None:
            lab = torch.as_tensor(np.asarray(labels_full) if not torch.is_tensor(labels_full) else labels_full).reshape(-1)
            if lab.shape[0] != n:
                raise ValueError("labels_full must be [n]")
            self.labels_full_ori = lab.to(dev).to(torch.int32).contiguous()
            self.labels_qv_ori = self.labels_full_ori[unique_map]
        bc = torch.cat([torch.zeros((coords_qv.shape[0], 1), dtype=torch.int32, device=dev), coords_qv.to(torch.int32)], 1)
        data = SparseTensor(coordinates=bc, features=col32[unique_map], device=dev)
        self._backbone = self.model.forward_backbone(data, raw_coordinates=self.raw_coords_qv)
        self.faces = faces_dev
        self._corner_lists = corner_lists
        self.scene_name = str(name)
        self.out_dir = out_dir
        if out_dir is not None:
            self._mask_host = torch.empty(n, dtype=torch.int32).pin_memory()
            os.makedirs(os.path.join(out_dir, MASK_DIR), exist_ok=True)
            os.makedirs(os.path.join(out_dir, CLICK_DIR), exist_ok=True)
        self._reset_clicks()
        return self

    def load_scene_dir(self, path, out_dir=None):
        """A scene folder in the ``InteractiveDataLoader`` layout (interactive_tool/dataloader.py): ``scan.ply`` (binary;
        a point cloud or a triangle mesh with x, y, z and red, green, blue), optionally ``label.ply`` with a ``label``
        property.  The scene's name is the folder's without its ``scene_`` prefix."""
        scan = os.path.join(path, "scan.ply")
        faces = None
        if ply.is_triangular_mesh(scan):
            v, faces = ply.read_ply(scan, triangular_mesh=True)
        else:
            v = ply.read_ply(scan)
        names = v.dtype.names
        if not all(k in names for k in ("x", "y", "z", "red", "green", "blue")):
            raise ValueError(f"{scan}: vertex properties x, y, z, red, green, blue expected, found {names}")
        xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64)
        rgb = np.stack([v["red"], v["green"], v["blue"]], 1)
        rgb = rgb.astype(np.float64) / 255.0 if rgb.dtype.kind in "ui" else rgb.astype(np.float64)
        labels = None
        lab_file = os.path.join(path, "label.ply")
        if os.path.exists(lab_file):
            lv = ply.read_ply(lab_file, triangular_mesh=True)[0] if ply.is_triangular_mesh(lab_file) else ply.read_ply(lab_file)
            labels = lv["label"].astype(np.int32)
        base = os.path.basename(os.path.normpath(path))
        name = base[len("scene_"):] if base.startswith("scene_") else base
        return self.load_scene(xyz, rgb, labels, name=name, out_dir=out_dir, faces=faces)

    def reset(self):
        """A new annotation of the same scene: clicks, relabelled ground truth and labels start over; the backbone output
        (and with it the scene's first-layer cache of ``forward_mask``) stays, and so does the section (``set_section``): it
        belongs to the view, not to the annotation."""
        self._need_scene()
        self._reset_clicks()

    def _need_scene(self):
        if self._backbone is None:
            raise RuntimeError("no scene loaded (load_scene / load_scene_dir)")

    # ------------------------------------------------------------------ the section
    def set_section(self, section):
        """Makes ``section`` (a ``Section``, or ``None`` for none) what ``pick``, ``click_ray`` and ``render`` apply when
        they are given no other: section planes to look into the scan, back-face culling to look through the walls that
        face away.  A property of the view: ``reset`` and edits of the click list keep it, ``load_scene`` drops it."""
        self._need_scene()
        if section is not None and not isinstance(section, Section):
            raise TypeError("set_section takes a Section or None")
        self.section = section
        return self

    def _section_of(self, section, mesh):
        """(the ``Section`` a call applies -- its own, else the session's -- or ``None`` when that leaves everything in; the
        ``lib.Section`` of it)."""
        sec = self.section if section is None else section
        if sec is not None and not isinstance(sec, Section):
            raise TypeError("section must be a Section or None")
        if sec is None or (sec.n_planes == 0 and sec.cull == "none"):
            return None, None
        if not mesh and sec.cull != "none" and not self._cloud_culls():
            raise ValueError(f"a section with cull={sec.cull!r} on a point cloud: only a mesh has faces to cull")
        return sec, sec.struct()

    def _cloud_culls(self):
        """Whether the scene is a cloud whose normals have been estimated: only then a cloud has sides to cull."""
        return self.faces is None and self.normals is not None

    def _cloud_under(self, sec, cut, eye):
        """``(coordinates, lib.Section or None)`` a point-cloud call runs on under ``sec`` (with its ``lib.Section`` ``cut``) for
        an ``eye`` (fp32 [3]).  Without culling: the scene's own coordinates and ``cut``, today's call.  With it: the culled copy
        for that eye and mode (``a3d_cull_points``; the culled vertices have NaN coordinates, which no pick, render or
        selection sees) and the section's planes alone -- ``None`` when it has none: the call without a section."""
        if sec is None or sec.cull == "none":
            return self.coords_full, cut
        key = (np.ascontiguousarray(eye, np.float32).tobytes(), sec.cull)
        xyz = self._culled.pop(key, None)
        if xyz is None:
            while len(self._culled) >= _MAX_CULLED:
                self._culled.pop(next(iter(self._culled)))              # (the one used longest ago)
            xyz = V.cull_points(self.coords_full, self.normals, eye, sec.cull, hidden=False, count=False)[0]
        self._culled[key] = xyz                                         # (most recently used: last)
        return xyz, sec.with_cull("none").struct() if sec.n_planes else None

    # ------------------------------------------------------------------ pick and click
    def pick(self, origin, direction, radius=None, surface=None, section=None):
        """The point a pointer ray meets, ``[x, y, z]``, or ``None`` ("clicked on nothing").  Both rules are this library's.
        A point cloud (``a3d_pick_ray``): among the vertices in front of ``origin`` within ``radius`` (default
        ``voxel_size``) of the ray, the first along it; ties go to the one closer to the ray, then to the lower index.  A
        triangle mesh (``a3d_pick_mesh``): the point where the ray first crosses a face -- what the GUI's unprojection of
        the rendered depth yields and what ``click`` takes.  ``surface=None`` uses the surface rule when the scene has
        faces, ``False`` forces the vertex rule, ``True`` without faces raises ``ValueError``.  ``section``: a ``Section``
        to pick under (``a3d_pick_mesh_section`` / ``a3d_pick_ray_section``; default: the session's, ``set_section``; an empty
        ``Section()`` picks without one); culling under the vertex rule raises ``ValueError`` -- except on a cloud after
        ``estimate_normals()``: the pick then runs on the copy of the cloud culled for ``origin`` (``a3d_cull_points``)."""
        self._need_scene()
        o = _f3(origin, "origin")
        d64 = np.asarray(direction, dtype=np.float64).reshape(-1)
        if d64.shape != (3,) or not np.isfinite(d64).all() or not np.linalg.norm(d64) > 0:
            raise ValueError("direction must be three finite numbers, not all zero")
        d = np.ascontiguousarray((d64 / np.linalg.norm(d64)).astype(np.float32))
        if surface is None:
            surface = self.faces is not None
        if surface:
            if self.faces is None:
                raise ValueError("pick(surface=True): the scene has no faces (load_scene(..., faces=) or a mesh scan.ply)")
            sec, cut = self._section_of(section, True)
            if sec is None:
                out = V.pick_mesh(self.coords_full, self.faces, o, d, out=self._small[:8], workspace=self._ws)
            else:
                out = V.pick_mesh_section(self.coords_full, self.faces, o, d, cut, out=self._small[:8], workspace=self._ws)
            hit = V.read_pick_mesh(out.cpu().numpy())[0]
            return None if hit["face"] < 0 else [float(hit[k]) for k in "xyz"]
        r = self.voxel_size if radius is None else float(radius)
        sec, cut = self._section_of(section, False)
        xyz, cut = self._cloud_under(sec, cut, o)       # (the scene's own coordinates unless a cloud is culled: the eye is the ray's origin)
        if cut is None:
            out = V.pick_ray(xyz, o, d, r, out=self._small[:4], workspace=self._ws)
        else:
            out = V.pick_ray_section(xyz, o, d, r, cut, out=self._small[:4], workspace=self._ws)
        index, xyz = V.read_pick(out.cpu().numpy())
        return None if index < 0 else [float(v) for v in xyz]

    # ------------------------------------------------------------------ the view
    def default_view(self, width, height, fov_deg=35.0):
        """``(intrinsic, extrinsic)`` of a camera that frames the loaded scene -- ``render(*ses.default_view(w, h), w, h)``
        shows all of it: ``framing_view`` on the host copy of the coordinates.  The counterpart of the GUI's camera setup
        (gui.py:561-565), from which it departs: the GUI hard-codes the eye at (0, -15, 0) for data at the origin; here
        the eye is ``centre + (0, -dist, 0)`` with ``dist`` from the scene's bounding sphere, wherever the scene lies."""
        self._need_scene()
        return framing_view(self._coords_host, width, height, fov_deg)

    def _vertex_normals(self):
        """``ses.normals`` of a mesh scene: ``a3d_vertex_normals`` once per scene, on first use."""
        if self.normals is None:
            self.normals = V.vertex_normals(self.coords_full, self.faces, *self._corner_lists)
        return self.normals

    def render(self, intrinsic, extrinsic, width, height, colors=None, radius=None, background=(1.0, 1.0, 1.0), lit=False,
               ambient=0.35, depth_strength=8.0, section=None, cloud_shade="auto"):
        """Id, depth and colour images of the scene for a pinhole camera (``camera_from_matrices``): pixel by pixel what
        ``pick`` returns for the ray through the pixel's centre -- faces when the scene has them (``a3d_render_mesh``),
        else vertices within ``radius`` (default ``voxel_size``) of the ray (``a3d_render_points``).  ``colors`` [n, 3]
        per-vertex colours on the device (default: those of the last ``infer`` / ``preview``, the scan's own before any);
        ``background``: the colour of pixels that show nothing.  ``lit=False``: flat colours (``a3d_render_shade``).
        ``lit=True``: on a mesh the colours are lit from the camera, double-sided, by the vertex normals (``ses.normals``,
        computed once per scene on first use; ``a3d_render_shade_lit``: colour x (``ambient`` + (1 - ``ambient``) |cos| of
        the angle between the interpolated normal and the pixel's ray)); on a cloud, which has no normals, a pixel darkens
        by how far it lies behind its four neighbours (``a3d_render_shade_depth``: colour / (1 + ``depth_strength`` x the
        summed relative depth steps)).  A cloud whose normals have been estimated (``estimate_normals()``) is lit as a mesh
        is, by its vertices' normals (``a3d_render_shade_lit_points``; a vertex without a valid normal keeps its colour),
        and may be rendered under a culling section (on the copy culled for the camera's centre, ``a3d_cull_points``);
        ``cloud_shade="depth"`` still asks for the depth shade (``"auto"``: the normals when there are some).
        ``ambient`` in [0, 1] and ``depth_strength`` >= 0 are used only when ``lit``; their
        defaults, 0.35 and 8.0, are this project's settings, not the reference's (Open3D's lit material is not
        reproduced).  ``section``: the ``Section`` to render under (``a3d_render_mesh_section`` /
        ``a3d_render_points_section``; default: the session's; an empty ``Section()`` renders without one; culling on a cloud
        raises ``ValueError``) -- the image stays what ``pick`` under the same section returns, and ``result.section`` keeps
        it for ``annotate`` and ``click_at``.  Returns a ``RenderResult``.  One small device-to-host
        copy (the result header) per attempt; a view that needs more (tile, primitive) pairs than the scene's workspace
        holds is rendered again with a larger one."""
        self._need_scene()
        cam = camera_from_matrices(intrinsic, extrinsic, width, height)
        w, h = cam.width, cam.height
        dev = self.device
        bg = _f3(background, "background")
        ambient, depth_strength = float(ambient), float(depth_strength)
        if not 0.0 <= ambient <= 1.0:                   # (NaN fails both)
            raise ValueError("ambient must lie in [0, 1]")
        if not (np.isfinite(depth_strength) and depth_strength >= 0.0):
            raise ValueError("depth_strength must be finite and >= 0")
        n = self.coords_full.shape[0]
        col = self._colors_last if colors is None else colors
        col = self.colors_full if col is None else col
        if not torch.is_tensor(col) or col.device != dev or col.dtype != torch.float32 or tuple(col.shape) != (n, 3):
            raise ValueError(f"colors must be a float32 tensor [{n}, 3] on the session's device")
        col = col.contiguous()
        mesh = self.faces is not None
        sec, cut = self._section_of(section, mesh)
        if cloud_shade not in ("auto", "depth"):
            raise ValueError("cloud_shade must be 'auto' or 'depth'")
        xyz = self.coords_full
        if not mesh:                                    # (a culled cloud: the copy for the camera's centre, and the planes alone)
            xyz, cut = self._cloud_under(sec, cut, np.array(cam.o[:], np.float32))
        n_prim = self.faces.shape[0] if mesh else n
        r = self.voxel_size if radius is None else float(radius)
        ids = t = u = v = None                      # (allocated by the first attempt, written again by a retry)
        header = self._small[16:20]
        capacity = max(4 * n_prim, 1 << 16)
        for attempt in range(3):
            need = V.render_workspace_bytes(n_prim, w, h, capacity)
            if self._render_ws is None or self._render_ws.numel() < need:
                self._render_ws = None              # (dropped first: the old and the new one need not live together)
                self._render_ws = torch.empty(need, dtype=torch.uint8, device=dev)
            ws = self._render_ws
            if mesh and sec is None:
                ids, t, u, v, _ = V.render_mesh(self.coords_full, self.faces, cam, ids, t, u, v, header=header, workspace=ws)
            elif mesh:
                ids, t, u, v, _ = V.render_mesh_section(self.coords_full, self.faces, cam, cut, ids, t, u, v, header=header,
                                                        workspace=ws)
            elif cut is None:
                ids, t, _ = V.render_points(xyz, r, cam, ids, t, header=header, workspace=ws)
            else:
                ids, t, _ = V.render_points_section(xyz, r, cam, cut, ids, t, header=header, workspace=ws)
            flags, n_every, pairs = V.read_render_header(header.cpu().numpy())
            if not flags & L.A3D_RENDER_OVERFLOW:
                break
            capacity = pairs + pairs // 8           # this view's pairs and room for the next one
        else:
            raise RuntimeError("a3d_render: the pair capacity it asked for did not suffice")
        if flags & L.A3D_RENDER_BAD_INDEX:
            raise RuntimeError("a3d_render_mesh: face indices out of range")
        if lit and mesh:
            rgb = V.render_shade_lit(ids, u, v, self.faces, col, self._vertex_normals(), cam, ambient, bg)
        elif lit and self.normals is not None and cloud_shade == "auto":
            rgb = V.render_shade_lit_points(ids, col, self.normals, cam, ambient, bg)
        elif lit:
            rgb = V.render_shade_depth(ids, t, None, None, None, col, depth_strength, bg)
        else:
            rgb = V.render_shade(ids, u, v, self.faces, col, bg)
        return RenderResult(ids=ids, t=t, rgb=rgb, u=u, v=v, camera=cam, mesh=mesh, lit=bool(lit), pairs=pairs,
                            n_everywhere=n_every, section=sec)

    def pick_from_render(self, result, u, v):
        """The point a click through pixel ``(u, v)`` (column, row) of ``result`` takes -- what ``pick`` returns for that
        pixel's ray: on a mesh the combination of the face's vertices with the rendered weights, (w a + u b) + v c in fp32
        with w = (1 - u) - v; on a cloud the vertex; ``None`` where the pixel shows nothing."""
        self._need_scene()
        u, v = int(u), int(v)
        h, w = result.ids.shape
        if not (0 <= u < w and 0 <= v < h):
            raise ValueError(f"pixel ({u}, {v}) outside the {w} x {h} image")
        if result.mesh != (self.faces is not None):
            raise ValueError("the render belongs to another scene")
        idx = int(result.ids[v, u].cpu())
        if idx < 0:
            return None
        if not result.mesh:
            return [float(x) for x in self._coords_host[idx]]
        f32 = np.float32
        wu, wv = f32(result.u[v, u].cpu().numpy()), f32(result.v[v, u].cpu().numpy())
        pa, pb, pc = self._coords_host[self.faces[idx].cpu().numpy()]
        ww = f32(f32(1.0) - wu) - wv
        return [float(x) for x in (ww * pa + wu * pb) + wv * pc]

    # ------------------------------------------------------------------ the annotation in the view
    def _view_labels(self, result, labels):
        """(labels int32 [n] on the device, the images ``(ids, u, v, faces)`` as ``view.render_labels`` takes them)."""
        self._need_scene()
        if result.mesh != (self.faces is not None):
            raise ValueError("the render belongs to another scene")
        n = self.coords_full.shape[0]
        lab = self._labels_last if labels is None else labels
        if lab is None:                             # before any infer / preview: all background
            lab = torch.zeros(n, dtype=torch.int32, device=self.device)
        if not torch.is_tensor(lab) or lab.device != self.device or lab.dtype != torch.int32 or tuple(lab.shape) != (n,):
            raise ValueError(f"labels must be an int32 tensor [{n}] on the session's device")
        return lab.contiguous(), (result.ids, result.u, result.v, self.faces)

    def label_image(self, result, labels=None):
        """int32 [h, w] on the device: the object id each pixel of ``result`` shows (``a3d_render_labels``) -- 0 =
        background, -1 = the pixel shows nothing.  ``labels`` int32 [n] per-vertex labels on the device (default: the
        full-resolution labels of the last ``infer`` / ``preview``, all background before any).  On a cloud a pixel shows
        its vertex's label; on a mesh that of the heaviest corner of its face, which cuts a face among its vertices by
        crisp borders -- not the vertex ``click`` would snap to, which is the nearest by Euclidean distance."""
        lab, (ids, u, v, faces) = self._view_labels(result, labels)
        return V.render_labels(ids, u, v, faces, lab)

    def object_at(self, result, u, v, labels=None):
        """The object id under pixel ``(u, v)`` (column, row) of ``result`` -- ``label_image``'s value there, computed for
        that pixel alone -- or ``None`` where the pixel shows nothing.  One small device-to-host copy."""
        lab, (ids, wu, wv, faces) = self._view_labels(result, labels)
        u, v = int(u), int(v)
        h, w = result.ids.shape
        if not (0 <= u < w and 0 <= v < h):
            raise ValueError(f"pixel ({u}, {v}) outside the {w} x {h} image")
        one = lambda image: None if image is None else image[v:v + 1, u:u + 1]
        obj = int(V.render_labels(one(ids), one(wu), one(wv), faces, lab, out=self._small[20:21].view(1, 1)).cpu())
        return None if obj < 0 else obj

    def annotate(self, result, labels=None, outlines=True, markers=True, outline_color=(0.0, 0.0, 0.0), marker_px=6.0,
                 marker_border_px=1.5, marker_border_color=(1.0, 1.0, 1.0), depth_slack=None):
        """uint8 [h, w, 3], a new tensor: ``result.rgb`` (left untouched) with the state of the annotation drawn over it
        (``a3d_render_annotate``).  ``outlines``: a pixel of an object (``label_image(result, labels)`` >= 1) with a
        4-neighbour inside the image that shows something else takes ``outline_color`` -- a border one pixel wide on
        either side between two objects, none along the image's edge, none around the background.  ``markers``: every
        click of the session, in click order (later clicks on top), is a disc of radius ``marker_px`` pixels around the
        projection of its picked point (``view.marker_table``), in its cube's colour with a rim ``marker_border_px`` wide in
        ``marker_border_color`` -- also a click that has no vertex in its cube and so leaves ``preview``'s colours alone.
        A click shows through pixels whose surface lies up to ``depth_slack`` world units (default ``cube_size``) in front of
        it and is hidden behind nearer ones.  A click whose picked point the planes of ``result.section`` cut away has no
        marker (``visible_clicks``: the vertex rule on the point, so a click made exactly on a plane may lose its marker to
        the rounding of the point).  The defaults -- black outlines, 6-pixel discs with a white 1.5-pixel rim --
        are this project's settings, not the reference's (the GUI shows clicks as recoloured vertices only)."""
        marker_px, marker_border_px = float(marker_px), float(marker_border_px)
        slack = self.cube_size if depth_slack is None else float(depth_slack)
        if not (np.isfinite(marker_px) and 0.0 <= marker_border_px <= marker_px):      # (NaN fails)
            raise ValueError("marker_px must be finite and marker_border_px lie in [0, marker_px]")
        if not (np.isfinite(slack) and slack >= 0.0):
            raise ValueError("depth_slack must be finite and >= 0")
        outline = _f3(outline_color, "outline_color") if outlines else None
        border = _f3(marker_border_color, "marker_border_color")
        lab, images = self._view_labels(result, labels)
        label_image = V.render_labels(*images, lab) if outlines else None
        table = None
        if markers and self.num_clicks:
            cubes = self._cubes[:self.num_clicks]
            cubes = cubes[visible_clicks(result.section, cubes[:, :3])]
            rows = V.marker_table(result.camera, cubes[:, :3], cubes[:, 3:])
            table = torch.from_numpy(rows).to(self.device) if len(rows) else None
        return V.render_annotate(result.rgb, label_image, result.t, table, marker_px, marker_px - marker_border_px, slack,
                                 outline, border)

    def nearest(self, point):
        """(voxel row, full-resolution vertex) nearest to ``point``: both searches in one launch pair, exact."""
        self._need_scene()
        q = _f3(point, "point")
        rows = V.nearest_rows([self.raw_coords_qv, self.coords_full], q[None], out=self._small[:2].view(2, 1),
                              workspace=self._ws)
        return tuple(rows.view(2).cpu().tolist())

    def click(self, point, obj: int):
        """One click at ``point`` for object ``obj`` (0 = background, k >= 1 = object k), booked as gui.py:290-331 does:
        the voxel row nearest to the point joins ``click_idx``, the running click count ``click_time_idx``, the nearest
        full-resolution vertex's coordinates ``click_positions``; the first click of a new object relabels the ground
        truth (every vertex of the instance under the clicked voxel becomes ``obj``).  The click joins the session's click
        list, from which all of this derives (``click_state``), and empties the redo stack.  Returns (voxel row, vertex)."""
        self._need_scene()
        obj = int(obj)
        key = str(obj)
        n_obj = len(self.click_idx) - 1
        if obj < 0 or obj > 255:
            raise ValueError("object ids are 0 (background) .. 255")
        if key not in self.click_idx and obj != n_obj + 1:
            raise ValueError(f"object {obj} would leave a gap: the next new object is {n_obj + 1} (forward_mask needs ids 1..K)")
        if self.num_clicks + 1 + self.model.num_bg_queries > L.A3D_MAX_QUERIES:
            raise ValueError(f"too many queries: {self.num_clicks + 1} clicks + {self.model.num_bg_queries} background queries "
                             f"> {L.A3D_MAX_QUERIES}")
        q = _f3(point, "point")
        row_qv, row_full = self.nearest(q)
        new_object = key not in self.click_idx
        self._clicks.append({"obj": obj, "point": tuple(float(x) for x in q), "row_qv": row_qv, "row_full": row_full,
                             "position": self._coords_host[row_full].tolist()})
        self._redo.clear()
        self._guide_logits = self._guide_last = None    # the kept logits belong to the list before this click
        self.click_idx, self.click_time_idx, self.click_positions = click_state(self._clicks)
        if new_object and self.new_labels is not None:
            self._launch_edit(None)
        colour = self.background_click_color if obj == 0 else self._palette_entry(obj)
        k = self.num_clicks
        self._cubes[k] = (q[0], q[1], q[2], colour[0], colour[1], colour[2])
        self._cubes_dev[k].copy_(self._cubes_host[k], non_blocking=True)      # (a row of its own in pinned memory: never rewritten while in flight)
        self.num_clicks += 1
        return row_qv, row_full

    def click_ray(self, origin, direction, obj: int, section=None):
        """``pick`` then ``click``: the click a pointer ray makes for object ``obj``.  Returns what ``click`` returns, or
        ``None`` -- with nothing booked -- when the ray meets nothing.  ``section``: as ``pick``'s."""
        point = self.pick(origin, direction, section=section)
        if point is None:
            return None
        return self.click(point, obj)

    # ------------------------------------------------------------------ editing the click list
    def clicks(self):
        """The click list: one dict per click in time order -- ``index`` (its time index), ``obj``, ``point`` (the picked
        point), ``row_qv``, ``row_full``, ``position`` (the vertex's coordinates).  Copies: changing them changes nothing."""
        return [self._click_dict(i) for i in range(len(self._clicks))]

    def _click_dict(self, i):
        c = self._clicks[i]
        return {"index": i, "obj": c["obj"], "point": list(c["point"]), "row_qv": c["row_qv"], "row_full": c["row_full"],
                "position": list(c["position"])}

    def _launch_edit(self, lut):
        """ONE ``a3d_session_edit`` call: the relabelled ground truth of the click list (scenes that have one) and, with a
        ``lut``, the renumbering of the last inference's voxel labels."""
        relabel = self.new_labels is not None
        if not relabel and lut is None:
            return
        instances = None
        if relabel:
            rows = instance_rows(self._clicks)
            if rows:                                    # gathered on the device: the ids never visit the host
                instances = self.labels_qv_ori[torch.tensor(rows, dtype=torch.int64, device=self.device)]
        V.session_edit(labels_ori=self.labels_full_ori if relabel else None, instances=instances,
                       new_labels=self.new_labels if relabel else None, labels=None if lut is None else self._labels_qv,
                       lut=lut, err=None if lut is None else self._edit_err)

    def _set_clicks(self, clicks, lut):
        """Makes ``clicks`` the session's click list and rebuilds what derives from it: the dictionaries, the cube table
        (pinned and on the device, colours from the new ids), the relabelled ground truth, the last inference's labels
        through ``lut`` (``None``: left alone) and, by a ``preview()``, what the view shows."""
        state = click_state(clicks)                     # (refuses a list with a gap before anything changes)
        torch.cuda.current_stream(self.device).synchronize()   # no copy from a pinned cube row is in flight past this point
        before, n = self.num_clicks, len(clicks)
        self._clicks = list(clicks)
        self._guide_logits = self._guide_last = None    # the kept logits belong to the list before the edit
        self.click_idx, self.click_time_idx, self.click_positions = state
        self.num_clicks = n
        for k, c in enumerate(self._clicks):
            colour = self.background_click_color if c["obj"] == 0 else self._palette_entry(c["obj"])
            self._cubes[k] = (*c["point"], colour[0], colour[1], colour[2])
        self._cubes[n:max(n, before)] = 0.0
        if max(n, before):
            self._cubes_dev[:max(n, before)].copy_(self._cubes_host[:max(n, before)], non_blocking=True)
        self._launch_edit(lut)
        layer = lut is not None and self._manual is not None
        if layer:                                       # the manual layer's ids go through the same table as the voxels' labels
            V.session_edit(labels=self._manual[1], lut=lut, err=self._manual_err)
        self.preview()
        if lut is not None and int(self._edit_err.cpu()[0]):
            raise RuntimeError("a3d_session_edit: a voxel label outside 0 .. 255")
        if layer and int(self._manual_err.cpu()[0]):
            raise RuntimeError("a3d_session_edit: a manual label outside 0 .. 255")

    def _remove(self, index):
        before = self._clicks
        n_obj = len(self.click_idx) - 1
        clicks, lut = remove_from_clicks(before, index)
        removed = self._click_dict(index)
        self._set_clicks(clicks, lut)
        removed["id_map"] = {k: int(lut[k]) for k in range(1, n_obj + 1)}
        return removed, before, lut

    def remove_click(self, index):
        """Takes click ``index`` (its time index; ``IndexError`` outside ``[0, num_clicks)``) out of the annotation
        (``remove_from_clicks``): later clicks move up by one time index, and if it was its object's only click the object
        is gone and the ids above it drop by one.  The dictionaries, ``click_positions``, the cubes and the relabelled
        ground truth follow the new list; the labels of the last inference are renumbered (a removed object's voxels show
        as background until the next ``infer()``), and ``render`` / ``label_image`` / ``annotate`` show that at once.
        Synchronises the stream once.  Empties the redo stack.  Returns the removed click's dict (``clicks()``) with
        ``id_map``: {old object id: new id, 0 = gone}."""
        self._need_scene()
        removed = self._remove(index)[0]
        self._redo.clear()
        return removed

    def undo(self):
        """``remove_click`` of the last click, except that the list as it was goes onto the redo stack.  Returns the removed
        click, or ``None`` -- with nothing changed -- when there is no click."""
        self._need_scene()
        if not self._clicks:
            return None
        removed, before, lut = self._remove(len(self._clicks) - 1)
        self._redo.append((before, restore_lut(lut)))
        return removed

    def redo(self):
        """Takes the last ``undo()`` back: the click list is again what it was before it; an object that had disappeared
        comes back under its id and the ids at or above it move back up.  What does NOT come back is that object's labels:
        the undo turned its voxels into background, and they stay background until the next ``infer()`` (labels after an
        edit are the last inference renumbered, not an earlier one restored).  Returns the restored click, or ``None`` when
        there is nothing to redo (``click``, ``remove_click``, ``restore_*``, ``reset`` and ``load_scene`` empty the stack)."""
        self._need_scene()
        if not self._redo:
            return None
        clicks, lut = self._redo.pop()
        self._set_clicks(clicks, lut)
        return self._click_dict(len(clicks) - 1)

    def restore_clicks(self, click_idx, click_time_idx):
        """Resumes an annotation from its click dictionaries (voxel rows and time indices per object, as ``infer()`` and the
        reference tool save them): ``reset()``, then the click list rebuilt in time order.  A file keeps no picked points,
        so a click's point is its voxel's coordinates ``raw_coords_qv[row]``, and its vertex (``a3d_nearest_rows``, 64
        queries per launch) the one nearest to that -- ``click_idx``, ``click_time_idx`` and the relabelled ground truth are
        the saving session's, cubes, markers and ``click_positions`` lie at most a voxel off.  ``ValueError``, with the
        session untouched, for what ``clicks_from_dicts`` refuses: keys other than "0".."K", times that are no permutation
        of 0..m-1, rows outside the voxels, more clicks than ``click()`` accepts."""
        self._need_scene()
        pairs = clicks_from_dicts(click_idx, click_time_idx, self.raw_coords_qv.shape[0],
                                  L.A3D_MAX_QUERIES - self.model.num_bg_queries)
        self.reset()
        if not pairs:
            return self
        rows = torch.tensor([r for _, r in pairs], dtype=torch.int64, device=self.device)
        points = self.raw_coords_qv[rows].cpu().numpy()
        rows_full = []
        for s in range(0, len(pairs), L.A3D_NEAREST_MAX_QUERIES):
            chunk = points[s:s + L.A3D_NEAREST_MAX_QUERIES]
            rows_full += V.nearest_rows([self.coords_full], chunk, workspace=self._ws)[0].cpu().tolist()
        self._set_clicks([{"obj": o, "point": tuple(float(x) for x in p), "row_qv": r, "row_full": rf,
                           "position": self._coords_host[rf].tolist()} for (o, r), p, rf in zip(pairs, points, rows_full)], None)
        return self

    def restore_file(self, path):
        """``restore_clicks`` from a ``clicks/click_*.npy`` as ``infer()`` and the reference tool write it: a pickled dict
        with ``click_idx`` and ``click_time`` (a pickle: load files you trust)."""
        saved = np.load(path, allow_pickle=True)
        saved = saved.item() if isinstance(saved, np.ndarray) and saved.shape == () else saved
        if not isinstance(saved, dict) or "click_idx" not in saved or "click_time" not in saved:
            raise ValueError(f"{path}: a dict with click_idx and click_time expected")
        return self.restore_clicks(saved["click_idx"], saved["click_time"])

    def click_at(self, result, u, v, marker_px=6.0, depth_slack=None):
        """The time index of the click whose marker ``annotate(result, marker_px=, depth_slack=)`` draws on top at pixel
        ``(u, v)`` (column, row), or ``None`` -- for a viewer that deletes the click under the pointer
        (``remove_click(click_at(...))``).  ``annotate``'s cover test (``marker_hit``) on the host, from ``view.marker_table``
        and one pixel of ``result.t``: one small device-to-host copy."""
        self._need_scene()
        u, v = int(u), int(v)
        h, w = result.t.shape
        if not (0 <= u < w and 0 <= v < h):
            raise ValueError(f"pixel ({u}, {v}) outside the {w} x {h} image")
        marker_px = float(marker_px)
        slack = self.cube_size if depth_slack is None else float(depth_slack)
        if not (np.isfinite(marker_px) and marker_px >= 0.0 and np.isfinite(slack) and slack >= 0.0):
            raise ValueError("marker_px and depth_slack must be finite and >= 0")
        if not self.num_clicks:
            return None
        cubes = self._cubes[:self.num_clicks]
        visible = visible_clicks(result.section, cubes[:, :3])      # (as annotate: no marker in the cut-away part)
        cubes = cubes[visible]
        rows, kept = V.marker_table(result.camera, cubes[:, :3], cubes[:, 3:], return_kept=True)
        hit = marker_hit(rows, u, v, result.t[v, u].cpu().numpy(), marker_px, slack)
        return None if hit is None else int(visible[kept[hit]])

    def _palette_entry(self, obj):
        n = self.palette.shape[0]
        return self.palette[obj if obj < n else 1 + (obj - 1) % (n - 1)]

    # ------------------------------------------------------------------ paint and infer
    def _launch_paint(self, labels_qv, paint_cubes):
        cubes = self._cubes_dev[:self.num_clicks] if paint_cubes and self.num_clicks else None
        err = self._counts[3 * _N_IDS + 1:].view(torch.int32)[:1]       # (the low word of the slot behind the IoU counts)
        return V.session_paint(labels_qv, self.inverse_map, self.coords_full, self.colors_full, self._palette_dev, cubes,
                               self.cube_size, err=err)[:2]

    def preview(self, paint_cubes=True):
        """Labels and colours of the current state WITHOUT running the model: the last inference's labels (background
        before the first) with the clicks' cubes on top -- what the GUI shows between a click and the next inference."""
        self._need_scene()
        labels_full, colors = self._launch_paint(self._labels_qv, paint_cubes)
        if int(self._counts[3 * _N_IDS + 1:].cpu()[0]) & 0xffffffff:
            raise RuntimeError("a3d_session_paint: inverse_map or labels out of range")
        self._colors_last, self._labels_last = colors, labels_full
        return labels_full, colors

    def _launch_iou(self, labels, inverse_map):
        """IoU counts of ``labels`` (read through ``inverse_map`` when given) against the relabelled ground truth into the head
        of ``self._counts`` on the current stream; zeros when the scene has none."""
        head = self._counts[:3 * _N_IDS + 1]
        if self.new_labels is not None:
            K.launch_iou_counts([labels], [self.new_labels], [inverse_map], _N_IDS, head.view(1, -1))
        else:
            head.zero_()

    def _read_iou(self, host):
        """``(miou, iou_per_object)`` from the host copy of ``self._counts``; two Nones without a ground truth."""
        if self.new_labels is None:
            return None, None
        t, per_obj = K.mean_iou_from_counts(host[:3 * _N_IDS].reshape(3, _N_IDS).copy())
        return t.tolist(), per_obj

    def infer(self, paint_cubes=False, logits=None):
        """The arithmetic of ``get_next_click(run_model=True)``: ``forward_mask`` on the session's clicks, arg-max with the
        clicked rows keeping their object, the lift to full resolution with colours (and cubes when asked), the IoU
        against the relabelled ground truth -- then ONE host round trip.  ``logits`` ([n_voxels, 1 + K], device):
        use these instead of calling the model (replaying recorded logits)."""
        self._need_scene()
        num_obj = len(self.click_idx) - 1
        if self.num_clicks == 0:
            raise ValueError("infer() without a click (the reference returns early; here it is an error)")
        if num_obj == 0:
            raise ValueError("infer() needs a click on at least one object (the reference divides by the object count)")
        dev = self.device
        if logits is None:
            out = self.model.forward_mask(*self._backbone, click_idx=[self.click_idx], click_time_idx=[self.click_time_idx])
            logits = out["pred_masks"][0]
        logits = logits.contiguous()
        labels_qv = K.argmax_labels(logits, self.click_idx)
        labels_full, colors = self._launch_paint(labels_qv, paint_cubes)
        self._launch_iou(labels_qv, self.inverse_map)
        mask_host = None
        try:
            self._counts_host.copy_(self._counts, non_blocking=True)
            if self.out_dir is not None:
                mask_host = self._mask_host
                mask_host.copy_(labels_full, non_blocking=True)
        finally:
            torch.cuda.current_stream(dev).synchronize()      # the one host round trip
        host = self._counts_host.numpy()
        if host[3 * _N_IDS] or (int(host[3 * _N_IDS + 1]) & 0xffffffff):
            raise RuntimeError("inverse_map or labels out of range")
        self._labels_qv = labels_qv
        self._colors_last, self._labels_last = colors, labels_full
        self._guide_logits, self._guide_last = (logits, self.click_idx), None
        miou, per_obj = self._read_iou(host)
        res = SessionResult(labels_full=labels_full, colors=colors, miou=miou, iou_per_object=per_obj, num_obj=num_obj,
                            avg_clicks=round(self.num_clicks / num_obj, 1))
        if self.out_dir is not None:
            iou = format_iou(miou)
            res.record = record_line(self.clock(), self.scene_name, num_obj, self.num_clicks, iou)
            with open(os.path.join(self.out_dir, RECORD_FILE), "a") as f:
                f.write(res.record)
            res.mask_path = os.path.join(self.out_dir, MASK_DIR, mask_file_name(self.num_clicks, num_obj, iou))
            res.click_path = os.path.join(self.out_dir, CLICK_DIR, click_file_name(self.num_clicks, num_obj, iou))
            np.save(res.mask_path, mask_host.numpy().astype(np.int64))           # the reference saves an int64 arg-max
            np.save(res.click_path, {"click_idx": self.click_idx, "click_time": self.click_time_idx})
        return res

    # ------------------------------------------------------------------ where the labels are unsure
    def guide(self, threshold=1.0, full_margin=4.0, doubt_color=(1.0, 1.0, 1.0), max_suggestions=5, regions="pairs"):
        """Where the LAST ``infer()`` is unsure, and where a next click would help most.  From the logits that inference
        used (``ValueError`` when there are none: before the first ``infer()``, and after anything that changed the click
        list or the scene since -- ``click``, ``undo``, ``redo``, ``remove_click``, ``restore_*``, ``reset``, ``load_scene``):

        * per voxel the winning object, the runner-up and the MARGIN between their logits (``a3d_session_guide``; a clicked
          voxel has margin +inf), lifted to the vertices through the inverse map;
        * the confidence view ``colors``: a vertex's object colour (its own for the background) faded towards ``doubt_color``
          as the margin falls from ``full_margin`` to 0 -- ``render(colors=g.colors)`` shows it as it is;
        * voxels and contested voxels per object; a voxel is CONTESTED when its margin lies below ``threshold``;
        * ``suggestions``: the contested voxels form regions, one per (runner-up, winner) pair; each region's deepest voxel
          -- the one farthest from everything outside the region, found by the click simulator's search
          (``a3d_click_clusters`` with the runner-up as the wanted label) -- is a suggested click for the RUNNER-UP, ranked by
          that depth (``rank_suggestions``), at most ``max_suggestions``.  ``ses.click(s["point"], s["object"])`` takes one.
          A region that covers every voxel has no border and no depth: the suggestion is then the least confident voxel
          alone, with ``size = inf`` (``suggest_clicks``) -- a case for logits without a clicked voxel, which is never
          contested and so lies outside every region.

        ``threshold`` and ``full_margin`` are in logit units.  The defaults, 1.0 and 4.0, are this project's choice and are
        NOT tuned on real scans.  A region is told from another by the simulator's cluster id, 96 x runner-up + 11 x winner,
        which is unique while object ids stay below 96; above that two regions can share an id and count as one.
        One ``a3d_session_guide`` call, the cluster search, then ONE host round trip.  Returns a ``GuideResult``.

        ``regions="connected"`` tells regions apart by WHERE they lie: a SPOT is a connected piece (26-connectivity,
        ``a3d_label_pieces``) of the contested voxels with one (runner-up, winner) pair -- key ``256 x runner-up + winner``,
        -1 on the other voxels -- so two doubtful places between the same two objects are two spots and get a suggestion
        each.  The spots are ranked by size, ties to the lower root (``rank_spots``); the first ``MAX_SPOTS`` = 255 get the
        pseudo ids 1..255 in a per-voxel array built on the device, and the same exact search runs with these as the wanted
        labels over a prediction of 0 everywhere: each spot's deepest voxel is the one farthest from every voxel outside THAT
        spot.  Suggestions are ranked by depth as before, the object is the spot's runner-up, and each carries ``voxels`` (the
        spot's size) and ``root`` (its smallest voxel row); ``n_spots`` and ``n_spots_searched`` say how many spots there are
        and how many were searched.  A spot that covers every voxel falls back to the least confident voxel as above.  This
        mode costs a SECOND small host round trip: the choice of spots needs the record list on the host.  ``"pairs"``, the
        default, is the behaviour described first and keeps its one round trip."""
        self._need_scene()
        if regions not in ("pairs", "connected"):
            raise ValueError('regions must be "pairs" or "connected"')
        if self._guide_logits is None:
            raise ValueError("guide() describes the last infer(): there is none, or the clicks or the scene changed since "
                             "(call infer() first)")
        logits, click_idx = self._guide_logits
        n_ids = max(len(click_idx), logits.shape[1])
        rows, objs = K.click_lists(click_idx)        # dict order, as a3d_argmax_labels applied them in infer()
        dev = self.device
        labels, runner, margin, want, margin_full, colors, _ = V.session_guide(
            logits, rows, objs, threshold, inverse_map=self.inverse_map, colors=self.colors_full, palette=self._palette_dev,
            doubt_color=doubt_color, full_margin=full_margin, summary=self._guide_sum)
        search_pred, search_want, spots = labels, want, None
        if regions == "connected":
            search_pred, search_want, spots, n_spots = self._contested_spots(labels, want)
        try:
            out, out_host = K.launch_clusters(search_pred, search_want, self.raw_coords_qv)
            self._guide_sum_host.copy_(self._guide_sum, non_blocking=True)
            out_host.copy_(out, non_blocking=True)
        finally:
            torch.cuda.current_stream(dev).synchronize()      # the one host round trip
        summary = V.read_guide_summary(self._guide_sum_host.numpy())
        if summary["err"] & V.GUIDE_BAD_INDEX:
            raise RuntimeError("a3d_session_guide: inverse_map out of range")
        if summary["err"] & V.GUIDE_NAN_MARGIN:
            raise RuntimeError("a3d_session_guide: the logits hold a NaN (or two infinities of one sign in a row)")
        clusters = K.read_clusters(out_host.numpy(), bad_ids="a3d_click_clusters: labels outside 0 .. 255",
                                   too_many="a3d_click_clusters: {} contested regions", whole_sample_ok=True)
        if spots is not None:                        # a cluster's `label` is its spot's pseudo id: back to the spot's two objects
            by_row = {}
            for c in clusters:
                spot = spots[c["label"] - 1]
                c["label"], c["pred"] = int(spot["key"]) >> 8, int(spot["key"]) & 255
                by_row[c["row"]] = spot
        suggestions = suggest_clicks(clusters, summary["least"], self._coords_qv_host, max_suggestions)
        if spots is not None:
            for s in suggestions:                    # (the fallback's row is the least confident voxel of the one spot there is)
                spot = by_row.get(s["row"], spots[0])
                s["voxels"], s["root"] = int(spot["voxels"]), int(spot["root"])
        res = GuideResult(labels_qv=labels, runner_qv=runner, margin_qv=margin, margin_full=margin_full, colors=colors,
                          object_voxels=summary["voxels"][:n_ids].copy(),
                          object_contested=summary["contested"][:n_ids].copy(), least_confident=summary["least"],
                          n_contested=int(summary["contested"].sum()), suggestions=suggestions,
                          threshold=float(threshold), full_margin=float(full_margin))
        if spots is not None:
            res.n_spots, res.n_spots_searched = n_spots, len(spots)
        self._guide_last = res
        return res

    # ------------------------------------------------------------------ where in space a label lies
    def _scene_handle(self):
        return self._backbone[0]._a3d.scene

    def _click_rows(self):
        return [int(r) for rows in self.click_idx.values() for r in rows]

    def _label_pieces(self, keys, connectivity, click_rows=(), lift=False, max_out=1024, workspace=None, similar=None, also=None):
        """``a3d_label_pieces`` -- with ``similar``, a dict of ``view.similar_pieces``' normals, colours and thresholds,
        ``a3d_similar_pieces`` -- on the session's voxels and the copy of its record list: ``(piece_qv, piece_full, records,
        n_pieces)``.  One library call and ONE host round trip; when there are more pieces than ``max_out`` records, once
        more with the reported count (as ``render`` grows its pair buffer).  ``also``: a function of ``(piece_qv,
        piece_full)`` that returns a tensor to bring along in that round trip; its host copy is then a fifth value."""
        dev, scene = self.device, self._scene_handle()
        name = "a3d_label_pieces" if similar is None else "a3d_similar_pieces"
        for _ in range(2):
            buf = torch.empty(max_out * V.PIECE.itemsize + 8, dtype=torch.uint8, device=dev)
            records, count = buf[:max_out * V.PIECE.itemsize], buf[max_out * V.PIECE.itemsize:].view(torch.int32)
            shared = dict(connectivity=connectivity, click_rows=click_rows, inverse_map=self.inverse_map if lift else None,
                          records=records, count=count, workspace=workspace)
            if similar is None:
                piece_qv, piece_full, _, _, workspace = V.label_pieces(scene, keys, **shared)
            else:
                piece_qv, piece_full, _, _, workspace = V.similar_pieces(scene, keys, **similar, **shared)
            extra = None if also is None else also(piece_qv, piece_full).contiguous().view(-1).view(torch.uint8)
            host = (buf if extra is None else torch.cat([buf, extra])).cpu().numpy()       # the one host round trip
            recs, n_pieces, err = V.read_pieces(host[:buf.numel() - 8], host[buf.numel() - 8:buf.numel()])
            if err & V.PIECES_BAD_INDEX:
                raise RuntimeError(f"{name}: inverse_map out of range")
            if n_pieces <= max_out:
                return (piece_qv, piece_full, recs, n_pieces) + (() if also is None else (host[buf.numel():].copy(),))
            max_out = n_pieces
        raise RuntimeError(f"{name}: the record list did not fit twice")

    def _contested_spots(self, labels, want):
        """What ``guide(regions="connected")`` hands to the cluster search: ``(pred = 0 everywhere, the pseudo id of every
        voxel's spot (0: none), the records of the searched spots in pseudo-id order, the number of spots)``."""
        key = torch.where(want != labels, want * 256 + labels, torch.full_like(labels, -1))
        piece_qv, _, recs, n_spots = self._label_pieces(key, 26)
        spots = [recs[k] for k in rank_spots(recs)]
        return torch.zeros_like(labels), self._spot_ids(piece_qv, spots), spots, n_spots

    def _spot_ids(self, piece_qv, spots):
        """int32 [n_voxels]: the pseudo id -- position in ``spots`` (records of ``a3d_label_pieces``) + 1 -- of the piece every
        voxel lies in, 0 for a voxel of no piece or of one that is not among ``spots``: the wanted labels of the cluster search."""
        n = piece_qv.numel()
        table = torch.zeros(n + 1, dtype=torch.int32, device=self.device)                   # root row -> pseudo id; slot n: no piece
        if spots:
            roots = torch.tensor([int(r["root"]) for r in spots], dtype=torch.int64).to(self.device)
            table[roots] = torch.arange(1, len(spots) + 1, dtype=torch.int32, device=self.device)
        return table[torch.where(piece_qv >= 0, piece_qv, torch.full_like(piece_qv, n)).long()].contiguous()

    def pieces(self, connectivity=26, labels=None):
        """The connected PIECES of the session's current voxel labelling -- what ``preview()`` paints, so valid from
        ``load_scene`` on -- or of ``labels`` (int32 [n_voxels] on the device, object ids 0..255): voxels that are neighbours
        under ``connectivity`` (6: faces, 18: faces and edges, 26: faces, edges and corners) and carry the same object id
        belong to one piece, named by its smallest voxel row (``a3d_label_pieces``; the adjacency is the scene's own
        neighbour table).  Returns a ``PiecesResult``: which piece every voxel and vertex lies in, one record per piece
        (object id, voxels, whether it holds a clicked voxel, bounding box in voxel coordinates) and the pieces per object.
        One library call and ONE host round trip (a second of each when there are more than 1024 pieces)."""
        self._need_scene()
        keys = self._labels_qv if labels is None else labels
        piece_qv, piece_full, recs, n_pieces = self._label_pieces(keys, connectivity, self._click_rows(), lift=True)
        n_ids = max(len(self.click_idx), int(recs["key"].max()) + 1 if len(recs) else 1)
        return PiecesResult(piece_qv=piece_qv, piece_full=piece_full, records=recs, n_pieces=n_pieces,
                            object_pieces=np.bincount(recs["key"], minlength=n_ids).astype(np.int64), connectivity=connectivity)

    def piece_at(self, result, u, v, pieces=None):
        """The record (a ``view.PIECE`` row: root, key, voxels, clicked, lo, hi) of the piece that pixel ``(u, v)`` (column,
        row) of ``result`` shows, or ``None`` where the pixel shows nothing -- resolved as ``confidence_at`` resolves a vertex:
        the pixel's vertex on a cloud, the heaviest corner of its face on a mesh.  ``pieces``: a ``PiecesResult`` of this scene
        (default: ``pieces()`` of the current labelling, computed here)."""
        self._need_scene()
        pieces = self.pieces() if pieces is None else pieces
        if tuple(pieces.piece_full.shape) != (self.coords_full.shape[0],):
            raise ValueError("the pieces belong to another scene")
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        root = int(pieces.piece_full[vertex].cpu())
        k = int(np.searchsorted(pieces.records["root"], root))
        return pieces.records[k] if root >= 0 and k < len(pieces.records) and pieces.records["root"][k] == root else None

    def despeckle(self, min_voxels=8, connectivity=26, paint_cubes=False):
        """The current voxel labelling with its SPECKS removed, without touching the session: every piece (``pieces``) of
        fewer than ``min_voxels`` voxels that holds no clicked voxel takes the object most of its differently labelled
        neighbour pairs vote for (ties: the lowest id; a piece with no neighbour of another label keeps its own) -- ONE
        simultaneous step on the labels as they are (``a3d_absorb_pieces``).  Returns a ``DespeckleResult``: ``labels_qv``,
        ``labels_full`` and ``colors`` (through ``a3d_session_paint``), ``miou`` / ``iou_per_object`` against the relabelled
        ground truth when the scene has one, and the counts of small, relabelled and kept-isolated pieces.  It changes NO
        session state -- not the clicks, not the labels ``preview()`` paints, not the logits ``guide()`` reads:
        ``annotate(result, labels=r.labels_full)`` and ``render(colors=r.colors)`` show it.  The default ``min_voxels`` = 8 is
        this project's choice and is NOT tuned on real scans.  One host round trip (a second when there are more than 4096
        small pieces)."""
        self._need_scene()
        dev, scene, n = self.device, self._scene_handle(), self._labels_qv.numel()
        labels, rows = self._labels_qv, self._click_rows()
        capacity = 4096
        for _ in range(2):
            ws = V.pieces_workspace(n, dev, capacity, _N_IDS)
            piece_qv = V.label_pieces(scene, labels, connectivity, rows, records=torch.empty(0, dtype=torch.uint8, device=dev),
                                      workspace=ws)[0]
            labels_qv, summary = V.absorb_pieces(scene, labels, piece_qv, ws, min_voxels, connectivity, rows, _N_IDS, capacity)
            labels_full, colors = self._launch_paint(labels_qv, paint_cubes)
            self._launch_iou(labels_qv, self.inverse_map)
            packed = torch.cat([self._counts.view(torch.uint8), summary]).cpu().numpy()      # the one host round trip
            host, s = packed[:-V.ABSORB_SUMMARY.itemsize].view(np.int64), V.read_absorb_summary(packed[-V.ABSORB_SUMMARY.itemsize:])
            if not s["err"] & V.ABSORB_OVERFLOW:
                break
            capacity = s["small_pieces"]
        if s["err"] & V.ABSORB_BAD_LABEL or host[3 * _N_IDS] or (int(host[3 * _N_IDS + 1]) & 0xffffffff):
            raise RuntimeError("despeckle: inverse_map or labels out of range")
        miou, per_obj = self._read_iou(host)
        return DespeckleResult(labels_full=labels_full, colors=colors, miou=miou, iou_per_object=per_obj, labels_qv=labels_qv,
                               small_pieces=s["small_pieces"], relabelled_pieces=s["relabelled_pieces"],
                               relabelled_voxels=s["relabelled_voxels"], kept_isolated=s["kept_isolated"],
                               min_voxels=int(min_voxels), connectivity=connectivity)

    # ------------------------------------------------------------------ which voxels belong to one surface
    def _patch_inputs(self, normal_deg, color_tol, normals):
        """``(normals_qv or None, colors_qv or None, cos_min or None, tol2 or None)`` of ``patches`` / ``wand_at``."""
        cos_min, tol2 = patch_thresholds(normal_deg, color_tol)
        n = self._labels_qv.numel()
        normal_qv = feat_qv = None
        if cos_min is not None:
            res = self._normals_last if normals is None and self.faces is None else normals
            if res is None:
                raise ValueError("no normals: call estimate_normals() first (on a mesh it keeps none with the scene: pass its "
                                 "result as normals=), or switch the normal test off with normal_deg=None")
            if not isinstance(res, NormalsResult) or not torch.is_tensor(res.normals_qv) or res.normals_qv.device != self.device \
                    or tuple(res.normals_qv.shape) != (n, 3):
                raise ValueError("normals must be a NormalsResult of this scene (estimate_normals())")
            normal_qv = res.normals_qv.contiguous()
        if tol2 is not None:
            if self._colors_qv is None:
                self._colors_qv = self.colors_full[self._unique_map].contiguous()       # what load_scene fed the backbone
            feat_qv = self._colors_qv
        return normal_qv, feat_qv, cos_min, tol2

    def patches(self, normal_deg=15.0, color_tol=None, connectivity=26, within="all", oriented=False, normals=None):
        """The SMOOTH PATCHES of the scan: voxels that are neighbours under ``connectivity`` belong to one patch when their
        normals differ by at most ``normal_deg`` degrees (``|dot| >= cos_min = float32(cos(radians(normal_deg)))``; with
        ``oriented=True`` the sign counts: ``dot >= cos_min``) and, with ``color_tol``, their colours -- ``colors_full`` of the
        vertex each voxel was made from, what ``load_scene`` fed the backbone -- lie within ``color_tol`` of each other
        (squared distance ``<= float32(color_tol) ** 2``); ``None`` switches a test off, and the colour test is off by
        default (``a3d_similar_pieces``; the rule, fp32 with one rounding per operation, is stated in
        include/agile3d_hip.h).  A patch is a class of the transitive closure -- a CHAIN: a wall is one patch, and so is a
        smoothly curved surface however far it turns; a crease of more than ``normal_deg`` separates.  ``normals``: a
        ``NormalsResult``; ``None`` takes the one ``estimate_normals()`` left with a cloud -- a mesh keeps none, so there it
        must be passed; with neither, ``ValueError``.  ``within`` as in ``grow``: ``"all"``, ``"label"`` (a patch stays inside
        one object of the current labelling), an int32 tensor of keys or a uint8 / bool mask over the voxels.  Returns a
        ``PatchesResult``; ``grow(..., within=r.piece_qv)`` then stays on the patch it starts on, and ``snap(r)`` votes.
        LIMITS: a voxel's normal is blended over its 27-voxel neighbourhood, so the voxels along a crease hold intermediate
        normals and fall out as tiny patches of their own; a voxel without a valid normal (zeros) joins nobody.  The defaults
        (15 degrees, no colour test, 26) are this project's choice and are NOT tuned on real scans.  One library call and ONE
        host round trip (a second of each when there are more than 16384 patches); no session state changes."""
        self._need_scene()
        connectivity = V._connectivity(connectivity)
        keys = self._grow_keys(within)
        normal_qv, feat_qv, cos_min, tol2 = self._patch_inputs(normal_deg, color_tol, normals)
        similar = dict(normals=normal_qv, feats=feat_qv, cos_min=1.0 if cos_min is None else cos_min,
                       tol2=0.0 if tol2 is None else tol2, oriented=oriented)
        ws = V.pieces_workspace(self._labels_qv.numel(), self.device)
        piece_qv, piece_full, recs, n_pieces = self._label_pieces(keys, connectivity, self._click_rows(), lift=True, max_out=16384,
                                                                  workspace=ws, similar=similar)
        per_object = None
        if isinstance(within, str) and within == "label":
            n_ids = max(len(self.click_idx), int(recs["key"].max()) + 1 if len(recs) else 1)
            per_object = np.bincount(recs["key"], minlength=n_ids).astype(np.int64)
        res = PatchesResult(piece_qv=piece_qv, piece_full=piece_full, records=recs, n_pieces=n_pieces, object_pieces=per_object,
                            connectivity=connectivity, normal_deg=normal_deg, cos_min=cos_min, color_tol=color_tol, tol2=tol2,
                            oriented=bool(oriented), within=within if isinstance(within, str) else "keys", workspace=ws)
        return res

    def wand_at(self, result, u, v, normal_deg=15.0, color_tol=None, mode="chain", within="all", connectivity=26, normals=None):
        """The MAGIC WAND: the patch under pixel ``(u, v)`` (column, row) of ``result`` as a selection, or ``None`` where the
        pixel shows nothing -- the vertex resolved as ``grow_at`` resolves it.  ``mode="chain"``: the patch of ``patches()``
        with these thresholds that holds the pixel's voxel (neighbour to neighbour; a curved surface is followed all the way
        round).  ``"seed"``: the connected voxels whose normal and colour lie within the thresholds of THE PIXEL'S VOXEL's own
        -- a paint program's tolerance from the clicked sample; neighbours are then joined whatever they hold (the pairwise
        thresholds are the loosest the library takes: ``cos_min = -1``, ``tol2`` = the largest fp32).  ``"both"``: both
        tests.  Normals are compared unoriented.  ``normal_deg``, ``color_tol``, ``within``, ``connectivity``, ``normals`` as
        in ``patches``.  Returns a ``WandResult``: ``selected`` uint8 [n_full] (``paint``, ``erase``, ``grow``, ``shrink``
        take the result), ``count``, the patch's ``record`` and the partition ``piece_qv``; a voxel that belongs to no patch
        (outside ``within``; under ``"seed"`` / ``"both"`` a voxel without a valid normal) selects nothing.  Like ``grow`` it
        ROUNDS UP TO WHOLE VOXELS.  The defaults are this project's choice and are NOT tuned on real scans.  ONE library
        call; beyond the pixel's small read (and, for ``"seed"`` / ``"both"``, one of the voxel's normal and colour) the
        host round trips of ``patches()``; no session state changes."""
        self._need_scene()
        if mode not in WAND_MODES:
            raise ValueError(f"mode must be one of {WAND_MODES}, not {mode!r}")
        connectivity = V._connectivity(connectivity)
        keys = self._grow_keys(within)
        normal_qv, feat_qv, cos_min, tol2 = self._patch_inputs(normal_deg, color_tol, normals)
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        dev, n_full = self.device, self.coords_full.shape[0]
        row = self.inverse_map[vertex]                                  # stays on the device
        made = dict(mode=mode, normal_deg=normal_deg, color_tol=color_tol, connectivity=connectivity,
                    within=within if isinstance(within, str) else "keys")
        similar = dict(normals=normal_qv, feats=feat_qv, cos_min=-1.0, tol2=float(np.finfo(np.float32).max), oriented=False)
        if mode != "seed":
            similar.update(cos_min=1.0 if cos_min is None else cos_min, tol2=0.0 if tol2 is None else tol2)
        if mode != "chain" and (normal_qv is not None or feat_qv is not None):
            seed = torch.cat([t[row] for t in (normal_qv, feat_qv) if t is not None]).cpu().numpy()     # the voxel's own sample
            if not np.isfinite(seed).all():
                return WandResult(selected=torch.zeros(n_full, dtype=torch.uint8, device=dev), count=0, record=None,
                                  piece_qv=torch.full_like(self._labels_qv, -1), **made)
            if normal_qv is not None:
                similar.update(ref_normal=seed[:3], ref_cos_min=cos_min)
            if feat_qv is not None:
                similar.update(ref_feat=seed[-3:], ref_tol2=tol2)
        kept = {}

        def also(piece_qv, piece_full):
            root = piece_qv[row]
            kept["selected"] = ((piece_full == root) & (root >= 0)).to(torch.uint8)
            return torch.stack([root.to(torch.int64), kept["selected"].sum()])

        piece_qv, _, recs, _, tail = self._label_pieces(keys, connectivity, self._click_rows(), lift=True, max_out=16384,
                                                        similar=similar, also=also)
        root, count = (int(x) for x in tail.view(np.int64))
        k = int(np.searchsorted(recs["root"], root))
        record = recs[k] if root >= 0 and k < len(recs) and recs["root"][k] == root else None
        return WandResult(selected=kept["selected"], count=count, record=record, piece_qv=piece_qv, **made)

    def snap(self, patches=None, min_voxels=8, min_share=(2, 3), paint_cubes=False):
        """The current voxel labelling SNAPPED to smooth patches, without touching the session: every patch of ``patches`` (a
        ``PatchesResult`` of this scene; ``None``: ``patches()`` with its defaults, computed here) with at least
        ``min_voxels`` voxels whose most frequent object (ties: the lowest id) holds at least ``min_share = (num, den)`` of
        its voxels gives ALL its voxels that object -- unless the patch holds a clicked voxel of another object: the snap
        never contradicts a click.  ONE simultaneous step on the labels as they are (``a3d_vote_pieces``); a boundary that
        cuts across a flat table top moves to the table's edge, which ``despeckle`` never does.  Returns a ``SnapResult``:
        ``labels_qv``, ``labels_full`` and ``colors`` (through ``a3d_session_paint``), ``miou`` / ``iou_per_object`` against
        the relabelled ground truth when the scene has one, and the counts of eligible, already uniform, relabelled, blocked
        and below-share patches.  It changes NO session state: ``annotate(result, labels=r.labels_full)`` and
        ``render(colors=r.colors)`` show it.  The defaults (8 voxels, 2/3) are this project's choice and are NOT tuned on real
        scans.  One host round trip (a second when there are more than 4096 eligible patches), after those of ``patches()``
        when it is computed here."""
        self._need_scene()
        dev, scene, n = self.device, self._scene_handle(), self._labels_qv.numel()
        min_voxels, num, den = V.vote_settings(min_voxels, min_share, _N_IDS, 0)[:3]
        patches = self.patches() if patches is None else patches
        held = getattr(patches, "workspace", None)
        if not isinstance(patches, PatchesResult) or held is None or tuple(patches.piece_qv.shape) != (n,) or \
                patches.piece_qv.device != dev:
            raise ValueError("patches must be a PatchesResult of this scene (patches())")
        labels, rows = self._labels_qv, self._click_rows()
        capacity = 4096
        for _ in range(2):
            ws = V.vote_workspace(n, dev, capacity, _N_IDS)
            ws[:held.numel()] = held                                  # the sizes at the roots, as patches() left them
            labels_qv, summary = V.vote_pieces(scene, labels, patches.piece_qv, ws, min_voxels, (num, den), rows, _N_IDS, capacity)
            labels_full, colors = self._launch_paint(labels_qv, paint_cubes)
            self._launch_iou(labels_qv, self.inverse_map)
            packed = torch.cat([self._counts.view(torch.uint8), summary]).cpu().numpy()      # the one host round trip
            host, s = packed[:-V.VOTE_SUMMARY.itemsize].view(np.int64), V.read_vote_summary(packed[-V.VOTE_SUMMARY.itemsize:])
            if not s["err"] & V.VOTE_OVERFLOW:
                break
            capacity = s["eligible_pieces"]
        if s["err"] & V.VOTE_BAD_LABEL or host[3 * _N_IDS] or (int(host[3 * _N_IDS + 1]) & 0xffffffff):
            raise RuntimeError("snap: inverse_map or labels out of range")
        miou, per_obj = self._read_iou(host)
        return SnapResult(labels_full=labels_full, colors=colors, miou=miou, iou_per_object=per_obj, labels_qv=labels_qv,
                          min_voxels=min_voxels, min_share=(num, den), **{k: s[k] for k in s if k != "err"})

    # ------------------------------------------------------------------ correcting by hand
    def region_mask(self, result, polygon=None, stroke=None, radius=None, mask=None, mode="replace"):
        """A region of the screen of ``result`` (a ``RenderResult``) as a mask: uint8 [h, w] on the device, 1 inside
        (``a3d_region_mask``).  ``polygon``: [k, 2] points ``(x, y)`` in pixels, 3 <= k <= 256, filled even-odd -- a lasso; it
        may cross itself and leave the image.  ``stroke``: [k, 2] points, 1 <= k <= 256, joined by segments and widened to
        ``radius`` > 0 pixels -- a brush; one point is a disc.  Exactly one of the two.  The centre of pixel (u, v) is the
        position (u, v).  ``mode``: ``"replace"`` (a new mask, or ``mask`` overwritten), ``"add"`` / ``"subtract"``: the
        region joined to / taken out of ``mask``, in place.  Any uint8 or bool tensor of that shape is as good a mask for
        ``select``: ``ses.label_image(result) == 3`` is "everything that shows as object 3"."""
        self._need_scene()
        if (polygon is None) == (stroke is None):
            raise ValueError("region_mask takes a polygon or a stroke, one of them")
        cam = result.camera
        shape, points = ("polygon", polygon) if stroke is None else ("stroke", stroke)
        return V.region_mask(shape, points, cam.width, cam.height, radius, mode, mask, self.device)

    def select(self, result, mask, through=False, slack=None, section=_RENDERED):
        """The vertices the camera of ``result`` sees inside ``mask`` (uint8 or bool [h, w] on the device: ``region_mask``, or
        any image of the caller's): a ``SelectResult`` (``a3d_select_vertices``).  A vertex is IN VIEW when it lies in front of
        the camera, projects to a pixel of the image and lies on the kept side of every plane of ``section`` (default: the
        section ``result`` was rendered under; ``None``: none; on a mesh too it is the vertex that is tested, and culling plays
        no part -- except on a cloud after ``estimate_normals()``, where a culling section leaves only the vertices it shows
        from the camera's centre).  It is selected when its pixel is set in the mask and -- unless ``through`` -- it lies no more than ``slack``
        world units behind what the pixel shows (``result.t``): the visible side of the scan.  ``through=True`` selects
        everything under the mask, whatever lies in front of it.  The default ``slack`` is the session's voxel size: a vertex
        shares its pixel with its neighbours a voxel away, of which only the nearest is shown.  This is this project's choice
        and is NOT tuned on real scans.  One host round trip; it changes no session state."""
        self._need_scene()
        if result.mesh != (self.faces is not None):
            raise ValueError("the render belongs to another scene")
        sec = result.section if section is _RENDERED else section
        if sec is not None and not isinstance(sec, Section):
            raise TypeError("section must be a Section or None")
        slack = self.voxel_size if slack is None else float(slack)
        if not (np.isfinite(slack) and slack >= 0.0):
            raise ValueError("slack must be finite and >= 0")
        if torch.is_tensor(mask) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)               # (the same bytes: 0 or 1)
        xyz = self.coords_full
        if sec is not None and sec.cull != "none" and self._cloud_culls():      # only the vertices the culled view shows
            xyz = self._cloud_under(sec, None, np.array(result.camera.o[:], np.float32))[0]
        selected, summary = V.select_vertices(xyz, result.camera, mask, None if through else result.t, slack,
                                              None if sec is None or sec.n_planes == 0 else sec.struct(),
                                              summary=self._region_sum[:V.SELECT_SUMMARY.itemsize])
        s = V.read_select_summary(summary.cpu().numpy())                # the one host round trip
        return SelectResult(selected=selected, count=s["selected"], in_view=s["in_view"], through=bool(through), slack=slack)

    def _selection(self, selection):
        sel = selection.selected if isinstance(selection, (SelectResult, GrowResult, WandResult)) else selection
        n = self.coords_full.shape[0]
        if not torch.is_tensor(sel) or sel.device != self.device or sel.dtype not in (torch.uint8, torch.bool) or tuple(sel.shape) != (n,):
            raise ValueError(f"the selection must be a SelectResult, GrowResult or WandResult of this scene, or a uint8 / bool tensor [{n}] on the "
                             "session's device")
        return (sel.view(torch.uint8) if sel.dtype == torch.bool else sel).contiguous()

    def _edit_layer(self, selection, op, obj):
        self._need_scene()
        sel = self._selection(selection)
        n = self.coords_full.shape[0]
        if self._manual is None:
            self._manual = (torch.zeros(n, dtype=torch.uint8, device=self.device), torch.zeros(n, dtype=torch.int32, device=self.device))
        # The model's labels at the vertices: those of the last infer / preview, which every change of the voxels' labels
        # refreshes (_set_clicks); there are none only while every voxel is still background.
        model = self._labels_last if self._labels_last is not None else torch.zeros(n, dtype=torch.int32, device=self.device)
        summary = V.session_overlay(model, *self._manual, sel, op, obj, summary=self._region_sum)[2]
        s = V.read_overlay_summary(summary.cpu().numpy())
        if s["err"]:
            raise RuntimeError("a3d_session_overlay: a label outside 0 .. 255")
        return s["changed"]

    def paint(self, selection, obj):
        """Says "these vertices belong to object ``obj``": the manual layer takes ``obj`` -- 0 (background) or the id of an object
        that has a click; ``ValueError`` otherwise -- on every vertex of ``selection`` (a ``SelectResult``, or a uint8 / bool
        tensor [n_full] on the device; one of another scene's length raises ``ValueError``).  The model is not run and its
        labels are not touched: ``corrected()`` lays the layer over them.  The layer follows the click list: ``load_scene``
        and ``reset`` clear it, and whatever renumbers the objects (``remove_click``, ``undo``, ``redo``) renumbers the paint
        by the same table -- a removed object's paint becomes background.  Returns how many vertices' layer entry changed.
        One host round trip."""
        obj = int(obj)
        if not 0 <= obj <= len(self.click_idx) - 1:
            raise ValueError(f"object {obj}: paint takes 0 (background) or an existing object id 1 .. {len(self.click_idx) - 1}")
        return self._edit_layer(selection, "paint", obj)

    def erase(self, selection):
        """Takes the manual layer off the vertices of ``selection``: they show the model's labels again.  Returns how many
        vertices' layer entry changed.  One host round trip."""
        return self._edit_layer(selection, "erase", 0)

    # ------------------------------------------------------------------ along the surface
    def _grow_keys(self, within):
        """The keys ``a3d_grow_voxels`` walks by (``None``: walk anywhere) of ``grow(within=)``."""
        n = self._labels_qv.numel()
        if isinstance(within, str):
            if within == "all":
                return None
            if within == "label":
                return self._labels_qv
        elif torch.is_tensor(within) and within.device == self.device and tuple(within.shape) == (n,):
            if within.dtype == torch.int32:
                return within.contiguous()
            if within.dtype in (torch.uint8, torch.bool):
                return (within != 0).to(torch.int32) - 1            # a mask: key 0 inside, -1 outside
        raise ValueError(f'within must be "all", "label", an int32 tensor [{n}] of keys or a uint8 / bool tensor [{n}] (a mask) on '
                         "the session's device")

    def _grow_seeds(self, seeds):
        """``(seed_qv, seed_full)`` of ``grow(seeds)``: one of the two is ``None``."""
        if isinstance(seeds, (SelectResult, GrowResult, WandResult)) or torch.is_tensor(seeds):
            return None, self._selection(seeds)
        n = self._labels_qv.numel()
        if isinstance(seeds, str):
            if seeds != "clicks":
                raise ValueError('seeds: the only name is "clicks"')
            rows = self._click_rows()
        else:
            try:
                rows = [int(r) for r in seeds]
            except (TypeError, ValueError):
                raise ValueError('seeds must be a SelectResult / GrowResult, a uint8 / bool tensor over the vertices, "clicks" or a '
                                 "list of voxel rows") from None
            if any(not 0 <= r < n for r in rows):
                raise ValueError(f"seeds: a voxel row outside 0 .. {n - 1}")
        seed_qv = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if rows:
            seed_qv[torch.tensor(rows, dtype=torch.int64).to(self.device)] = 1
        return seed_qv, None

    def _grow(self, seed_qv, seed_full, cost, limit, keys, connectivity, within):
        """``a3d_grow_voxels`` on the session's voxels, lifted to its vertices: ONE library call, ONE host round trip."""
        n_full = self.coords_full.shape[0]
        if self._grow_ws is None:
            self._grow_ws = V.grow_workspace(self._labels_qv.numel(), self.device)
        dist_qv, owner_qv, selected, dist_full, summary, _ = V.grow_voxels(
            self._scene_handle(), n_full, keys, seed_qv, seed_full, self.inverse_map, cost, limit, connectivity,
            summary=self._region_sum[:V.GROW_SUMMARY.itemsize], workspace=self._grow_ws)
        s = V.read_grow_summary(summary.cpu().numpy())                  # the one host round trip
        if s["err"] & V.GROW_BAD_INDEX:
            raise RuntimeError("a3d_grow_voxels: inverse_map out of range")
        unit = self.voxel_size / 1024.0 if cost == V.GROW_METRIC_COST else self.voxel_size
        return GrowResult(selected=selected, dist_full=dist_full, dist_qv=dist_qv, owner_qv=owner_qv, count=s["selected"],
                          reached_voxels=s["reached"], seeds=s["seeds"], max_distance=s["max_dist"] * unit, limit=limit,
                          cost=cost, connectivity=connectivity, within=within if isinstance(within, str) else "keys")

    def grow(self, seeds, radius=None, steps=None, within="all", connectivity=26):
        """Grows a selection ALONG THE SURFACE: everything within a distance of ``seeds``, the distance measured as the
        cheapest walk over neighbouring voxels, not across the screen or through the air (``a3d_grow_voxels``; the adjacency is
        the scene's own neighbour table, as in ``pieces()``).  ``seeds``: a ``SelectResult`` / ``GrowResult``, a uint8 / bool
        tensor [n_full] on the device (the voxels that hold a selected vertex are the seeds), ``"clicks"`` (the clicked voxels)
        or a list of voxel rows.  Exactly one of ``radius`` (world units >= 0: face, edge and corner steps cost 1024, 1448 and
        1774 = round(1024 (1, sqrt 2, sqrt 3)), and the walk may cost ``floor(radius / voxel_size * 1024)``, computed in
        float64) and ``steps`` (an int >= 0: every step costs 1).  More than ``view.GROW_MAX_STEPS`` voxel steps raise
        ``ValueError``: ``pieces()`` answers what is connected at all.  ``within``: ``"all"`` walks anywhere; ``"label"``
        stays inside the object of each seed -- the labels ``preview()`` paints; an int32 tensor [n_voxels] of keys walks
        between equal keys >= 0 -- ``patches().piece_qv`` keeps the walk on the smooth patch it starts on --; a uint8 / bool
        tensor [n_voxels] is a mask to stay inside.  ``connectivity``: 6, 18 or 26.
        Returns a ``GrowResult``: the selected vertices (``paint`` / ``erase`` take it), the distance of every vertex and
        voxel, and for every voxel the seed voxel nearest to it -- ``grow("clicks", ..., within="label")`` splits each object
        between its clicks.  A selection is ROUNDED UP TO WHOLE VOXELS: every vertex of a reached voxel is selected.  The
        voxel lattice is the resolution at which labels live; a mesh's own edges are not walked.  The costs and the default
        ``within`` are this project's choice and are NOT tuned on real scans.  One library call, one host round trip; it
        changes no session state."""
        self._need_scene()
        cost, limit = grow_limit(radius, steps, self.voxel_size)
        connectivity = V._connectivity(connectivity)
        keys = self._grow_keys(within)
        seed_qv, seed_full = self._grow_seeds(seeds)
        return self._grow(seed_qv, seed_full, cost, limit, keys, connectivity, within)

    def grow_at(self, result, u, v, radius=None, steps=None, within="label", connectivity=26):
        """The SURFACE BRUSH: ``grow`` from the vertex that pixel ``(u, v)`` (column, row) of ``result`` shows -- resolved as
        ``piece_at`` / ``confidence_at`` resolve it: the pixel's vertex on a cloud, the heaviest corner of its face on a mesh
        -- or ``None`` where the pixel shows nothing.  With the default ``within="label"`` the brush stays on the object under
        the pointer: over the edge of a chair's seat it does not take the floor that shows beside it.  That default is this
        project's choice and is NOT tuned on real scans.  One small device-to-host copy, then as ``grow``."""
        self._need_scene()
        cost, limit = grow_limit(radius, steps, self.voxel_size)
        connectivity = V._connectivity(connectivity)
        keys = self._grow_keys(within)
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        seed_full = torch.zeros(self.coords_full.shape[0], dtype=torch.uint8, device=self.device)
        seed_full[vertex] = 1
        return self._grow(None, seed_full, cost, limit, keys, connectivity, within)

    def shrink(self, selection, radius=None, steps=None, connectivity=26):
        """Pulls a selection IN by a margin (``radius`` or ``steps`` as in ``grow``).  The voxels that hold no selected vertex
        are the OUTSIDE (found by one ``grow`` at limit 0); a selected vertex stays when its voxel is NOT reached from the
        outside within the limit (a second ``grow``, seeded with the outside, walking anywhere).  Returns a ``GrowResult``
        whose ``selected`` is the eroded set and ``count`` its size; its distances and owners are the second call's, measured
        from the outside.  Like ``grow`` it ROUNDS A SELECTION UP TO WHOLE VOXELS: a voxel with one selected vertex is inside
        as a whole, so ``shrink(grow(s, steps=k), steps=k)`` keeps every vertex of ``s`` whose voxel is not near the border of
        the scene's own surface, and may keep more.  Two library calls, three host round trips; no session state changes."""
        self._need_scene()
        cost, limit = grow_limit(radius, steps, self.voxel_size)
        connectivity = V._connectivity(connectivity)
        sel = self._selection(selection)
        held = self._grow(None, sel, cost, 0, None, connectivity, "all")
        outside = (held.dist_qv < 0).to(torch.uint8)
        res = self._grow(outside, None, cost, limit, None, connectivity, "all")
        res.selected = ((sel != 0) & (res.selected == 0)).to(torch.uint8)
        res.count = int(res.selected.sum().cpu())
        return res

    def manual_labels(self):
        """``(on uint8 [n_full], obj int32 [n_full])``: copies of the manual layer on the device -- ``on`` 1 where a vertex is
        overridden, ``obj`` the object it is given (0 elsewhere).  For a caller's own history, or a file."""
        self._need_scene()
        n = self.coords_full.shape[0]
        if self._manual is None:
            return torch.zeros(n, dtype=torch.uint8, device=self.device), torch.zeros(n, dtype=torch.int32, device=self.device)
        on, obj = self._manual                          # (an erased vertex keeps its last object in the layer: not shown here)
        return on.clone(), torch.where(on != 0, obj, torch.zeros_like(obj))

    def set_manual(self, on, obj):
        """Makes ``(on, obj)`` -- as ``manual_labels()`` returns them; ``on`` uint8 or bool -- the manual layer.  ``obj`` is
        looked at only where ``on`` is set and must lie in 0..255 there (``ValueError``, the layer as it was); ids are not
        checked against the click list, as a file may be restored before its clicks.  One host round trip."""
        self._need_scene()
        n = self.coords_full.shape[0]
        for name, t, kinds in (("on", on, (torch.uint8, torch.bool)), ("obj", obj, (torch.int32,))):
            if not torch.is_tensor(t) or t.device != self.device or t.dtype not in kinds or tuple(t.shape) != (n,):
                raise ValueError(f"{name} must be a tensor [{n}] on the session's device (on: uint8 or bool, obj: int32)")
        new_on = (on != 0).to(torch.uint8)
        new_obj = torch.where(on != 0, obj, torch.zeros_like(obj))      # (what is off holds 0: a later renumbering reads every entry)
        summary = V.session_overlay(new_obj, new_on, new_obj, summary=self._region_sum)[2]     # its range check, nothing written
        if V.read_overlay_summary(summary.cpu().numpy())["err"]:
            raise ValueError("obj must lie in 0 .. 255 where on is set")
        self._manual = (new_on, new_obj)
        return self

    def corrected(self):
        """The labelling as corrected by hand: the current voxel labels -- those ``preview()`` paints -- lifted to the vertices
        with the manual layer laid over them (``a3d_session_overlay``): a ``CorrectedResult`` with ``labels_full``, ``colors``
        (the palette's, no click cubes), ``miou`` / ``iou_per_object`` against the relabelled ground truth when the scene has
        one, and how many vertices the layer holds and changes.  With an empty layer ``labels_full`` is ``preview()``'s.
        ``annotate(result, labels=r.labels_full)``, ``render(colors=r.colors)`` and ``measure(labels=r.labels_full)`` take it.
        It changes no session state.  One host round trip."""
        self._need_scene()
        n = self.coords_full.shape[0]
        model = self._launch_paint(self._labels_qv, False)[0]
        layer = self._manual
        if layer is None:
            layer = (torch.zeros(n, dtype=torch.uint8, device=self.device), torch.zeros(n, dtype=torch.int32, device=self.device))
        labels_full, colors, summary = V.session_overlay(model, *layer, colors=self.colors_full, palette=self._palette_dev,
                                                         summary=self._region_sum)
        self._launch_iou(labels_full, None)
        packed = torch.cat([self._counts.view(torch.uint8), summary]).cpu().numpy()      # the one host round trip
        host, s = packed[:-V.OVERLAY_SUMMARY.itemsize].view(np.int64), V.read_overlay_summary(packed[-V.OVERLAY_SUMMARY.itemsize:])
        if s["err"] or host[3 * _N_IDS] or (int(host[3 * _N_IDS + 1]) & 0xffffffff):
            raise RuntimeError("corrected: inverse_map or labels out of range")
        miou, per_obj = self._read_iou(host)
        return CorrectedResult(labels_full=labels_full, colors=colors, miou=miou, iou_per_object=per_obj,
                               overridden=s["overridden"], differing=s["differing"])

    # ------------------------------------------------------------------ how big an object is
    def _fixed_point_frame(self):
        """``(origin float64 [3], quantum, bits)`` of the scene, once per scene: the origin is the centre of the box of the finite
        vertices, ``quantum = 2^(e - bits)`` with ``2^e`` >= the largest half extent -- so every vertex lies within ``2^bits``
        quanta of the origin -- and ``bits`` the largest value up to 20 with ``n * 2^(2 bits) <= 2^62``."""
        if self._measure_frame is None:
            p = self._coords_host[np.isfinite(self._coords_host).all(1)].astype(np.float64)
            lo, hi = (p.min(0), p.max(0)) if len(p) else (np.zeros(3), np.zeros(3))
            origin = 0.5 * (lo + hi)
            half = float(np.maximum(hi - origin, origin - lo).max())
            e = int(np.ceil(np.log2(half))) if half > 0 else 0
            while 2.0 ** e < half:                    # (log2 rounds: make sure of the property itself)
                e += 1
            n = max(int(self._coords_host.shape[0]), 1)
            bits = min(L.A3D_MEASURE_MAX_BITS, (62 - (n - 1).bit_length()) // 2)
            self._measure_frame = (origin, 2.0 ** (e - bits), bits)
        return self._measure_frame

    def measure(self, labels=None, oriented=True):
        """The OBJECTS of a labelling, measured: per object id its vertices and voxels, centroid, exact axis-aligned box,
        covariance, the surface it covers (a mesh scene; ``None`` on a cloud), the volume of its occupied voxels and, with
        ``oriented=True``, the box along its principal axes.  Valid from ``load_scene`` on; it changes NO session state.  By
        default the current full-resolution labelling is measured -- the voxel labels ``preview()`` paints, lifted through the
        inverse map -- else ``labels``: int32 [n_full] on the device with object ids 0..255 (the ground truth, or
        ``despeckle().labels_full``); a voxel then carries the label of the vertex it was made from.

        One ``a3d_measure_objects`` call accumulates exact integers on the device (counts, fixed-point first and second
        moments about the centre of the scene's box, minima and maxima, face areas in quanta); ``object_table`` turns them into
        world units on the host and ``principal_axes`` into axes (PCA of the vertices: the stated definition, not a
        minimum-volume box); a second call, ``a3d_object_extents``, projects every vertex on its object's axes.  ONE host round
        trip, TWO with ``oriented=True``.  An error bit (a label outside 0..255, a coordinate that is not finite) raises
        ``RuntimeError``.  Returns a ``MeasureResult``."""
        self._need_scene()
        dev, n_full = self.device, self.coords_full.shape[0]
        if labels is None:
            labels_qv = self._labels_qv
            labels = labels_qv[self.inverse_map]
        else:
            if not torch.is_tensor(labels) or labels.dtype is not torch.int32 or tuple(labels.shape) != (n_full,) or labels.device != dev:
                raise ValueError(f"labels must be an int32 tensor [{n_full}] on {dev}")
            labels = labels.contiguous()
            labels_qv = labels[self._unique_map]
        origin, quantum, bits = self._fixed_point_frame()
        area_quantum = quantum * quantum * 256.0 if self.faces is not None else None
        rec_bytes = _N_IDS * V.OBJECT_MOMENTS.itemsize
        buf = torch.empty(rec_bytes + 8, dtype=torch.uint8, device=dev)
        V.measure_objects(self.coords_full, labels, origin, quantum, bits, _N_IDS, labels_qv=labels_qv, faces=self.faces,
                          area_quantum=area_quantum, records=buf[:rec_bytes], err=buf[rec_bytes:rec_bytes + 4].view(torch.int32))
        host = buf.cpu().numpy()                                          # the one host round trip
        err = int(host[rec_bytes:rec_bytes + 4].view(np.int32)[0])
        if err:
            raise RuntimeError(f"a3d_measure_objects: labels outside 0 .. {_N_IDS - 1} or coordinates out of range (error word {err})")
        moments = V.read_object_moments(host[:rec_bytes])
        used = np.flatnonzero((moments["vertices"] > 0) | (moments["voxels"] > 0))
        k = max(len(self.click_idx), int(used.max()) + 1 if len(used) else 1)
        moments = moments[:k]
        t = object_table(moments, origin, quantum, area_quantum, self.voxel_size)
        res = MeasureResult(vertices=t["vertices"], voxels=t["voxels"], centroid=t["centroid"], lo=moments["lo"].copy(),
                            hi=moments["hi"].copy(), cov=t["cov"], area=t["area"], volume=t["volume"], origin=origin,
                            quantum=quantum, bits=bits, area_quantum=area_quantum, moments=moments)
        if oriented:
            axes32 = np.tile(np.eye(3, dtype=np.float32), (_N_IDS, 1, 1))
            axes32[:k] = principal_axes(t["cov"], t["vertices"])[0].astype(np.float32)
            out = torch.empty(_N_IDS * 6 + 1, dtype=torch.float32, device=dev)
            V.object_extents(self.coords_full, labels, torch.from_numpy(axes32).to(dev), extents=out[:_N_IDS * 6].view(_N_IDS, 3, 2),
                             err=out[_N_IDS * 6:].view(torch.int32))
            host = out.cpu().numpy()                                      # the second host round trip
            if int(host[_N_IDS * 6:].view(np.int32)[0]):
                raise RuntimeError("a3d_object_extents: labels or coordinates out of range")
            span = host[:_N_IDS * 6].reshape(_N_IDS, 3, 2)[:k].astype(np.float64)
            axes = axes32[:k].astype(np.float64)
            empty = t["vertices"] == 0
            with np.errstate(invalid="ignore"):
                mid, size = 0.5 * (span[..., 0] + span[..., 1]), span[..., 1] - span[..., 0]
            mid[empty], size[empty] = np.nan, 0.0
            res.axes, res.extents = axes, size
            res.centre = np.einsum("kj,kjc->kc", mid, axes)
        return res

    def frame(self, obj, width, height, fov_deg=35.0, measure=None):
        """``(intrinsic, extrinsic)`` of a camera that frames object ``obj``: ``framing_view`` on the 8 corners of its
        axis-aligned box, so every vertex of the object has camera-space z > 0 and projects inside the image.  ``measure``: a
        ``MeasureResult`` of this scene (default: ``measure(oriented=False)`` of the current labelling, computed here).
        ``ValueError`` for an object without a vertex."""
        self._need_scene()
        m = self.measure(oriented=False) if measure is None else measure
        obj = int(obj)
        if not 0 <= obj < len(m.vertices) or m.vertices[obj] == 0:
            raise ValueError(f"object {obj} has no vertex")
        lo, hi = m.lo[obj].astype(np.float64), m.hi[obj].astype(np.float64)
        corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
        return framing_view(corners, width, height, fov_deg)

    def _vertex_at(self, result, u, v):
        """The vertex that pixel ``(u, v)`` of ``result`` shows (-1: none): on a cloud the pixel's vertex, on a mesh the
        heaviest corner of its face (``a3d_render_labels`` over the vertices' own indices).  One small device-to-host copy."""
        if result.mesh != (self.faces is not None):
            raise ValueError("the render belongs to another scene")
        n = self.coords_full.shape[0]
        u, v = int(u), int(v)
        h, w = result.ids.shape
        if not (0 <= u < w and 0 <= v < h):
            raise ValueError(f"pixel ({u}, {v}) outside the {w} x {h} image")
        if self._vertex_ids is None:
            self._vertex_ids = torch.arange(n, dtype=torch.int32, device=self.device)
        one = lambda image: None if image is None else image[v:v + 1, u:u + 1]
        return int(V.render_labels(one(result.ids), one(result.u), one(result.v), self.faces, self._vertex_ids,
                                   out=self._small[20:21].view(1, 1)).cpu())

    def confidence_at(self, result, u, v, guide=None):
        """The margin (a float; ``inf`` on a clicked voxel's vertices) of the vertex that pixel ``(u, v)`` (column, row) of
        ``result`` shows, or ``None`` where the pixel shows nothing: on a cloud the pixel's vertex, on a mesh the heaviest
        corner of its face -- the vertex whose object ``object_at`` reports (``a3d_render_labels`` over the vertices' own
        indices).  ``guide``: a ``GuideResult`` of this scene (default: the last ``guide()``'s; ``ValueError`` when the clicks
        or the scene changed since).  Two small device-to-host copies."""
        self._need_scene()
        guide = self._guide_last if guide is None else guide
        if guide is None:
            raise ValueError("confidence_at() reads the last guide(): there is none, or the clicks or the scene changed since")
        if result.mesh != (self.faces is not None):
            raise ValueError("the render belongs to another scene")
        if tuple(guide.margin_full.shape) != (self.coords_full.shape[0],):
            raise ValueError("the guide belongs to another scene")
        vertex = self._vertex_at(result, u, v)
        return None if vertex < 0 else float(guide.margin_full[vertex].cpu())

    # ------------------------------------------------------------------ which way the surface faces
    def estimate_normals(self, viewpoint="centre"):
        """One normal per voxel from the vertices of its 3 x 3 x 3 neighbourhood, lifted to the vertices
        (``a3d_estimate_normals``: exact integer moments in the fixed-point frame of ``measure()``, then one fixed sequence of
        double operations per voxel -- two calls give the same bytes).  ``viewpoint``: a point [x, y, z] the normals are
        turned towards; ``"centre"``, the centre of the scene's bounding box -- right for the walls, floor and ceiling of a
        room scanned from inside, and this project's choice, not tuned on real scans; or ``None``: the canonical sign (the
        component of largest magnitude positive).  A voxel whose neighbourhood holds fewer than 3 vertices, or only a line
        of them, gets no normal (zeros).  All vertices of a voxel share its normal: shading is faceted at the voxel size.

        On a CLOUD the normals are kept with the scene (``ses.normals``; ``load_scene`` drops them, ``reset`` keeps them, a
        second call replaces them): from then on ``render(lit=True)`` lights the cloud by them and a ``Section`` with
        ``cull="back"`` / ``"front"`` is accepted by ``pick``, ``click_ray``, ``render`` and ``select``, which run on the copy
        of the cloud culled for the call's eye -- the ray's origin, the camera's centre (``a3d_cull_points``; a few copies are
        kept, one per eye and mode).  On a MESH the result is returned and no session state changes: a mesh is lit and
        culled by its faces.  One host round trip (the summary).  Returns a ``NormalsResult``."""
        self._need_scene()
        origin, quantum, bits = self._fixed_point_frame()
        if viewpoint is None:
            vp = None
        elif isinstance(viewpoint, str):
            if viewpoint != "centre":
                raise ValueError("viewpoint must be a point, 'centre' or None")
            vp = np.array(origin, np.float64)
        else:
            vp = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
            if vp.shape != (3,) or not np.isfinite(vp).all():
                raise ValueError("viewpoint must be three finite numbers, 'centre' or None")
        normal_qv, variation_qv, count_qv, _, normal_full, summary, _ = V.estimate_normals(
            self._scene_handle(), self.coords_full, origin, quantum, bits, inverse_map=self.inverse_map, viewpoint=vp,
            moments_qv=False, summary=self._region_sum[:V.NORMALS_SUMMARY.itemsize])
        s = V.read_normals_summary(summary.cpu().numpy())               # the one host round trip
        if s["err"] & V.NORMALS_BAD_INDEX:
            raise RuntimeError("a3d_estimate_normals: inverse_map out of range")
        res = NormalsResult(normals_full=normal_full, normals_qv=normal_qv, variation_qv=variation_qv, count_qv=count_qv,
                            counted=s["counted"], valid=s["valid"], invalid=s["invalid"], err=s["err"], viewpoint=vp)
        if self.faces is None:
            self.normals, self._normals_last, self._culled = normal_full, res, {}
        return res

    def normal_at(self, result, u, v, normals=None):
        """``(normal fp32 [3], variation)`` of the vertex that pixel ``(u, v)`` (column, row) of ``result`` shows, or ``None``
        where the pixel shows nothing: on a cloud the pixel's vertex, on a mesh the heaviest corner of its face, as
        ``confidence_at`` resolves it.  ``normals``: a ``NormalsResult`` of this scene (default: the one ``estimate_normals()``
        left with a cloud; ``ValueError`` when there is none).  A vertex whose voxel has no valid normal gives zeros and 0.
        Two small device-to-host copies."""
        self._need_scene()
        normals = self._normals_last if normals is None else normals
        if not isinstance(normals, NormalsResult):
            raise ValueError("normal_at() reads a NormalsResult: estimate_normals() first (on a mesh, pass its result)")
        if tuple(normals.normals_full.shape) != (self.coords_full.shape[0], 3) or \
                tuple(normals.variation_qv.shape) != (self.raw_coords_qv.shape[0],):
            raise ValueError("the normals belong to another scene")
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        row = self.inverse_map[vertex]
        both = torch.cat([normals.normals_full[vertex], normals.variation_qv[row].reshape(1)]).cpu().numpy()
        return both[:3].copy(), float(both[3])

    # ------------------------------------------------------------------ one sign for a whole surface
    def _orient_source(self, normals):
        res = self._normals_last if normals is None and self.faces is None else normals
        if res is None:
            raise ValueError("no normals: call estimate_normals() first (on a mesh it keeps none with the scene: pass its result "
                             "as normals=)")
        n = self.raw_coords_qv.shape[0]
        if not isinstance(res, NormalsResult) or not torch.is_tensor(res.normals_qv) or res.normals_qv.device != self.device \
                or tuple(res.normals_qv.shape) != (n, 3):
            raise ValueError("normals must be a NormalsResult of this scene (estimate_normals())")
        return res

    def _orient_seeds(self, seeds):
        """``seed_qv`` uint8 [n_voxels] of ``orient_normals(seeds=)`` other than ``"nearest"``."""
        n = self.raw_coords_qv.shape[0]
        if isinstance(seeds, (SelectResult, GrowResult, WandResult)):
            seed_qv = torch.zeros(n, dtype=torch.uint8, device=self.device)
            seed_qv[self.inverse_map[self._selection(seeds) != 0]] = 1
            return seed_qv
        if torch.is_tensor(seeds):
            if seeds.device != self.device or seeds.dtype not in (torch.uint8, torch.bool) or tuple(seeds.shape) != (n,):
                raise ValueError(f"a seed mask must be a uint8 / bool tensor [{n}] over the voxels on the session's device")
            return (seeds != 0).to(torch.uint8)
        try:
            rows = [int(r) for r in seeds]
        except (TypeError, ValueError):
            raise ValueError('seeds must be "nearest", a SelectResult / GrowResult, a uint8 / bool mask over the voxels or a list '
                             "of voxel rows") from None
        if any(not 0 <= r < n for r in rows):
            raise ValueError(f"seeds: a voxel row outside 0 .. {n - 1}")
        seed_qv = torch.zeros(n, dtype=torch.uint8, device=self.device)
        if rows:
            seed_qv[torch.tensor(rows, dtype=torch.int64).to(self.device)] = 1
        return seed_qv

    def _orient(self, src, connectivity, sweeps, **seeds):
        """``a3d_orient_normals`` until it has converged: one library call and ONE host round trip (the summary) per batch of
        ``sweeps``; then, on a cloud, the oriented normals become the scene's."""
        n = self.raw_coords_qv.shape[0]
        nrm = src.normals_qv.contiguous()
        outs, launched, ws = None, 0, None
        for batch in range(n // sweeps + 2):                            # (a path has fewer than n edges: n sweeps always suffice)
            outs = V.orient_normals(self._scene_handle(), nrm, connectivity=connectivity, sweeps=sweeps, resume=batch > 0,
                                    inverse_map=self.inverse_map, workspace=ws,
                                    **(dict(zip(("normal_out_qv", "flipped_qv", "dist_qv", "owner_qv", "normal_full"), outs[:5]))
                                       if outs else {}), **seeds)
            ws = outs[6]
            launched += sweeps
            s = V.read_orient_summary(outs[5].cpu().numpy())            # the one host round trip of the batch
            if s["err"] & V.ORIENT_BAD_INDEX:
                raise RuntimeError("a3d_orient_normals: inverse_map out of range")
            if s["converged"]:
                break
        else:
            raise RuntimeError("a3d_orient_normals did not converge")
        normal_qv, flipped_qv, dist_qv, owner_qv, normal_full = outs[:5]
        kept = NormalsResult(normals_full=normal_full, normals_qv=normal_qv, variation_qv=src.variation_qv, count_qv=src.count_qv,
                             counted=src.counted, valid=src.valid, invalid=src.invalid, err=src.err, viewpoint=src.viewpoint)
        if self.faces is None:
            self.normals, self._normals_last, self._culled = normal_full, kept, {}
        return OrientResult(normals_full=normal_full, normals_qv=normal_qv, flipped_qv=flipped_qv, dist_qv=dist_qv,
                            owner_qv=owner_qv, launched=launched, connectivity=connectivity, result=kept,
                            **{k: s[k] for k in ("admitted", "seeds", "reached", "unreached", "flipped", "conflicts", "max_dist",
                                                 "err")})

    def orient_normals(self, seeds="nearest", viewpoint="centre", connectivity=26, normals=None, sweeps=512):
        """Gives the normals ONE CONSISTENT SIGN per connected surface, by propagation (``a3d_orient_normals``; the rule is
        stated in include/agile3d_hip.h).  ``estimate_normals()`` signs every voxel by one viewpoint, which is right for the
        walls of a room seen from inside and wrong for the far sides of whatever stands in it.  Here a trusted sign starts
        at SEED voxels and is carried from neighbour to neighbour (``connectivity`` 6, 18 or 26) along the cheapest path --
        an edge costs 1 where the two normals are parallel and up to 1024 where they are perpendicular, so the sign travels
        along smooth surface and crosses creases last -- and is turned wherever two neighbours disagree.
        ``seeds="nearest"``: per connected component of the voxels that have a normal (``a3d_label_pieces``) the voxel
        nearest to ``viewpoint`` -- a point, or ``"centre"``, the centre of the scene's box -- is the seed and is turned
        towards it.  Or the seeds are voxels whose sign is TRUSTED AS IT STANDS: a ``SelectResult`` / ``GrowResult`` (the
        voxels that hold a selected vertex), a uint8 / bool mask over the voxels, or a list of voxel rows; ``viewpoint`` then
        plays no part.  ``normals``: a ``NormalsResult``; ``None`` takes the one ``estimate_normals()`` left with a cloud
        (``ValueError`` when there is none, or when it belongs to another scene).
        On a CLOUD the oriented normals replace ``ses.normals`` and the culled copies are dropped, exactly as a second
        ``estimate_normals()`` does: ``render(lit=True)``, a ``Section`` with ``cull=`` and ``patches(oriented=True)`` see
        them from then on.  On a MESH the result is returned and no session state changes.
        ``sweeps`` (1 .. 4096) relaxation sweeps are launched per library call and the call is repeated, resuming, while it
        has not converged: ``ceil(depth / sweeps)`` calls and as many host round trips (one summary each), where depth is
        the largest number of edges on a seed's cheapest path -- one round trip on a room at the default.  The component
        labelling of ``"nearest"`` adds none.  Returns an ``OrientResult``.
        LIMITS: a shortest-path tree, not a minimum spanning tree; one normal per voxel, so a plate one voxel thick has one
        side; the cost scale, the ``"nearest"`` seed and the 26-connectivity default are this project's choices and are NOT
        tuned on real scans."""
        self._need_scene()
        connectivity = V._connectivity(connectivity)
        sweeps = V._int_in("sweeps", sweeps, 1, V.ORIENT_MAX_SWEEPS)
        src = self._orient_source(normals)
        if isinstance(seeds, str):
            if seeds != "nearest":
                raise ValueError('seeds: the only name is "nearest"')
            if isinstance(viewpoint, str):
                if viewpoint != "centre":
                    raise ValueError("viewpoint must be a point or 'centre'")
                vp = np.array(self._fixed_point_frame()[0], np.float64)
            else:
                vp = np.asarray(viewpoint, dtype=np.float64).reshape(-1)
                if vp.shape != (3,) or not np.isfinite(vp).all():
                    raise ValueError("viewpoint must be three finite numbers or 'centre'")
            nrm = src.normals_qv
            has = torch.isfinite(nrm).all(1) & (nrm != 0).any(1)
            comp = V.label_pieces(self._scene_handle(), has.to(torch.int32) - 1, connectivity,
                                  records=torch.empty(V.PIECE.itemsize, dtype=torch.uint8, device=self.device))[0]
            return self._orient(src, connectivity, sweeps, components=comp, positions=self.raw_coords_qv, viewpoint=vp)
        return self._orient(src, connectivity, sweeps, seed_qv=self._orient_seeds(seeds))

    def orient_at(self, result, u, v, normals=None, connectivity=26, sweeps=512):
        """THIS SURFACE FACES ME: orients from the voxel of the vertex that pixel ``(u, v)`` (column, row) of ``result`` shows --
        resolved as ``normal_at`` resolves it -- with its normal turned towards the camera's eye.  Only the voxels that seed
        reaches change; every other voxel keeps its bytes.  Returns an ``OrientResult`` as ``orient_normals`` does (and
        keeps it with a cloud in the same way), or ``None`` where the pixel shows nothing.  One small device-to-host copy,
        then as ``orient_normals``."""
        self._need_scene()
        connectivity = V._connectivity(connectivity)
        sweeps = V._int_in("sweeps", sweeps, 1, V.ORIENT_MAX_SWEEPS)
        src = self._orient_source(normals)
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        n = self.raw_coords_qv.shape[0]
        row = self.inverse_map[vertex]
        eye = torch.tensor([float(c) for c in result.camera.o[:]], dtype=torch.float64, device=self.device)
        towards = (src.normals_qv[row].to(torch.float64) * (eye - self.coords_full[vertex].to(torch.float64))).sum()
        seed_qv = torch.zeros(n, dtype=torch.uint8, device=self.device)
        seed_qv[row] = 1
        seed_flip = torch.zeros(n, dtype=torch.uint8, device=self.device)
        seed_flip[row] = (towards < 0).to(torch.uint8)
        return self._orient(src, connectivity, sweeps, seed_qv=seed_qv, seed_flip=seed_flip)

    # ------------------------------------------------------------------ the planes a room is made of
    def planes(self, normal_deg=20.0, dist_tol=None, min_voxels=200, max_planes=16, within="all", normals=None, up=(0, 0, 1)):
        """The few global PLANES the scan is made of -- floor, ceiling, walls, table tops --, their equations and the voxels on
        each (``a3d_find_planes``; the rule is stated in include/agile3d_hip.h).  Every voxel with a normal votes, in integers,
        for one cell of a Hough array over (direction, offset); round by round the strongest cell seeds a plane, which is
        fitted from exact integer sums, refitted twice from its inliers -- the voxels within ``dist_tol`` (world units;
        ``None``: 1.5 voxels) whose normal lies within ``normal_deg`` degrees of the plane's -- and recorded when it holds at
        least ``min_voxels`` voxels; at most ``max_planes`` (1 .. 16).  Unlike ``patches()``, which chains neighbours, a wall
        behind a shelf is ONE plane, and every plane has an equation.  The offset bins are one voxel wide.
        ``normals``: a ``NormalsResult``; ``None`` takes the one ``estimate_normals()`` left with a cloud -- a mesh keeps none,
        so there it must be passed; with neither, ``ValueError``.  ``within``: ``"all"``, ``"label"`` (background voxels
        only), an int32 tensor of keys over the voxels (keys >= 0 take part) or a uint8 / bool mask.  ``up`` names the
        planes (``plane_kinds``) and plays no part in finding them.  Returns a ``PlanesResult``: ``selection(k)`` for
        ``paint`` / ``grow``, ``section(k, ...)`` for ``set_section``, ``upright()`` for a tilted scan; ``grow(...,
        within=r.plane_qv)`` stays on a plane, and ``pieces(labels=...)`` over ``plane_qv`` gives a plane's connected parts.
        LIMITS: a direction cell is about 7 degrees wide; a plane whose normal lies on a cell border splits its votes and is
        found later, not lost; a plane more than 512 voxels from the centre of the scene's box is left out; no curved
        primitives.  The defaults (20 degrees, 1.5 voxels, 200 voxels) are this project's choice and are NOT tuned on real
        scans.  One library call and ONE host round trip; no session state changes."""
        self._need_scene()
        n = self._labels_qv.numel()
        up64 = _unit3(up, "up")
        res = self._normals_last if normals is None and self.faces is None else normals
        if res is None:
            raise ValueError("no normals: call estimate_normals() first (on a mesh it keeps none with the scene: pass its result "
                             "as normals=)")
        if not isinstance(res, NormalsResult) or not torch.is_tensor(res.normals_qv) or res.normals_qv.device != self.device \
                or tuple(res.normals_qv.shape) != (n, 3):
            raise ValueError("normals must be a NormalsResult of this scene (estimate_normals())")
        tol = 1.5 * self.voxel_size if dist_tol is None else dist_tol
        kinds_deg = min(float(normal_deg), 45.0) if isinstance(normal_deg, (int, float)) else normal_deg
        keys = self._grow_keys(within)
        candidate = None
        if keys is not None:
            candidate = ((keys == 0) if isinstance(within, str) else (keys >= 0)).to(torch.uint8)
        origin, quantum, bits = self._fixed_point_frame()
        plane_qv, plane_full, out, _ = V.find_planes(
            res.normals_qv.contiguous(), self.raw_coords_qv, origin, quantum, bits, offset_bin=self.voxel_size, normal_deg=normal_deg,
            dist_tol=tol, min_voxels=min_voxels, max_planes=max_planes, candidate=candidate, inverse_map=self.inverse_map)
        records, s = V.read_planes(out.cpu().numpy())                     # the one host round trip
        if s["err"] & V.PLANES_BAD_INDEX:
            raise RuntimeError("a3d_find_planes: inverse_map out of range")
        kinds = plane_kinds(records["normal"], records["offset"], up64, kinds_deg)
        first = lambda kind: kinds.index(kind) if kind in kinds else None
        return PlanesResult(plane_qv=plane_qv, plane_full=plane_full, records=records, n_planes=s["n_planes"], kinds=kinds,
                            floor=first("floor"), ceiling=first("ceiling"), walls=[k for k, x in enumerate(kinds) if x == "wall"],
                            rounds=s["rounds"], spent=s["spent"], admitted=s["admitted"], left_out=s["left_out"], up=up64,
                            normal_deg=float(normal_deg), dist_tol=float(tol), min_voxels=int(min_voxels),
                            max_planes=int(max_planes), within=within if isinstance(within, str) else "keys")

    def plane_at(self, result, u, v, planes=None):
        """The id of the plane that pixel ``(u, v)`` (column, row) of ``result`` shows, or ``None`` where the pixel shows nothing
        or its vertex lies on no plane -- resolved as ``piece_at`` resolves a vertex: the pixel's vertex on a cloud, the
        heaviest corner of its face on a mesh.  ``planes``: a ``PlanesResult`` of this scene (default: ``planes()``, computed
        here)."""
        self._need_scene()
        planes = self.planes() if planes is None else planes
        if not isinstance(planes, PlanesResult) or tuple(planes.plane_full.shape) != (self.coords_full.shape[0],):
            raise ValueError("the planes belong to another scene")
        vertex = self._vertex_at(result, u, v)
        if vertex < 0:
            return None
        k = int(planes.plane_full[vertex].cpu())
        return k if k >= 0 else None

    # ------------------------------------------------------------------ more objects like this one
    def _example_classes(self, obj, selection):
        """``(classes int32 [n_voxels] on the device: the object a voxel is an example of, -1 for none; the object ids that
        get a prototype)`` of ``lookalikes(obj=, selection=)``."""
        labels, n_objects = self._labels_qv, len(self.click_idx) - 1
        none = torch.full_like(labels, -1)
        if selection is not None:
            if obj is None:
                raise ValueError("selection names the examples of ONE object: obj is missing")
            obj = V._int_in("obj", obj, 1, 255)
            sel = self._selection(selection)
            hit = torch.zeros(labels.numel(), dtype=torch.int32, device=self.device).index_add_(0, self.inverse_map, sel.to(torch.int32))
            return torch.where(hit > 0, torch.full_like(labels, obj), none), [obj]
        if obj is None:
            if n_objects == 0:
                raise ValueError("lookalikes() needs an example: there is no object yet (click and infer(), or pass selection= with obj=)")
            return torch.where(labels > 0, labels, none), list(range(1, n_objects + 1))
        obj = V._int_in("obj", obj, 1, max(n_objects, 1), f"obj must be an existing object id 1 .. {n_objects}, or None (every object)")
        if n_objects == 0:
            raise ValueError("lookalikes() needs an example: there is no object yet (click and infer(), or pass selection= with obj=)")
        return torch.where(labels == obj, labels, none), [obj]

    def lookalikes(self, obj=None, selection=None, cos_min=0.9, min_voxels=8, within="background", connectivity=26,
                   max_candidates=10, features=None):
        """MORE OBJECTS LIKE THIS ONE, by the backbone's features: label one chair, ask for its lookalikes.  The EXAMPLES
        are voxels of the current voxel labelling (what ``preview()`` paints): with ``obj=None`` every object 1..K that has
        voxels gets a prototype, with ``obj=k`` that object alone; with ``selection`` (a ``SelectResult`` or a uint8 / bool
        mask over the vertices) and ``obj=k`` the voxels of the selected vertices are the examples of object k, whatever the
        labelling says.  No example voxel at all raises ``ValueError``.  An object's PROTOTYPE is the mean of its examples'
        feature rows (``a3d_feature_prototypes``: integer sums in fixed point, so it depends on no order; ``view.
        prototype_table``).  Every CANDIDATE voxel then takes the object whose prototype it is most similar to, provided the
        cosine reaches ``cos_min`` (``a3d_feature_match``; the rule, reproducible to the bit, is stated in
        include/agile3d_hip.h).  ``within="background"``: only voxels labelled 0 that are no example may match;
        ``"all"``: every voxel, except that an example never matches its own object.

        The matched voxels form REGIONS: connected pieces (``connectivity``, ``a3d_label_pieces``) of one matched object.
        Regions below ``min_voxels`` voxels are dropped; the rest are ranked by size, ties to the lower root
        (``rank_spots``), and for the first ``MAX_SPOTS`` = 255 the deepest voxel -- the one farthest from everything
        outside the region -- is found by the click simulator's search (``a3d_click_clusters``), as ``guide(regions=
        "connected")`` finds a spot's.  ``candidates`` holds one suggested click per searched region, deepest first
        (``rank_candidates``), at most ``max_candidates``: ``ses.click(c["point"], new_id)`` takes a candidate as a NEW
        object (or ``c["object"]`` to add it to the object it looks like).  ``colors`` is the similarity view: a matched
        vertex's own colour faded towards its matched object's palette colour by the score (``own * (1 - s) + palette *
        s``, s = the score clamped to [0, 1]); ``render(colors=res.colors)`` shows it as it is.

        ``features``: fp32 [n_voxels, 128] on the device, used instead of the backbone's output (``ses._backbone[0].F``),
        as ``infer(logits=)`` and ``patches(normals=)`` take theirs.  The default ``cos_min`` = 0.9 (and ``min_voxels`` = 8)
        is this project's choice and is NOT tuned on real scans: how alike two chairs' features are depends on the
        checkpoint.  Two library calls, the piece search and the cluster search; TWO host round trips, what ``guide(regions=
        "connected")`` pays: the regions' records (with the summaries and the example counts), then the search's result --
        one when no region is left to search.  The method reads the current labelling each call and changes no session
        state.  Returns a ``LookalikeResult``."""
        self._need_scene()
        if within not in ("background", "all"):
            raise ValueError('within must be "background" or "all"')
        connectivity = V._connectivity(connectivity)
        min_voxels = V._int_in("min_voxels", min_voxels, 1, (1 << 31) - 1)
        max_candidates = V._int_in("max_candidates", max_candidates, 0, (1 << 31) - 1)
        try:
            cos_min = float(cos_min)
        except (TypeError, ValueError):
            raise ValueError("cos_min must be a finite number in [0, 1]") from None
        if not 0.0 <= cos_min <= 1.0:
            raise ValueError("cos_min must be a finite number in [0, 1]")
        dev, labels = self.device, self._labels_qv
        n = labels.numel()
        feats = self._backbone[0].F if features is None else features
        if not torch.is_tensor(feats) or feats.device != dev or feats.dtype != torch.float32 or tuple(feats.shape) != (n, V.MATCH_CHANNELS):
            raise ValueError(f"features must be an fp32 tensor [{n}, {V.MATCH_CHANNELS}] on the session's device")
        feats = feats.contiguous()
        classes, ids = self._example_classes(obj, selection)
        sums, count, proto_sum = V.feature_prototypes(feats, classes, n_classes=ids[-1] + 1)
        id_rows = torch.tensor(ids, dtype=torch.int64).to(dev)
        protos = V.prototype_table(sums, count)[id_rows].contiguous()
        candidate = ((labels == 0) & (classes < 0)).to(torch.uint8) if within == "background" else None
        match_qv, _, score_qv, match_full, score_full, match_sum = V.feature_match(
            feats, protos, id_rows.to(torch.int32), cos_min, candidate=candidate, inverse_map=self.inverse_map)
        if within == "all":                          # an example never matches its own object
            match_qv = torch.where(match_qv == classes, torch.full_like(match_qv, -1), match_qv)
            match_full = torch.where(match_full == classes[self.inverse_map], torch.full_like(match_full, -1), match_full)
        piece_qv, _, recs, _, tail = self._label_pieces(
            match_qv, connectivity, also=lambda *_: torch.cat([proto_sum, match_sum, count.view(torch.uint8)]))   # round trip 1
        at = V.PROTOTYPES_SUMMARY.itemsize + V.MATCH_SUMMARY.itemsize
        ps, ms = V.read_prototypes_summary(tail[:V.PROTOTYPES_SUMMARY.itemsize]), V.read_match_summary(tail[V.PROTOTYPES_SUMMARY.itemsize:at])
        if ps["err"] or ms["err"]:
            raise RuntimeError(f"lookalikes: labels, inverse_map or prototypes out of range (error words {ps['err']}, {ms['err']})")
        per_class = tail[at:].view(np.int32)
        prototypes = {k: int(per_class[k]) for k in ids if per_class[k] > 0}
        if not prototypes:
            raise ValueError("lookalikes() needs an example: no voxel of " + (f"object {ids[0]}" if len(ids) == 1 else "any object")
                             + (" with features in range" if ps["examples_left_out"] else ""))
        kept = [r for r in recs if int(r["voxels"]) >= min_voxels]
        spots = [kept[k] for k in rank_spots(kept)]
        clusters = []
        if spots:
            launched = K.launch_clusters(torch.zeros_like(labels), self._spot_ids(piece_qv, spots), self.raw_coords_qv)
            try:
                launched[1].copy_(launched[0], non_blocking=True)
            finally:
                torch.cuda.current_stream(dev).synchronize()      # round trip 2
            clusters = K.read_clusters(launched[1].numpy(), bad_ids="a3d_click_clusters: labels outside 0 .. 255",
                                       too_many="a3d_click_clusters: {} regions", whole_sample_ok=True)
        own, s = self.colors_full, score_full.clamp(0.0, 1.0).unsqueeze(1)
        colors = torch.where((match_full >= 0).unsqueeze(1), own * (1.0 - s) + self._palette_colors(match_full) * s, own)
        return LookalikeResult(match_qv=match_qv, score_qv=score_qv, score_full=score_full, colors=colors,
                               candidates=rank_candidates(clusters, spots, self._coords_qv_host, max_candidates),
                               n_regions=len(kept), n_regions_searched=len(spots), prototypes=prototypes,
                               examples_left_out=ps["examples_left_out"], rows_nonfinite=ms["rows_nonfinite"], cos_min=cos_min,
                               min_voxels=min_voxels, within=within, connectivity=connectivity)

    def lookalike_at(self, result, u, v, **kw):
        """``lookalikes(obj=...)`` with the object under pixel ``(u, v)`` (column, row) of ``result`` as the example
        (``object_at``: the labels of the last ``infer`` / ``preview``); ``kw`` are ``lookalikes``' other arguments.  A pixel
        that shows the background or nothing raises ``ValueError``.  One small device-to-host copy more than ``lookalikes``."""
        self._need_scene()
        obj = self.object_at(result, u, v)
        if not obj:
            raise ValueError(f"pixel ({int(u)}, {int(v)}) shows " + ("nothing" if obj is None else "the background") + ": no object to look for")
        return self.lookalikes(obj=obj, **kw)

    # ------------------------------------------------------------------ labels to and from another point set
    def _points(self, name, points):
        """``points`` (numpy, or a tensor on any device) as fp32 [m, 3] on the session's device."""
        p = points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points))
        if p.dim() != 2 or p.shape[1] != 3 or not (p.dtype.is_floating_point or p.numel() == 0):
            raise ValueError(f"{name} must be [m, 3] floating-point coordinates")
        return p.to(self.device).to(torch.float32).contiguous()

    def _reach(self, max_distance):
        """``(max_distance, cell_size)`` as fp32 values: the cells are twice the reach, which is then exactly half a cell."""
        with np.errstate(over="ignore"):
            r = np.float32(self.voxel_size if max_distance is None else max_distance)
            cell = np.float32(2.0) * r
        if not (np.isfinite(cell) and r > 0):
            raise ValueError("max_distance must be finite and > 0 in fp32")
        return float(r), float(cell)

    def _vertex_index(self, cell):
        """The index over ``coords_full`` with cells of ``cell``: built on first use, kept with the scene."""
        index = self._point_indices.get(cell)
        if index is None:
            while len(self._point_indices) >= _MAX_POINT_INDICES:
                self._point_indices.pop(next(iter(self._point_indices))).close()
            index = self._point_indices[cell] = V.point_index_create(self.coords_full, cell)
        return index

    def _palette_colors(self, labels):
        """fp32 [m, 3]: the palette's colour of every label, ids beyond the table wrapped as ``_palette_entry`` wraps them."""
        n = self._palette_dev.shape[0]
        lab = labels.to(torch.int64).clamp_(min=0)
        return self._palette_dev[torch.where(lab < n, lab, 1 + (lab - 1) % (n - 1))]

    def _nearest(self, index, queries, r, labels_src, fill):
        nearest, d2, labels, summary = V.point_index_nearest(index, queries, r, labels_src=labels_src, fill=fill,
                                                             summary=self._transfer_sum)
        s = V.read_transfer_summary(summary.cpu().numpy())              # the one host round trip
        return TransferResult(nearest=nearest, distance2=d2, labels=labels, colors=None if labels is None else self._palette_colors(labels),
                              matched=s["matched"], unmatched=s["unmatched"], nonfinite=s["nonfinite"],
                              source_left_out=s["source_left_out"], max_distance=r)

    def nearest_vertices(self, points, max_distance=None):
        """For every row of ``points`` [m, 3] (numpy, or a tensor on any device) the scene's nearest vertex within
        ``max_distance`` (default ``voxel_size``), exactly: the first arg-min of the fp32 distance ``click`` searches by, over
        the finite vertices in reach (``a3d_point_index_nearest``); -1 where there is none.  The index over ``coords_full``
        has cells of twice ``max_distance``; it is built on first use and kept with the scene, one per cell size.  Returns a
        ``TransferResult`` (``labels`` and ``colors`` are ``None``).  One host round trip (the counts)."""
        self._need_scene()
        q = self._points("points", points)
        r, cell = self._reach(max_distance)
        return self._nearest(self._vertex_index(cell), q, r, None, 0)

    def transfer(self, points, labels=None, max_distance=None, fill=0):
        """The scene's labels carried to another point set: every row of ``points`` takes the label of its nearest vertex
        within ``max_distance`` (``nearest_vertices``' search; the labels are gathered in the same kernel), ``fill`` where
        no vertex is in reach.  ``labels`` int32 [n_full] on the session's device (default: the full-resolution labels of
        the last ``infer`` / ``preview``; ``ValueError`` before any).  Returns a ``TransferResult`` with ``labels`` and
        ``colors``.  One host round trip."""
        self._need_scene()
        n = self.coords_full.shape[0]
        lab = self._labels_last if labels is None else labels
        if lab is None:
            raise ValueError("transfer() carries the labels of the last infer() / preview(): there is none yet (or pass labels=)")
        if not torch.is_tensor(lab) or lab.device != self.device or lab.dtype != torch.int32 or tuple(lab.shape) != (n,):
            raise ValueError(f"labels must be an int32 tensor [{n}] on the session's device")
        q = self._points("points", points)
        r, cell = self._reach(max_distance)
        return self._nearest(self._vertex_index(cell), q, r, lab.contiguous(), fill)

    def import_labels(self, points, labels, max_distance=None, into="manual"):
        """A labelling held on another point set brought into the session: every vertex of the scene takes the label of
        its nearest row of ``points`` [k, 3] within ``max_distance`` (default ``voxel_size``); ``labels`` [k] integer ids
        (numpy, or a tensor on any device).  The index over ``points`` lives for the call only.  ``into="manual"``: the
        matched vertices go into the manual layer (``set_manual``: ids in 0..255, else ``ValueError`` and the layer as it
        was); the layer's other vertices stay as they were, so ``corrected()`` shows the imported labels.
        ``into="truth"``: the labels become the scene's ground truth (unmatched vertices 0) -- ``infer()`` then reports
        ``miou`` -- which is allowed only while the click list is empty (``ValueError`` otherwise, nothing changed).
        Returns the ``TransferResult`` of the scene's vertices."""
        self._need_scene()
        if into not in ("manual", "truth"):
            raise ValueError("into must be 'manual' or 'truth'")
        if into == "truth" and self._clicks:
            raise ValueError("the ground truth can be replaced only while the click list is empty (reset() first)")
        p = self._points("points", points)
        lab = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
        if lab.dim() != 1 or lab.shape[0] != p.shape[0] or lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise ValueError(f"labels must be [{p.shape[0]}] integer ids, one per point")
        lab = lab.to(self.device).to(torch.int32).contiguous()
        r, cell = self._reach(max_distance)
        index = V.point_index_create(p, cell)
        try:
            res = self._nearest(index, self.coords_full, r, lab, 0)
        finally:
            index.close()
        if into == "manual":
            on, obj = self.manual_labels()
            hit = res.nearest >= 0
            self.set_manual(on | hit.to(torch.uint8), torch.where(hit, res.labels, obj))
        else:
            self.labels_full_ori = res.labels
            self.labels_qv_ori = self.labels_full_ori[self._unique_map]
            self.new_labels = torch.zeros_like(self.labels_full_ori)
        return res
