"""Host mirror of the reference's ``utils/seg.py`` for the interactive loop, on the HIP library.

Same function names, argument meaning and return values as the reference (file:line cited per
function); the arithmetic runs in ``libagile3d_hip.so`` (``csrc/clicks.hip``): one exact
nearest-outside-point pass for all error clusters instead of one ``torch.cdist`` matrix per cluster.
There is no CPU path: tensors must live on the GPU.

Every library symbol is marshalled at ONE place here, every operand group is prepared by one function, and the batched
calls share one round (``_round``: launch, copy to pinned buffers, drain the stream, check, parse) and one chunking rule
(``MAX_ROUND_SAMPLES`` samples per library call).  ``session.py`` uses the public names ``click_lists``, ``launch_clusters``,
``read_clusters``, ``launch_iou_counts`` and ``mean_iou_from_counts``.
"""
from __future__ import annotations

import ctypes as C
import functools
import random

import numpy as np
import torch
from torch.utils.weak import WeakIdKeyDictionary

from . import lib as L

MAX_CLUSTERS = 1024
MAX_ROUND_SAMPLES = 64      # samples per batched library call (include/agile3d_hip.h: A3D_MAX_ROUND_SAMPLES, csrc/clicks.hip: kMaxClickBatch)
_REC = np.dtype([("cluster_id", "<i4"), ("row", "<i4"), ("label", "<i4"), ("pred", "<i4"), ("error_size", "<f4")])
_REC_BYTES = MAX_CLUSTERS * C.sizeof(L.ClickCluster)
_OUT_BYTES = _REC_BYTES + 16
_BAD_MAP = "iou_counts: inverse_map holds rows outside the prediction"


# ---------------------------------------------------------------- operands: one preparer per group
def _i32(t: torch.Tensor) -> torch.Tensor:
    """labels / predictions arrive as float, long or int tensors in the reference; ids are small ints."""
    if not t.is_cuda:
        raise RuntimeError("agile3d_amd.clicks runs on the GPU only (no CPU fallback); got a CPU tensor")
    return t.to(torch.int32).contiguous()


_I32P = C.POINTER(C.c_int32)


def click_lists(click_idx):
    """``{object id: [rows]}`` as two int32 arrays ``(rows, objs)`` in dict order -- the order the reference's "update
    prediction with sparse gt" loop applies them in (eval_multi_obj.py:119-134); empty lists and repeats are kept."""
    rows, objs = [], []
    for obj_id, cids in (click_idx or {}).items():
        rows += [int(c) for c in cids]
        objs += [int(obj_id)] * len(cids)
    return np.array(rows, dtype=np.int32), np.array(objs, dtype=np.int32)


def query_list(click_idx, click_time_idx):
    """One sample's click dictionaries (keys ``"0".."K"``: voxel rows / click times per object, 0 = background) as the
    decoder's query list (agile3d.py:201-240): ``(fg_rows, fg_times, counts, bg_rows, bg_times)`` -- the clicks of objects
    1..K in object order as Python ints, how many each object has, and the background's.  The inference decoder
    (``Engine.forward_mask``) and the training tape (``DecoderTape``) both order their queries this way; one pass over the
    clicks.  ``ValueError``: a key is missing, rows and times do not pair up, or an object >= 1 has no click."""
    K = len(click_idx) - 1
    fg_rows, fg_times, counts = [], [], []
    for o in list(range(1, K + 1)) + [0]:
        try:
            r, t = click_idx[str(o)], click_time_idx[str(o)]
        except KeyError:
            raise ValueError(f'click_idx and click_time_idx need the keys "0" .. "{K}" (no "{o}")') from None
        if len(r) != len(t):
            raise ValueError("click_idx / click_time_idx length mismatch")
        if o == 0:
            return fg_rows, fg_times, counts, [int(v) for v in r], [int(v) for v in t]
        if len(r) == 0:    # an empty group has no maximum
            raise ValueError(f"object {o} has no click (the reference fails on an empty max, agile3d.py:353)")
        fg_rows.extend(map(int, r))
        fg_times.extend(map(int, t))
        counts.append(len(r))


def _logits(logits):
    logits = logits.contiguous()
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 2:
        raise RuntimeError("argmax_labels: logits must be a CUDA float32 [N, 1+K] tensor")
    return logits


def _iou_operands(pred, labels, inverse_map):
    p, l = _i32(pred), _i32(labels)
    inv = None
    if inverse_map is not None:
        inv = inverse_map.to(device=p.device, dtype=torch.int64).contiguous()
        if inv.numel() != l.numel():
            raise RuntimeError("iou_counts: inverse_map and labels differ in length")
    elif p.numel() != l.numel():
        raise RuntimeError("iou_counts: pred and labels differ in length")
    return p, l, inv


def _cluster_operands(pred, labels, coords):
    p, l = _i32(pred), _i32(labels)
    if not coords.is_cuda:
        raise RuntimeError("error_clusters: coords must live on the GPU")
    xyz = coords.to(torch.float32).contiguous()
    n = p.numel()
    if n and (xyz.shape != (n, 3) or l.numel() != n):
        raise RuntimeError("error_clusters: pred [N], labels [N], coords [N,3] expected")
    return p, l, xyz


_buffers: dict = {}


def _buffer(device, purpose, size, dtype=torch.uint8, pinned=False):
    """The module's buffer for ``purpose`` on ``device`` (``pinned``: in page-locked host memory), at least ``size`` elements
    of ``dtype``; allocated on first use and again only to grow.  A buffer is free for its next user once the stream the
    last one launched on is drained, which every function below does before it returns."""
    key = (device.index, purpose, pinned)
    buf = _buffers.get(key)
    if buf is None or buf.numel() < size:
        buf = _buffers[key] = (torch.empty(size, dtype=dtype, pin_memory=True) if pinned
                               else torch.empty(size, dtype=dtype, device=device))
    return buf


def _pair(device, purpose, rows, cols, dtype=torch.uint8):
    """A device buffer [rows, cols] and its pinned host twin."""
    return tuple(_buffer(device, purpose, rows * cols, dtype, pinned)[:rows * cols].view(rows, cols) for pinned in (False, True))


@functools.lru_cache(maxsize=None)
def _argmax_workspace_bytes(ns):
    return L.load().a3d_argmax_labels_batch_workspace_bytes(ns)


def _workspace(device, n, slot=0):
    """Cluster-search workspace of one sample in flight (slot = 1 + its place in a batch, 0 for the per-sample call)."""
    return _buffer(device, ("work", slot), L.load().a3d_click_workspace_bytes(n))


# ---------------------------------------------------------------- arg-max
def argmax_labels(logits: torch.Tensor, click_idx: dict | None = None) -> torch.Tensor:
    """``p.argmax(-1)`` followed by "update prediction with sparse gt" (eval_multi_obj.py:119-134):
    int32 labels [N]; rows listed in ``click_idx`` are overwritten with their object id, dict order.  The clicks travel by
    value (``a3d_argmax_labels``: no workspace, no staging copy -- the session's and the single-scene latency path)."""
    logits = _logits(logits)
    r, o = click_lists(click_idx)
    pred = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    L.check(L.load().a3d_argmax_labels(logits.data_ptr(), logits.shape[0], logits.shape[1], r.ctypes.data_as(_I32P),
                                       o.ctypes.data_as(_I32P), len(r), pred.data_ptr(), L.stream(logits.device)),
            "a3d_argmax_labels")
    return pred


def argmax_labels_batch(logits_list, click_idx_list=None):
    """``argmax_labels`` of every sample of a round in two launches per ``MAX_ROUND_SAMPLES`` samples
    (``a3d_argmax_labels_batch``; the per-sample calls were two launches each: 32 per lock-step evaluation round of 16
    scenes).  Same results, in sample order.  The chunks run one after the other on one stream: one workspace serves them."""
    lib = L.load()
    preds = []
    for c0 in range(0, len(logits_list), MAX_ROUND_SAMPLES):
        part = [_logits(lg) for lg in logits_list[c0:c0 + MAX_ROUND_SAMPLES]]
        dev = part[0].device
        arr = (L.ArgmaxSample * len(part))()
        keep = []                                # the host lists are read before the library call returns
        for k, lg in enumerate(part):
            r, o = click_lists(click_idx_list[c0 + k] if click_idx_list is not None else None)
            pred = torch.empty(lg.shape[0], dtype=torch.int32, device=dev)
            sp = arr[k]
            sp.logits_dev, sp.n, sp.n_classes, sp.n_clicks = lg.data_ptr(), lg.shape[0], lg.shape[1], len(r)
            sp.click_row, sp.click_obj, sp.pred_dev = r.ctypes.data_as(_I32P), o.ctypes.data_as(_I32P), pred.data_ptr()
            keep.append((r, o))
            preds.append(pred)
        need = _argmax_workspace_bytes(len(part))
        ws = _buffer(dev, "argmax", need)
        L.check(lib.a3d_argmax_labels_batch(C.cast(arr, C.c_void_p), len(part), ws.data_ptr(), need, L.stream(dev)),
                "a3d_argmax_labels_batch")
    return preds


# ---------------------------------------------------------------- IoU
def launch_iou_counts(preds, labels, inverse_maps, n_ids, counts):
    """IoU counts of all samples into ``counts`` [ns][3 n_ids + 1] (int64, device; the last slot of a row is its error word)
    on the current stream: ONE launch + one clear per ``MAX_ROUND_SAMPLES`` samples (``a3d_iou_counts_batch``).  Returns the
    tensors the launches read; they and ``counts`` are in use until the stream is drained."""
    lib = L.load()
    keep = [_iou_operands(pr, lb, None if inverse_maps is None else inverse_maps[i]) for i, (pr, lb) in enumerate(zip(preds, labels))]
    for c0 in range(0, len(keep), MAX_ROUND_SAMPLES):
        part = keep[c0:c0 + MAX_ROUND_SAMPLES]
        arr = (L.IouSample * len(part))()
        for k, (p, l, inv) in enumerate(part):
            sp = arr[k]
            sp.pred_dev, sp.n_pred, sp.inverse_map_dev = p.data_ptr(), p.numel(), inv.data_ptr() if inv is not None else None
            sp.labels_dev, sp.n_full = l.data_ptr(), l.numel()
        L.check(lib.a3d_iou_counts_batch(C.cast(arr, C.c_void_p), len(part), n_ids, counts[c0].data_ptr(), L.stream(counts.device)),
                "a3d_iou_counts_batch")
    return keep


def mean_iou_from_counts(c):
    """(mean IoU as a 0-d float32 tensor, {object id: IoU}) of one sample's counts [3][n_ids]; the fp32 arithmetic (int
    counts -> fp32 divide -> sequential fp32 sum) is the reference's (utils/seg.py:10-18,44-59)."""
    ids = [i for i in range(1, c.shape[1]) if c[2, i] > 0]
    total = np.float32(0.0)
    per_obj = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in ids:
            v = np.float32(c[0, i]) / np.float32(c[1, i] + c[2, i] - c[0, i])
            per_obj[i] = float(v)
            total = np.float32(total + v)
        total = np.float32(total / np.float32(len(ids))) if ids else np.float32(np.nan)
    return torch.tensor(total, dtype=torch.float32), per_obj


# ---------------------------------------------------------------- error clusters
def launch_clusters(pred, labels, coords):
    """One sample's cluster search on the current stream (``a3d_click_clusters``: no spatial order).  Returns ``(out,
    out_host)``: the records on the device and a pinned buffer of their size -- ``read_clusters`` reads a host copy once
    the stream is drained, and both buffers are the next call's after that --, or ``None`` for a sample of no points."""
    p, l, xyz = _cluster_operands(pred, labels, coords)
    if p.numel() == 0:
        return None
    work = _workspace(p.device, p.numel())
    out, out_host = (b[0] for b in _pair(p.device, "records", 1, _OUT_BYTES))
    L.check(L.load().a3d_click_clusters(xyz.data_ptr(), p.data_ptr(), l.data_ptr(), p.numel(), out.data_ptr(), MAX_CLUSTERS,
                                        out.data_ptr() + _REC_BYTES, work.data_ptr(), work.numel(), L.stream(p.device)),
            "a3d_click_clusters")
    return out, out_host


def read_clusters(host: np.ndarray, bad_ids="error_clusters: labels / predictions must be object ids in 0..255",
                  too_many="error_clusters: {} error clusters", whole_sample_ok=False):
    """The host copy of one sample's records (uint8 [_OUT_BYTES]) as a list of dicts {cluster_id, row, label, pred,
    error_size}, ascending cluster id.  ``bad_ids`` / ``too_many``: the caller's words for the two errors the search
    reports; ``whole_sample_ok``: keep a cluster that covers the whole sample (its ``error_size`` is inf)."""
    count = int(host[_REC_BYTES:_REC_BYTES + 4].view(np.int32)[0])
    if count < 0:
        raise RuntimeError(bad_ids)
    if count > MAX_CLUSTERS:
        raise RuntimeError(f"{too_many.format(count)} > {MAX_CLUSTERS}")
    recs = np.frombuffer(host[:count * C.sizeof(L.ClickCluster)].tobytes(), dtype=_REC)
    if not whole_sample_ok and not np.isfinite(recs["error_size"]).all():
        raise RuntimeError("error cluster covers the whole sample (the reference fails here too)")
    # one conversion of all records to Python scalars (field-by-field access to numpy records cost 25 us per sample and round
    # between the device's cluster search and the next decoder pass)
    return [dict(zip(_REC.names, t)) for t in recs.tolist()]


def error_clusters(pred, labels, coords):
    """Per error cluster (ascending cluster id = 96*label + 11*pred, utils/seg.py:186): the point
    farthest from everything outside the cluster and that distance.  List of dicts
    {cluster_id, row, label, pred, error_size}."""
    launched = launch_clusters(pred, labels, coords)
    return read_clusters(launched[0].cpu().numpy()) if launched is not None else []


_ORDER_FROM = 20000        # csrc/clicks.hip: kCoarseFrom -- smaller samples run no first bounding stage
_orders = WeakIdKeyDictionary()      # the caller's coordinate tensor -> (its version, order, inv); an entry dies with its tensor


def _spatial_order(xyz):
    """Morton order of a sample's coordinates and its inverse (``a3d_click_spatial_order``), or ``None`` below
    ``_ORDER_FROM`` points.  Cached on the tensor the caller passed -- a scene's coordinates do not change over its click
    rounds (eval_multi_obj.py:112-166, engine.py:83-116) and the callers hand over the same tensor every round --, whatever
    its dtype and layout; writing to the tensor in place (its version moves) computes the order anew."""
    n = xyz.shape[0]
    if n < _ORDER_FROM:
        return None
    hit = _orders.get(xyz)
    if hit is None or hit[0] != xyz._version:
        lib = L.load()
        x = xyz.to(torch.float32).contiguous()
        order = torch.empty(n, dtype=torch.int32, device=x.device)
        inv = torch.empty(n, dtype=torch.int32, device=x.device)
        ws = torch.empty(lib.a3d_click_spatial_order_workspace_bytes(n), dtype=torch.uint8, device=x.device)
        L.check(lib.a3d_click_spatial_order(x.data_ptr(), n, order.data_ptr(), inv.data_ptr(), ws.data_ptr(), ws.numel(),
                                            L.stream(x.device)), "a3d_click_spatial_order")
        hit = _orders[xyz] = (xyz._version, order, inv)
    return hit[1:]


def _launch_clusters_batch(preds, labels, coords, keep):
    """The cluster search of the non-empty samples on the current stream -- ONE ``a3d_click_clusters_batch`` call (a dozen
    launches whatever the number of samples) per ``MAX_ROUND_SAMPLES`` of them, the device table in the chunk's first
    workspace -- and the copy of all their records into one pinned buffer.  Returns (host buffer, slot of every sample or
    None); ``keep`` collects what must outlive the stream's work."""
    dev = preds[0].device
    slots, live = [], []
    for i, (pr, lb, xyz) in enumerate(zip(preds, labels, coords)):
        p, l, x = _cluster_operands(pr, lb, xyz)
        if p.numel() == 0:
            slots.append(None)
            continue
        slots.append(len(live))
        live.append((p, l, x, _workspace(dev, p.numel(), slot=1 + i), xyz))
    if not live:
        return None, slots
    keep.append(live)
    out, host = _pair(dev, "records", len(live), _OUT_BYTES)
    for c0 in range(0, len(live), MAX_ROUND_SAMPLES):
        part = live[c0:c0 + MAX_ROUND_SAMPLES]
        arr = (L.ClickSample * len(part))()
        for k, (p, l, x, work, xyz) in enumerate(part):
            sp, o = arr[k], out[c0 + k].data_ptr()
            sp.xyz_dev, sp.pred_dev, sp.labels_dev, sp.n = x.data_ptr(), p.data_ptr(), l.data_ptr(), p.numel()
            sp.out_dev, sp.n_out_dev, sp.max_out = o, o + _REC_BYTES, MAX_CLUSTERS
            sp.workspace_dev, sp.workspace_bytes = work.data_ptr(), work.numel()
            so = _spatial_order(xyz)             # (keyed on the caller's tensor, not on its fp32 copy `x`)
            sp.order_dev, sp.inv_dev = (so[0].data_ptr(), so[1].data_ptr()) if so is not None else (None, None)
        L.check(L.load().a3d_click_clusters_batch(C.cast(arr, C.c_void_p), len(part), L.stream(dev)), "a3d_click_clusters_batch")
    host.copy_(out, non_blocking=True)
    return host, slots


# ---------------------------------------------------------------- one round of the interactive protocol
def _round(preds, clusters_of=None, iou_of=None, n_ids=256):
    """What a round needs from the device with ONE host synchronisation: the error clusters of every sample against
    ``clusters_of`` = (labels, coords) and / or its IoU counts against ``iou_of`` = (labels, inverse maps or None), all on the
    current stream, their records back through pinned buffers, everything awaited once.  Returns ``(counts, clusters)``:
    int64 [ns, 3, n_ids] and a list of ``error_clusters`` results, or ``None`` for the half not asked for."""
    dev, ns = preds[0].device, len(preds)
    keep, host, counts_host = [], None, None
    try:                     # the stream is drained before ANY exit: the inputs and the cached buffers are in use until then
        if clusters_of is not None:
            host, slots = _launch_clusters_batch(preds, *clusters_of, keep)
        if iou_of is not None:
            counts, counts_host = _pair(dev, "iou", ns, 3 * n_ids + 1, torch.int64)
            keep.append(launch_iou_counts(preds, *iou_of, n_ids, counts))
            counts_host.copy_(counts, non_blocking=True)
    finally:
        torch.cuda.current_stream(dev).synchronize()
    counts = clusters = None
    if iou_of is not None:
        hc = counts_host.numpy()
        if hc[:, -1].any():
            raise RuntimeError(_BAD_MAP)
        counts = hc[:, :-1].reshape(ns, 3, n_ids).copy()
    if clusters_of is not None:
        hn = host.numpy() if host is not None else None
        clusters = [[] if k is None else read_clusters(hn[k]) for k in slots]
    return counts, clusters


def error_clusters_batch(preds, labels, coords):
    """``error_clusters`` of several samples with ONE set of launches and ONE host synchronisation (the kernels take the
    samples from a device table -- csrc/clicks.hip).  Same results as the per-sample call, in sample order."""
    return _round(preds, clusters_of=(labels, coords))[1] if preds else []


def iou_counts_batch(preds, labels, inverse_maps=None, n_ids: int = 256):
    """``iou_counts`` of several samples with one launch and one device-to-host copy: list of int64 [3][n_ids] arrays."""
    return list(_round(preds, iou_of=(labels, inverse_maps), n_ids=n_ids)[0]) if preds else []


def iou_counts(pred, labels, inverse_map=None, n_ids: int | None = None) -> np.ndarray:
    """int64 [3][n_ids]: |pred==id & label==id|, |pred==id|, |label==id| with pred read through
    ``inverse_map`` (voxel -> full-resolution points, eval_multi_obj.py:138) when given."""
    return iou_counts_batch([pred], [labels], [inverse_map], 256 if n_ids is None else n_ids)[0]


def mean_iou_scene_batch(preds, labels, inverse_maps=None):
    """``mean_iou_scene`` per sample of a batch, one host round trip for all of them."""
    return [mean_iou_from_counts(c) for c in iou_counts_batch(preds, labels, inverse_maps)]


def mean_iou_scene(pred, labels, inverse_map=None):
    """utils/seg.py:44-59.  Returns (mean IoU as a 0-d float32 tensor, {object id: IoU})."""
    return mean_iou_from_counts(iou_counts(pred, labels, inverse_map))


def mean_iou_and_clusters_batch(preds, labels_iou, inverse_maps, labels_qv, coords, n_ids: int = 256):
    """One round with ONE host synchronisation: returns ``(ious, clusters)`` = what ``mean_iou_scene_batch(preds,
    labels_iou, inverse_maps)`` and ``error_clusters_batch(preds, labels_qv, coords)`` return."""
    if not preds:
        return [], []
    counts, clusters = _round(preds, (labels_qv, coords), (labels_iou, inverse_maps), n_ids)
    return [mean_iou_from_counts(c) for c in counts], clusters


def _pick_clicks(clusters, coords_qv, num_obj, current_num_clicks, training):
    """The host half of utils/seg.py:173-226 (ranking, the one ``random.shuffle``, the click dictionaries)."""
    if not clusters:
        return None, None, None, None
    by_id = {c["cluster_id"]: c for c in clusters}
    # ranked by error size, largest first; equal sizes keep ascending-id order (stable sort)
    ranked = sorted(by_id, key=lambda cid: by_id[cid]["error_size"], reverse=True)
    if training:
        chosen = ranked[:num_obj] if len(ranked) >= num_obj else ranked
    else:
        chosen = ranked if current_num_clicks == 0 else ranked[:1]
    random.shuffle(chosen)
    new_clicks, new_pos, new_time = {}, {}, {}
    for order, cid in enumerate(chosen):
        c = by_id[cid]
        key = str(c["label"])
        new_clicks.setdefault(key, []).append(c["row"])
        new_pos.setdefault(key, []).append(coords_qv[c["row"]])
        new_time.setdefault(key, []).append(order)
    return new_clicks, len(chosen), new_pos, new_time


def pick_clicks_batch(clusters, labels, coords, current_num_clicks=None, training=True, num_objs=None):
    """The host half of ``get_simulated_clicks_batch`` for clusters that are already there (sample order: the global
    ``random`` stream is consumed exactly as by the per-sample loop).  ``num_objs`` (training): the number of objects per
    sample when the caller knows it -- saves a ``torch.unique`` + host round trip per sample and round."""
    out = []
    for i, cl in enumerate(clusters):
        num_obj = None
        if training and cl:
            num_obj = num_objs[i] if num_objs is not None else int((torch.unique(labels[i]) != 0).sum())
        out.append(_pick_clicks(cl, coords[i], num_obj, current_num_clicks, training))
    return out


def get_simulated_clicks_batch(preds, labels, coords, current_num_clicks=None, training=True, num_objs=None):
    """``get_simulated_clicks`` for every sample of a batch (engine.py:103-116 / eval_multi_obj.py:162-166 loop over the
    samples): the error clusters of all samples in one round (``error_clusters_batch``), the clicks then picked in sample
    order (``pick_clicks_batch``)."""
    return pick_clicks_batch(error_clusters_batch(preds, labels, coords), labels, coords, current_num_clicks, training, num_objs)


def get_simulated_clicks(pred_qv, labels_qv, coords_qv, current_num_clicks=None, training=True):
    """utils/seg.py:173-226.  Same returns: (new_clicks {str(label): [rows]}, click_num,
    new_click_pos {str(label): [xyz tensors]}, new_click_time {str(label): [order]}), or four Nones when
    the prediction is already right.  Consumes the global ``random`` stream like the reference
    (one ``random.shuffle`` of the selected cluster ids)."""
    clusters = error_clusters(pred_qv, labels_qv, coords_qv)
    num_obj = int((torch.unique(labels_qv) != 0).sum()) if training and clusters else None
    return _pick_clicks(clusters, coords_qv, num_obj, current_num_clicks, training)


def extend_clicks(current_clicks, current_clicks_time, new_clicks, new_click_time):
    """utils/seg.py:229-239."""
    offset = sum(len(v) for v in current_clicks_time.values())
    for obj_id, rows in new_clicks.items():
        current_clicks[obj_id].extend(rows)
        current_clicks_time[obj_id].extend(t + offset for t in new_click_time[obj_id])
    return current_clicks, current_clicks_time


def cal_click_loss_weights(batch_idx, raw_coords, labels, click_idx, alpha=0.8, beta=2.0, tita=0.3, ranges=None):
    """utils/seg.py:72-89: per sample, weights[i] = alpha + (beta-alpha)(1 - min(d_i, tita)/tita) with
    d_i the distance of point i to the nearest click of any object.  ``ranges`` [(first row, end row)] per sample, when the
    caller knows them (the rows of a sample are contiguous in a collated batch): no boolean-mask gathers, no host syncs."""
    lib = L.load()
    if not raw_coords.is_cuda:
        raise RuntimeError("cal_click_loss_weights runs on the GPU only")
    weights = []
    for i in range(len(ranges) if ranges is not None else int(batch_idx.max()) + 1):
        xyz = (raw_coords[ranges[i][0]:ranges[i][1]] if ranges is not None else raw_coords[batch_idx == i]).to(torch.float32).contiguous()
        r = click_lists(click_idx[i])[0]
        w = torch.empty(xyz.shape[0], dtype=torch.float32, device=xyz.device)
        L.check(lib.a3d_click_loss_weights(xyz.data_ptr(), xyz.shape[0], r.ctypes.data_as(_I32P), len(r), tita, alpha, beta,
                                           w.data_ptr(), L.stream(xyz.device)), "a3d_click_loss_weights")
        weights.append(w)
    return weights
