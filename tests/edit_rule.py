"""The rules of an edit of the session's click list restated in numpy, for ``test_session_edit_host.py`` (CPU) and
``test_gpu_session_edit.py`` (not collected, like ``pick_rule.py``).  Stated in include/agile3d_hip.h at ``a3d_session_edit``
and in ``agile3d_amd/session.py``; written here a second time, independently: numpy only, no import of the package.

``relabel_numpy``   a3d_session_edit's relabel half.
``remap_numpy``     its remap half.
``list_truth``      the relabelled ground truth of a click list, from ``(obj, voxel row)`` pairs in time order.
``removal_lut``     the old -> new id table of removing an object.
"""
import numpy as np


def relabel_numpy(labels_ori, instances):
    """int32 [n]: the largest k in 1..K with ``instances[k - 1] == labels_ori[i]``, else 0.  Objects are written in
    ascending order, so where two stand for one instance the higher id is what remains."""
    labels_ori = np.asarray(labels_ori, np.int32)
    out = np.zeros(labels_ori.shape, np.int32)
    for k, inst in enumerate(np.asarray(instances, np.int32).reshape(-1), start=1):
        out[labels_ori == inst] = k
    return out


def remap_numpy(labels, lut):
    """``(int32 [n], flag)``: ``lut[labels]`` with 0 where a label lies outside 0..255; flag 1 if any did, else 0."""
    labels, lut = np.asarray(labels, np.int32), np.asarray(lut, np.uint8)
    assert lut.shape == (256,)
    ok = (labels >= 0) & (labels <= 255)
    return np.where(ok, lut[np.where(ok, labels, 0)], 0).astype(np.int32), int(not ok.all())


def list_truth(pairs, labels_qv_ori, labels_full_ori):
    """int32 [n_full] for ``pairs`` = [(obj, voxel row), ...] in time order: object k's instance is the original label of
    the voxel under its EARLIEST click; a vertex gets the highest object whose instance it carries."""
    n_obj = max([o for o, _ in pairs], default=0)
    instances = [next(int(labels_qv_ori[r]) for o, r in pairs if o == k) for k in range(1, n_obj + 1)]
    return relabel_numpy(labels_full_ori, instances)


def removal_lut(k):
    """uint8 [256]: removed id ``k`` -> 0, j -> j - 1 above it, j -> j below (``k`` None: the identity)."""
    lut = np.arange(256)
    if k is not None:
        lut = np.where(lut == k, 0, np.where(lut > k, lut - 1, lut))
    return lut.astype(np.uint8)
