"""The rules of ``a3d_session_guide`` (include/agile3d_hip.h) restated in numpy, independently of the package (not
collected; numpy only, no import of ``agile3d_amd``).  The scans are written as the header words them -- column by column,
replace on ``>`` -- and every fp32 operation is a single numpy float32 operation, so the kernel is held to these bit for
bit."""
import numpy as np

F32 = np.float32
NAN_MARGIN, BAD_INDEX = 1, 2                     # the bits of the error word


def first_max(logits, skip=None):
    """Per row the column of the FIRST maximum: scan from column 0 (over the columns other than ``skip[row]``, when given),
    replace on ``>``.  A NaN never replaces and is never replaced."""
    x = np.asarray(logits, F32)
    n, c = x.shape
    rows = np.arange(n)
    arg = np.zeros(n, np.int64) if skip is None else np.where(np.asarray(skip) == 0, 1, 0)
    best = x[rows, arg]
    for col in range(c):
        with np.errstate(invalid="ignore"):
            take = x[:, col] > best
        take &= col > arg                         # (the scan starts behind its first column)
        if skip is not None:
            take &= col != skip
        best = np.where(take, x[:, col], best)
        arg = np.where(take, col, arg)
    return arg


def guide_numpy(logits, click_rows, click_objs, threshold):
    """``dict(label, runner, margin, want, contested, voxels, contested_per_label, least, err)``: int32 labels, runner-ups
    and wanted labels, fp32 margins, the bool contested mask, int64 [256] counts, ``least`` = ``(row, margin)`` of the
    smallest FINITE margin (ties: the lowest row) or ``None``, ``err`` = ``NAN_MARGIN`` if a row's margin is NaN."""
    x = np.ascontiguousarray(logits, F32)
    n, c = x.shape
    assert 2 <= c <= 256
    rows = np.arange(n)
    label = first_max(x)
    runner = first_max(x, skip=label)
    with np.errstate(invalid="ignore"):
        margin = (x[rows, label] - x[rows, runner]).astype(F32)
    err = NAN_MARGIN if np.isnan(margin).any() else 0
    for r, o in zip(click_rows, click_objs):      # in order: the last entry of a row wins
        if 0 <= r < n:
            label[r] = runner[r] = o
            margin[r] = np.inf
    with np.errstate(invalid="ignore"):
        contested = margin < F32(threshold)
    want = np.where(contested, runner, label)
    finite = np.isfinite(margin)
    least = None
    if finite.any():
        m = margin[finite].min()
        row = int(np.flatnonzero(finite & (margin == m))[0])
        least = (row, float(margin[row]))
    return dict(label=label.astype(np.int32), runner=runner.astype(np.int32), margin=margin, want=want.astype(np.int32),
                contested=contested, voxels=np.bincount(label, minlength=256).astype(np.int64),
                contested_per_label=np.bincount(label[contested], minlength=256).astype(np.int64), least=least, err=err)


def lift_numpy(values_qv, inverse_map, sentinel):
    """``(values[inverse_map], valid, err)``: entries outside ``0 .. n_qv - 1`` keep ``sentinel`` and raise ``BAD_INDEX``;
    ``inverse_map`` ``None`` is the identity."""
    v = np.asarray(values_qv)
    inv = np.arange(len(v)) if inverse_map is None else np.asarray(inverse_map, np.int64)
    valid = (inv >= 0) & (inv < len(v))
    out = np.full(inv.shape + v.shape[1:], sentinel, v.dtype)
    out[valid] = v[inv[valid]]
    return out, valid, (0 if valid.all() else BAD_INDEX)


def blend_numpy(label_full, margin_full, colors_full, palette, doubt, full_margin):
    """fp32 [n, 3]: ``base * s + doubt * (1 - s)`` with ``s = x if x < 1 else 1``, ``x = margin * (1 / full_margin)``;
    ``base`` = the palette entry of a label > 0 (labels >= len(palette) wrap over entries 1 .. len - 1), the vertex's own
    colour for label 0.  One float32 operation at a time."""
    lab = np.asarray(label_full, np.int64)
    pal = np.asarray(palette, F32)
    k = len(pal)
    entry = np.where(lab < k, lab, 1 + (lab - 1) % (k - 1))
    base = np.where((lab > 0)[:, None], pal[np.clip(entry, 0, k - 1)], np.asarray(colors_full, F32))
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.asarray(margin_full, F32) * (F32(1.0) / F32(full_margin))
        s = np.where(x < F32(1.0), x, F32(1.0)).astype(F32)
        w = F32(1.0) - s
        first = (base * s[:, None]).astype(F32)
        second = (np.asarray(doubt, F32)[None, :] * w[:, None]).astype(F32)
        return (first + second).astype(F32)
