"""The checks every marshalling module (``view.py``, ``decoder_ops.py``, ``backward.py``) makes on a tensor argument before the
library is reached: ``ValueError`` naming the argument."""
from __future__ import annotations

import torch

I32, I64, F32, U8 = torch.int32, torch.int64, torch.float32, torch.uint8


def _device(name, t):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a tensor on the GPU (there is no CPU path)")
    return t.device


def _ptr(name, t, dtype, shape, dev, optional=False):
    """The device pointer of tensor argument ``name`` (``shape``: ``None`` = any extent) -- ``None`` for a tensor without
    elements and for an absent ``optional`` one."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype is not dtype:
        raise ValueError(f"{name} must be a {dtype} tensor")
    if t.device != dev:
        raise ValueError(f"{name} must live on {dev}")
    got = t.shape
    if got != shape and (len(got) != len(shape) or any(s is not None and s != g for s, g in zip(shape, got))):
        raise ValueError(f"{name} must have shape {list(shape)} (None: any), not {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr() if t.numel() else None


def _out(name, t, dtype, shape, dev):
    """The output tensor ``name``: the caller's, checked, or a new one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    _ptr(name, t, dtype, shape, dev)
    return t


def _contig(name, t, shape, dev):
    """Input ``name`` (float32 of ``shape`` on ``dev``; None: any extent) as a contiguous tensor, copied if it is not one."""
    t = t.contiguous() if isinstance(t, torch.Tensor) else t
    _ptr(name, t, F32, shape, dev)
    return t


def _vectors(dev, C_, optional=False, **named):
    """Every named per-channel operand is a contiguous float32 [C_] on ``dev`` (``optional``: or None)."""
    for name, t in named.items():
        _ptr(name, t, F32, (C_,), dev, optional)


def _row_view(name, t, rows, C_, dev, out=False, more_rows=False):
    """Operand ``name`` as a row view the conv and BatchNorm kernels take in place (pointer + row stride): float32
    [rows, >= C_] (``more_rows``: rows or more) on ``dev``, unit channel stride, row stride a multiple of 4 floats.  An input
    in another layout is copied, an output (``out``) refused."""
    sh = t.shape if isinstance(t, torch.Tensor) else ()
    if len(sh) != 2 or t.dtype is not F32 or t.device != dev or sh[1] < C_ or (sh[0] < rows if more_rows else sh[0] != rows):
        raise ValueError(f"{name} must be a float32 [{rows}{' or more' if more_rows else ''}, >= {C_}] tensor on {dev}, not "
                         f"{getattr(t, 'dtype', type(t))} {list(sh)} on {getattr(t, 'device', None)}")
    if t.stride(1) == 1 and t.stride(0) % 4 == 0:
        return t
    if out:
        raise ValueError(f"{name} must have unit channel stride and a row stride of a multiple of 4 floats (it is written in "
                         f"place), not strides {t.stride()}")
    return t.contiguous()
