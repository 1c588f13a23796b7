"""The checks every marshalling module (``view.py``, ``decoder_ops.py``) makes on a tensor argument before the library is
reached: ``ValueError`` naming the argument."""
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
