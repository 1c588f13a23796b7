"""Backward of the sparse convolutions (first part of SURVEY.md section 8 row f-2, the training path):

    conv_input_grad(scene, kind, level_in, w, dy)        dL/dx of conv / conv_tr (models/modules/common.py:125-188)
    conv_weight_grad(scene, kind, level_in, x, dy, K)    dL/dW [K, Cin, Cout]

for the four kernel-map kinds of the backbone (3^3 stride 1, 2^3 stride 2, 2^3 transposed, 1x1) -- what autograd does
inside MinkowskiEngine for ``engine.py:137-150`` (``losses.backward()``) -- plus the wrappers of the other training
kernels (BatchNorm in training mode, LayerNorm, column sums, the input conv's forward and weight gradient): the one place
where these calls are marshalled, as ``decoder_ops.py`` is for the decoder's.  The tapes that string them together are
``train_backbone.py`` / ``train_decoder.py``; the iteration is ``train_step.py``.

The input gradient needs no new kernel: it is the FORWARD kernel on the transposed kernel map with transposed
weights -- for the 3^3 stride-1 map offset k of row i is row j exactly when offset 26-k of j is i, so
dx = conv3(dy, W'[k] = W[26-k]^T) on the same neighbour tables; the stride-2 conv's input gradient is the transposed
conv with W_s^T and vice versa; 1x1 is a GEMM with W^T.  The weight gradient is its own kernel (csrc/wgrad.hip).
All tensors are in the scene's internal row order (the order of the op program's activation buffers), on the GPU.

Every tensor operand is checked before the library is reached -- dtype, device (the scene's, else ``x``'s), the rows the
scene's level asks for (``n + 1`` where a kernel gathers or writes the zero row), the channels the call uses -- and refused
with a ``ValueError`` naming the argument (``RuntimeError`` where a CPU tensor always was).  A [rows, C] operand of the conv
and BatchNorm kernels is a row view (``_args._row_view``: pointer + row stride, a column slice of a wider buffer is never
copied; an input in another layout is copied, an output refused); everything else must be contiguous (``_args._ptr``).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import lib as L
from ._args import F32, _contig, _device, _ptr, _row_view as _view, _vectors

_KVOL = {L.OP_CONV3: 27, L.OP_DOWN: 8, L.OP_UP: 8, L.OP_LINEAR: 1}
BACK_KIND = {L.OP_CONV3: L.OP_CONV3, L.OP_DOWN: L.OP_UP, L.OP_UP: L.OP_DOWN, L.OP_LINEAR: L.OP_LINEAR}   # forward -> input gradient
_GPU_ONLY = "agile3d_amd.backward runs on the GPU only (fp32 CUDA tensors)"

_arena: dict = {}
_POISON = os.environ.get("A3D_POISON", "0") == "1"   # debugging aid, see tests/conftest.py


def _workspace(nbytes, device, tag):
    """The scratch of a call whose ``*_workspace_bytes`` answered ``nbytes`` (0: the library refuses the sizes, raised with
    its message): one growing allocation per (device, stream, tag) -- the training tapes issue hundreds of calls per
    iteration on one stream, each used to allocate (and zero) its own -- or, ``tag`` None, a new one of just that size."""
    if nbytes == 0:
        raise L.A3DError(L.load().a3d_last_error().decode() or "the library refuses these sizes")
    if tag is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, tag)
    ws = _arena.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _arena[key] = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
    if _POISON:
        ws.fill_(255)   # NaN patterns: a kernel that reads scratch it did not write shows up in the results
    return ws


def _ws(n, C_, device):
    return _workspace(L.load().a3d_bn_workspace_bytes(n, C_), device, "bn")


def _channels(C_, device):
    """Two new per-channel vectors (mean and rstd, dgamma and dbeta)."""
    return torch.empty(C_, dtype=F32, device=device), torch.empty(C_, dtype=F32, device=device)


def _dims(name, t):
    """(device, rows, channels) of the [rows, C] operand that sets the sizes of a BatchNorm / LayerNorm call."""
    if _device(name, t) and t.dim() != 2:
        raise ValueError(f"{name} must be [rows, channels], not {list(t.shape)}")
    return t.device, t.shape[0], t.shape[1]


def _take(state):
    return state.take() if state is not None else None


class StateArena:
    """The conv kernels' hand-off state (ticket, failure word, flags: a3d_conv_state_bytes() per launch) for every conv of
    a training iteration, zeroed with ONE memset when the tape starts instead of one per launch."""

    def __init__(self, device, slots):
        self.bytes = int(L.load().a3d_conv_state_bytes())
        self.buf = torch.zeros(slots * self.bytes, dtype=torch.uint8, device=device)
        self.next, self.slots = 0, slots

    def take(self):
        if self.next >= self.slots:          # more launches than planned: a fresh zeroed block
            self.buf = torch.zeros(self.slots * self.bytes, dtype=torch.uint8, device=self.buf.device)
            self.next = 0
        p = self.buf.data_ptr() + self.next * self.bytes
        self.next += 1
        return C.c_void_p(p)


def level_out(kind, level_in):
    return level_in + (1 if kind == L.OP_DOWN else -1 if kind == L.OP_UP else 0)


def _conv_dims(scene, kind, level_in):
    """(the scene's device, output level, input rows, output rows) of an op of ``kind`` from ``level_in``."""
    lo = level_out(kind, level_in)
    if not (0 <= level_in < len(scene.n) and 0 <= lo < len(scene.n)):
        raise ValueError(f"kind {kind} from level {level_in} leaves the scene's {len(scene.n)} levels")
    return scene.workspace.device, lo, scene.n[level_in], scene.n[lo]


def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[K, Cin, Cout] (ME layout) -> the MFMA fragment order the conv kernels read (a3d_pack_conv_weight)."""
    lib = L.load()
    dev = _device("w", w)
    w = _contig("w", w, (None, None, None), dev)
    out = torch.empty(lib.a3d_conv_weight_packed_floats(w.shape[0], w.shape[1], w.shape[2]), dtype=F32, device=dev)
    L.check(lib.a3d_pack_conv_weight(L.ptr(w), w.shape[0], w.shape[1], w.shape[2], L.ptr(out), L.stream()), "a3d_pack_conv_weight")
    return out


def pack_weights_multi(table, n_jobs, n_chunks):
    """a3d_pack_conv_weights_multi: every job of ``table`` (lib.pack_job_table) repacked by one launch."""
    tp = _ptr("table", table, torch.uint8, (n_jobs * L.PACK_JOB.itemsize,), _device("table", table))
    L.check(L.load().a3d_pack_conv_weights_multi(tp, n_jobs, n_chunks, L.stream()), "a3d_pack_conv_weights_multi")


def input_grad_slices(cin):
    """[(first column, width)] of the launches that write the ``cin`` columns of an input gradient: the conv kernels write
    32 / 64 / 96 or a multiple of 128 output columns, so the concatenated inputs of the decoder blocks (192 = 128 + 64
    channels) get their gradient in column slices."""
    slices, c0 = [], 0
    while c0 < cin:
        rest = cin - c0
        width = rest if (rest % 128 == 0 or rest in (32, 64, 96)) else max(w_ for w_ in (128, 96, 64, 32) if w_ <= rest)
        slices.append((c0, width))
        c0 += width
    return slices


def _input_grad_weight(kind, w):
    """W' [K, Cout, Cin] of the input-gradient conv of y = conv(x; w): W^T, and for the 3^3 map the offsets reversed (offset k
    of the backward map is offset 26-k of the forward map)."""
    wt = w.transpose(1, 2)
    return wt.flip(0) if kind == L.OP_CONV3 else wt


def packed_input_grad_weights(kind, w: torch.Tensor):
    """The packed weight slices of the input-gradient conv of y = conv(x; w): [(first input channel, width, packed)]."""
    wt = _input_grad_weight(kind, w)
    return [(c0, width, pack_weight(wt[:, :, c0:c0 + width].contiguous())) for c0, width in input_grad_slices(w.shape[1])]


def _run_op(scene, kind, level_in, cin, cout, kernel_volume, w, x=None, feats3=None):
    """A one-op program on ``scene``: ``x`` [n_in, cin] is copied into the program's input buffer (OP_STEM reads the
    caller-ordered ``feats3`` instead) -> a new [n_out + 1, cout] in the internal row order, the zero row last."""
    lib = L.load()
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    descs = ([L.BufDesc(level_in, cin)] if x is not None else []) + [L.BufDesc(lo, cout)]
    nb = len(descs)
    bufs = (L.BufDesc * nb)(*descs)
    o = L.Op()
    o.kind, o.level_in, o.cin, o.cout = kind, level_in, cin, cout
    o.in_buf, o.in_coff, o.out_buf, o.out_coff = (0 if x is not None else L.BUF_NONE), 0, nb - 1, 0
    o.res_buf, o.res_coff, o.relu, o.kernel_volume = L.BUF_NONE, 0, 0, kernel_volume
    o.w_dev, o.scale_dev, o.shift_dev = w.data_ptr(), None, None
    ops = (L.Op * 1)(o)
    nbytes = lib.a3d_program_workspace_bytes(scene.handle, bufs, nb, ops, 1)
    ws = _workspace(nbytes, dev, "program")

    def view(i, rows, ch):
        off = lib.a3d_program_buffer_offset(scene.handle, bufs, nb, i)
        return ws[off:off + (rows + 1) * ch * 4].view(F32).view(rows + 1, ch)
    if x is not None:
        ws[:nbytes].zero_()                  # the input's zero row
        view(0, n_in, cin)[:n_in].copy_(x)
    L.check(lib.a3d_program_run(scene.handle, bufs, nb, ops, 1, L.ptr(feats3), None, 0, L.ptr(ws), nbytes, L.stream()),
            "a3d_program_run")
    return view(nb - 1, n_out, cout).clone()


def run_conv(scene, kind, level_in, w_packed, x, cin, cout):
    """One conv of the op program on its own: x [n_in, cin] -> [n_out, cout] (no BatchNorm / ReLU / residual)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32:
        raise RuntimeError(_GPU_ONLY)
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    if x.shape != (n_in, cin):
        raise ValueError(f"input must be [{n_in}, {cin}], got {tuple(x.shape)}")
    _ptr("w_packed", w_packed, F32, (None,), dev)
    return _run_op(scene, kind, level_in, cin, cout, _KVOL[kind], w_packed, x=x)[:n_out]


def stem_forward(scene, w, feats3, kernel_volume):
    """conv0p1s1 on its own (OP_STEM reads the caller-ordered features ``feats3`` [n0, 3]; ``w`` [K, 3, 32], not packed)
    -> [n0 + 1, 32] in the internal row order, zero row last."""
    dev = scene.workspace.device
    _ptr("feats3", feats3, F32, (scene.n[0], 3), dev), _ptr("w", w, F32, (kernel_volume, 3, 32), dev)
    return _run_op(scene, L.OP_STEM, 0, 3, 32, kernel_volume, w, feats3=feats3)


def conv_apply(scene, kind, level_in, w_packed, x, cin, cout, out=None, out_cols=None, zero_row=True):
    """a3d_conv_apply: one conv directly on the caller's tensors.  ``x`` [n_in + 1, ldx] with its zero row (row n_in);
    returns y [n_out + 1, cout] (row n_out zeroed) or writes ``cout`` columns into ``out[:, out_cols[0]:]``."""
    lib = L.load()
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    xp, wp = _ptr("x", x, F32, (n_in + 1, None), dev), _ptr("w_packed", w_packed, F32, (None,), dev)
    if out is None:
        out = torch.empty((n_out + 1, cout), dtype=F32, device=dev)
    else:
        _ptr("out", out, F32, (n_out + 1, None), dev)
    y = out[:, out_cols[0]:] if out_cols else out
    if x.shape[1] < cin or y.shape[1] < cout:
        raise ValueError(f"x must have {cin} columns and out {cout} from out_cols[0] on, not {x.shape[1]} and {y.shape[1]}")
    ws = _workspace(lib.a3d_conv_apply_workspace_bytes(scene.handle, kind, level_in, cin, cout), dev, "conv")
    L.check(lib.a3d_conv_apply(scene.handle, kind, level_in, xp, x.shape[1], cin, wp, cout, y.data_ptr(), out.shape[1],
                               int(zero_row), L.ptr(ws), ws.numel(), L.stream()), "a3d_conv_apply")
    return out


def _conv_acc(scene, kind, level_in, wp, x, cin, cout, y, acc, zero_row, state):
    """a3d_conv_apply_acc on checked operands."""
    lib = L.load()
    ws = _workspace(lib.a3d_conv_apply_workspace_bytes(scene.handle, kind, level_in, cin, cout), x.device, "conv")
    L.check(lib.a3d_conv_apply_acc(scene.handle, kind, level_in, L.ptr(x), x.stride(0), cin, L.ptr(wp), cout, L.ptr(y),
                                   y.stride(0), int(zero_row), L.ptr(y) if acc else None, y.stride(0) if acc else 0,
                                   _take(state), L.ptr(ws), ws.numel(), L.stream()), "a3d_conv_apply_acc")
    return y


def conv_apply_acc(scene, kind, level_in, w_packed, x, cin, cout, y, acc=False, zero_row=True, state=None):
    """a3d_conv_apply_acc: y[:, :cout] (a [n_out + 1, >= cout] view, any row stride) = conv(x) (+ y when ``acc``: the
    accumulation happens in the conv kernel's epilogue).  ``x`` [n_in + 1, >= cin] view carrying the zero row."""
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    x = _view("x", x, n_in + 1, cin, dev)
    _view("y", y, n_out + 1, cout, dev, out=True), _ptr("w_packed", w_packed, F32, (None,), dev)
    return _conv_acc(scene, kind, level_in, w_packed, x, cin, cout, y, acc, zero_row, state)


def conv_input_grad_into(scene, kind, level_in, parts, dy, cin, cout, out, acc=False, state=None):
    """dL/dx written (or, with ``acc``, added in the kernels' epilogues) into ``out`` [n_in + 1, >= cin] (a view: the
    gradient buffer of a node, possibly a column slice of a concatenation's); ``dy`` [n_out + 1, cout] with its zero row;
    ``parts`` = packed_input_grad_weights of the forward weight."""
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    dy = _view("dy", dy, n_out + 1, cout, dev)
    _view("out", out, n_in + 1, cin, dev, out=True)
    for c0, width, wp in parts:
        _ptr("parts", wp, F32, (None,), dev)
        if not 0 <= c0 <= cin - width:
            raise ValueError(f"parts must lie within the {cin} input channels, not reach [{c0}, {c0 + width})")
    for c0, width, wp in parts:
        _conv_acc(scene, BACK_KIND[kind], lo, wp, dy, cout, width, out[:, c0:c0 + width], acc, True, state)
    return out


def conv_bn_train_forward(scene, kind, level_in, w_packed, x, cin, cout, gamma, beta, eps, res, relu, y, running_mean,
                          running_var, momentum, state=None):
    """a3d_conv_bn_train_forward: raw = conv(x); y = relu?(BatchNorm_train(raw) (+ res)) with the batch statistics taken
    in the conv kernel's epilogue.  ``x`` [n_in + 1, >= cin] view with its zero row, ``y`` [n_out + 1, >= cout] view (row
    n_out is written as zeros), ``res`` [>= n_out, >= cout] view or None.  Returns (raw [n_out, cout], mean, rstd)."""
    lib = L.load()
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    x = _view("x", x, n_in + 1, cin, dev)
    res = _view("res", res, n_out, cout, dev, more_rows=True) if res is not None else None
    _view("y", y, n_out + 1, cout, dev, out=True), _ptr("w_packed", w_packed, F32, (None,), dev)
    _vectors(dev, cout, gamma=gamma, beta=beta)
    _vectors(dev, cout, True, running_mean=running_mean, running_var=running_var)
    raw = torch.empty((n_out, cout), dtype=F32, device=dev)
    mean, rstd = _channels(cout, dev)
    ws = _workspace(lib.a3d_conv_bn_train_workspace_bytes(scene.handle, kind, level_in, cin, cout), dev, "convbn")
    L.check(lib.a3d_conv_bn_train_forward(scene.handle, kind, level_in, L.ptr(x), x.stride(0), cin, L.ptr(w_packed), cout,
                                          L.ptr(raw), cout, L.ptr(gamma), L.ptr(beta), eps, L.ptr(res),
                                          res.stride(0) if res is not None else 0, int(relu), L.ptr(y), y.stride(0), 1,
                                          L.ptr(mean), L.ptr(rstd), L.ptr(running_mean), L.ptr(running_var), momentum,
                                          _take(state), L.ptr(ws), ws.numel(), L.stream()), "a3d_conv_bn_train_forward")
    return raw, mean, rstd


def conv_dgrad_bn(scene, kind, level_in, part, dy, cout_fwd, out, acc, y, raw, mean, rstd, relu, state=None):
    """a3d_conv_dgrad_bn for the conv y' = conv(x; w) of kind / level_in (FORWARD op) whose input x is the output of a
    BatchNorm(+ReLU) unit (y, raw, mean, rstd): ``out`` [n_in + 1, cin] gets g = (dL/dx (+ out when ``acc``)) masked by y > 0;
    returns the fp64 sums [2, cin] (sum g, sum g xhat).  ``part`` = the single (c0 = 0, width = cin, packed) entry of
    packed_input_grad_weights, ``dy`` [n_out + 1, cout_fwd] with its zero row; ``y`` [>= n_in, cin] (read with ``relu``
    only) and ``raw`` [n_in, cin] views."""
    lib = L.load()
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    c0, width, wp = part
    if c0 != 0:
        raise ValueError(f"part must be the single slice of the input gradient, not one from column {c0}")
    dy, raw = _view("dy", dy, n_out + 1, cout_fwd, dev), _view("raw", raw, n_in, width, dev)
    yy = _view("y", y, n_in, width, dev, more_rows=True) if relu else None
    _view("out", out, n_in + 1, width, dev, out=True), _ptr("part", wp, F32, (None,), dev)
    _vectors(dev, width, mean=mean, rstd=rstd)
    back_kind = BACK_KIND[kind]
    ws = _workspace(lib.a3d_conv_bn_train_workspace_bytes(scene.handle, back_kind, lo, cout_fwd, width), dev, "convbn")
    sums = torch.empty((2, width), dtype=torch.float64, device=dev)
    L.check(lib.a3d_conv_dgrad_bn(scene.handle, back_kind, lo, L.ptr(dy), dy.stride(0), cout_fwd, L.ptr(wp), width, L.ptr(out),
                                  out.stride(0), int(acc), L.ptr(yy), yy.stride(0) if yy is not None else 0, L.ptr(raw),
                                  raw.stride(0), L.ptr(mean), L.ptr(rstd), int(relu), L.ptr(sums), _take(state), L.ptr(ws),
                                  ws.numel(), L.stream()), "a3d_conv_dgrad_bn")
    return sums


def conv_input_grad(scene, kind, level_in, w: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dL/dx [n_in, Cin] of y = conv(x; W) from dL/dy [n_out, Cout]; ``w`` is the forward weight [K, Cin, Cout]."""
    K, cin, cout = w.shape
    if K != _KVOL[kind]:
        raise ValueError(f"kind {kind} needs kernel volume {_KVOL[kind]}, got {K}")
    dy = dy.contiguous()
    parts = [run_conv(scene, BACK_KIND[kind], level_out(kind, level_in), wp, dy, cout, width)
             for c0, width, wp in packed_input_grad_weights(kind, w)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 1)


def conv_weight_grad(scene, kind, level_in, x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dL/dW [K, Cin, Cout] = sum over the kernel map's (input row, output row) pairs of offset k of x_in^T dy_out."""
    lib = L.load()
    if not (isinstance(x, torch.Tensor) and isinstance(dy, torch.Tensor) and x.is_cuda and dy.is_cuda and
            x.dtype == dy.dtype == F32):
        raise RuntimeError(_GPU_ONLY)
    dev, lo, n_in, n_out = _conv_dims(scene, kind, level_in)
    if x.dim() != 2 or dy.dim() != 2 or x.shape[0] != n_in or dy.shape[0] != n_out:
        raise ValueError("x / dy row counts do not match the scene levels")
    cin, cout = x.shape[1], dy.shape[1]
    x, dy = _view("x", x, n_in, cin, dev), _view("dy", dy, n_out, cout, dev)
    dw = torch.empty((_KVOL[kind], cin, cout), dtype=F32, device=dev)
    scene.prepare_wgrad()
    ws = _workspace(lib.a3d_conv_wgrad_workspace_bytes(scene.handle, kind, level_in, cin, cout), dev, "wgrad")
    L.check(lib.a3d_conv_wgrad(scene.handle, kind, level_in, L.ptr(x), x.stride(0), L.ptr(dy), dy.stride(0), cin, cout,
                               L.ptr(dw), L.ptr(ws), ws.numel(), L.stream()), "a3d_conv_wgrad")
    return dw


def stem_weight_grad(scene, feats3, dy, kernel_volume=125):
    """dW [K, 3, 32] of the input convolution; ``feats3`` [n0, 3] in the caller's row order, ``dy`` [n0, 32] internal."""
    lib = L.load()
    dev, n0 = scene.workspace.device, scene.n[0]
    feats3, dy = _contig("feats3", feats3, (n0, 3), dev), _view("dy", dy, n0, 32, dev)
    if kernel_volume not in (125, 27):       # (the byte count below answers 0 for it, but the library leaves no message)
        raise L.A3DError("stem_weight_grad: kernel volume must be 125 or 27")
    dw = torch.empty((kernel_volume, 3, 32), dtype=F32, device=dev)
    ws = _workspace(lib.a3d_stem_wgrad_scene_workspace_bytes(scene.handle, kernel_volume), dev, "stem_wgrad")
    L.check(lib.a3d_stem_wgrad(scene.handle, L.ptr(feats3), L.ptr(dy), dy.stride(0), kernel_volume, L.ptr(dw), L.ptr(ws),
                               ws.numel(), L.stream()), "a3d_stem_wgrad")
    return dw


def bn_train_forward(x, gamma, beta, eps=1e-5, res=None, relu=False, running_mean=None, running_var=None, momentum=0.1,
                     zero_row=False):
    """ME.MinkowskiBatchNorm in training mode (+ residual, + ReLU): returns (y, save_mean, save_rstd); running
    statistics, when given, are updated in place like torch's.  ``zero_row``: y gets one extra all-zero row (what a
    missing neighbour gathers when y feeds a3d_conv_apply)."""
    lib = L.load()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != F32:
        raise RuntimeError(_GPU_ONLY)
    dev, n, C_ = _dims("x", x)
    x = x.contiguous()
    res = _contig("res", res, (n, C_), dev) if res is not None else None
    _vectors(dev, C_, gamma=gamma, beta=beta)
    _vectors(dev, C_, True, running_mean=running_mean, running_var=running_var)
    y = torch.empty((n + 1 if zero_row else n, C_), dtype=F32, device=dev)
    mean, rstd = _channels(C_, dev)
    ws = _ws(n, C_, dev)
    L.check(lib.a3d_bn_train_forward(L.ptr(x), C_, n, C_, L.ptr(gamma), L.ptr(beta), eps, L.ptr(res), C_, int(relu), L.ptr(y),
                                     C_, L.ptr(mean), L.ptr(rstd), L.ptr(running_mean), L.ptr(running_var), momentum,
                                     int(zero_row), L.ptr(ws), ws.numel(), L.stream()), "a3d_bn_train_forward")
    return y, mean, rstd


def _bn_operands(x, y, dy, gamma, mean, rstd, relu, zero_row=True, **outputs):
    """The checked operands of a BatchNorm backward over x [n, C] -> (n, C, x, y or None, dy) as row views; gamma / mean /
    rstd are [C], the caller's ``outputs`` (dx, dres; or None) [n + 1, >= C] row views ([n, >= C] without ``zero_row``)."""
    dev, n, C_ = _dims("x", x)
    x, dy = _view("x", x, n, C_, dev), _view("dy", dy, n, C_, dev, more_rows=True)
    y = _view("y", y, n, C_, dev, more_rows=True) if relu else None
    _vectors(dev, C_, gamma=gamma, mean=mean, rstd=rstd)
    for name, t in outputs.items():
        if t is not None:
            _view(name, t, n + 1 if zero_row else n, C_, dev, out=True)
    return n, C_, x, y, dy


def _ld(t, absent=0):
    return t.stride(0) if t is not None else absent


def _bn_backward_apply(x, y, dy, n, C_, gamma, mean, rstd, relu, sums, n_global, local, dx, dres, zero_row, absent_ld=0):
    """a3d_bn_backward_apply on checked row views: dx (and dres) from the global fp64 ``sums`` [2, C] over ``n_global`` rows,
    dgamma / dbeta from this rank's ``local`` sums -> (dgamma, dbeta).  ``absent_ld``: the row stride stated for an absent
    y / dres (the library does not read it)."""
    dgamma, dbeta = _channels(C_, x.device)
    L.check(L.load().a3d_bn_backward_apply(L.ptr(x), x.stride(0), L.ptr(y), _ld(y, absent_ld), L.ptr(dy), dy.stride(0), n, C_,
                                           L.ptr(gamma), L.ptr(mean), L.ptr(rstd), int(relu), L.ptr(sums), int(n_global),
                                           L.ptr(local), L.ptr(dx), dx.stride(0), L.ptr(dres), _ld(dres, absent_ld),
                                           L.ptr(dgamma), L.ptr(dbeta), int(zero_row), L.stream()), "a3d_bn_backward_apply")
    return dgamma, dbeta


def bn_backward_from_sums(x, g, gamma, mean, rstd, sums, dx):
    """BatchNorm backward from the sums a3d_conv_dgrad_bn produced: g [>= n, C] (already masked by the ReLU), x = raw [n, C],
    dx [n + 1, C] (row n written as zeros).  Returns (dgamma, dbeta)."""
    dev, n, C_ = _dims("x", x)
    x, g = _view("x", x, n, C_, dev), _view("g", g, n, C_, dev, more_rows=True)
    _view("dx", dx, n + 1, C_, dev, out=True), _ptr("sums", sums, torch.float64, (2, C_), dev)
    _vectors(dev, C_, gamma=gamma, mean=mean, rstd=rstd)
    return _bn_backward_apply(x, None, g, n, C_, gamma, mean, rstd, False, sums, n, sums, dx, None, 1)


def bn_train_backward_into(x, y, dy, gamma, mean, rstd, relu, dx, dres=None, zero_row=True):
    """a3d_bn_train_backward on views: x (raw) [n, C], y / dy [>= n, C] views (any row stride), dx [n + 1, C] (row n is
    written as zeros; [n, C] without ``zero_row``), dres view like dx or None.  Returns (dgamma, dbeta)."""
    n, C_, x, yy, dy = _bn_operands(x, y, dy, gamma, mean, rstd, relu, zero_row, dx=dx, dres=dres)
    dgamma, dbeta = _channels(C_, x.device)
    ws = _ws(n, C_, x.device)
    L.check(L.load().a3d_bn_train_backward(L.ptr(x), x.stride(0), L.ptr(yy), _ld(yy), L.ptr(dy), dy.stride(0), n, C_,
                                           L.ptr(gamma), L.ptr(mean), L.ptr(rstd), int(relu), L.ptr(dx), dx.stride(0), L.ptr(dres),
                                           _ld(dres), L.ptr(dgamma), L.ptr(dbeta), int(zero_row), L.ptr(ws), ws.numel(),
                                           L.stream()), "a3d_bn_train_backward")
    return dgamma, dbeta


def _bn_outputs(x, want_dres, zero_row):
    dev, n, C_ = _dims("x", x)
    dx = torch.empty((n + 1 if zero_row else n, C_), dtype=F32, device=dev)
    return dx, torch.empty_like(dx) if want_dres else None


def bn_train_backward(x, y, dy, gamma, mean, rstd, relu=False, want_dres=False, zero_row=False):
    """-> (dx, dgamma, dbeta, dres or None); ``y`` (the forward output) gives the ReLU mask.  ``zero_row``: dx / dres get
    one extra all-zero row (they feed a3d_conv_apply as the input-gradient convs' dy)."""
    dx, dres = _bn_outputs(x, want_dres, zero_row)
    dgamma, dbeta = bn_train_backward_into(x, y, dy, gamma, mean, rstd, relu, dx, dres, zero_row)
    return dx, dgamma, dbeta, dres


def bn_sync_forward(x, gamma, beta, eps=1e-5, res=None, relu=False, running_mean=None, running_var=None, momentum=0.1,
                    group=None, zero_row=False):
    """BatchNorm in training mode with statistics over the rows of ALL data-parallel ranks (SyncBN): the reference
    normalises over every row of the batch on one device (models/modules/common.py:20-22); with the batch's scenes
    spread over ranks the strict equivalent exchanges [2C+1] numbers per layer.  Per rank: row
    count, mean, sum of squared deviations (a3d_bn_local_stats, fp64) -> one all_gather -> Chan's parallel combination
    -> the same mean / rstd on every rank -> a3d_bn_apply.  Returns (y, mean, rstd, n_global)."""
    from .optim import dist_all_gather
    lib = L.load()
    dev, n, C_ = _dims("x", x)
    x = _contig("x", x, (n, C_), dev)
    res = _contig("res", res, (n, C_), dev) if res is not None else None
    _vectors(dev, C_, gamma=gamma, beta=beta)
    _vectors(dev, C_, True, running_mean=running_mean, running_var=running_var)
    ws = _ws(n, C_, dev)
    st = torch.empty(2 * C_ + 1, dtype=torch.float64, device=dev)
    L.check(lib.a3d_bn_local_stats(L.ptr(x), C_, n, C_, L.ptr(st), L.ptr(ws), ws.numel(), L.stream()), "a3d_bn_local_stats")
    st[2 * C_] = float(n)
    allst = dist_all_gather(st, group)                           # [world, 2C+1]
    cnt = allst[:, 2 * C_:2 * C_ + 1]                            # [world, 1]
    n_glob = cnt.sum()
    mean = (allst[:, :C_] * cnt).sum(0) / n_glob
    m2 = (allst[:, C_:2 * C_] + cnt * (allst[:, :C_] - mean) ** 2).sum(0)
    var = m2 / n_glob
    mean_f = mean.to(F32)
    rstd = (1.0 / torch.sqrt(var.to(F32) + eps))
    if running_mean is not None:
        unbiased = (m2 / (n_glob - 1.0)).to(F32) if float(n_glob) > 1 else var.to(F32)
        running_mean.mul_(1.0 - momentum).add_(mean_f, alpha=momentum)
        running_var.mul_(1.0 - momentum).add_(unbiased, alpha=momentum)
    y = torch.empty((n + 1 if zero_row else n, C_), dtype=F32, device=dev)
    L.check(lib.a3d_bn_apply(L.ptr(x), C_, n, C_, L.ptr(gamma), L.ptr(beta), L.ptr(mean_f), L.ptr(rstd), L.ptr(res), C_,
                             int(relu), L.ptr(y), C_, int(zero_row), L.stream()), "a3d_bn_apply")
    return y, mean_f, rstd, int(n_glob.item())


def bn_sync_backward(x, y, dy, gamma, mean, rstd, n_global, relu=False, want_dres=False, group=None, zero_row=False):
    """Backward of ``bn_sync_forward``: sum g and sum g xhat are all-reduced (2C numbers), dx uses the global sums and
    row count; dgamma / dbeta are this rank's sums (the gradient all-reduce averages them with everything else)."""
    from .optim import dist_all_reduce
    n, C_, x, yy, dy = _bn_operands(x, y, dy, gamma, mean, rstd, relu)
    x, dy, yy = x.contiguous(), dy[:n].contiguous(), yy[:n].contiguous() if yy is not None else None
    ws = _ws(n, C_, x.device)
    local = torch.empty(2 * C_, dtype=torch.float64, device=x.device)
    L.check(L.load().a3d_bn_backward_sums(L.ptr(x), C_, L.ptr(yy), C_, L.ptr(dy), C_, n, C_, L.ptr(mean), L.ptr(rstd), int(relu),
                                          L.ptr(local), L.ptr(ws), ws.numel(), L.stream()), "a3d_bn_backward_sums")
    glob = dist_all_reduce(local.clone(), group)
    dx, dres = _bn_outputs(x, want_dres, zero_row)
    # (this path has always stated C as the row stride of an absent y / dres)
    dgamma, dbeta = _bn_backward_apply(x, yy, dy, n, C_, gamma, mean, rstd, relu, glob, n_global, local, dx, dres, zero_row, C_)
    return dx, dgamma, dbeta, dres


def column_sums(x):
    dev, n, C_ = _dims("x", x)
    x = _contig("x", x, (n, C_), dev)
    out = torch.empty(C_, dtype=F32, device=dev)
    ws = _ws(n, C_, dev)
    L.check(L.load().a3d_column_sums(L.ptr(x), C_, n, C_, L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), "a3d_column_sums")
    return out


def layernorm_forward(x, gamma, beta, eps=1e-5):
    dev, n, C_ = _dims("x", x)
    x = _contig("x", x, (n, C_), dev)
    _vectors(dev, C_, gamma=gamma, beta=beta)
    y = torch.empty_like(x)
    L.check(L.load().a3d_layernorm_forward(L.ptr(x), C_, n, C_, L.ptr(gamma), L.ptr(beta), eps, L.ptr(y), C_, L.stream()),
            "a3d_layernorm_forward")
    return y


def layernorm_backward(x, dy, gamma, eps=1e-5):
    """-> (dx, dgamma, dbeta) of y = LayerNorm(x) over the channels of every row."""
    dev, n, C_ = _dims("x", x)
    x, dy = _contig("x", x, (n, C_), dev), _contig("dy", dy, (n, C_), dev)
    _ptr("gamma", gamma, F32, (C_,), dev)
    dx = torch.empty_like(x)
    dgamma, dbeta = _channels(C_, dev)
    ws = _ws(n, C_, dev)
    L.check(L.load().a3d_layernorm_backward(L.ptr(x), C_, L.ptr(dy), C_, n, C_, L.ptr(gamma), eps, L.ptr(dx), L.ptr(dgamma),
                                            L.ptr(dbeta), L.ptr(ws), ws.numel(), L.stream()), "a3d_layernorm_backward")
    return dx, dgamma, dbeta


def _linear_operands(x, dy):
    """(device, n, cin, cout, x, dy) of x^T dy for [n, Cin], [n, Cout], both contiguous."""
    dev, n, cin = _dims("x", x)
    x, dy = _contig("x", x, (n, cin), dev), _contig("dy", dy, (n, None), dev)
    return dev, n, cin, dy.shape[1], x, dy


def linear_weight_grad(x, dy):
    """dW [Cin, Cout] = x^T dy for [n, Cin], [n, Cout] (weights in the [in, out] layout the kernels use)."""
    lib = L.load()
    dev, n, cin, cout, x, dy = _linear_operands(x, dy)
    ws = _workspace(lib.a3d_linear_wgrad_workspace_bytes(n, cin, cout), dev, None)
    dw = torch.empty((cin, cout), dtype=F32, device=dev)
    L.check(lib.a3d_linear_wgrad(L.ptr(x), cin, L.ptr(dy), cout, n, cin, cout, L.ptr(dw), L.ptr(ws), ws.numel(), L.stream()),
            "a3d_linear_wgrad")
    return dw


def linear_weight_grad_into(x, dy, dw, transposed=True, accumulate=False, db=None, db_accumulate=False):
    """x^T dy written (or added) into ``dw`` -- a contiguous [Cout, Cin] block (``transposed``: nn.Linear.weight's layout, e.g. a
    row slice of an in_proj matrix) or [Cin, Cout] -- and, with ``db`` [Cout], the bias gradient (column sums of dy) from the
    same pass over dy: a3d_linear_wgrad_into."""
    lib = L.load()
    dev, n, cin, cout, x, dy = _linear_operands(x, dy)
    want = (cout, cin) if transposed else (cin, cout)
    _ptr("dw", dw, F32, want, dev), _ptr("db", db, F32, (cout,), dev, optional=True)
    ws = _workspace(lib.a3d_linear_wgrad_into_workspace_bytes(n, cin, cout), dev, None)
    L.check(lib.a3d_linear_wgrad_into(L.ptr(x), cin, L.ptr(dy), cout, n, cin, cout, L.ptr(dw), want[1], 1 if transposed else 0,
                                      1 if accumulate else 0, L.ptr(db), 1 if db_accumulate else 0, L.ptr(ws), ws.numel(),
                                      L.stream()), "a3d_linear_wgrad_into")
