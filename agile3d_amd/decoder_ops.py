"""The training decoder's library calls -- ``a3d_linear`` as the tape uses it and the attention, dropout and mask-head
primitives of ``csrc/attn_train.hip``, ``csrc/attn_flash.hip`` and ``csrc/dropout.hip`` -- as functions of device tensors: the
one place where they are marshalled, as ``view.py`` is for the session calls.  ``train_decoder.py`` and the tests call these.

Every wrapper takes device tensors and derives the sizes it hands to the library from them: no extent is passed next to
the tensor it describes.  Every other tensor's shape is checked against those sizes, with dtype, device and contiguity
(``ValueError`` naming the argument, before the library is reached; the checks are ``_args.py``'s, shared with ``view.py``).  Outputs and scratch are
the caller's when passed (``out=``, ``o=``, ``stats=``, ``workspace=`` ...) and a fresh ``torch.empty`` otherwise; calls
launch on the current stream; nothing synchronises or copies to the host.  ``drop=None`` calls an entry point, an
``L.Dropout`` its ``_dropout`` twin.  There is no CPU path.

Below the wrappers, the three implementations of softmax(q k^T / sqrt(dh) + mask) v per head that the tape chooses from,
each a (forward, backward) pair on unscaled q, k, v that returns what its backward needs:
  ``c2s_*``    few queries over the N points, masked        (csrc/attn_flash.hip: no [8, Lq, Lk] matrix)
  ``s2c_*``    the N points as queries over few keys        (csrc/attn_flash.hip)
  ``dense_*``  scores materialised (csrc/attn_train.hip): the click-to-click self attention, and everything when
               ``train_decoder.FLASH`` is False (the path the flash kernels are checked against)
"""
from __future__ import annotations

import torch

from . import backward as B
from . import lib as L
from ._args import F32, I32, U8, _device, _out, _ptr as _arg

H, DH = 8, 16          # heads x channels per head of the decoder's attentions (the flash kernels are built for these)
C_ATT = H * DH


def _scratch(name, workspace, need, dev):
    """The uint8 scratch of a call that needs ``need`` bytes: the caller's (at least that long) or a new one."""
    if workspace is None:
        return torch.empty(need, dtype=U8, device=dev)
    _arg(name, workspace, U8, (None,), dev)
    if workspace.numel() < need:
        raise ValueError(f"{name} must hold at least {need} bytes, not {workspace.numel()}")
    return workspace


def _drop(drop):
    if drop is not None and not isinstance(drop, L.Dropout):
        raise ValueError("drop must be a lib.Dropout or None")
    return drop


# ---- nn.Linear ---------------------------------------------------------------------------------------------------------------
def pack_linear(w_in_out):
    """``packed`` of ``linear`` from w [cin, cout]: (the weight in the GEMM kernels' layout, cin, cout)."""
    cin, cout = w_in_out.shape
    return B.pack_weight(w_in_out.reshape(1, cin, cout)), cin, cout


def linear(x, packed, bias=None, acc=None, out=None, res=None):
    """x [n, cin] @ w [cin, cout] (+ bias) through a3d_linear; ``packed`` = pack_linear(w).  ``acc`` [n, cout]: the product is
    ADDED to it in place (the kernel's residual input and its output are the same rows: one rounding, like ``acc + product``).
    ``out`` [n, cout] contiguous rows (e.g. a sample's row range of a batched tensor): the product is written there.
    ``res`` [n, cout]: a residual read in the GEMM's epilogue, y = res + x w (+ bias) in fresh rows (or in ``out``).  ``acc``
    excludes ``out`` and ``res``."""
    wp, cin, cout = packed
    # checked inline, not through _arg: x may be non-contiguous (it always could), and this is the tape's most frequent call
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != F32 or x.dim() != 2 or x.shape[1] != cin:
        raise ValueError(f"x must be a float32 [n, {cin}] tensor on the GPU")
    x = x.contiguous()
    n = x.shape[0]
    for name, t, shape in (("bias", bias, (cout,)), ("acc", acc, (n, cout)), ("out", out, (n, cout)), ("res", res, (n, cout))):
        if t is not None and (t.shape != shape or t.dtype != F32 or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 {list(shape)} block on {x.device}")
    if acc is not None and (out is not None or res is not None):
        raise ValueError("acc excludes out and res")
    y = acc if acc is not None else out if out is not None else torch.empty((n, cout), dtype=F32, device=x.device)
    r = acc if acc is not None else res
    L.check(L.load().a3d_linear(L.ptr(x), cin, None, 0, n, cin, cout, L.ptr(wp), None, L.ptr(bias), L.ptr(r),
                                cout if r is not None else 0, 0, L.ptr(y), cout, None, 0, L.stream()), "a3d_linear")
    return y


# ---- the materialised attention: scores, softmax, apply ----------------------------------------------------------------------
def attn_scores(a, b, scale, mask=None, out=None, heads=H):
    """``a3d_attn_scores``: S[h][i][j] = scale * a[i, head h] . b[j, head h] for a [La, C], b [Lb, C] -> fp32 [heads, La, Lb];
    ``mask`` uint8 [La, Lb], non-zero = blocked (-inf)."""
    dev = _device("a", a)
    ap = _arg("a", a, F32, (None, None), dev)
    La, C_ = a.shape
    if heads < 1 or C_ % heads:
        raise ValueError(f"a must have a multiple of heads = {heads} channels, not {C_}")
    bp = _arg("b", b, F32, (None, C_), dev)
    Lb = b.shape[0]
    mp = _arg("mask", mask, U8, (La, Lb), dev, optional=True)
    out = _out("out", out, F32, (heads, La, Lb), dev)
    L.check(L.load().a3d_attn_scores(ap, bp, La, Lb, heads, C_ // heads, scale, mp, out.data_ptr(), L.stream()),
            "a3d_attn_scores")
    return out


def _rows(name, S):
    """(device, rows, L) of a softmax over the last dimension of ``S``."""
    dev = _device(name, S)
    if S.dim() < 1:
        raise ValueError(f"{name} must have a last dimension")
    return dev, S.numel() // max(1, S.shape[-1]), S.shape[-1]


def softmax_rows(S):
    """``a3d_softmax_rows``: in place over the last dimension of fp32 ``S`` [..., L]; returns ``S``."""
    dev, rows, n = _rows("S", S)
    sp = _arg("S", S, F32, S.shape, dev)
    L.check(L.load().a3d_softmax_rows(sp, rows, n, L.stream()), "a3d_softmax_rows")
    return S


def softmax_rows_backward(P, dP):
    """``a3d_softmax_rows_backward``: dP <- P * (dP - sum_j P dP) in place over the last dimension; returns ``dP``."""
    dev, rows, n = _rows("P", P)
    pp, dp = _arg("P", P, F32, P.shape, dev), _arg("dP", dP, F32, P.shape, dev)
    L.check(L.load().a3d_softmax_rows_backward(pp, dp, rows, n, L.stream()), "a3d_softmax_rows_backward")
    return dP


def softmax_cols(S):
    """``a3d_softmax_cols``: in place over the MIDDLE dimension of fp32 ``S`` [heads, Lq, Lk]; returns ``S``."""
    dev = _device("S", S)
    sp = _arg("S", S, F32, (None, None, None), dev)
    L.check(L.load().a3d_softmax_cols(sp, *S.shape, L.stream()), "a3d_softmax_cols")
    return S


def softmax_cols_backward(P, dP):
    """``a3d_softmax_cols_backward``: the backward of ``softmax_cols``, ``dP`` in place; returns ``dP``."""
    dev = _device("P", P)
    pp = _arg("P", P, F32, (None, None, None), dev)
    dp = _arg("dP", dP, F32, P.shape, dev)
    L.check(L.load().a3d_softmax_cols_backward(pp, dp, *P.shape, L.stream()), "a3d_softmax_cols_backward")
    return dP


def attn_apply_workspace_bytes(A, B_, heads, dh, transposed):
    """``a3d_attn_apply_workspace_bytes``: the scratch of ``attn_apply`` on P [heads, A, B] and ``dh`` channels per head."""
    return L.load().a3d_attn_apply_workspace_bytes(A, B_, heads, dh, int(bool(transposed)))


def attn_apply(P, V, transposed, scale, out=None, workspace=None):
    """``a3d_attn_apply`` for P fp32 [heads, A, B]: ``transposed`` false, out[i] = scale * sum_j P[h][i][j] V[j] with V [B, C]
    -> [A, C]; true, out[j] = scale * sum_i P[h][i][j] V[i] with V [A, C] -> [B, C] (h = the head of the channel)."""
    dev = _device("P", P)
    pp = _arg("P", P, F32, (None, None, None), dev)
    heads, A, B_ = P.shape
    rows_in, rows_out = (A, B_) if transposed else (B_, A)
    vp = _arg("V", V, F32, (rows_in, None), dev)
    C_ = V.shape[1]
    if heads < 1 or C_ % heads:
        raise ValueError(f"V must have a multiple of P's {heads} heads as channels, not {C_}")
    out = _out("out", out, F32, (rows_out, C_), dev)
    ws = _scratch("workspace", workspace, attn_apply_workspace_bytes(A, B_, heads, C_ // heads, transposed), dev)
    L.check(L.load().a3d_attn_apply(pp, vp, A, B_, heads, C_ // heads, int(bool(transposed)), scale, out.data_ptr(), L.ptr(ws),
                                    ws.numel(), L.stream()), "a3d_attn_apply")
    return out


def attn_dropout(P, transposed, drop, out=None):
    """``a3d_attn_dropout``: out = Z o P for P fp32 [heads, Lq, Lk], or stored [heads, Lk, Lq] with ``transposed`` (the site's
    rows are the Lq queries either way); ``out`` may be ``P``."""
    dev = _device("P", P)
    pp = _arg("P", P, F32, (None, None, None), dev)
    heads, Lq, Lk = P.shape if not transposed else (P.shape[0], P.shape[2], P.shape[1])
    if not isinstance(drop, L.Dropout):
        raise ValueError("drop must be a lib.Dropout")
    out = _out("out", out, F32, P.shape, dev)
    L.check(L.load().a3d_attn_dropout(pp, heads, Lq, Lk, int(bool(transposed)), out.data_ptr(), drop, L.stream()),
            "a3d_attn_dropout")
    return out


# ---- the flash attentions: the raw ABI (pre-scaled operand in, its gradient out) ------------------------------------------
def flash_c2s_workspace_bytes(Lq, Lk):
    """``a3d_flash_c2s_workspace_bytes``: the scratch of ``flash_c2s_forward`` and ``flash_c2s_backward``."""
    return L.load().a3d_flash_c2s_workspace_bytes(Lq, Lk)


def flash_s2c_workspace_bytes(Lq, Lk):
    """``a3d_flash_s2c_workspace_bytes``: the scratch of ``flash_s2c_backward``."""
    return L.load().a3d_flash_s2c_workspace_bytes(Lq, Lk)


def _qkv(qname, q, kname, k, v):
    """(device, Lq, Lk, the three pointers) of q [Lq, 128], k, v [Lk, 128] under the names the caller gives them."""
    dev = _device(qname, q)
    qp = _arg(qname, q, F32, (None, C_ATT), dev)
    kp = _arg(kname, k, F32, (None, C_ATT), dev)
    return dev, q.shape[0], k.shape[0], qp, kp, _arg("v", v, F32, (k.shape[0], C_ATT), dev)


def flash_c2s_forward(qs, k, v, mask, o=None, stats=None, workspace=None, drop=None):
    """``a3d_flash_c2s_forward`` (``_dropout`` with ``drop``): ``qs`` = q / 4 [Lq, 128] over k, v [Lk, 128], ``mask`` uint8
    [Lq, Lk] or None -> (o [Lq, 128], stats [2, 8, Lq]: row maximum, row sum)."""
    dev, Lq, Lk, qp, kp, vp = _qkv("qs", qs, "k", k, v)
    mp = _arg("mask", mask, U8, (Lq, Lk), dev, optional=True)
    o, stats = _out("o", o, F32, (Lq, C_ATT), dev), _out("stats", stats, F32, (2, H, Lq), dev)
    lib = L.load()
    ws = _scratch("workspace", workspace, lib.a3d_flash_c2s_workspace_bytes(Lq, Lk), dev)
    head = (qp, kp, vp, mp, Lq, Lk, o.data_ptr(), stats.data_ptr(), L.ptr(ws), ws.numel())
    if _drop(drop) is None:
        L.check(lib.a3d_flash_c2s_forward(*head, L.stream()), "a3d_flash_c2s_forward")
    else:
        L.check(lib.a3d_flash_c2s_forward_dropout(*head, drop, L.stream()), "a3d_flash_c2s_forward_dropout")
    return o, stats


def flash_c2s_backward(qs, k, v, mask, o, stats, do, dq=None, dk=None, dv=None, workspace=None, drop=None):
    """``a3d_flash_c2s_backward`` (``_dropout`` with ``drop``) from the forward's ``o`` and ``stats`` and dL/do ->
    (dq, dk, dv); ``dq`` is the gradient of the pre-scaled ``qs``."""
    dev, Lq, Lk, qp, kp, vp = _qkv("qs", qs, "k", k, v)
    mp = _arg("mask", mask, U8, (Lq, Lk), dev, optional=True)
    op, sp = _arg("o", o, F32, (Lq, C_ATT), dev), _arg("stats", stats, F32, (2, H, Lq), dev)
    dop = _arg("do", do, F32, (Lq, C_ATT), dev)
    dq, dk, dv = (_out("dq", dq, F32, (Lq, C_ATT), dev), _out("dk", dk, F32, (Lk, C_ATT), dev),
                  _out("dv", dv, F32, (Lk, C_ATT), dev))
    lib = L.load()
    ws = _scratch("workspace", workspace, lib.a3d_flash_c2s_workspace_bytes(Lq, Lk), dev)
    head = (qp, kp, vp, mp, Lq, Lk, op, sp, dop, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), L.ptr(ws), ws.numel())
    if _drop(drop) is None:
        L.check(lib.a3d_flash_c2s_backward(*head, L.stream()), "a3d_flash_c2s_backward")
    else:
        L.check(lib.a3d_flash_c2s_backward_dropout(*head, drop, L.stream()), "a3d_flash_c2s_backward_dropout")
    return dq, dk, dv


def flash_s2c_forward(q, ks, v, o=None, stats=None, drop=None):
    """``a3d_flash_s2c_forward`` (``_dropout`` with ``drop``): q [Lq, 128] over ``ks`` = k / 4 and v [Lk, 128] ->
    (o [Lq, 128], stats [Lq, 8, 2]).  No scratch."""
    dev, Lq, Lk, qp, kp, vp = _qkv("q", q, "ks", ks, v)
    o, stats = _out("o", o, F32, (Lq, C_ATT), dev), _out("stats", stats, F32, (Lq, H, 2), dev)
    lib = L.load()
    head = (qp, kp, vp, Lq, Lk, o.data_ptr(), stats.data_ptr())
    if _drop(drop) is None:
        L.check(lib.a3d_flash_s2c_forward(*head, L.stream()), "a3d_flash_s2c_forward")
    else:
        L.check(lib.a3d_flash_s2c_forward_dropout(*head, drop, L.stream()), "a3d_flash_s2c_forward_dropout")
    return o, stats


def flash_s2c_backward(q, ks, v, o, stats, do, dq=None, dk=None, dv=None, workspace=None, drop=None):
    """``a3d_flash_s2c_backward`` (``_dropout`` with ``drop``) -> (dq, dk, dv); ``dk`` is the gradient of the pre-scaled
    ``ks``."""
    dev, Lq, Lk, qp, kp, vp = _qkv("q", q, "ks", ks, v)
    op, sp = _arg("o", o, F32, (Lq, C_ATT), dev), _arg("stats", stats, F32, (Lq, H, 2), dev)
    dop = _arg("do", do, F32, (Lq, C_ATT), dev)
    dq, dk, dv = (_out("dq", dq, F32, (Lq, C_ATT), dev), _out("dk", dk, F32, (Lk, C_ATT), dev),
                  _out("dv", dv, F32, (Lk, C_ATT), dev))
    lib = L.load()
    ws = _scratch("workspace", workspace, lib.a3d_flash_s2c_workspace_bytes(Lq, Lk), dev)
    head = (qp, kp, vp, Lq, Lk, op, sp, dop, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), L.ptr(ws), ws.numel())
    if _drop(drop) is None:
        L.check(lib.a3d_flash_s2c_backward(*head, L.stream()), "a3d_flash_s2c_backward")
    else:
        L.check(lib.a3d_flash_s2c_backward_dropout(*head, drop, L.stream()), "a3d_flash_s2c_backward_dropout")
    return dq, dk, dv


# ---- the mask head ---------------------------------------------------------------------------------------------------------
def group_max(lq, q_begin, q_end, out=None, arg=None):
    """``a3d_group_max``: per group g the maximum of lq [N, Q] over the columns q_begin[g] .. q_end[g] - 1 (int32 [G] each)
    -> (out fp32 [N, G], arg int32 [N, G]: the column of the first maximum)."""
    dev = _device("lq", lq)
    lp = _arg("lq", lq, F32, (None, None), dev)
    N, Q = lq.shape
    bp = _arg("q_begin", q_begin, I32, (None,), dev)
    G = q_begin.shape[0]
    ep = _arg("q_end", q_end, I32, (G,), dev)
    out, arg = _out("out", out, F32, (N, G), dev), _out("arg", arg, I32, (N, G), dev)
    L.check(L.load().a3d_group_max(lp, N, Q, bp, ep, G, out.data_ptr(), arg.data_ptr(), L.stream()), "a3d_group_max")
    return out, arg


def group_max_backward(dy, arg, n_cols, out=None):
    """``a3d_group_max_backward``: dy fp32 [N, G] routed to the columns ``arg`` int32 [N, G] of fp32 [N, n_cols], zeros
    elsewhere (``n_cols``: the width of ``group_max``'s input, which no operand here carries)."""
    dev = _device("dy", dy)
    dp = _arg("dy", dy, F32, (None, None), dev)
    N, G = dy.shape
    ap = _arg("arg", arg, I32, (N, G), dev)
    out = _out("out", out, F32, (N, int(n_cols)), dev)
    L.check(L.load().a3d_group_max_backward(dp, ap, N, int(n_cols), G, out.data_ptr(), L.stream()), "a3d_group_max_backward")
    return out


def next_layer_mask(logits, grp_of_query, out=None, workspace=None):
    """uint8 [Q, N] attention mask of the next layer's click-to-scene attention from this layer's [N, G = 1 + K] mask logits
    and the group of each of the Q queries (int32 [Q]; agile3d.py:362-383): ``a3d_next_layer_mask`` -- label arg-max +
    histogram, then the mask, instead of eight torch launches."""
    dev = _device("logits", logits)
    lp = _arg("logits", logits, F32, (None, None), dev)
    N, G = logits.shape
    if G > 256:
        raise ValueError("logits must have one column per group (at most 256)")
    gp = _arg("grp_of_query", grp_of_query, I32, (None,), dev)
    Q = grp_of_query.shape[0]
    out = _out("out", out, U8, (Q, N), dev)
    lib = L.load()
    ws = _scratch("workspace", workspace, lib.a3d_next_layer_mask_workspace_bytes(N, G), dev)
    L.check(lib.a3d_next_layer_mask(lp, N, G, gp, Q, out.data_ptr(), L.ptr(ws), ws.numel(), L.stream()), "a3d_next_layer_mask")
    return out


# ---- dropout on rows, the keep mask ----------------------------------------------------------------------------------------
def dropout_rows_forward(x, res, relu, drop, out=None):
    """``a3d_dropout_rows_forward``: y = res + Z o f(x) on one sample's rows x [rows, cols], f = relu or the identity;
    ``res`` may be None."""
    dev = _device("x", x)
    xp = _arg("x", x, F32, (None, None), dev)
    rp = _arg("res", res, F32, x.shape, dev, optional=True)
    if not isinstance(drop, L.Dropout):
        raise ValueError("drop must be a lib.Dropout")
    out = _out("out", out, F32, x.shape, dev)
    L.check(L.load().a3d_dropout_rows_forward(xp, rp, out.data_ptr(), x.shape[0], x.shape[1], int(bool(relu)), drop, L.stream()),
            "a3d_dropout_rows_forward")
    return out


def dropout_rows_backward(dy, x_pre, drop, out=None):
    """``a3d_dropout_rows_backward``: dx = Z o dy (o [x_pre > 0] with ``x_pre``, the forward's input under a ReLU)."""
    dev = _device("dy", dy)
    dp = _arg("dy", dy, F32, (None, None), dev)
    xp = _arg("x_pre", x_pre, F32, dy.shape, dev, optional=True)
    if not isinstance(drop, L.Dropout):
        raise ValueError("drop must be a lib.Dropout")
    out = _out("out", out, F32, dy.shape, dev)
    L.check(L.load().a3d_dropout_rows_backward(dp, xp, out.data_ptr(), dy.shape[0], dy.shape[1], drop, L.stream()),
            "a3d_dropout_rows_backward")
    return out


def dropout_mask(seed, sample, site, p, heads, rows, cols, out=None):
    """``a3d_dropout_mask``: the keep mask itself, uint8 [heads, rows, cols] (1 = kept), on ``out``'s device or the current
    one.  For tests: the hot path never writes a mask."""
    dev = _device("out", out) if out is not None else torch.device("cuda", torch.cuda.current_device())
    out = _out("out", out, U8, (heads, rows, cols), dev)
    L.check(L.load().a3d_dropout_mask(seed, sample, site, p, heads, rows, cols, out.data_ptr() if out.numel() else None,
                                      L.stream(dev)), "a3d_dropout_mask")
    return out


# ---- the tape's three attentions on unscaled q, k, v -----------------------------------------------------------------------
# forward(q, k, v, mask, o=None, drop=None) -> (o, what the backward needs);
# backward(q, k, v, mask, o, saved, do, dq=None, dk=None, dv=None, drop=None) -> (dq, dk, dv), the gradients of the UNSCALED operands
def dense_forward(q, k, v, mask, o=None, drop=None):
    Lq, Lk = q.shape[0], k.shape[0]
    scale = 1.0 / (DH ** 0.5)
    transposed = mask is None and Lq >= 1024 and Lq > 8 * Lk      # the long index fastest in every kernel
    if transposed:
        Pm = softmax_cols(attn_scores(k, q, scale))                   # P^T[h][key][query], the softmax over the keys
    else:
        Pm = softmax_rows(attn_scores(q, k, scale, mask))
    # the dropped probabilities multiply V; the softmax backward needs the undropped ones
    Pd = Pm if drop is None else attn_dropout(Pm, transposed, drop)
    o = attn_apply(Pd, v, transposed, 1.0, o)
    return o, ((Pm, transposed) if drop is None else (Pm, transposed, Pd))


def dense_backward(q, k, v, mask, o, saved, do, dq=None, dk=None, dv=None, drop=None):
    Pm, transposed = saved[:2]
    Pd = saved[2] if drop is not None else Pm
    scale = 1.0 / (DH ** 0.5)
    dP = torch.empty_like(Pm)
    if transposed:
        attn_scores(v, do, 1.0, out=dP)
        dv = attn_apply(Pd, do, False, 1.0, dv)                       # dv[key] = sum_query P^T dO
        if drop is not None:
            attn_dropout(dP, True, drop, out=dP)                      # Z o dP
        softmax_cols_backward(Pm, dP)
        dq = attn_apply(dP, k, True, scale, dq)                       # dq[query] = sum_key dS^T k
        dk = attn_apply(dP, q, False, scale, dk)                      # dk[key] = sum_query dS^T q
    else:
        attn_scores(do, v, 1.0, out=dP)
        dv = attn_apply(Pd, do, True, 1.0, dv)
        if drop is not None:
            attn_dropout(dP, False, drop, out=dP)                     # Z o dP
        softmax_rows_backward(Pm, dP)                                 # dP <- dS
        dq = attn_apply(dP, k, False, scale, dq)
        dk = attn_apply(dP, q, True, scale, dk)
    return dq, dk, dv


def c2s_forward(q, k, v, mask, o=None, drop=None):
    qs = q * 0.25                                                     # 1 / sqrt(16): exact
    o, stats = flash_c2s_forward(qs, k, v, mask, o=o, drop=drop)
    return o, (qs, stats)


def c2s_backward(q, k, v, mask, o, saved, do, dq=None, dk=None, dv=None, drop=None):
    qs, stats = saved
    dq, dk, dv = flash_c2s_backward(qs, k, v, mask, o, stats, do, dq=dq, dk=dk, dv=dv, drop=drop)
    dq *= 0.25
    return dq, dk, dv


def s2c_forward(q, k, v, mask=None, o=None, drop=None):      # ``mask`` is not read: the kernels take none
    # the 1 / sqrt(16) goes on the FEW keys, not on the N queries: q . (k / 4) has the bits of (q / 4) . k (a power of two),
    # and the kernel's dq = dS (k / 4) is then already the gradient of the unscaled queries
    ks = k * 0.25
    o, stats = flash_s2c_forward(q, ks, v, o=o, drop=drop)
    return o, (ks, stats)


def s2c_backward(q, k, v, mask, o, saved, do, dq=None, dk=None, dv=None, drop=None):
    ks, stats = saved
    dq, dk, dv = flash_s2c_backward(q, ks, v, o, stats, do, dq=dq, dk=dk, dv=dv, drop=drop)
    dk *= 0.25
    return dq, dk, dv
