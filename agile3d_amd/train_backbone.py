"""Training-mode forward and backward of the backbone (Res16UNet34C + lin_squeeze_head) on the HIP kernels -- the
backbone half of SURVEY.md section 8 row f-2 (``engine.py:26-179``: ``model.train()``, ``losses.backward()``).

    tape = BackboneTape(model, scene, feats3)        forward: res16unet.py:222-295 with BatchNorm on batch statistics
    pcd = tape.output                                [N, 128] in the caller's row order (agile3d.py:179)
    grads = tape.backward(d_pcd)                     {state-dict key: gradient} for every backbone parameter

Every FLOP runs in libagile3d_hip (conv forward = the inference kernel on the caller's buffers, a3d_conv_apply; conv input
gradient = the same kernel on the transposed maps; k_wgrad; the BatchNorm training kernels; k_stem_wgrad); this module is
the reverse-mode bookkeeping: which activation feeds which layer, the two-way fan-outs of the residual / skip
connections (a tensor add), the channel split of the concatenations.  Activations and gradients carry the zero row the
conv kernels gather for a missing neighbour ([n + 1, C] tensors, written by the producing kernel), both orientations of
every conv weight are packed once per weight version (``PackedWeights``), workspaces come from one arena.  The decoder's
half is ``train_decoder.DecoderTape``, the whole iteration ``train_step.train_one_step``.
"""
from __future__ import annotations

import os
from dataclasses import make_dataclass
from types import SimpleNamespace

import torch

from . import backward as B
from . import lib as L
from .modules import walk_res16unet34c


class _T:
    """Activation node: value [n + 1, C] (row n = the zero row; possibly a column slice of a concatenation's buffer),
    level, gradient buffer (same shape; ``ginit`` says whether something has been written to it yet -- the first
    contribution is a plain write, later ones are added inside the producing kernel's epilogue)."""
    __slots__ = ("v", "level", "g", "ginit", "bn", "pending", "sums")

    def __init__(self, v, level):
        self.v, self.level, self.g, self.ginit = v, level, None, False
        self.bn = None        # (raw, mean, rstd, relu) of the conv + BatchNorm unit that produced this node (fused path)
        self.pending = 0      # gradient contributions still to come (consumers of the forward pass)
        self.sums = None      # fp64 [2, C]: the BatchNorm-backward sums, when the LAST contribution's conv produced them

    def grad_buffer(self):
        if self.g is None:
            self.g = torch.empty((self.v.shape[0], self.v.shape[1]), dtype=torch.float32, device=self.v.device)
        return self.g


# one conv's entry of PackedWeights: _version(conv) when the packed forward weight and the input-gradient parts
# (backward.packed_input_grad_weights) were last written, the conv and its kind
_Packed = make_dataclass("_Packed", ["version", "forward", "parts", "conv", "kind"])


class PackedWeights:
    """Both orientations of every sparse-conv kernel in the MFMA fragment order, packed once per weight version: the
    forward weight and the slices of the input-gradient conv's W' (backward.packed_input_grad_weights).  A tape asks
    ``get(conv)``; entries are refreshed when the parameter tensor was written (torch bumps ``_version``), after a step of
    the library's own AdamW (it writes through raw pointers and bumps ``optim.WEIGHT_EPOCH``) or after ``invalidate()``.

    ``refresh_all()`` (called when a tape starts) repacks EVERY known entry that went stale with one launch of
    ``a3d_pack_conv_weights_multi`` into the buffers the entries already own: after an optimiser step that is all of them
    -- one launch instead of ~230 packs plus the transposes / flips / slice copies that fed them."""

    def __init__(self):
        self._c = {}             # id(param) -> _Packed
        self.epoch = 0
        self._table = None       # (device job table, n_jobs, n_chunks, signature)

    def invalidate(self):
        self.epoch += 1

    def _version(self, conv):
        from .optim import WEIGHT_EPOCH
        return (int(conv.kernel._version), self.epoch, WEIGHT_EPOCH[0], conv.kernel.data_ptr())

    def get(self, conv, kind):
        key = id(conv.kernel)
        ver = self._version(conv)
        hit = self._c.get(key)
        if hit is None or hit.version != ver:
            w = conv.kernel3().detach().contiguous()
            hit = self._c[key] = _Packed(ver, B.pack_weight(w), B.packed_input_grad_weights(kind, w), conv, kind)
            self._table = None
        return hit.forward, hit.parts

    def _build_table(self):
        rows, chunk, sig, dev = [], 0, [], None
        for key, e in self._c.items():
            w = e.conv.kernel3().detach()
            K, cin, cout = w.shape
            if not w.is_contiguous():
                return None          # a weight the one-launch pack does not cover (strided view)
            dev = w.device
            jobs = [(w.data_ptr(), e.forward.data_ptr(), K, cin, cout, cin, cout, 0, 0, 0)]
            for c0, width, pk in e.parts:
                jobs.append((w.data_ptr(), pk.data_ptr(), K, cout, width, cin, cout, 1, 1 if e.kind == L.OP_CONV3 else 0, c0))
            for j in jobs:
                rows.append(j + (chunk, 0))
                chunk += (j[2] * j[3] * j[4] + 4095) // 4096
            sig.append((key, w.data_ptr()))
        if not rows:
            return None
        return (L.pack_job_table(rows, dev), len(rows), chunk, tuple(sig))

    def refresh_all(self):
        if all(e.version == self._version(e.conv) for e in self._c.values()):
            return
        sig = tuple((k, e.conv.kernel3().data_ptr()) for k, e in self._c.items())
        if self._table is None or self._table[3] != sig:
            self._table = self._build_table()
        if self._table is None:
            return                   # get() repacks entry by entry
        tab, n_jobs, n_chunks, _ = self._table
        B.pack_weights_multi(tab, n_jobs, n_chunks)
        for e in self._c.values():
            e.version = self._version(e.conv)


def packed_weights_of(model) -> PackedWeights:
    if getattr(model, "_a3d_packed_train", None) is None:
        object.__setattr__(model, "_a3d_packed_train", PackedWeights())
    return model._a3d_packed_train


def _sync_bn_default():
    """SyncBN is opt-in: ``A3D_SYNC_BN=1`` (or ``BackboneTape(..., sync_bn=True)``) and an initialised process group of
    more than one rank.  Off, every rank normalises over its own scenes (what plain DDP does)."""
    import torch.distributed as dist
    return os.environ.get("A3D_SYNC_BN", "0") == "1" and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


_side_streams = {}


def _wgrad_stream(device):
    """The stream the weight-gradient kernels of the backward pass run on (one per device): a unit's weight gradient and its
    input gradient both depend only on d(raw), so they run side by side -- k_wgrad's waves wait for gathered rows half of
    the time (0.42-0.5 of the matrix peak), the input-gradient conv's workgroups fill in.  A3D_WGRAD_STREAM=0: one stream."""
    if os.environ.get("A3D_WGRAD_STREAM", "1") == "0":
        return None
    key = str(device)
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


class BackboneTape:
    """Round 5: one library call per conv + BatchNorm (+ residual)(+ ReLU) unit in the forward (the batch statistics come
    out of the conv kernel's epilogue: no statistics pass over the raw output), concatenations are column slices of one
    buffer (producers write into their slice, nothing is copied), and in the backward every fan-in is summed inside the
    producing kernel's epilogue (the input-gradient convs accumulate into the node's gradient buffer): no torch add /
    cat / copy on the tape.  ``sync_bn`` keeps the layer-at-a-time BatchNorm."""

    def __init__(self, model, scene, feats3: torch.Tensor, sync_bn=None):
        if not feats3.is_cuda:
            raise RuntimeError("BackboneTape runs on the GPU only")
        self.model, self.scene = model, scene
        self.sync_bn = _sync_bn_default() if sync_bn is None else bool(sync_bn)
        self.fused_bn = not self.sync_bn
        self.fuse_bwd = os.environ.get("A3D_FUSE_BN_BWD", "1") != "0"     # tests / A-B: the layer-at-a-time BatchNorm backward
        self.feats3 = feats3.to(torch.float32).contiguous()
        self.steps = []          # backward closures, in forward order
        self.wgrad_stream, self._side_used = _wgrad_stream(self.feats3.device), False
        scene.prepare_wgrad()                 # on THIS stream, before the side stream's first weight gradient
        self.relu_levels = []
        self.grads = {}
        self._names = {id(p): n for n, p in model.named_parameters()}
        self.packed = packed_weights_of(model)
        self.packed.refresh_all()
        self.state = B.StateArena(self.feats3.device, 320)    # 63 forward convs + <= 4 launches per conv in the backward
        self._bns = []           # the BatchNorms this forward pass ran through (running statistics updated in place)
        walk_res16unet34c(model.backbone, model.lin_squeeze_head, self)      # the forward pass (res16unet.py:222-295)
        # the kernels wrote running_mean / running_var through raw device pointers: torch's version counters did not
        # move, so (1) count the batch like nn.BatchNorm1d does (state-dict parity with torch, one multi-tensor launch;
        # the buffers' version bump is what refresh_weights_if_stale(check_versions=True) sees) and (2) tell the
        # inference engine directly that its folded backbone program is out of date
        if self._bns:
            torch._foreach_add_([b.num_batches_tracked for b in self._bns], 1)
        eng = getattr(model, "_engine", None)
        if eng is not None:
            eng.backbone_statistics_moved()

    # ------------------------------------------------------------------ layers
    def _pgrad(self, param, g):
        name = self._names[id(param)]
        g = g.reshape(param.shape)
        self.grads[name] = g if name not in self.grads else self.grads[name] + g

    def _new(self, level, C_):
        return torch.empty((self.scene.n[level] + 1, C_), dtype=torch.float32, device=self.feats3.device)

    def _bn_forward(self, b, x, res, relu, out):
        """BatchNorm on batch statistics of x [n, C] (+ res)(ReLU) as a layer of its own, over the rows of all ranks with
        ``sync_bn``, into the view ``out`` [n + 1, C] (its zero row included) -> (mean, rstd, global row count or None)."""
        fn = B.bn_sync_forward if self.sync_bn else B.bn_train_forward
        y, *stats = fn(x, b.weight.detach(), b.bias.detach(), b.eps, res, relu, b.running_mean, b.running_var, b.momentum,
                       zero_row=True)
        out.copy_(y)
        return tuple(stats) if self.sync_bn else (*stats, None)

    def _bn_backward(self, gamma, x, y, g, stats, relu, dx, dres):
        """Backward of ``_bn_forward`` (``stats`` from it) into dx [n + 1, C] and, unless None, dres -> (dgamma, dbeta)."""
        mean, rstd, n_glob = stats
        if not self.sync_bn:
            return B.bn_train_backward_into(x, y, g, gamma, mean, rstd, relu, dx, dres)
        n = x.shape[0]
        d, dg, db, dr = B.bn_sync_backward(x, y[:n], g[:n], gamma, mean, rstd, n_glob, relu, dres is not None, zero_row=True)
        dx.copy_(d)
        if dres is not None:
            dres.copy_(dr)
        return dg, db

    def _conv_backward(self, kind, x: _T, conv, wb, dy, side):
        """The conv half of a backward step for y = conv(x) with dL/dy = ``dy`` [n_out + 1, cout]: the weight gradient (on the
        stream ``side``, None: this one), then the input gradient written / accumulated into the input node's buffer."""
        sc = self.scene
        K, cin, cout = conv.kernel3().shape
        n_in, n_out = sc.n[x.level], sc.n[B.level_out(kind, x.level)]
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())           # dy is complete
            with torch.cuda.stream(side):
                dw = B.conv_weight_grad(sc, kind, x.level, x.v[:n_in], dy[:n_out])
            dy.record_stream(side)                                  # its memory is not handed out again before the kernel is done
            self._side_used = True
        else:
            dw = B.conv_weight_grad(sc, kind, x.level, x.v[:n_in], dy[:n_out])
        self._pgrad(conv.kernel, dw)
        x.pending -= 1
        if x.pending == 0 and x.bn is not None and len(wb) == 1:
            # this conv completes dL/dx and x is the output of a conv + BatchNorm unit: mask + BatchNorm-backward sums in
            # this launch's epilogue (a3d_conv_dgrad_bn)
            xr, xm, xs, xrelu = x.bn
            x.sums = B.conv_dgrad_bn(sc, kind, x.level, wb[0], dy, cout, x.grad_buffer(), x.ginit, x.v, xr, xm, xs, xrelu,
                                     state=self.state)
        else:
            B.conv_input_grad_into(sc, kind, x.level, wb, dy, cin, cout, x.grad_buffer(), acc=x.ginit, state=self.state)
        x.ginit = True

    def _conv_bn(self, kind, x: _T, conv, norm, res: _T | None = None, relu=True, out=None) -> _T:
        """conv -> BatchNorm on batch statistics (+ res)(ReLU): one unit of res16unet.py:222-295 / resnet_block.py:48-64.
        ``out``: the [n_out + 1, cout] view the result is written to (a slice of a concatenation's buffer)."""
        K, cin, cout = conv.kernel3().shape
        wf, wb = self.packed.get(conv, kind)
        sc, b = self.scene, norm.bn
        self._bns.append(b)
        lo = B.level_out(kind, x.level)
        n_out = sc.n[lo]
        yv = out if out is not None else self._new(lo, cout)
        gamma = b.weight.detach()
        if self.fused_bn:
            raw, *stats = B.conv_bn_train_forward(sc, kind, x.level, wf, x.v, cin, cout, gamma, b.bias.detach(), b.eps,
                                                  res.v if res is not None else None, relu, yv, b.running_mean,
                                                  b.running_var, b.momentum, state=self.state)
            stats.append(None)
        else:
            rawz = self._new(lo, cout)
            B.conv_apply_acc(sc, kind, x.level, wf, x.v, cin, cout, rawz, zero_row=False, state=self.state)
            raw = rawz[:n_out]
            stats = self._bn_forward(b, raw, res.v[:n_out] if res is not None else None, relu, yv)
        y = _T(yv, lo)
        if self.fused_bn and self.fuse_bwd:
            y.bn = (raw, stats[0], stats[1], relu)
        x.pending += 1
        if res is not None:
            res.pending += 1
        if relu:
            self.relu_levels.append((lo, SimpleNamespace(v=yv[:n_out])))   # forward order of the ReLUs (tests read the 0/1 masks)

        def back():
            # BatchNorm: g = dy (y > 0) -> d(raw) (with its zero row: the input-gradient conv gathers it), d(res) = g
            draw = self._new(lo, cout)
            dres = None
            if res is not None:
                if res.ginit:   # (not an assert: under python -O a second writer would silently OVERWRITE the first gradient)
                    raise RuntimeError("BackboneTape: the residual branch's gradient must be the first contribution to its node "
                                       "(a block input that is also a skip tensor or another block's residual is not a "
                                       "topology this tape's first-write rule covers)")
                res.pending -= 1
                if y.sums is None:
                    dres = res.grad_buffer()
                res.ginit = True
            if y.sums is not None:
                # the last contribution to dL/dy was an input-gradient conv that masked it (g) and summed g, g xhat in its
                # epilogue: no pass over dy / y / raw for the sums, and d(res) = g IS the buffer (no copy)
                dg, db = B.bn_backward_from_sums(raw, y.g, gamma, stats[0], stats[1], y.sums, draw)
                if res is not None:
                    res.g = y.g
            else:
                dg, db = self._bn_backward(gamma, raw, yv, y.g, stats, relu, draw, dres)
            self._pgrad(b.weight, dg)
            self._pgrad(b.bias, db)
            y.g = None
            self._conv_backward(kind, x, conv, wb, draw, self.wgrad_stream)
        self.steps.append(back)
        return y

    def _cat(self, buf, a: _T, b: _T) -> _T:
        """me.cat(a, b) (res16unet.py:257,267,277,287): both producers already wrote into their column slices of ``buf``;
        in the backward the consumers write into one gradient buffer whose slices ARE the producers' gradients."""
        y = _T(buf, a.level)
        ca = a.v.shape[1]
        a.bn = b.bn = None          # their gradients arrive as column slices of the concatenation's: no fused BatchNorm backward

        def back():
            g = y.g
            a.g, a.ginit = g[:, :ca], True                 # the up-sampled half has no other consumer
            if b.g is None:
                b.g, b.ginit = g[:, ca:], True              # the skip half: its encoder-side consumer accumulates into it later
            else:
                b.g.add_(g[:, ca:])
        self.steps.append(back)
        return y

    def _block(self, blk, x: _T, out=None) -> _T:
        """BasicBlock.forward (resnet_block.py:48-64)."""
        h = self._conv_bn(L.OP_CONV3, x, blk.conv1, blk.norm1)
        res = x
        if blk.downsample is not None:
            res = self._conv_bn(L.OP_LINEAR, x, blk.downsample[0], blk.downsample[1], relu=False)
        # conv2 -> norm2 (+ residual) -> ReLU.  Backward order inside the closure list: this unit first (its d(res) is the
        # first write into the residual node), then the projection, then conv1 -- both accumulate into x
        return self._conv_bn(L.OP_CONV3, h, blk.conv2, blk.norm2, res=res, relu=True, out=out)

    # ------------------------------------------------------------------ the builder's verbs (modules.walk_res16unet34c)
    def concat_buffer(self, level, c_up, c_skip):      # both halves are written straight into their column slices
        return SimpleNamespace(buf=self._new(level, c_up + c_skip), c_up=c_up, up=None, skip=None)      # up, skip: the nodes

    def stem(self, conv, bn, cat) -> _T:
        sc = self.scene
        w0 = conv.kernel3().detach().contiguous()
        stem = _T(B.stem_forward(sc, w0, self.feats3, w0.shape[0]), 0)
        self.steps.append(lambda: self._pgrad(conv.kernel, B.stem_weight_grad(sc, self.feats3, stem.g[:sc.n[0]], w0.shape[0])))
        cat.skip = self._bn_only(stem, bn, cat.buf[:, cat.c_up:])
        return cat.skip

    def down(self, conv, bn, x: _T) -> _T:
        return self._conv_bn(L.OP_DOWN, x, conv, bn)

    def layer(self, blocks, x: _T, skip_of=None) -> _T:
        into = skip_of.buf[:, skip_of.c_up:] if skip_of is not None else None
        for i, blk in enumerate(blocks):
            x = self._block(blk, x, into if i == len(blocks) - 1 else None)
        if skip_of is not None:
            skip_of.skip = x
        return x

    def up(self, conv, bn, x: _T, cat):
        cat.up = self._conv_bn(L.OP_UP, x, conv, bn, out=cat.buf[:, :cat.c_up])

    def concat(self, cat) -> _T:
        return self._cat(cat.buf, cat.up, cat.skip)

    def head(self, head, out: _T):
        """lin_squeeze_head: 1x1 conv + bias (agile3d.py:43-45,179), back to the caller's row order."""
        sc = self.scene
        K, cin, cout = head.kernel3().shape
        wf, wb = self.packed.get(head, L.OP_LINEAR)
        n0 = sc.n[0]
        yh = self._new(0, cout)
        B.conv_apply_acc(sc, L.OP_LINEAR, 0, wf, out.v, cin, cout, yh, state=self.state)
        self.head_out = _T(yh, 0)
        out.pending += 1
        # (the head's weight gradient has always run on this stream, the units' run on the side stream)
        self.steps.append(lambda: self._conv_backward(L.OP_LINEAR, out, head, wb, self.head_out.g, None))
        self.orig_row = sc.table_dev(0, L.TAB_ORIGROW)[:n0].long()
        bias = head.bias.detach().reshape(1, -1)
        pcd = torch.empty((n0, cout), dtype=torch.float32, device=yh.device)
        pcd[self.orig_row] = yh[:n0] + bias
        self.output = pcd

    def _bn_only(self, x: _T, norm, out) -> _T:
        """bn0 + ReLU behind the input convolution (res16unet.py:225-227): the stem kernel has no statistics epilogue."""
        b = norm.bn
        self._bns.append(b)
        n = self.scene.n[x.level]
        xv = x.v[:n]
        stats = self._bn_forward(b, xv, None, True, out)
        y = _T(out, x.level)
        self.relu_levels.append((x.level, SimpleNamespace(v=out[:n])))

        def back():
            dg, db = self._bn_backward(b.weight.detach(), xv, out, y.g, stats, True, x.grad_buffer(), None)
            x.ginit = True
            self._pgrad(b.weight, dg)
            self._pgrad(b.bias, db)
        self.steps.append(back)
        return y

    def release(self):
        """Drop the recorded steps and activations (the backward closures and the tape refer to each other: without this the
        activations of an iteration live until Python's cycle collector runs, see DecoderTape.release)."""
        self.steps, self.relu_levels = [], []
        self.head_out = None

    # ------------------------------------------------------------------ backward
    def backward(self, d_output: torch.Tensor, on_grad=None) -> dict:
        """``d_output`` = dL/d(pcd_features) [N, 128] in the caller's row order -> gradients keyed like state_dict().
        ``on_grad(name, tensor)`` is called for every parameter as soon as its gradient is final (every backbone
        parameter is used by exactly one layer): the data-parallel all-reduce starts on the upper U-Net's gradients
        while the encoder is still being differentiated (optim.OverlappedAllReduce)."""
        head = self.model.lin_squeeze_head
        n0 = self.scene.n[0]
        g = torch.zeros((n0 + 1, d_output.shape[1]), dtype=torch.float32, device=d_output.device)
        g[:n0] = d_output.to(torch.float32)[self.orig_row]                    # internal row order + the zero row
        self.grads = {}
        self._pgrad(head.bias, B.column_sums(g[:n0]))
        self.head_out.g = g
        seen = set()
        for back in reversed(self.steps):
            back()
            if on_grad is not None and len(self.grads) != len(seen):
                self._join_wgrad_stream()                               # the gradients handed over are complete on THIS stream
                for k in self.grads:
                    if k not in seen:
                        seen.add(k)
                        on_grad(k, self.grads[k])
        self._join_wgrad_stream()
        return self.grads

    def _join_wgrad_stream(self):
        if self._side_used:
            torch.cuda.current_stream().wait_stream(self.wgrad_stream)
            self._side_used = False
