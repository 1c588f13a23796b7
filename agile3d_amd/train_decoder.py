"""Training-mode forward and backward of the click decoder (``Agile3d.forward_mask`` for one batch sample,
agile3d.py:192-339) on the HIP library -- the decoder half of SURVEY.md section 8 row f-2.

    tape = DecoderTape(model, pcd_features, pos_enc, click_idx, click_time_idx)
    tape.logits                    [3 x [N, 1+K]]: aux outputs and 'pred_masks' (last)
    grads, d_pcd = tape.backward([dL/dlogits_l ...])      gradients keyed like state_dict() + dL/d(pcd_features)

The inference path runs the decoder in a handful of fused kernels that keep nothing; training needs the intermediate
activations, so this path is the plain composition of attention_block.py -- nn.Linear = ``a3d_linear`` (the MFMA GEMM
kernels), their gradients = ``a3d_linear`` with the transposed weight + ``a3d_linear_wgrad``, LayerNorm, and the
attention / mask-head primitives of csrc/attn_train.hip with the score matrices materialised.  This module is the
reverse-mode bookkeeping (which tensor feeds which op; fan-outs are tensor adds, ReLU a mask multiply); the library calls
themselves are marshalled in decoder_ops.py (and backward.py), none here.  A parity
executor: every FLOP of consequence is in libagile3d_hip, nothing is tuned yet.  Dropout (``dropout=p > 0``, main.py
--dropout) is applied at the eight sites of every decoder pass with masks regenerated in the kernels from a
counter-based RNG: one 64-bit seed per tape, the sample index and the site decide every mask, nothing mask-shaped is kept.
"""
from __future__ import annotations

import torch

from . import backward as B
from . import decoder_ops as ops
from . import lib as L
from .clicks import query_list
from .decoder_ops import DH, H
from .engine import time_table

# FLASH = False (tests set it): the attentions over the N points keep their [8, Lq, Lk] score matrices (attn_train.hip), the
# path the flash kernels (attn_flash.hip) are checked against
FLASH = True


class _T:
    """A value of the tape with its accumulated gradient.  ``needs_grad=False`` (the position encodings: no parameter
    behind them) drops what flows there instead of summing [N, 128] tensors nobody reads.  ``own`` says that ``g`` is a
    tensor only this node refers to (a sum made here), so further contributions are added in place."""
    __slots__ = ("v", "g", "needs_grad", "own")

    def __init__(self, v, needs_grad=True):
        self.v, self.g, self.needs_grad, self.own = v, None, needs_grad, False

    def add_grad(self, g, fresh=False):
        """``fresh``: ``g`` was made for this call and nobody else refers to it (a GEMM's output, a kernel's dx): the node owns
        it from the start, so the NEXT contribution is already added in place / in a GEMM's epilogue instead of by a
        three-operand torch add over [N, 128]."""
        if not self.needs_grad:
            return
        if self.g is None:
            self.g, self.own = g, bool(fresh)    # not fresh: may be shared with other nodes (e.g. both inputs of an add)
        elif self.own:
            self.g.add_(g)
        else:
            self.g, self.own = self.g + g, True

    def add_grad_rows(self, rows, vals):
        """g[rows] += vals (a row listed twice gets both) without a zero-filled [N, C] temporary + a full-size add."""
        if not self.needs_grad:
            return
        if self.g is None:
            self.g, self.own = torch.zeros_like(self.v), True
        elif not self.own:
            self.g, self.own = self.g.clone(), True
        self.g.index_add_(0, rows, vals)


def _rows_as_one(ts):
    """The samples' row blocks as ONE [N_total, C] tensor: a view when they already lie back to back in one storage (the
    training step hands over slices of the backbone's output and of the batch's position encodings: torch.cat would copy
    164 MB per tensor at 4 x 80 k voxels to put them where they are), the concatenation otherwise."""
    if len(ts) == 1:
        return ts[0]
    t0 = ts[0]
    at = t0.data_ptr()
    for t in ts:
        if (t.dim() != 2 or not t.is_contiguous() or t.dtype != t0.dtype or t.shape[1] != t0.shape[1] or t.data_ptr() != at or
                t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr()):
            return torch.cat(ts, 0)
        at += t.numel() * t.element_size()
    return torch.as_strided(t0, (sum(t.shape[0] for t in ts), t0.shape[1]), (t0.shape[1], 1), t0.storage_offset())


class _Alias:
    """x + c with c a constant of the tape (the position encodings): the sum's gradient IS x's, so the node forwards every
    contribution to x -- a GEMM that would add into the sum's gradient adds into x's (no [N, 128] add when the sum is done)."""
    __slots__ = ("v", "t")

    def __init__(self, v, target):
        self.v, self.t = v, target

    g = property(lambda self: self.t.g)
    own = property(lambda self: self.t.own)
    needs_grad = property(lambda self: self.t.needs_grad)

    def add_grad(self, g, fresh=False):
        self.t.add_grad(g, fresh)

    def add_grad_rows(self, rows, vals):
        self.t.add_grad_rows(rows, vals)


# dropout sites of one decoder pass: site code = 8 * pass + site
SITE_C2S_ATTN, SITE_C2S_OUT, SITE_C2C_ATTN, SITE_C2C_OUT, SITE_FFN_HIDDEN, SITE_FFN_OUT, SITE_S2C_ATTN, SITE_S2C_OUT = range(8)


def draw_seed():
    """One 64-bit dropout seed from torch's default CPU generator (``torch.manual_seed`` makes a run repeatable)."""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) * 2 + int(torch.randint(0, 2, (1,)).item())


class DecoderPacks:
    """Packed weights of the decoder's nn.Linear layers for the training tape, both orientations: entry (name, row slice) ->
    (forward pack of W^T [in, out], backward pack of W [out, in]).  Keyed on the parameter's version, the
    library optimiser's WEIGHT_EPOCH and the storage pointer; after an optimiser step every entry is stale and all of them are
    repacked by ONE launch of a3d_pack_conv_weights_multi into the buffers they already own (was: two packs and two
    transposing copies per layer and iteration, ~100 launches)."""

    def __init__(self):
        self.e = {}            # (name, rows) -> [version, (packed, cin, cout) fwd, (packed, cin, cout) bwd, bias, param, rows]
        self._table = None     # (device table, n_jobs, n_chunks, signature)

    @staticmethod
    def _version(p):
        from .optim import WEIGHT_EPOCH
        return (int(p._version), WEIGHT_EPOCH[0], p.data_ptr())

    def get(self, p, name, rows):
        key = (name, rows)
        hit = self.e.get(key)
        if hit is None:
            out_f, in_f = p.shape
            r0, r1 = rows if rows is not None else (0, out_f)
            n = (r1 - r0) * in_f
            dev = p.device
            hit = self.e[key] = [None, (torch.empty(n, dtype=torch.float32, device=dev), in_f, r1 - r0),
                                 (torch.empty(n, dtype=torch.float32, device=dev), r1 - r0, in_f), None, p, (r0, r1)]
            self._table = None
        if hit[0] != self._version(p):
            self._refresh()
        return hit[1], hit[2]

    def _refresh(self):
        sig = tuple((k, h[4].data_ptr()) for k, h in self.e.items())
        if self._table is None or self._table[3] != sig:
            rows_, chunk = [], 0
            for (name, _), h in self.e.items():
                p, (r0, r1) = h[4], h[5]
                if not p.is_contiguous():
                    raise RuntimeError(f"DecoderPacks: parameter {name} is not contiguous")
                out_f, in_f = p.shape
                w = r1 - r0
                # forward: packed(W^T): element (ci = in, co = out) = W[r0 + co][ci]  -> a transposed job over the [out, in] source
                rows_.append((p.data_ptr(), h[1][0].data_ptr(), 1, in_f, w, out_f, in_f, 1, 0, r0, chunk, 0))
                chunk += (in_f * w + 4095) // 4096
                # backward: packed(W): element (ci = out, co = in) = W[r0 + ci][co]  -> a plain job on the slice's rows
                rows_.append((p.data_ptr() + 4 * r0 * in_f, h[2][0].data_ptr(), 1, w, in_f, w, in_f, 0, 0, 0, chunk, 0))
                chunk += (in_f * w + 4095) // 4096
            dev = next(iter(self.e.values()))[4].device
            self._table = (L.pack_job_table(rows_, dev), len(rows_), chunk, sig)
        tab, n_jobs, n_chunks, _ = self._table
        B.pack_weights_multi(tab, n_jobs, n_chunks)
        for h in self.e.values():
            h[0] = self._version(h[4])


class DecoderTape:
    """One tape for a whole batch: ``pcd_features`` / ``pos_enc`` / ``click_idx`` / ``click_time_idx`` are lists with one
    entry per batch sample (agile3d.py:192 loops over the samples: they only share the weights), or single objects for a
    one-sample tape.  Row-wise operations (projections, LayerNorm, FFN, residual adds) run ONCE over the concatenated rows
    of all samples -- points [N_total, 128] and queries [Q_total, 128] --, attention and the mask head per sample on row
    ranges: a third of the launches and of the host-side bookkeeping of one tape per sample."""

    def __init__(self, model, pcd_features, pos_enc, click_idx, click_time_idx, dropout=0.0, seed=None, sample_base=0):
        """``dropout``: p of the decoder's dropout sites (0: none, the tape without dropout bit for bit); ``seed``: the 64-bit
        key of the masks (None: one drawn from torch's default generator when p > 0); the batch samples are numbered
        ``sample_base``, ``sample_base + 1``, ... in the masks -- a one-sample tape of sample b passes ``sample_base=b``, so
        that it draws the masks of a batched tape's sample b."""
        self._single = torch.is_tensor(pcd_features)
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout must lie in [0, 1), got {dropout}")
        self.p = float(dropout)
        self.seed = (draw_seed() if seed is None else int(seed) & (2 ** 64 - 1)) if self.p > 0 else None
        self.sample_base = int(sample_base)
        self._pass = 0
        if self._single:
            pcd_features, pos_enc, click_idx, click_time_idx = [pcd_features], [pos_enc], [click_idx], [click_time_idx]
        if not pcd_features[0].is_cuda:
            raise RuntimeError("DecoderTape runs on the GPU only")
        self.model = model
        self.P = dict(model.named_parameters())
        self.steps, self.grads, self._packed, self._grad_written = [], {}, {}, set()
        self.relu_masks, self.attn_masks, self.args = [], [], []      # what a reference needs to follow the same branch
        self._group_tabs = {}
        self._forward([p.to(torch.float32).contiguous() for p in pcd_features],
                      [p.to(torch.float32).contiguous() for p in pos_enc], list(click_idx), list(click_time_idx))

    # ------------------------------------------------------------------ primitive ops with their backward
    def _pg(self, name, g):
        g = g.reshape(self.P[name].shape)
        self.grads[name] = g if name not in self.grads else self.grads[name] + g

    def _grad_block(self, name, rows):
        """The block of parameter ``name``'s gradient an nn.Linear writes (all of it, or the row slice ``rows`` of a packed in_proj
        parameter) and whether this is its first contribution of the backward pass (-> assigned, not added).  A sliced
        parameter starts as zeros: a slice nothing flows to keeps a zero gradient."""
        g = self.grads.get(name)
        if g is None:
            P = self.P[name]
            g = self.grads[name] = torch.zeros_like(P) if rows is not None else torch.empty_like(P)
        key = (name, rows)
        first = key not in self._grad_written
        self._grad_written.add(key)
        return (g if rows is None else g[rows[0]:rows[1]]), first

    def _drop(self, b, site):
        """The a3d_dropout of site ``site`` of the current decoder pass for the tape's sample ``b``."""
        return L.Dropout(self.seed, self.p, self.sample_base + b, 8 * self._pass + site, 0)

    def _rows_drop(self, x, res, ranges, site, relu=False):
        """y = res + Z o f(x) per sample on its row range (f = relu or the identity; res may be None)."""
        y = torch.empty_like(x)
        for b, (r0, r1) in enumerate(ranges):
            if r1 > r0:
                ops.dropout_rows_forward(x[r0:r1], res[r0:r1] if res is not None else None, relu, self._drop(b, site), out=y[r0:r1])
        return y

    def _rows_drop_bwd(self, dy, x_pre, ranges, drops):
        """dx = Z o dy (o [x_pre > 0]) per sample, with the forward's a3d_dropout structs ``drops``."""
        dx = torch.empty_like(dy)
        for (r0, r1), d in zip(ranges, drops):
            if r1 > r0:
                ops.dropout_rows_backward(dy[r0:r1], x_pre[r0:r1] if x_pre is not None else None, d, out=dx[r0:r1])
        return dx

    def add(self, a: _T, b: _T) -> _T:
        if a.needs_grad and not b.needs_grad:
            return _Alias(a.v + b.v, a)
        if b.needs_grad and not a.needs_grad:
            return _Alias(a.v + b.v, b)
        y = _T(a.v + b.v)

        def back():
            if y.g is None:
                return
            a.add_grad(y.g)
            b.add_grad(y.g)
        self.steps.append(back)
        return y

    def lin(self, x: _T, wname, bname=None, rows=None, res: _T = None, drop=None) -> _T:
        """nn.Linear with weight [out, in] (optionally the row slice ``rows`` of an in_proj matrix).  ``res``: a residual added in
        the GEMM's epilogue -- y = res + x W^T + b as ONE node (the ``tgt + dropout(attn)`` / ``src + ...`` of
        attention_block.py:96,153,207 without a separate [N, 128] add); its gradient is y's, like an add's.  ``drop`` =
        (site, row ranges of the samples) with dropout on: y = res + dropout(x W^T + b), the product's mask applied in one
        pass that also adds the residual, and to dy before the input- and weight-gradient GEMMs."""
        W = self.P[wname].detach()
        b = self.P[bname].detach() if bname else None
        if rows is not None:
            W, b = W[rows[0]:rows[1]], (b[rows[0]:rows[1]] if b is not None else None)
        # both orientations packed once per weight version (DecoderPacks: every entry that went stale -- after an optimiser
        # step, all of them -- is repacked by ONE launch when the next tape asks for its first weight)
        packs = getattr(self.model, "_a3d_packed_dec", None)
        if not isinstance(packs, DecoderPacks):
            packs = DecoderPacks()
            object.__setattr__(self.model, "_a3d_packed_dec", packs)
        fwd_w, bwd_w = packs.get(self.P[wname], wname, rows)
        bc = b                 # a contiguous slice of the 1-D parameter: always current, nothing to cache
        drops = None
        if drop is not None and self.p > 0:
            site, ranges = drop
            drops = [self._drop(b_, site) for b_ in range(len(ranges))]
            y = _T(self._rows_drop(ops.linear(x.v, fwd_w, bc), res.v.contiguous() if res is not None else None, ranges, site))
        else:
            y = _T(ops.linear(x.v, fwd_w, bc, res=res.v.contiguous() if res is not None else None))

        def back():
            if y.g is None:
                return
            dy = y.g.contiguous()
            if drops is not None:
                dy = self._rows_drop_bwd(dy, None, drop[1], drops)            # Z o dy: what reaches the product
            if x.needs_grad and x.g is not None and x.own and x.g.is_contiguous():
                ops.linear(dy, bwd_w, acc=x.g)                              # x.g += dy @ W in the GEMM's epilogue (no [N, 128] add)
            elif x.needs_grad:
                x.add_grad(ops.linear(dy, bwd_w), fresh=True)               # dy @ W
            # dW [out, in] and the bias gradient from ONE pass over dy, written (a parameter's / slice's first contribution) or
            # added where the tape keeps the parameter's gradient: no transposing copy, no zero-filled full-size matrix + slice
            # copy + add per in_proj slice, no column-sum launches
            gw, first_w = self._grad_block(wname, rows)
            gb, first_b = self._grad_block(bname, rows) if bname else (None, True)
            B.linear_weight_grad_into(x.v, dy, gw, transposed=True, accumulate=not first_w, db=gb, db_accumulate=not first_b)
            if res is not None:
                # last, when nothing reads dy any more: a gradient this node owned exclusively passes to the residual WITH its
                # ownership, so what arrives there later is added in place / in a GEMM epilogue (no copy-add over [N, 128])
                res.add_grad(y.g, fresh=y.own)
        self.steps.append(back)
        return y

    def relu(self, x: _T, drop=None) -> _T:
        mask = x.v > 0
        self.relu_masks.append(mask)
        if drop is not None and self.p > 0:        # dropout(relu(x)) in one pass each way; relu_masks stays the ReLU's alone
            site, ranges = drop
            drops = [self._drop(b_, site) for b_ in range(len(ranges))]
            y = _T(self._rows_drop(x.v, None, ranges, site, relu=True))

            def back_drop():
                if y.g is not None:
                    x.add_grad(self._rows_drop_bwd(y.g.contiguous(), x.v, ranges, drops), fresh=True)
            self.steps.append(back_drop)
            return y
        y = _T(x.v * mask)

        def back():
            if y.g is not None:
                x.add_grad(y.g * mask, fresh=True)
        self.steps.append(back)
        return y

    def ln(self, x: _T, prefix) -> _T:
        g_, b_ = self.P[prefix + "weight"].detach(), self.P[prefix + "bias"].detach()
        y = _T(B.layernorm_forward(x.v, g_, b_))

        def back():
            if y.g is None:
                return
            dx, dg, db = B.layernorm_backward(x.v, y.g, g_)
            x.add_grad(dx, fresh=True)
            self._pg(prefix + "weight", dg)
            self._pg(prefix + "bias", db)
        self.steps.append(back)
        return y

    # ---- attention, per batch sample on row ranges of the batched tensors: one of decoder_ops' three implementations
    # ("s2c" and "c2s": the flash kernels with the N points on one side; "dense": scores materialised -- the click-to-click
    # self attention, and everything when FLASH is False)
    def attention_seg(self, q: _T, k: _T, v: _T, q_ranges, k_ranges, masks=None, site=None) -> _T:
        """Attention of every batch sample on ITS rows: sample b's queries are rows q_ranges[b] of ``q``, its keys / values
        rows k_ranges[b] of ``k`` / ``v`` (contiguous row ranges of the batched tensors: views, no copies); masks[b] uint8
        [Lq_b, Lk_b] (1 = blocked) or None; ``site``: the dropout site of the probabilities (with dropout on).  One tape step
        for the whole batch."""
        qv, kv, vv = q.v.contiguous(), k.v.contiguous(), v.v.contiguous()
        out = torch.empty((qv.shape[0], H * DH), dtype=torch.float32, device=qv.device)
        saved = []
        for b, ((q0, q1), (k0, k1)) in enumerate(zip(q_ranges, k_ranges)):
            mask = masks[b] if masks is not None else None
            Lq, Lk = q1 - q0, k1 - k0
            if FLASH and mask is None and Lq >= 1024 and Lq > 8 * Lk:
                kind = "s2c"
            elif FLASH and Lk >= 1024 and Lk > 8 * Lq:
                kind = "c2s"
            else:
                kind = "dense"
            fwd = {"s2c": ops.s2c_forward, "c2s": ops.c2s_forward, "dense": ops.dense_forward}[kind]
            o = out[q0:q1]                                  # the sample's rows of the batched result: written in place
            drop = self._drop(b, site) if site is not None and self.p > 0 else None
            _, sv = fwd(qv[q0:q1], kv[k0:k1], vv[k0:k1], mask, o, drop)
            saved.append((kind, o, sv, mask, drop))
        y = _T(out)

        def back():
            if y.g is None:
                return
            do = y.g.contiguous()
            dq, dk, dv = torch.empty_like(qv), torch.empty_like(kv), torch.empty_like(vv)
            for ((q0, q1), (k0, k1)), (kind, o, sv, mask, drop) in zip(zip(q_ranges, k_ranges), saved):
                bwd = {"s2c": ops.s2c_backward, "c2s": ops.c2s_backward, "dense": ops.dense_backward}[kind]
                bwd(qv[q0:q1], kv[k0:k1], vv[k0:k1], mask, o, sv, do[q0:q1], dq[q0:q1], dk[k0:k1], dv[k0:k1], drop)
            q.add_grad(dq, fresh=True)
            k.add_grad(dk, fresh=True)
            v.add_grad(dv, fresh=True)
        self.steps.append(back)
        return y

    def mha(self, prefix, query: _T, key: _T, value: _T, q_ranges, k_ranges, masks=None, res: _T = None, sites=None) -> _T:
        """nn.MultiheadAttention (attention_block.py:25-26,88-94): in_proj slices (one GEMM each over the rows of the whole
        batch), attention per sample, out_proj (+ ``res``: the layer's residual, added in out_proj's epilogue).  ``sites``:
        the dropout sites (probabilities, out_proj output) of this attention."""
        w, b = prefix + "in_proj_weight", prefix + "in_proj_bias"
        q = self.lin(query, w, b, rows=(0, 128))
        k = self.lin(key, w, b, rows=(128, 256))
        v = self.lin(value, w, b, rows=(256, 384))
        s_attn, s_out = sites if sites is not None else (None, None)
        a = self.attention_seg(q, k, v, q_ranges, k_ranges, masks, site=s_attn)
        return self.lin(a, prefix + "out_proj.weight", prefix + "out_proj.bias", res=res,
                        drop=(s_out, q_ranges) if s_out is not None else None)

    def mask_head(self, queries: _T, src: _T, n_ranges, q_ranges, groups):
        """Agile3d.mask_module (agile3d.py:342-384): per-object max over its queries of src . MLP(LN(q)); the MLP runs over
        the queries of the whole batch, the products per sample.  Returns one [N_b, 1 + K_b] node per sample."""
        e = self.ln(queries, "decoder_norm.")
        e = self.relu(self.lin(e, "mask_embed_head.0.weight", "mask_embed_head.0.bias"))
        E = self.lin(e, "mask_embed_head.2.weight", "mask_embed_head.2.bias")
        dev = src.v.device
        outs, saved = [], []

        def padded(Q):      # the GEMM kernels write 32 / 64 / 96 or multiples of 128 output columns
            return 32 if Q <= 32 else 64 if Q <= 64 else 96 if Q <= 96 else (Q + 127) // 128 * 128
        for (n0, n1), (q0, q1), grp in zip(n_ranges, q_ranges, groups):
            Q = q1 - q0
            Qp = padded(Q)
            sv = src.v[n0:n1]
            # logits of every query on the matrix cores: [N, 128] x [128, Qp] with the embeddings zero-padded to Qp
            # columns (round 5; the one-thread-per-output kernel took 170 us per sample and layer at 80 k points); the
            # padded columns stay in the row layout, no group covers them
            Ep = torch.zeros((Qp, 128), dtype=torch.float32, device=dev)
            Ep[:Q] = E.v[q0:q1]
            lq = ops.linear(sv, ops.pack_linear(Ep.t().contiguous()))
            tabs = self._group_tabs.get(id(grp))       # the groups' query ranges: the same in every layer of the pass
            if tabs is None:
                tabs = self._group_tabs[id(grp)] = (torch.tensor([g[0] for g in grp], dtype=torch.int32, device=dev),
                                                    torch.tensor([g[1] for g in grp], dtype=torch.int32, device=dev), grp)
            qb, qe = tabs[0], tabs[1]
            out, arg = ops.group_max(lq, qb, qe)
            outs.append(_T(out))
            saved.append((arg, Ep, Qp))
            self.args.append(arg)

        def back():
            dsrc = torch.empty_like(src.v)                # every sample's rows are written below (or cleared: no loss there)
            dE = torch.zeros_like(E.v)
            for (n0, n1), (q0, q1), grp, y, (arg, Ep, Qp) in zip(n_ranges, q_ranges, groups, outs, saved):
                if y.g is None:
                    dsrc[n0:n1].zero_()
                    continue
                Q = q1 - q0
                dlq = ops.group_max_backward(y.g.contiguous(), arg, Qp)
                # d(src) = dlq Ep and dE = dlq^T src: both on the matrix cores (a GEMM and a weight-gradient reduction over
                # the N rows, wgrad.hip), the padded query columns carry zeros
                ops.linear(dlq, ops.pack_linear(Ep), out=dsrc[n0:n1])      # straight into the sample's rows (no [N, 128] copy)
                dE[q0:q1] = B.linear_weight_grad(dlq, src.v[n0:n1])[:Q]
            src.add_grad(dsrc, fresh=True)
            E.add_grad(dE, fresh=True)
        self.steps.append(back)
        return outs

    # ------------------------------------------------------------------ forward (agile3d.py:192-323), whole batch
    def _forward(self, pcds, pos_encs, click_idxs, click_time_idxs):
        dev = pcds[0].device
        tt = time_table(128, 200).to(dev)
        bgq, bgp = self.P["bg_query_feat.weight"].detach(), self.P["bg_query_pos.weight"].detach()
        n_bgl = bgq.shape[0]
        n_ranges, q_ranges, groups, samples = [], [], [], []
        n_at = q_at = 0
        q_parts, qpos_parts = [], []
        for pcd, pos_enc, click_idx, click_time_idx in zip(pcds, pos_encs, click_idxs, click_time_idxs):
            fg_rows, fg_times, fg_split, bg_rows, bg_times = query_list(click_idx, click_time_idx)
            n_fg = len(fg_rows)
            rows = torch.tensor(fg_rows + bg_rows, dtype=torch.long, device=dev)
            fixed_pos = pos_enc[rows] + tt[torch.tensor(fg_times + bg_times, dtype=torch.long, device=dev)]
            # queries: clicked rows of pcd_features (+ learned background queries in between), their position encodings
            q_parts += [pcd[rows[:n_fg]], bgq, pcd[rows[n_fg:]]]
            qpos_parts += [fixed_pos[:n_fg], bgp, fixed_pos[n_fg:]]
            Q = n_fg + n_bgl + len(bg_rows)
            grp = [(n_fg, Q)]                       # column 0 = background queries, then the objects
            s_ = 0
            for c in fg_split:
                grp.append((s_, s_ + c))
                s_ += c
            gq = [0] * Q
            for g_i, (b0, b1) in enumerate(grp):
                for qq in range(b0, b1):
                    gq[qq] = g_i
            samples.append({"rows": rows, "n_fg": n_fg, "Q": Q, "n0": n_at, "q0": q_at,
                            "grp_of_query": torch.tensor(gq, dtype=torch.int32, device=dev)})   # mask-head column of each query
            n_ranges.append((n_at, n_at + pcd.shape[0]))
            q_ranges.append((q_at, q_at + Q))
            groups.append(grp)
            n_at += pcd.shape[0]
            q_at += Q
        self.n_ranges, self.q_ranges = n_ranges, q_ranges
        pcd_all = _rows_as_one(pcds)
        self.pcd = _T(pcd_all.contiguous())
        pos = _T(_rows_as_one(pos_encs).contiguous(), needs_grad=False)
        q0 = _T(torch.cat(q_parts, 0).contiguous())
        qpos = _T(torch.cat(qpos_parts, 0).contiguous())

        def q0_back():
            g = q0.g
            dbq = torch.zeros_like(bgq)
            dbp = torch.zeros_like(bgp)
            for sm in samples:
                a0, n_fg, Q = sm["q0"], sm["n_fg"], sm["Q"]
                gs = g[a0:a0 + Q]
                self.pcd.add_grad_rows(sm["rows"] + sm["n0"], torch.cat([gs[:n_fg], gs[n_fg + n_bgl:]], 0))   # a row clicked twice gets both
                dbq += gs[n_fg:n_fg + n_bgl]
                if qpos.g is not None:
                    dbp += qpos.g[a0 + n_fg:a0 + n_fg + n_bgl]
            self._pg("bg_query_feat.weight", dbq)
            if qpos.g is not None:
                self._pg("bg_query_pos.weight", dbp)
        self.steps.append(q0_back)
        src, tgt, masks = self.pcd, q0, None
        self.logits_nodes = []                     # [layer][sample]
        for d in range(self.model.num_decoders):
            li = 0 if self.model.shared_decoder else d
            self._pass = d                      # the pass's dropout sites: 8 d + site (a shared decoder draws anew per pass)
            src_pos = self.add(src, pos)        # the keys of click-to-scene AND the queries of scene-to-click (src changes after both)
            # every residual (x + sublayer(x), attention_block.py:96,153,207) rides in the sublayer's last GEMM
            a = self.mha(f"c2s_attention.{li}.0.multihead_attn.", self.add(tgt, qpos), src_pos, src, q_ranges, n_ranges, masks, res=tgt,
                         sites=(SITE_C2S_ATTN, SITE_C2S_OUT))
            tgt = self.ln(a, f"c2s_attention.{li}.0.norm.")
            qk = self.add(tgt, qpos)
            a = self.mha(f"c2c_attention.{li}.0.self_attn.", qk, qk, tgt, q_ranges, q_ranges, res=tgt, sites=(SITE_C2C_ATTN, SITE_C2C_OUT))
            tgt = self.ln(a, f"c2c_attention.{li}.0.norm.")
            h = self.relu(self.lin(tgt, f"ffn_attention.{li}.0.linear1.weight", f"ffn_attention.{li}.0.linear1.bias"),
                          drop=(SITE_FFN_HIDDEN, q_ranges))
            f = self.lin(h, f"ffn_attention.{li}.0.linear2.weight", f"ffn_attention.{li}.0.linear2.bias", res=tgt,
                         drop=(SITE_FFN_OUT, q_ranges))
            tgt = self.ln(f, f"ffn_attention.{li}.0.norm.")
            a = self.mha(f"s2c_attention.{li}.0.multihead_attn.", src_pos, self.add(tgt, qpos), tgt, n_ranges, q_ranges, res=src,
                         sites=(SITE_S2C_ATTN, SITE_S2C_OUT))
            src = self.ln(a, f"s2c_attention.{li}.0.norm.")
            outs = self.mask_head(tgt, src, n_ranges, q_ranges, groups)
            self.logits_nodes.append(outs)
            # attention masks of the next layer from this layer's labels (agile3d.py:362-383): not differentiated.  No host
            # round trip: "all points blocked -> nothing blocked" (agile3d.py:369,375) is "no point carries the group's
            # label", i.e. a zero in the label histogram; a `bool(row.all())` per group would drain the GPU queue G + 1
            # times per layer and sample
            masks = []
            for out, sm, grp in zip(outs, samples, groups):
                masks.append(ops.next_layer_mask(out.v, sm["grp_of_query"]))
            self.attn_masks.append(masks[0] if self._single else masks)
        if self._single:
            self.logits = [layer[0].v for layer in self.logits_nodes]
        else:
            self.logits = [[n.v for n in layer] for layer in self.logits_nodes]

    def release(self):
        """Drop the recorded steps and activations.  The backward closures refer to the tape and the tape to them: a
        reference cycle, i.e. without this every iteration's activations (gigabytes at 4 x 80 k voxels) stay allocated
        until Python's cycle collector gets to them -- the caching allocator then answers the next iteration with fresh
        hipMallocs (measured: 350 device allocations and +12 GB reserved per iteration, 107 GB after ten)."""
        self.steps, self.logits_nodes, self.relu_masks, self.attn_masks, self.args = [], [], [], [], []
        self.pcd, self._group_tabs = None, {}

    # ------------------------------------------------------------------ backward
    def backward(self, d_logits):
        """``d_logits``: dL/dlogits per decoder layer -- one [N, 1+K] tensor per layer for a single-sample tape, a list over
        the samples per layer for a batched one (None = no loss there).  Returns (gradients keyed like state_dict(),
        dL/d(pcd_features) [N_total, 128])."""
        self.grads, self._grad_written = {}, set()
        for nodes, g in zip(self.logits_nodes, d_logits):
            gs = [g] if self._single else list(g)
            for node, gg in zip(nodes, gs):
                node.g = gg.to(torch.float32).contiguous() if gg is not None else torch.zeros_like(node.v)
        for back in reversed(self.steps):
            back()
        return self.grads, self.pcd.g
