"""Host side of the hot path: packs the model's weights for the HIP library, describes the
Res16UNet34C topology as an op program, and implements ``forward_backbone`` /
``forward_mask`` on top of the C ABI (include/agile3d_hip.h).

Mirrors the reference's host code for this path:
  * ``models/res16unet.py:222-295``  (layer sequence, skip concatenations)
  * ``models/resnet.py:96-149`` / ``models/modules/resnet_block.py:48-64`` (BasicBlock)
  * ``models/agile3d.py:141-181``   (forward_backbone, get_pos_encs)
  * ``models/agile3d.py:183-339``   (forward_mask: per-sample loop, output dict)
PyTorch is used for device memory, streams and parameter storage only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import lib as L
from .clicks import query_list
from .modules import walk_res16unet34c
from .sparse import SparseTensor
from .train_backbone import BackboneTape, packed_weights_of


class Scene:
    """Owner of one ``a3d_scene`` handle and its device workspace."""

    def __init__(self, coords: torch.Tensor):
        lib = L.load()
        assert coords.is_cuda and coords.dtype == torch.int32 and coords.dim() == 2 and coords.shape[1] == 4
        self.coords = coords.contiguous()
        n = self.coords.shape[0]
        nbytes = lib.a3d_scene_workspace_bytes(n)
        if nbytes == 0:
            raise L.A3DError(f"cannot build a scene of {n} voxels")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=coords.device)
        h = C.c_void_p()
        L.check(lib.a3d_scene_create(L.ptr(self.coords), n, L.ptr(self.workspace), nbytes, L.stream(), C.byref(h)),
                "a3d_scene_create")
        self.handle = h
        self.n = [int(lib.a3d_scene_level_size(h, i)) for i in range(L.A3D_NUM_LEVELS)]
        starts = (C.c_int64 * 1024)()
        nb = lib.a3d_scene_batch_ranges(h, starts, 1024)
        ends = [int(starts[i + 1]) for i in range(nb - 1)] + [n]
        self.batch_ranges = [(int(starts[i]), ends[i]) for i in range(nb)]
        dims = (C.c_int * 3)()
        # level-0 lookups go through a dense voxel grid when the batch's bounding box is small, else a hash table
        self.grid_dims = tuple(dims) if lib.a3d_scene_grid_dims(h, dims) == 1 else None

    def prepare_wgrad(self):
        """The weight-gradient work lists of this scene (a3d_scene_build_wgrad_lists), requested on the current stream at the
        first call (no synchronisation: the first weight gradient waits for their lengths); a3d_conv_wgrad refuses a scene
        without them."""
        if getattr(self, "_wgrad_lists", None) is None:
            lib = L.load()
            nbytes = lib.a3d_scene_wgrad_lists_bytes(self.handle)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.workspace.device)
            L.check(lib.a3d_scene_build_wgrad_lists(self.handle, L.ptr(ws), nbytes, L.stream()), "a3d_scene_build_wgrad_lists")
            self._wgrad_lists = ws

    def wgrad_lists(self):
        """The weight-gradient work lists on the host (tests / debugging; synchronises):
        ``{(kind, level): (lists [K, stride] int32, counts [K] int32)}`` for kind in (OP_CONV3, OP_DOWN, OP_UP), level = the
        level that owns the list (OP_UP: the FINE level, level_in - 1 of the op) -- ``lists[k, :counts[k]]`` are the ascending
        16-position groups that have offset k.  The library states the layout once, as the table kWgradMaps of csrc/wgrad.hip
        (walked by wgrad_list_set): the maps behind one another in the table's order, each [K][stride] ints with stride =
        ceil(ngroups / 64) * 64 and ngroups = ceil(positions / 16) (pos_above: positions of level + 1); the counts, one int per
        (map, offset) in the same order, start at byte align256(4 * ints).  The loop below restates that order on purpose: it
        is the tests' independent statement of the layout."""
        self.prepare_wgrad()
        torch.cuda.current_stream(self.workspace.device).synchronize()
        raw = self._wgrad_lists.cpu().numpy()
        maps, off, jobs = [], 0, 0
        for kind in (L.OP_CONV3, L.OP_DOWN, L.OP_UP):
            for level in range(L.A3D_NUM_LEVELS - (0 if kind == L.OP_CONV3 else 1)):
                K = 27 if kind == L.OP_CONV3 else 8
                npos = self.n[level + 1] if kind == L.OP_DOWN else self.n[level]
                stride = ((npos + 15) // 16 + 63) // 64 * 64
                maps.append((kind, level, K, stride, off, jobs))
                off, jobs = off + K * stride, jobs + K
        counts = raw[(4 * off + 255) // 256 * 256:][:4 * jobs].view(np.int32)
        return {(kind, level): (raw[4 * o:4 * (o + K * stride)].view(np.int32).reshape(K, stride).copy(), counts[j:j + K].copy())
                for kind, level, K, stride, o, j in maps}

    def table(self, level: int, which: int) -> np.ndarray:
        """Copy one scene table to the host (tests / debugging)."""
        lib = L.load()
        p, cnt = C.c_void_p(), C.c_int64()
        L.check(lib.a3d_scene_table(self.handle, level, which, C.byref(p), C.byref(cnt)), "a3d_scene_table")
        dt = np.uint32 if which in (L.TAB_GMASK27, L.TAB_GMASKDOWN, L.TAB_GMASKUP) else np.int32
        out = np.empty(cnt.value, dtype=dt)
        L.check(lib.a3d_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, out.nbytes, L.stream()), "a3d_memcpy_d2h")
        return out

    def table_dev(self, level: int, which: int) -> torch.Tensor:
        """One scene table as an int32 tensor VIEW of the scene's device workspace (no copy, no synchronisation; valid as
        long as this Scene lives)."""
        lib = L.load()
        p, cnt = C.c_void_p(), C.c_int64()
        L.check(lib.a3d_scene_table(self.handle, level, which, C.byref(p), C.byref(cnt)), "a3d_scene_table")
        off = p.value - self.workspace.data_ptr()
        assert 0 <= off and off + 4 * cnt.value <= self.workspace.numel() and off % 4 == 0
        return self.workspace[off:off + 4 * cnt.value].view(torch.int32)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                L.load().a3d_scene_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _Pool:
    """Activation buffers of the op program; buffers are recycled once their last reader ran."""

    def __init__(self):
        self.descs = []
        self.free = {}

    def get(self, level, ch):
        lst = self.free.get((level, ch))
        if lst:
            return lst.pop()
        self.descs.append((level, ch))
        return len(self.descs) - 1

    def put(self, i):
        self.free.setdefault(self.descs[i], []).append(i)


# what the walk of the topology passes around: ``ch`` columns from ``coff`` of pool buffer ``buf`` (``temp``: back to the pool
# once the layer that reads it ran).  A concatenation's buffer goes around as its skip half: the columns from c_up = ``coff``
_Act = namedtuple("_Act", "buf coff ch level temp")


class BackboneProgram:
    """Res16UNet34C + lin_squeeze_head as a list of ``a3d_op`` (built once per weight version): a builder of
    ``modules.walk_res16unet34c``, which states the topology."""

    def __init__(self, model, device, fuse_proj=None):
        self.keep = []          # tensors referenced by raw pointers
        self.ops = []
        self.pool = _Pool()
        self.dev = device
        # the residual projections (BasicBlock.downsample) run inside the block's second conv (a3d_op.proj_*);
        # A3D_FUSE_PROJ=0 keeps the separate 1x1 launches (tests compare the two)
        self.fuse_proj = os.environ.get("A3D_FUSE_PROJ", "1") != "0" if fuse_proj is None else fuse_proj
        self.fused_projections = 0
        self.fm_bufs = [x.buf for x in walk_res16unet34c(model.backbone, model.lin_squeeze_head, self)]    # buffers of the 5 feature maps
        self.n_ops = len(self.ops)
        self.ops_arr = (L.Op * self.n_ops)(*self.ops)
        self.n_bufs = len(self.pool.descs)
        self.bufs_arr = (L.BufDesc * self.n_bufs)(*[L.BufDesc(lv, ch) for lv, ch in self.pool.descs])

    def _pack(self, conv, w=None):
        lib = L.load()
        w = (conv.kernel3().detach() if w is None else w).to(self.dev, torch.float32).contiguous()
        K, cin, cout = w.shape
        out = torch.empty(lib.a3d_conv_weight_packed_floats(K, cin, cout), dtype=torch.float32, device=self.dev)
        L.check(lib.a3d_pack_conv_weight(L.ptr(w), K, cin, cout, L.ptr(out), L.stream()), "a3d_pack_conv_weight")
        self.keep.append(out)
        return out

    def _fold(self, bn):
        b = bn.bn
        scale = (b.weight.detach() / torch.sqrt(b.running_var.detach() + b.eps)).to(self.dev, torch.float32)
        shift = (b.bias.detach() - b.running_mean.detach() * scale.to(b.bias.device)).to(self.dev, torch.float32)
        scale, shift = scale.contiguous(), shift.contiguous()
        self.keep += [scale, shift]
        return scale, shift

    def _op(self, kind, level_in, cin, cout, src, dst, res, relu, kvol, w, scale, shift, proj=None):
        o = L.Op()
        o.kind, o.level_in, o.cin, o.cout = kind, level_in, cin, cout
        o.in_buf, o.in_coff = src
        o.out_buf, o.out_coff = dst
        o.res_buf, o.res_coff = res if res is not None else (L.BUF_NONE, 0)
        o.relu, o.kernel_volume = int(relu), kvol
        o.w_dev = w.data_ptr()
        o.scale_dev = scale.data_ptr() if scale is not None else None
        o.shift_dev = shift.data_ptr() if shift is not None else None
        if proj is not None:
            (o.proj_buf, o.proj_coff), o.proj_cin = proj[0], proj[1]
        self.ops.append(o)

    def _basic_block(self, blk, level, src, cin, cout, dst):
        """BasicBlock.forward (resnet_block.py:48-64); src/dst = (buffer, column offset)."""
        tmp = self.pool.get(level, cout)
        s1, h1 = self._fold(blk.norm1)
        self._op(L.OP_CONV3, level, cin, cout, src, (tmp, 0), None, True, 27, self._pack(blk.conv1), s1, h1)
        res, proj = src, None
        if blk.downsample is not None and self.fuse_proj and cin % 32 == 0:
            # out = relu(s2 conv2(h) + h2 + sp (x Wp) + hp): both scales into the weights, one accumulator, one launch.
            # (the kernel's stage width at these shapes is 32 or 64 channels; the 32 -> 64 block of level 2 runs its
            # 64 -> 64 conv with 32-channel stages so that its 32-channel projection is a whole stage: all seven fused)
            s2, h2 = self._fold(blk.norm2)
            sp, hp = self._fold(blk.downsample[1])
            w2 = blk.conv2.kernel3().detach().to(self.dev, torch.float32) * s2[None, None, :]
            wp = blk.downsample[0].kernel3().detach().to(self.dev, torch.float32) * sp[None, None, :]
            both = torch.cat([self._pack(None, w2), self._pack(None, wp)]).contiguous()
            shift = (h2 + hp).contiguous()
            self.keep += [both, shift]
            self._op(L.OP_CONV3, level, cout, cout, (tmp, 0), dst, None, True, 27, both, None, shift, proj=(src, cin))
            self.fused_projections += 1
            self.pool.put(tmp)
            return
        if blk.downsample is not None:
            proj = self.pool.get(level, cout)
            sp, hp = self._fold(blk.downsample[1])
            self._op(L.OP_LINEAR, level, cin, cout, src, (proj, 0), None, False, 1, self._pack(blk.downsample[0]), sp, hp)
            res = (proj, 0)
        s2, h2 = self._fold(blk.norm2)
        self._op(L.OP_CONV3, level, cout, cout, (tmp, 0), dst, res, True, 27, self._pack(blk.conv2), s2, h2)
        self.pool.put(tmp)
        if proj is not None:
            self.pool.put(proj)

    def _unit(self, kind, conv, bn, x, y):
        """Strided / transposed conv + BatchNorm + ReLU from the activation ``x`` into ``y``."""
        s, h = self._fold(bn)
        self._op(kind, x.level, conv.cin, conv.cout, x[:2], y[:2], None, True, 8, self._pack(conv), s, h)
        return y

    # ---------------------------------------------------------------- the builder's verbs (modules.walk_res16unet34c)
    def concat_buffer(self, level, c_up, c_skip):
        return _Act(self.pool.get(level, c_up + c_skip), c_up, c_skip, level, False)

    def stem(self, conv, bn, cat):
        s, h = self._fold(bn)
        w0 = conv.kernel3().detach().to(self.dev, torch.float32).contiguous()
        self.keep.append(w0)
        self._op(L.OP_STEM, 0, conv.cin, conv.cout, (L.BUF_NONE, 0), cat[:2], None, True, w0.shape[0], w0, s, h)
        return cat

    def down(self, conv, bn, x):
        return self._unit(L.OP_DOWN, conv, bn, x, _Act(self.pool.get(x.level + 1, conv.cout), 0, conv.cout, x.level + 1, True))

    def layer(self, blocks, x, skip_of=None):
        cout = blocks[-1].conv2.cout
        out = skip_of if skip_of is not None else _Act(self.pool.get(x.level, cout), 0, cout, x.level, False)
        for i, blk in enumerate(blocks):
            y = out if i == len(blocks) - 1 else _Act(self.pool.get(x.level, cout), 0, cout, x.level, True)
            self._basic_block(blk, x.level, x[:2], x.ch, cout, y[:2])
            if x.temp:
                self.pool.put(x.buf)
            x = y
        return out

    def up(self, conv, bn, x, cat):
        self._unit(L.OP_UP, conv, bn, x, cat._replace(coff=0))

    def concat(self, cat):
        return _Act(cat.buf, 0, cat.coff + cat.ch, cat.level, False)

    def head(self, head, x):
        """lin_squeeze_head: 1x1 conv + bias into the caller-ordered output (agile3d.py:179)."""
        hb = head.bias.detach().reshape(-1).to(self.dev, torch.float32).contiguous()
        self.keep.append(hb)
        hw = self._pack(head)
        last = self.ops[-1]                   # block8's last conv: its workgroups hold complete 96-column output rows
        if (os.environ.get("A3D_FUSE_HEAD", "0") == "1" and last.kind == L.OP_CONV3 and last.out_buf == x.buf
                and last.proj_cin == 0):
            # lin_squeeze_head as a second GEMM in that conv's epilogue (SURVEY 2.1's second fusion): the [N, 96] rows are
            # not read back, one launch less.  The library runs the head as its own 1x1 launch where no fused build exists.
            # OPT-IN (A3D_FUSE_HEAD=1): built and measured in round 5 -- the fused launch takes 2 650-2 760 us on the 16-scene
            # batch against 2 190 + 336 for conv + k_dense (four workgroups per CU each stream the 48 KB head weights through
            # the CU's L1 for every 64-row tile), 640-643 vs 643-646 scenes/s; one scene: 208 vs 172 + 33 us
            # (profiles/r05_experiments.txt).  The separate launch stays the default.
            last.head_w_dev, last.head_bias_dev, last.head_cout = hw.data_ptr(), hb.data_ptr(), head.cout
            self.fused_head = True
        else:
            self._op(L.OP_LINEAR, 0, x.ch, head.cout, x[:2], (L.BUF_EXT_OUT, 0), None, False, 1, hw, None, hb)
            self.fused_head = False

    def run(self, scene: Scene, feats: torch.Tensor, out: torch.Tensor):
        lib = L.load()
        nbytes = lib.a3d_program_workspace_bytes(scene.handle, self.bufs_arr, self.n_bufs, self.ops_arr, self.n_ops)
        if nbytes == 0:
            raise L.A3DError("a3d_program_workspace_bytes: " + lib.a3d_last_error().decode())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=feats.device)
        L.check(lib.a3d_program_run(scene.handle, self.bufs_arr, self.n_bufs, self.ops_arr, self.n_ops,
                                    L.ptr(feats), L.ptr(out), out.shape[1], L.ptr(ws), nbytes, L.stream()),
                "a3d_program_run")
        return ws

    def feature_map(self, scene: Scene, ws: torch.Tensor, i: int) -> torch.Tensor:
        lib = L.load()
        b = self.fm_bufs[i]
        off = lib.a3d_program_buffer_offset(scene.handle, self.bufs_arr, self.n_bufs, b)
        level, ch = self.pool.descs[b]
        n = scene.n[level]
        return ws[off:off + n * ch * 4].view(torch.float32).view(n, ch)


def time_table(d_model=128, length=200):
    """PositionalEncoding1D (position_embedding.py:210-225)."""
    pe = torch.zeros(length, d_model)
    position = torch.arange(0, length).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position.float() * div_term)
    pe[:, 1::2] = torch.cos(position.float() * div_term)
    return pe


class DecoderPack:
    """``a3d_decoder_weights`` for the model's current parameters."""

    def __init__(self, model, device):
        lib = L.load()
        self.keep = []
        dev = device
        W = L.DecoderWeights()
        n_layers = model.num_decoders
        if n_layers > L.A3D_MAX_DEC_LAYERS:
            raise L.A3DError("too many decoder layers")
        W.n_layers = n_layers
        W.n_bg_queries = model.num_bg_queries
        W.dim_ff = model.args.dim_feedforward

        def dv(t):
            t = t.detach().to(dev, torch.float32).contiguous()
            self.keep.append(t)
            return t.data_ptr()

        def tr(t):   # query-side matrices stay in torch layout [out][in]
            return dv(t)

        def packed(wt_in_out):  # [in][out] -> MFMA fragment order
            w = wt_in_out.detach().to(dev, torch.float32).contiguous().unsqueeze(0)
            out = torch.empty_like(w)
            L.check(lib.a3d_pack_conv_weight(L.ptr(w), 1, w.shape[1], w.shape[2], L.ptr(out), L.stream()),
                    "a3d_pack_conv_weight")
            self.keep.append(out)
            return out.data_ptr()

        d = model.mask_dim
        for l in range(n_layers):
            li = 0 if model.shared_decoder else l
            c2s = model.c2s_attention[li][0]
            c2c = model.c2c_attention[li][0]
            ffn = model.ffn_attention[li][0]
            s2c = model.s2c_attention[li][0]
            lw = W.layers[l]
            a = c2s.multihead_attn
            lw.c2s_in_w, lw.c2s_in_b = tr(a.in_proj_weight), dv(a.in_proj_bias)
            lw.c2s_out_w, lw.c2s_out_b = tr(a.out_proj.weight), dv(a.out_proj.bias)
            lw.c2s_norm_w, lw.c2s_norm_b = dv(c2s.norm.weight), dv(c2s.norm.bias)
            lw.c2s_wk_packed = packed(a.in_proj_weight[d:2 * d].t())
            lw.c2s_wv_packed = packed(a.in_proj_weight[2 * d:].t())
            a = c2c.self_attn
            lw.c2c_in_w, lw.c2c_in_b = tr(a.in_proj_weight), dv(a.in_proj_bias)
            lw.c2c_out_w, lw.c2c_out_b = tr(a.out_proj.weight), dv(a.out_proj.bias)
            lw.c2c_norm_w, lw.c2c_norm_b = dv(c2c.norm.weight), dv(c2c.norm.bias)
            lw.ffn_w1, lw.ffn_b1 = tr(ffn.linear1.weight), dv(ffn.linear1.bias)
            lw.ffn_w2, lw.ffn_b2 = tr(ffn.linear2.weight), dv(ffn.linear2.bias)
            lw.ffn_norm_w, lw.ffn_norm_b = dv(ffn.norm.weight), dv(ffn.norm.bias)
            a = s2c.multihead_attn
            lw.s2c_in_w, lw.s2c_in_b = tr(a.in_proj_weight), dv(a.in_proj_bias)
            lw.s2c_out_w, lw.s2c_out_b = tr(a.out_proj.weight), dv(a.out_proj.bias)
            lw.s2c_norm_w, lw.s2c_norm_b = dv(s2c.norm.weight), dv(s2c.norm.bias)
            lw.s2c_wq_packed = packed(a.in_proj_weight[:d].t())
            lw.s2c_wo_packed = packed(a.out_proj.weight.t())
        W.decoder_norm_w, W.decoder_norm_b = dv(model.decoder_norm.weight), dv(model.decoder_norm.bias)
        m0, m2 = model.mask_embed_head[0], model.mask_embed_head[2]
        W.mask_w0, W.mask_b0 = tr(m0.weight), dv(m0.bias)
        W.mask_w2, W.mask_b2 = tr(m2.weight), dv(m2.bias)
        W.bg_query_feat, W.bg_query_pos = dv(model.bg_query_feat.weight), dv(model.bg_query_pos.weight)
        # what the position-encoding kernels read: gauss_B (fourier), inv_freq (legacy), nothing (sine) -- the model's
        # current buffer, so a loaded checkpoint's reaches the device with the next pack
        kind = getattr(model, "pos_enc_type", "fourier")
        W.gauss_B = dv(model.pos_enc.gauss_B) if kind == "fourier" else None
        self.posenc_table_ptr = dv(model.pos_enc.inv_freq) if kind == "legacy" else W.gauss_B
        W.time_table = dv(time_table(d, 200))
        # the query side's matrices once more, in the order the single-block layer kernel's waves read them
        for l in range(n_layers):
            qp = torch.empty(lib.a3d_decoder_query_pack_floats(W.dim_ff), dtype=torch.float32, device=dev)
            L.check(lib.a3d_decoder_pack_query_weights(C.byref(W), l, L.ptr(qp), L.stream()), "a3d_decoder_pack_query_weights")
            self.keep.append(qp)
            W.layers[l].query_pack = qp.data_ptr()
        mp = torch.empty(lib.a3d_decoder_mask_pack_floats(), dtype=torch.float32, device=dev)
        L.check(lib.a3d_decoder_pack_query_weights(C.byref(W), -1, L.ptr(mp), L.stream()), "a3d_decoder_pack_query_weights")
        self.keep.append(mp)
        W.mask_pack = mp.data_ptr()
        self.W = W
        self.n_layers = n_layers
        self.gauss_B_ptr = W.gauss_B


_KV_MB = None


def _kv_cache_mb():
    """Cap of the per-scene key / value cache of forward_mask in MB (A3D_KV_CACHE_MB, default 4096; 0 = off)."""
    global _KV_MB
    if _KV_MB is None:
        _KV_MB = int(os.environ.get("A3D_KV_CACHE_MB", "4096"))
    return _KV_MB


class _SceneState:
    """Everything forward_mask needs from forward_backbone; rides on the returned pcd_features."""

    def __init__(self, engine_id, ranges, posenc, minmax, scene=None, ws=None, train=False):
        self.engine_id = engine_id
        self.ranges = ranges
        self.posenc = posenc    # list[Tensor [n_b,128]]
        self.minmax = minmax    # list[Tensor [6]]
        self.scene, self.ws = scene, ws
        self.train = train      # produced by the training-mode forward (no inference workspace, aux placeholders)
        # per-scene cache of the first decoder layer's click-to-scene keys / values (click-independent): allocated and
        # filled by the SECOND forward_mask on this backbone output, read by every later one
        self.mask_calls = 0
        self.kv0 = None         # list[Tensor [3, n_b, 128]]: keys, values, scene-to-click queries of the first layer
        self.kv0_version = None


def _is_backbone(name):
    """Whether a state-dict key belongs to forward_backbone's half of the model (the rest is forward_mask's)."""
    return name.startswith(("backbone.", "lin_squeeze_head."))


class Engine:
    def __init__(self, model, device):
        L.load()
        self.model = model
        self.device = device
        self._stale = True
        self._stale_dec = True
        self._version = None
        self._version_dec = None
        self._dec_epoch = 0          # counts the decoder packs: what a scene's cached keys / values were made with
        self._dec_tensors = None
        self._all_tensors = None
        self.program = None
        self.decoder = None

    def backbone_statistics_moved(self):
        """The BatchNorm running statistics were written through raw pointers (a training-mode forward, BackboneTape): the
        folded backbone program is out of date."""
        self._stale = True

    def mark_stale(self):
        """The weights were written behind torch's back (the library's AdamW, load_state_dict): every pack is out of date,
        the training tapes' packed conv weights included."""
        self._stale = True
        self._stale_dec = True
        packed_weights_of(self.model).invalidate()

    def _weights_version(self, decoder_only=False):
        if self._dec_tensors is None:
            sd = self.model.state_dict(keep_vars=True)
            self._all_tensors = list(sd.values())
            self._dec_tensors = [v for k, v in sd.items() if not _is_backbone(k)]
        return sum(int(t._version) for t in (self._dec_tensors if decoder_only else self._all_tensors))

    def refresh_weights_if_stale(self, check_versions=False):
        """Packed weights of the inference path: the folded/packed backbone program and the decoder pack.  They are
        rebuilt when marked stale or (``check_versions``) when a parameter tensor was written since (an optimiser step)."""
        if not self._stale and check_versions:
            if self._weights_version() != self._version:
                self._stale = self._stale_dec = True
        if self._stale:
            with torch.no_grad():
                self.program = BackboneProgram(self.model, self.device)
            self._version = self._weights_version()
            self._stale = False
        self.refresh_decoder_if_stale()

    def refresh_decoder_if_stale(self, check_versions=False):
        """The decoder's packed weights only: what forward_mask needs (the no-grad click rounds of a training
        iteration, engine.py:82-115, must not re-fold and re-pack the whole backbone)."""
        if not self._stale_dec and check_versions and self._weights_version(True) != self._version_dec:
            self._stale_dec = True
        if self._stale_dec or self.decoder is None:
            with torch.no_grad():
                self.decoder = DecoderPack(self.model, self.device)
            self._version_dec = self._weights_version(True)
            self._stale_dec = False
            self._dec_epoch += 1

    # ---------------------------------------------------------------- forward_backbone
    def _raw_rows(self, raw_coordinates, n):
        """``raw_coordinates`` as the fp32 [n, 3] tensor on this device that the position encodings are made from."""
        if raw_coordinates is None:
            raise ValueError("forward_backbone needs raw_coordinates (agile3d.py:163)")
        raw = raw_coordinates.to(self.device, torch.float32).contiguous()
        if raw.shape != (n, 3):
            raise ValueError("raw_coordinates must be [N,3]")
        return raw

    def _sparse_input(self, x, raw_coordinates):
        """``x`` as a SparseTensor on this device and its raw coordinates (``_raw_rows``)."""
        if not isinstance(x, SparseTensor) or x.device != self.device:
            x = SparseTensor(features=x.F, coordinates=x.C, device=self.device)
        return x, self._raw_rows(raw_coordinates, len(x))

    def _backbone_result(self, feats, coords, raw, st):
        """What forward_backbone returns (agile3d.py:181), with ``st`` riding on pcd_features: (pcd_features, aux,
        coordinates, pos_encodings_pcd) -- only the finest level's position encodings exist (hlevels = [4])."""
        pcd_features = SparseTensor(features=feats, coordinates=coords)
        pcd_features._a3d = st
        aux = [None] * 5 if st.train else _AuxList(self.program, st) if st.ws is not None else None
        pos_encodings_pcd = [[[None] * len(st.ranges)] for _ in range(4)] + [[list(st.posenc)]]
        return pcd_features, aux, SparseTensor(features=raw, coordinates=coords), pos_encodings_pcd

    def forward_backbone(self, x, raw_coordinates=None):
        self.refresh_weights_if_stale(check_versions=True)
        x, raw = self._sparse_input(x, raw_coordinates)
        with torch.no_grad():
            scene = Scene(x.C)
            out = torch.empty((len(x), self.model.mask_dim), dtype=torch.float32, device=self.device)
            ws = self.program.run(scene, x.F, out)
            ranges = scene.batch_ranges      # from the scene build's single read-back, no torch kernels
            st = _SceneState(id(self), ranges, *self._posenc_batch(raw, ranges), scene=scene, ws=ws)
        return self._backbone_result(out, x.C, raw, st)

    def forward_backbone_train(self, x, raw_coordinates=None):
        """``forward_backbone`` of a model in training mode (engine.py:53 of the reference): BatchNorm on the statistics
        of this batch (running statistics updated), every activation kept for the backward pass (BackboneTape), the
        result tied into torch.autograd -- ``pcd_features.F`` depends on every backbone parameter."""
        from .autograd import BackboneFn, _Holder
        self.refresh_decoder_if_stale(check_versions=True)      # gauss_B / inv_freq for the position encodings
        x, raw = self._sparse_input(x, raw_coordinates)
        with torch.no_grad():
            packed_weights_of(self.model).refresh_all()      # scene-independent: queued before the scene build's host round trip
            scene = Scene(x.C)
            tape = BackboneTape(self.model, scene, x.F.detach())
            ranges = scene.batch_ranges
            st = _SceneState(id(self), ranges, *self._posenc_batch(raw, ranges), scene=scene, train=True)
        named = [(k, p) for k, p in self.model.named_parameters() if _is_backbone(k)]
        holder = _Holder(tape=tape, names=[k for k, _ in named])
        out = BackboneFn.apply(holder, *[p for _, p in named]) if torch.is_grad_enabled() else tape.output
        return self._backbone_result(out, x.C, raw, st)

    def decoder_inputs(self, feats128: torch.Tensor, raw_xyz: torch.Tensor):
        """Single-sample decoder inputs from an explicit [N,128] feature matrix (what
        forward_backbone would have produced) -- used by the golden-vector parity tests, which
        hold the reference's decoder inputs directly."""
        self.refresh_decoder_if_stale(check_versions=True)
        feats = feats128.to(self.device, torch.float32).contiguous()
        n = feats.shape[0]
        raw = self._raw_rows(raw_xyz, n)
        with torch.no_grad():
            pe, mm = self._posenc(raw)
        coords = torch.zeros((n, 4), dtype=torch.int32, device=self.device)
        return self._backbone_result(feats, coords, raw, _SceneState(id(self), [(0, n)], [pe], [mm]))

    def decoder_inputs_batch(self, feats128: torch.Tensor, raw_xyz: torch.Tensor, ranges):
        """Decoder inputs of a whole batch from an explicit feature matrix (rows of sample i = ``ranges[i]``): what
        forward_backbone returns for it -- the training iteration runs its no-grad click rounds on the training-mode
        backbone's features this way (engine.py:82-116 of the reference)."""
        self.refresh_decoder_if_stale(check_versions=True)
        feats = feats128.to(self.device, torch.float32).contiguous()
        n = feats.shape[0]
        raw = self._raw_rows(raw_xyz, n)
        coords = torch.zeros((n, 4), dtype=torch.int32, device=self.device)
        ranges = [(int(s), int(e)) for s, e in ranges]
        with torch.no_grad():
            for b, (s, e) in enumerate(ranges):
                coords[s:e, 0] = b
            st = _SceneState(id(self), ranges, *self._posenc_batch(raw, ranges))
        return self._backbone_result(feats, coords, raw, st)

    def _posenc(self, raw, starts=None):
        """The position encoding this model was built with (args.positional_encoding_type, args.normalize_pos_enc;
        DESIGN.md §4.8) of the rows ``raw`` [n, 3]: one sample (``starts`` None: ([n, 128], [6] min / max)) or the samples
        ``[starts[b], starts[b + 1])`` (ctypes int64 array; ([n, 128], [ns, 6])).  The min / max is None where the
        encoding does not normalise (no reduction runs)."""
        lib = L.load()
        m = self.model
        kind, norm = L.POSENC_KINDS[m.pos_enc_type], int(m.normalize_pos_enc and m.pos_enc_type != "legacy")
        n = raw.shape[0]
        ns = None if starts is None else len(starts) - 1
        pe = torch.empty((n, 128), dtype=torch.float32, device=self.device)
        mm = tmp = None
        if norm:
            mm = torch.empty(6 if ns is None else (ns, 6), dtype=torch.float32, device=self.device)
            tmp = torch.empty(256 * 6 * 4 if ns is None else lib.a3d_posenc_batch_workspace_bytes(ns), dtype=torch.uint8,
                              device=self.device)
        tail = (L.ptr(mm), L.ptr(pe), L.ptr(tmp), tmp.numel() if norm else 0, L.stream())
        table = self.decoder.posenc_table_ptr
        if ns is None:
            L.check(lib.a3d_posenc(kind, norm, L.ptr(raw), n, table, *tail), "a3d_posenc")
        else:
            L.check(lib.a3d_posenc_batch(kind, norm, L.ptr(raw), starts, ns, table, *tail), "a3d_posenc_batch")
        return pe, mm

    def _posenc_batch(self, raw, ranges):
        """Position encodings of every sample of a batch (agile3d.py:141-161 loops over the samples; each has its
        own min / max) in three launches: (list of [n_b, 128] views of one matrix, list of [6] min/max views; None where
        the model's encoding uses no min / max)."""
        ns = len(ranges)
        if ns > 64 or any(ranges[i][1] != ranges[i + 1][0] for i in range(ns - 1)) or any(e <= s for s, e in ranges):
            pairs = [self._posenc(raw[s:e]) for (s, e) in ranges]          # unusual layouts: sample by sample
            return [p for p, _ in pairs], [m for _, m in pairs]
        s0, e1 = ranges[0][0], ranges[-1][1]
        starts = (C.c_int64 * (ns + 1))(*([r[0] - s0 for r in ranges] + [e1 - s0]))
        pe_all, mm_all = self._posenc(raw[s0:e1], starts)
        return [pe_all[s - s0:e - s0] for (s, e) in ranges], [None if mm_all is None else mm_all[b] for b in range(ns)]

    # ---------------------------------------------------------------- forward_mask
    def _mask_state(self, pcd_features, click_idx, click_time_idx):
        """The state forward_backbone left on ``pcd_features``, after the argument checks of both forward_masks."""
        st = getattr(pcd_features, "_a3d", None)
        if st is None or st.engine_id != id(self):
            raise RuntimeError("forward_mask needs the objects returned by this model's forward_backbone")
        if click_idx is None or click_time_idx is None:
            raise ValueError("click_idx and click_time_idx are required")
        return st

    def _mask_result(self, preds, pcd_features):
        """forward_mask's dictionary (agile3d.py:325-339) from ``preds[layer][sample]``."""
        out = {"pred_masks": preds[-1], "backbone_features": pcd_features}
        if self.model.aux:
            out["aux_outputs"] = [{"pred_masks": p} for p in preds[:-1]]
        return out

    def forward_mask_train(self, pcd_features, aux, coordinates, pos_encodings_pcd, click_idx=None, click_time_idx=None):
        """``forward_mask`` of a model in training mode (engine.py:120-122): one DecoderTape per batch sample
        (agile3d.py:192 loops over the samples), logits tied into torch.autograd."""
        from .autograd import DecoderFn, _Holder
        from .train_decoder import DecoderTape, draw_seed
        st = self._mask_state(pcd_features, click_idx, click_time_idx)
        named = [(k, p) for k, p in self.model.named_parameters() if not _is_backbone(k)]
        names, params = [k for k, _ in named], [p for _, p in named]
        n_layers = self.model.num_decoders
        preds = [[] for _ in range(n_layers)]
        # dropout: one seed per call, sample b's masks keyed by b -- the masks a batched tape of the same seed draws
        p = getattr(self.model, "dropout", 0.0)
        seed = draw_seed() if p > 0 else None
        for b, (s, e) in enumerate(st.ranges):
            rows = pcd_features.F[s:e]
            with torch.no_grad():
                tape = DecoderTape(self.model, rows.detach(), st.posenc[b], click_idx[b], click_time_idx[b], dropout=p, seed=seed,
                                   sample_base=b)
            if torch.is_grad_enabled():
                logits = DecoderFn.apply(_Holder(tape=tape, names=names), rows, *params)
            else:
                logits = tape.logits
            for l in range(n_layers):
                preds[l].append(logits[l])
        return self._mask_result(preds, pcd_features)

    def forward_mask(self, pcd_features, aux, coordinates, pos_encodings_pcd, click_idx=None, click_time_idx=None):
        lib = L.load()
        st = self._mask_state(pcd_features, click_idx, click_time_idx)
        self.refresh_decoder_if_stale(check_versions=True)
        W = self.decoder.W
        n_layers = self.decoder.n_layers
        preds = [[] for _ in range(n_layers)]
        # The interactive loop calls forward_mask ~100 times on one backbone output (eval_multi_obj.py:112-160): from the
        # second call on the scene's first-layer keys / values / scene-to-click queries are kept (123 MB per 80 k voxels; A3D_KV_CACHE_MB caps the
        # total, 0 switches the cache off).  A single call per scene -- the throughput benchmark -- allocates nothing.
        st.mask_calls += 1
        kv_state = 0
        kv_fill = None
        # what the cached keys / values were made from: the decoder pack AND the feature rows (a tensor swapped or
        # written in place between two calls must not be served stale keys)
        F_ = pcd_features.F
        kv_key = (self._dec_epoch, F_.data_ptr(), int(F_._version), tuple(st.ranges))
        if st.mask_calls >= 2 and _kv_cache_mb() > 0:
            if st.kv0 is not None and st.kv0_version == kv_key:
                kv_state = 2
            else:
                st.kv0, st.kv0_version = None, None
                total = sum(e - s for s, e in st.ranges) * 3 * 128 * 4      # keys, values, scene-to-click queries of the first layer
                if total <= _kv_cache_mb() * (1 << 20):
                    kv_fill = [torch.empty((3, e - s, 128), dtype=torch.float32, device=self.device) for s, e in st.ranges]
                    kv_state = 1
        kv_bufs = st.kv0 if kv_state == 2 else kv_fill
        with torch.no_grad():
            # the reference loops over the batch samples (agile3d.py:192); here every sample is described once and
            # the whole batch goes through a3d_decoder_forward_batch (one launch of each wide kernel per layer)
            samples = (L.DecoderSample * len(st.ranges))()
            keep = []                                   # host arrays / tensors the library reads during the call
            for b, (s, e) in enumerate(st.ranges):
                nb = e - s
                # the queries: the clicks of objects 1..K in object order, then the background's (clicks.query_list)
                rows, times, counts, bg_rows, bg_times = query_list(click_idx[b], click_time_idx[b])
                K = len(counts)
                objs = []
                for o, c in enumerate(counts, start=1):
                    objs += [o] * c
                objs += [0] * len(bg_rows)
                rows += bg_rows
                times += bg_times
                nc = len(rows)
                nq = nc + W.n_bg_queries
                wsb = lib.a3d_decoder_workspace_bytes(nb, nq)
                if wsb == 0:
                    raise L.A3DError(f"too many queries ({nq} > {L.A3D_MAX_QUERIES})")
                ws = torch.empty(wsb, dtype=torch.uint8, device=self.device)
                logits = torch.empty((n_layers, nb, K + 1), dtype=torch.float32, device=self.device)
                arr = lambda v: (C.c_int32 * max(1, len(v)))(*v)
                feats = pcd_features.F.detach()[s:e]
                a_rows, a_objs, a_times = arr(rows), arr(objs), arr(times)
                keep += [ws, feats, a_rows, a_objs, a_times]
                sp = samples[b]
                sp.feats128_dev, sp.posenc_dev, sp.n = L.ptr(feats), L.ptr(st.posenc[b]), nb
                sp.click_row = C.cast(a_rows, C.POINTER(C.c_int32))
                sp.click_obj = C.cast(a_objs, C.POINTER(C.c_int32))
                sp.click_time = C.cast(a_times, C.POINTER(C.c_int32))
                sp.n_clicks, sp.n_objects = nc, K
                sp.logits_dev, sp.workspace_dev, sp.workspace_bytes = L.ptr(logits), L.ptr(ws), wsb
                sp.kv0_dev, sp.kv0_state = (L.ptr(kv_bufs[b]), kv_state) if kv_state else (None, 0)
                sp.kv0_blocks = int(kv_bufs[b].shape[0]) if kv_state else 0
                for l in range(n_layers):
                    preds[l].append(logits[l])
            try:
                L.check(lib.a3d_decoder_forward_batch(C.byref(W), samples, len(st.ranges), L.stream()),
                        "a3d_decoder_forward_batch")
            except Exception:
                st.kv0, st.kv0_version = None, None     # a failed call leaves no cache behind (filled or being read)
                raise
            if kv_state == 1:                           # stamped valid only once the fill has been issued without an error
                st.kv0, st.kv0_version = kv_fill, kv_key
        return self._mask_result(preds, pcd_features)


class _AuxFeature:
    """One of the 5 backbone feature maps (res16unet.py:250-290), rows in the library's internal
    order with matching coordinates.  The reference's forward_mask never reads ``aux``."""

    def __init__(self, program, st, i):
        self._p, self._st, self._i = program, st, i

    @property
    def F(self):
        return self._p.feature_map(self._st.scene, self._st.ws, self._i)

    @property
    def C(self):
        level = 4 - self._i
        t = torch.from_numpy(self._st.scene.table(level, L.TAB_XYZB).reshape(-1, 4).astype(np.int32))
        scale = 1 << level
        c = torch.stack([t[:, 3], t[:, 0] * scale, t[:, 1] * scale, t[:, 2] * scale], 1)
        return c.to(self._st.ws.device)

    @property
    def device(self):
        return self._st.ws.device


class _AuxList(list):
    def __init__(self, program, st):
        super().__init__(_AuxFeature(program, st, i) for i in range(5))
