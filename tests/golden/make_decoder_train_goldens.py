#!/usr/bin/env python3
"""Generate the decoder training fixtures by RUNNING THE REFERENCE's own ``Agile3d.forward_mask`` in training mode, its
own ``SetCriterion`` and ``loss.backward()``.

Runs only where the reference checkout (REF) is present; the tests read only the fixtures it writes.  The reference's
``models`` package is imported over the MinkowskiEngine stub of ``make_goldens.py`` (the decoder is pure torch), built
with ``args.dropout = p``, loaded with ``strict=True`` (the committed ``decoder_weights.npz`` for every decoder entry,
the stub's own zeros for the backbone, which the decoder never reads) and run in float64 (the click position encodings
in float32, as the reference's ``pos_enc`` casts) in ``.train()``.  The loss is the reference's ``SetCriterion``
(models/criterion.py) with bce and dice, coefficients 1 and 2, and the aux levels; the per-point weights come from the
reference's ``utils/seg.py: cal_click_loss_weights`` (loaded by path).

Inputs are the committed forward cases ``decoder_case_<name>.npz`` (feats128, xyz, pos_enc, clicks), not stored again.
Before anything is written, the float64 run at p = 0 must reproduce each case's committed logits0..2 (1e-5) and
attn_mask0/1 (exactly): the new fixtures stand on the forward that is already pinned.  Targets label the points within
TARGET_RADIUS of an object's clicks with that object (later objects win, everything else 0).

Dropout: ``torch.nn.functional.dropout`` is replaced for the run (in torch 2.10 both nn.Dropout and the need_weights
path of ``F.multi_head_attention_forward`` call it).  The replacement numbers the calls of every decoder pass as sites
0-7, asserts 8 calls per pass with ``training=True``, the case's p and the site's shape ([8,Q,N], [Q,128], [8,Q,Q],
[Q,128], [Q,1024], [Q,128], [8,N,Q], [N,128]) and multiplies by ``tests/dropout_ref.py``'s keep mask of
(seed, sample, 8 d + s) scaled by 1 / (1 - p).  That pins the placement of the sites against the reference's modules.

The batch case runs each sample alone (the reference's CPU branch handles one sample per call) with its own sample
index in the masks, and hands both samples' outputs to ONE criterion call: the loss is the reference's mean over the
samples, so the batch gradient is the mean of the per-sample gradients.

Stored per fixture (``decoder_train_<name>.npz``, each < 1 MiB):
  meta            input case names, p, seed
  s<b>::*         per sample: targets (int8), weights (float32), logits of the 3 passes on every LOGIT_ROW_STEP-th row
                  and their float64 column sums over all rows, the attention masks of passes 1-2 (packed bits), the ReLU
                  decisions of the FFN hidden layer [Q, 1024] and the mask-MLP hidden layer [Q, 128] per pass (packed
                  bits, query order: clicks, learned background queries, background clicks) with every pre-activation
                  of |z| < RELU_NEAR listed, and dL/d(pcd_features): every click row, every D_PCD_ROW_STEP-th row, the
                  column sums, sum and sum of squares
  loss::<key>     the loss dict (float64) and ``total`` = sum of weight_dict[k] * loss[k]
  grad::<name>    float64 gradient of every decoder parameter: in full up to GRAD_FULL_MAX elements, else the rows
                  ``grad_rows::<name>`` (evenly spread, GRAD_KEEP elements at least); ``grad_sum::`` / ``grad_sumsq::``
                  over the whole tensor.  (Full storage up to 20 k elements would put the nine 128 x 128 out_proj
                  gradients alone over the file budget.)

  python tests/golden/make_decoder_train_goldens.py            write the fixtures
  python tests/golden/make_decoder_train_goldens.py --check    regenerate and compare with the committed files (bit for bit)
"""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_goldens import ST, install_me_stub  # noqa: E402
from dropout_ref import keep_mask  # noqa: E402

MAX_FILE_BYTES = 1 << 20
LOGIT_ROW_STEP = 4
D_PCD_ROW_STEP = 16
GRAD_FULL_MAX = 4096
GRAD_KEEP = 1024
RELU_NEAR = 1e-3
TARGET_RADIUS = 0.8
N_SITES = 8

# fixture -> (input cases, p, dropout seed)
CASES = {
    "q75": (["n1500_k7_q75"], 0.0, 0),
    "q205": (["n220_k10_q205"], 0.0, 0),
    "dup": (["n1024_k2_dup"], 0.0, 0),
    "drop": (["n777_k4_ragged"], 0.1, 0x5EED_0001_D20B_0710),
    "batch2": (["n777_k4_ragged", "n2048_k3_bg"], 0.5, 0xB47C_4002_0000_0005),
}


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_input(name):
    z = np.load(os.path.join(HERE, f"decoder_case_{name}.npz"))
    return {k: z[k] for k in z.files}


def clicks_of(c):
    K = int(c["K"])
    ci = {str(o): [] for o in range(K + 1)}
    ct = {str(o): [] for o in range(K + 1)}
    for r, o, t in zip(c["click_rows"].tolist(), c["click_objs"].tolist(), c["click_times"].tolist()):
        ci[str(o)].append(int(r))
        ct[str(o)].append(int(t))
    return ci, ct


def make_targets(c):
    xyz = c["xyz"].astype(np.float64)
    t = np.zeros(len(xyz), np.int8)
    for r, o in zip(c["click_rows"].tolist(), c["click_objs"].tolist()):
        if o > 0:
            t[np.linalg.norm(xyz - xyz[r], axis=1) < TARGET_RADIUS] = o
    return t


class DropoutSites:
    """Stands in for torch.nn.functional.dropout during a run: numbers the calls as (pass, site), checks them and applies
    the project's keep masks."""

    def __init__(self, p, seed):
        self.p, self.seed, self.sample, self.calls, self.shapes = p, seed, 0, 0, None

    def __call__(self, x, p=0.5, training=True, inplace=False):
        d, s = divmod(self.calls, N_SITES)
        self.calls += 1
        assert training is True and not inplace and p == self.p, (training, inplace, p)
        assert tuple(x.shape) == self.shapes[s], (d, s, tuple(x.shape), self.shapes[s])
        heads, rows, cols = x.shape if x.dim() == 3 else (1,) + tuple(x.shape)
        keep = torch.from_numpy(keep_mask(self.seed, self.sample, N_SITES * d + s, p, heads, rows, cols)).reshape(x.shape)
        return x * keep.to(x.dtype) * (1.0 / (1.0 - p))

    def start(self, sample, Q, N):
        self.sample, self.calls = sample, 0
        self.shapes = [(8, Q, N), (Q, 128), (8, Q, Q), (Q, 128), (Q, 1024), (Q, 128), (8, N, Q), (N, 128)]


def build_reference(p, decoder_weights):
    install_me_stub()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    if REPO not in sys.path:
        sys.path.insert(1, REPO)
    import models as ref_models
    from agile3d_amd.model import default_args
    args = default_args(dropout=p, bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"], aux=True)
    ref = ref_models.build_model(args)
    sd = ref.state_dict()
    missing = [k for k in decoder_weights if k not in sd]
    assert not missing, missing
    sd.update({k: torch.from_numpy(v) for k, v in decoder_weights.items()})
    print("strict load into the reference:", ref.load_state_dict(sd, strict=True))
    ref.double()
    ref.pos_enc.float()          # the click encodings run in float32 (agile3d.py casts the coordinates with .float())
    crit = load_by_path("ref_criterion", os.path.join(REF, "models", "criterion.py")).build_mask_criterion(args)
    return ref.train(), crit


def _packbits(m):
    return np.packbits(np.asarray(m, bool).reshape(-1))


def run_fixture(name, decoder_weights, seg):
    in_names, p, seed = CASES[name]
    ref, crit = build_reference(p, decoder_weights)
    params = {k: v for k, v in ref.named_parameters()}
    for v in params.values():
        v.grad = None
    sites = DropoutSites(p, seed)
    pre = []             # pre-activations of the FFN hidden layer and the mask MLP, in call order
    hooks = [ref.ffn_attention[d][0].linear1.register_forward_hook(lambda m, i, o: pre.append(("ffn", o.detach())))
             for d in range(3)]
    hooks.append(ref.mask_embed_head[0].register_forward_hook(lambda m, i, o: pre.append(("mlp", o.detach()))))
    recorded = []
    orig_mask_module = ref.mask_module

    def mask_module(*a, **k):
        out = orig_mask_module(*a, **k)
        recorded.append(out[1].clone())
        return out
    ref.mask_module = mask_module
    samples, preds, targets, weights = [], [], [], []
    orig_dropout = F.dropout
    if p > 0:
        F.dropout = sites
    try:
        for b, in_name in enumerate(in_names):
            c = load_input(in_name)
            ci, ct = clicks_of(c)
            N = len(c["feats128"])
            Q = len(c["click_rows"]) + ref.bg_query_feat.weight.shape[0]
            sites.start(b, Q, N)
            pcd = torch.from_numpy(c["feats128"]).double().requires_grad_(True)
            xyz = torch.from_numpy(c["xyz"])
            C = torch.zeros(N, 4, dtype=torch.int32)
            pos = [[[torch.from_numpy(c["pos_enc"]).double()]] for _ in range(5)]
            pre.clear()
            recorded.clear()
            out = ref.forward_mask(ST(pcd, C), None, ST(xyz, C), pos, click_idx=[ci], click_time_idx=[ct])
            if p > 0:
                assert sites.calls == 3 * N_SITES, sites.calls
            logits = [a["pred_masks"][0] for a in out["aux_outputs"]] + [out["pred_masks"][0]]
            masks = [m.clone() for m in recorded]
            if p == 0:           # the forward that is already pinned
                for l in range(3):
                    err = (logits[l].detach() - torch.from_numpy(c[f"logits{l}"]).double()).abs().max().item()
                    assert err <= 1e-5 * max(1.0, np.abs(c[f"logits{l}"]).max()), (in_name, l, err)
                for l in range(2):
                    assert np.array_equal(masks[l].numpy(), c[f"attn_mask{l}"]), (in_name, l)
            assert [k for k, _ in pre] == ["ffn", "mlp", "mlp"] * 3, [k for k, _ in pre]
            relu = []
            for l in range(3):
                ffn, mfg, mbg = (z for _, z in pre[3 * l:3 * l + 3])
                relu += [ffn, torch.cat([mfg, mbg], 0)]
            t = make_targets(c)
            w = seg.cal_click_loss_weights(torch.zeros(N, dtype=torch.long), xyz, [torch.from_numpy(t)], [ci])[0]
            samples.append(dict(c=c, ci=ci, pcd=pcd, logits=logits, masks=masks, relu=relu, N=N, Q=Q))
            preds.append(logits)
            targets.append(torch.from_numpy(t).long())
            weights.append(w)
    finally:
        F.dropout = orig_dropout
        ref.mask_module = orig_mask_module
        for h in hooks:
            h.remove()
    outputs = {"pred_masks": [lg[2] for lg in preds],
               "aux_outputs": [{"pred_masks": [lg[l] for lg in preds]} for l in range(2)]}
    losses = crit(outputs, targets, weights)
    total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
    total.backward()

    arrays = dict(input_cases=np.array(in_names), p=np.float64(p), seed=np.uint64(seed))
    for k, v in losses.items():
        arrays[f"loss::{k}"] = np.float64(v.item())
    arrays["loss::total"] = np.float64(total.item())
    for b, s in enumerate(samples):
        pre_ = f"s{b}::"
        c, N = s["c"], s["N"]
        arrays[pre_ + "targets"] = targets[b].numpy().astype(np.int8)
        arrays[pre_ + "weights"] = weights[b].numpy().astype(np.float32)
        rows = np.arange(0, N, LOGIT_ROW_STEP, dtype=np.int64)
        arrays[pre_ + "logit_rows"] = rows
        for l in range(3):
            lg = s["logits"][l].detach()
            arrays[pre_ + f"logits{l}"] = lg[torch.from_numpy(rows)].numpy()
            arrays[pre_ + f"logits{l}_colsum"] = lg.sum(0).numpy()
        for l in range(2):
            arrays[pre_ + f"attn_mask{l}"] = _packbits(s["masks"][l].numpy())
        near_idx, near_val = [], []
        for j, z in enumerate(s["relu"]):
            kind = ("ffn", "mlp")[j % 2]
            arrays[pre_ + f"relu_{kind}{j // 2}"] = _packbits((z > 0).numpy())
            r, col = torch.nonzero(z.abs() < RELU_NEAR, as_tuple=True)
            near_idx.append(np.stack([np.full(len(r), j), r.numpy(), col.numpy()], 1))
            near_val.append(z[r, col].numpy())
        arrays[pre_ + "relu_near_idx"] = np.concatenate(near_idx).astype(np.int32)
        arrays[pre_ + "relu_near_val"] = np.concatenate(near_val)
        g = s["pcd"].grad
        crow = np.unique(c["click_rows"]).astype(np.int64)
        drow = np.arange(0, N, D_PCD_ROW_STEP, dtype=np.int64)
        arrays[pre_ + "d_pcd_click_rows"] = crow
        arrays[pre_ + "d_pcd_clicks"] = g[torch.from_numpy(crow)].numpy()
        arrays[pre_ + "d_pcd_rows"] = drow
        arrays[pre_ + "d_pcd"] = g[torch.from_numpy(drow)].numpy()
        arrays[pre_ + "d_pcd_colsum"] = g.sum(0).numpy()
        arrays[pre_ + "d_pcd_sum"] = np.float64(g.sum().item())
        arrays[pre_ + "d_pcd_sumsq"] = np.float64((g * g).sum().item())
    n_grad = 0
    for k, v in params.items():
        if v.grad is None:
            assert k.startswith(("backbone.", "lin_squeeze_head.")), k
            continue
        g = v.grad.detach()
        arrays[f"grad_sum::{k}"] = np.float64(g.sum().item())
        arrays[f"grad_sumsq::{k}"] = np.float64((g * g).sum().item())
        if g.numel() > GRAD_FULL_MAX:
            cols = g.numel() // g.shape[0]
            n_rows = max(2, -(-GRAD_KEEP // cols))
            rows = np.linspace(0, g.shape[0] - 1, n_rows).round().astype(np.int64)
            arrays[f"grad_rows::{k}"] = rows
            g = g[torch.from_numpy(rows)]
        arrays[f"grad::{k}"] = g.numpy()
        n_grad += 1
    summary = {k[6:]: round(float(v), 5) for k, v in arrays.items() if k.startswith("loss::")}
    print(f"{name}: inputs {in_names}, p {p}, Q {[s['Q'] for s in samples]}, {n_grad} parameter gradients, "
          f"{sum(len(arrays[f's{b}::relu_near_idx']) for b in range(len(samples)))} ReLU inputs within {RELU_NEAR} of 0, "
          f"target histograms {[np.bincount(t.numpy()).tolist() for t in targets]}; losses {summary}")
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--check", action="store_true", help="regenerate and compare with the committed fixtures")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    torch.set_num_threads(1)            # one summation order: --check compares bit for bit
    z = np.load(os.path.join(HERE, "decoder_weights.npz"))
    decoder_weights = {k: z[k] for k in z.files}
    seg = load_by_path("ref_seg", os.path.join(REF, "utils", "seg.py"))
    for name in a.cases.split(","):
        arrays = run_fixture(name, decoder_weights, seg)
        path = os.path.join(a.out, f"decoder_train_{name}.npz")
        if a.check:
            old = np.load(path)
            assert sorted(old.files) == sorted(arrays), (name, set(old.files) ^ set(arrays))
            for k, v in arrays.items():
                o = old[k]
                assert o.shape == v.shape and o.dtype == v.dtype and np.array_equal(o, v), (name, k)
            print(f"{path}: reproduces bit for bit")
        else:
            with tempfile.NamedTemporaryFile(dir=a.out, suffix=".npz", delete=False) as f:
                np.savez_compressed(f, **arrays)
            os.replace(f.name, path)
            os.chmod(path, 0o644)
            size = os.path.getsize(path)
            print(f"{path}: {size / 1024:.0f} KiB")
            assert size < MAX_FILE_BYTES, (name, size)


if __name__ == "__main__":
    main()
