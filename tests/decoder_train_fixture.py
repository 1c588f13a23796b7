"""The decoder training fixtures (tests/golden/make_decoder_train_goldens.py): loading, the float64 oracle run that
follows a fixture, and the comparison of a run with a fixture.  Shared by test_oracle_decoder_train_goldens.py (the
oracle against the reference's own backward, CPU) and test_gpu_decoder_train_goldens.py (the HIP tape against it)."""
import functools
import os

import numpy as np
import torch

from dropout_ref import keep_mask
from oracle import criterion as ocrit
from oracle import decoder as od

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHT_DICT = {f"loss_{n}{s}": c for s in ("", "_0", "_1", "_2") for n, c in (("bce", 1.0), ("dice", 2.0))}
QUANTITIES = ("logits", "logit sums", "loss", "grad", "grad sums", "d_pcd", "d_pcd sums")


def names():
    return sorted(f[len("decoder_train_"):-4] for f in os.listdir(GOLDEN) if f.startswith("decoder_train_"))


def _npz(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def load(name):
    """The fixture's arrays plus ``samples``: per batch sample its forward case, clicks, targets, weights, attention masks
    of passes 1-2 (bool [Q, N]), ReLU decisions (6 float64 0/1 tensors: FFN hidden and mask MLP per pass) and the listed
    near-zero pre-activations {(tensor, row, col): value}."""
    f = _npz(os.path.join(GOLDEN, f"decoder_train_{name}.npz"))
    f["samples"] = []
    for b, case in enumerate(f["input_cases"].tolist()):
        c = _npz(os.path.join(GOLDEN, f"decoder_case_{case}.npz"))
        K = int(c["K"])
        ci = {str(o): [] for o in range(K + 1)}
        ct = {str(o): [] for o in range(K + 1)}
        for r, o, t in zip(c["click_rows"].tolist(), c["click_objs"].tolist(), c["click_times"].tolist()):
            ci[str(o)].append(int(r))
            ct[str(o)].append(int(t))
        N, Q = len(c["feats128"]), len(c["click_rows"]) + 10
        s = f"s{b}::"

        def bits(key, shape):
            return torch.from_numpy(np.unpackbits(f[s + key])[:int(np.prod(shape))].reshape(shape).astype(bool))
        relu = []
        for l in range(3):
            relu += [bits(f"relu_ffn{l}", (Q, 1024)).double(), bits(f"relu_mlp{l}", (Q, 128)).double()]
        near = {tuple(i): v for i, v in zip(f[s + "relu_near_idx"].tolist(), f[s + "relu_near_val"].tolist())}
        f["samples"].append(dict(case=c, ci=ci, ct=ct, N=N, Q=Q, n_fg=sum(len(ci[str(o)]) for o in range(1, K + 1)),
                                 targets=torch.from_numpy(f[s + "targets"].astype(np.int64)),
                                 weights=torch.from_numpy(f[s + "weights"]),
                                 attn_masks=[bits(f"attn_mask{l}", (Q, N)) for l in range(2)], relu=relu, near=near))
    return f


@functools.lru_cache(maxsize=256)
def _keep(seed, sample, code, p, shape):
    heads, rows, cols = shape if len(shape) == 3 else (1,) + shape
    return torch.from_numpy(keep_mask(seed, sample, code, p, heads, rows, cols)).reshape(shape).double()


def reference_dropout(seed, sample, p, site_of=lambda s: s):
    """``forward_mask``'s dropout hook as the fixture generator applies it: site s of pass d keeps the elements of
    dropout_ref.keep_mask(seed, sample, 8 d + s) and scales by 1 / (1 - p).  ``site_of`` remaps the sites (a negative
    control)."""
    def drop(d, s, x):
        return x * _keep(seed, sample, 8 * d + site_of(s), p, tuple(x.shape)) * (1.0 / (1.0 - p))
    return drop


def state_dict(decoder_weights):
    """float64 leaves of every decoder parameter (pos_enc.gauss_B stays float32 and constant: the reference computes the
    click encodings in float32)."""
    return {k: (v.clone() if k == "pos_enc.gauss_B" else v.double().clone().requires_grad_(True))
            for k, v in decoder_weights.items() if not k.startswith("lin_squeeze_head.")}


def oracle_run(f, decoder_weights, relu=None, samples=None, site_of=lambda s: s, detach_queries=False):
    """float64 autograd through oracle/decoder.py + oracle/criterion.py for the fixture ``f``, under the fixture's attention
    masks and with the ReLU decisions ``relu`` (per sample, the fixture's own when None).  ``samples``: the sample index
    of each batch sample in the dropout masks (default 0, 1, ...).  Returns the run in the form ``errors`` reads."""
    sd = state_dict(decoder_weights)
    p, seed = float(f["p"]), int(f["seed"])
    outs, pcds, seen = [], [], []
    for b, s in enumerate(f["samples"]):
        c = s["case"]
        seq = []
        for l in range(3):
            ffn, mlp = (relu[b] if relu is not None else s["relu"])[2 * l:2 * l + 2]
            seq += [ffn, mlp[:s["n_fg"]], mlp[s["n_fg"]:]]
        it = iter(seq)

        def relu_fn(z):
            m = next(it)
            seen.append(z.detach())
            return z * m
        pcd = torch.from_numpy(c["feats128"]).double().requires_grad_(True)
        drop = reference_dropout(seed, b if samples is None else samples[b], p, site_of) if p > 0 else None
        saved = od.RELU
        od.RELU = relu_fn
        try:
            o = od.forward_mask(sd, pcd, torch.from_numpy(c["xyz"]), torch.from_numpy(c["pos_enc"]).double(), s["ci"], s["ct"],
                                grad=True, force_masks=s["attn_masks"] + [None], dropout=drop,
                                query_features=pcd.detach() if detach_queries else None)
        finally:
            od.RELU = saved
        outs.append(o)
        pcds.append(pcd)
    outputs = {"pred_masks": [o[2] for o in outs], "aux_outputs": [{"pred_masks": [o[l] for o in outs]} for l in range(2)]}
    losses = ocrit.criterion(outputs, [s["targets"] for s in f["samples"]], [s["weights"].double() for s in f["samples"]])
    total = sum(losses[k] * WEIGHT_DICT[k] for k in losses)
    total.backward()
    losses = {k: v.item() for k, v in losses.items()}
    losses["total"] = total.item()
    return dict(logits=[[t.detach() for t in o] for o in outs], losses=losses, d_pcd=[p_.grad for p_ in pcds],
                grads={k: v.grad for k, v in sd.items() if v.requires_grad and v.grad is not None}, pre=seen)


def decisions(run, f):
    """The ReLU decisions of an oracle run (its own branch), per sample in the fixture's layout."""
    out, it = [], iter(run["pre"])
    for s in f["samples"]:
        d = []
        for l in range(3):
            ffn, mfg, mbg = next(it), next(it), next(it)
            d += [(ffn > 0).double(), (torch.cat([mfg, mbg], 0) > 0).double()]
        out.append(d)
    return out


def _norm_err(g, ref_sumsq, scale):
    """| ||g|| - ||ref|| | in units of sqrt(numel) x scale: at most the worst elementwise error in units of scale."""
    return abs(g.norm().item() - float(ref_sumsq) ** 0.5) / (g.numel() ** 0.5 * scale)


def errors(f, got, delta=None):
    """Worst relative error per quantity of the run ``got`` (float64 CPU tensors in oracle_run's form) against the fixture.
    ``delta``: a run-shaped correction added to the fixture's gradients and d_pcd (the kink correction: an oracle run
    with the decisions of the implementation under test minus one with the fixture's).  Denominators: logits
    max(1, max|ref|); loss values |ref|; gradients max(1e-3, max|ref|); d_pcd max|ref| over the stored rows; every
    sum by what the elementwise bound allows: numel x scale for a sum, sqrt(numel) x scale for the L2 norm (from the
    stored sum of squares).
    Returns {quantity: (worst, where)}."""
    worst = {q: (0.0, "") for q in QUANTITIES}

    def put(q, v, where):
        if not v <= worst[q][0]:           # NaN wins
            worst[q] = (v, where)

    def t(a):
        return torch.from_numpy(np.asarray(a)).double()
    for k, v in got["losses"].items():
        ref = float(f[f"loss::{k}"])
        put("loss", abs(v - ref) / abs(ref), k)
    for b, s in enumerate(f["samples"]):
        pre = f"s{b}::"
        rows = torch.from_numpy(f[pre + "logit_rows"])
        for l in range(3):
            lg, ref = got["logits"][b][l].double(), t(f[pre + f"logits{l}"])
            sc = max(1.0, ref.abs().max().item())
            put("logits", (lg[rows] - ref).abs().max().item() / sc, f"sample {b} pass {l}")
            put("logit sums", (lg.sum(0) - t(f[pre + f"logits{l}_colsum"])).abs().max().item() / (s["N"] * sc), f"sample {b} pass {l}")
        g = got["d_pcd"][b].double()
        dg = delta["d_pcd"][b] if delta is not None else torch.zeros_like(g)
        crow, drow = torch.from_numpy(f[pre + "d_pcd_click_rows"]), torch.from_numpy(f[pre + "d_pcd_rows"])
        rc, rd = t(f[pre + "d_pcd_clicks"]) + dg[crow], t(f[pre + "d_pcd"]) + dg[drow]
        sc = max(rc.abs().max().item(), rd.abs().max().item())
        put("d_pcd", (g[crow] - rc).abs().max().item() / sc, f"sample {b} click rows")
        put("d_pcd", (g[drow] - rd).abs().max().item() / sc, f"sample {b} rows")
        n = g.numel()
        put("d_pcd sums", (g.sum(0) - t(f[pre + "d_pcd_colsum"]) - dg.sum(0)).abs().max().item() / (s["N"] * sc), f"sample {b} columns")
        put("d_pcd sums", abs(g.sum().item() - float(f[pre + "d_pcd_sum"]) - dg.sum().item()) / (n * sc), f"sample {b} sum")
        if delta is None:           # (a corrected reference has no known sum of squares)
            put("d_pcd sums", _norm_err(g, f[pre + "d_pcd_sumsq"], sc), f"sample {b} norm")
    names_ = sorted(k[len("grad::"):] for k in f if k.startswith("grad::"))
    assert set(names_) == set(got["grads"]), set(names_) ^ set(got["grads"])
    for k in names_:
        g = got["grads"][k].double()
        dg = delta["grads"][k] if delta is not None else torch.zeros_like(g)
        ref = t(f[f"grad::{k}"])
        if f"grad_rows::{k}" in f:
            rows = torch.from_numpy(f[f"grad_rows::{k}"])
            gs, ref = g[rows], ref + dg[rows]
        else:
            gs, ref = g, ref + dg
        sc = max(1e-3, ref.abs().max().item())
        put("grad", (gs - ref).abs().max().item() / sc, k)
        n = g.numel()
        put("grad sums", abs(g.sum().item() - float(f[f"grad_sum::{k}"]) - dg.sum().item()) / (n * sc), k + " sum")
        if delta is None:
            put("grad sums", _norm_err(g, f[f"grad_sumsq::{k}"], sc), k + " norm")
    return worst


# the bars the HIP tape is held to at the most (those of test_gpu_backward.py::test_decoder_training_step_matches_autograd;
# test_gpu_decoder_train_goldens.py tightens some), in the units of ``errors``: a negative control must miss by 100x these
GPU_BARS = {"logits": 2e-4, "logit sums": 2e-4, "loss": 1e-5, "grad": 2e-3, "grad sums": 2e-3, "d_pcd": 2e-3,
            "d_pcd sums": 2e-3}


def report(tag, worst, bars=None):
    parts = []
    for q in QUANTITIES:
        v, where = worst[q]
        parts.append(f"{q} {v:.2e}" + (f" ({v / bars[q]:.1f}x bar)" if bars else "") + (f" [{where}]" if where else ""))
    print(f"{tag}: " + "; ".join(parts))
