"""Decoder dropout on the GPU: the in-kernel masks against the numpy restatement of their RNG, every
dropout primitive against float64 autograd with those masks, the whole decoder tape at p = 0.1 against the reference
layers with the same masks, the p = 0 / eval invariance, and repeatable training runs."""
import random

import numpy as np
import pytest
import torch

from agile3d_amd import decoder_ops as ops
from agile3d_amd import lib as L
from agile3d_amd.synthetic import make_scene
from attn_kit import DEV, check as _check, mha_ref as _mha_ref, zmat
from dropout_ref import keep_mask

pytestmark = pytest.mark.gpu


def gpu_mask(seed, sample, site, p, heads, rows, cols):
    return ops.dropout_mask(seed, sample, site, p, heads, rows, cols)


# ---------------------------------------------------------------------------------------------------- 1. the masks
@pytest.mark.parametrize("seed,sample,site,p,shape", [(0, 0, 0, 0.1, (8, 37, 5003)), (2 ** 64 - 1, 3, 23, 0.5, (1, 1, 1)),
                                                      (0x1234_5678_9abc_def0, 1, 14, 0.3, (8, 130, 17)),
                                                      (99, 2, 7, 0.9, (1, 1031, 130))])
def test_mask_matches_the_numpy_restatement(seed, sample, site, p, shape):
    got = gpu_mask(seed, sample, site, p, *shape).cpu().numpy()
    assert np.array_equal(got, keep_mask(seed, sample, site, p, *shape))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_statistics(p):
    n = 8 * 400 * 400
    a = gpu_mask(7, 0, 0, p, 8, 400, 400).double()
    b = gpu_mask(7, 0, 1, p, 8, 400, 400).double()          # another site
    c = gpu_mask(8, 0, 0, p, 8, 400, 400).double()          # another seed
    sd = (p * (1 - p) / n) ** 0.5
    assert abs(a.mean().item() - (1 - p)) <= 6 * sd
    agree = (1 - p) ** 2 + p ** 2
    sd2 = (agree * (1 - agree) / n) ** 0.5
    for other in (b, c):
        assert abs((a == other).double().mean().item() - agree) <= 6 * sd2


# ---------------------------------------------------------------------------------------------------- 2. primitives
def _inputs(Lq, Lk, masked, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, 128, generator=g) for n in (Lq, Lk, Lk))
    w = torch.randn(Lq, 128, generator=g)
    mask = None
    if masked:
        mask = (torch.rand(Lq, Lk, generator=g) < 0.6)
        mask[:, 5] = False
        mask = mask.to(torch.uint8)
    return q, k, v, w, mask


def _flash_c2s(q, k, v, w, mask, drop):
    qs, kd, vd, wd = (q * 0.25).to(DEV), k.to(DEV), v.to(DEV), w.to(DEV)
    md = mask.to(DEV).contiguous() if mask is not None else None
    o, stats = ops.flash_c2s_forward(qs, kd, vd, md, drop=drop)
    dq, dk, dv = ops.flash_c2s_backward(qs, kd, vd, md, o, stats, wd, drop=drop)
    return o, dq * 0.25, dk, dv


@pytest.mark.parametrize("Lq,Lk,masked", [(37, 5003, True), (20, 3000, False), (130, 1700, True)])
def test_flash_c2s_dropout_vs_float64_autograd(Lq, Lk, masked):
    p, seed, sample, site = 0.1, 0xdead_beef_0123, 1, 8
    q, k, v, w, mask = _inputs(Lq, Lk, masked, Lq * 7 + Lk)
    Z = zmat(seed, sample, site, p, 8, Lq, Lk)
    want = _mha_ref(q, k, v, w, mask, Z)
    got = _flash_c2s(q, k, v, w, mask, L.Dropout(seed, p, sample, site, 0))
    _check(f"flash c2s dropout {Lq}x{Lk}", got, want)


@pytest.mark.parametrize("Lq,Lk", [(5003, 37), (1700, 130)])
def test_flash_s2c_dropout_vs_float64_autograd(Lq, Lk):
    p, seed, sample, site = 0.1, 77, 2, 6
    q, k, v, w, _ = _inputs(Lq, Lk, False, Lq * 3 + Lk)
    Z = zmat(seed, sample, site, p, 8, Lq, Lk)
    want = _mha_ref(q, k, v, w, None, Z)
    drop = L.Dropout(seed, p, sample, site, 0)
    qd, ks, vd, wd = q.to(DEV), (k * 0.25).to(DEV), v.to(DEV), w.to(DEV)
    o, stats = ops.flash_s2c_forward(qd, ks, vd, drop=drop)
    dq, dk, dv = ops.flash_s2c_backward(qd, ks, vd, o, stats, wd, drop=drop)
    _check(f"flash s2c dropout {Lq}x{Lk}", (o, dq, dk * 0.25, dv), want)


def _dense(q, k, v, w, mask, drop):
    qd, kd, vd, wd = q.to(DEV), k.to(DEV), v.to(DEV), w.to(DEV)
    md = mask.to(DEV).contiguous() if mask is not None else None
    o, saved = ops.dense_forward(qd, kd, vd, md, drop=drop)
    dq, dk, dv = ops.dense_backward(qd, kd, vd, md, o, saved, wd, drop=drop)
    return o, dq, dk, dv, saved[1]


@pytest.mark.parametrize("Lq,Lk,masked", [(37, 700, True), (16, 16, False), (1500, 20, False)])
def test_dense_dropout_vs_float64_autograd(Lq, Lk, masked):
    p, seed, sample, site = 0.1, 5, 0, 2
    q, k, v, w, mask = _inputs(Lq, Lk, masked, Lq + Lk)
    Z = zmat(seed, sample, site, p, 8, Lq, Lk)
    want = _mha_ref(q, k, v, w, mask, Z)
    *got, transposed = _dense(q, k, v, w, mask, L.Dropout(seed, p, sample, site, 0))
    assert transposed == (Lq == 1500)                        # both layouts of the materialised path are covered
    _check(f"dense dropout {Lq}x{Lk}", got, want)


def test_flash_and_dense_dropout_agree():
    p, seed, sample, site = 0.1, 31, 1, 16
    q, k, v, w, mask = _inputs(20, 3000, True, 4)
    drop = L.Dropout(seed, p, sample, site, 0)
    fl = _flash_c2s(q, k, v, w, mask, drop)
    de = _dense(q, k, v, w, mask, drop)[:4]
    for name, a, b in zip(("o", "dq", "dk", "dv"), fl, de):
        rel = (a - b).abs().max().item() / b.abs().max().item()
        assert rel <= 1e-5, (name, rel)


def test_linear_residual_dropout_vs_float64():
    """y = res + dropout(x W^T + b) as the tape composes it (GEMM, then the residual-dropout pass) and its backward (mask
    on dy before both gradient GEMMs, dy itself to the residual)."""
    from agile3d_amd.train_decoder import DecoderTape
    from agile3d_amd import build_model, default_args
    torch.manual_seed(3)
    model = build_model(default_args(dropout=0.1)).cuda().train()
    g = torch.Generator().manual_seed(4)
    n = 301
    x = torch.randn(n, 128, generator=g)
    r = torch.randn(n, 128, generator=g)
    dyv = torch.randn(n, 128, generator=g)
    tape = DecoderTape.__new__(DecoderTape)
    tape.model, tape.P, tape.steps, tape.grads, tape._grad_written = model, dict(model.named_parameters()), [], {}, set()
    tape.p, tape.seed, tape.sample_base, tape._pass = 0.1, 1234, 1, 2
    from agile3d_amd.train_decoder import _T
    xt, rt = _T(x.cuda()), _T(r.cuda())
    wname, bname = "c2c_attention.2.0.self_attn.out_proj.weight", "c2c_attention.2.0.self_attn.out_proj.bias"
    W, b = tape.P[wname].detach().cpu().double(), tape.P[bname].detach().cpu().double()
    y = tape.lin(xt, wname, bname, res=rt, drop=(5, [(0, n)]))
    y.g = dyv.cuda()
    for s in reversed(tape.steps):
        s()
    Z = zmat(1234, 1, 8 * 2 + 5, 0.1, 1, n, 128)[0]
    xr, Wr, br, rr = (t.clone().requires_grad_(True) for t in (x.double(), W, b, r.double()))
    yr = rr + (xr @ Wr.T + br) * Z
    (yr * dyv.double()).sum().backward()
    _check("linear + residual dropout", (y.v, xt.g, rt.g, tape.grads[wname], tape.grads[bname]),
           (yr, xr.grad, rr.grad, Wr.grad, br.grad), names=("y", "dx", "dres", "dW", "db"))


def test_relu_dropout_vs_float64():
    g = torch.Generator().manual_seed(9)
    n = 77
    x, dy = torch.randn(n, 1024, generator=g), torch.randn(n, 1024, generator=g)
    drop = L.Dropout(555, 0.1, 3, 12, 0)
    xd, dyd = x.to(DEV), dy.to(DEV)
    y = ops.dropout_rows_forward(xd, None, True, drop)
    dx = ops.dropout_rows_backward(dyd, xd, drop)
    Z = zmat(555, 3, 12, 0.1, 1, n, 1024)[0]
    xr = x.double().requires_grad_(True)
    yr = torch.relu(xr) * Z
    (yr * dy.double()).sum().backward()
    _check("relu + dropout", (y, dx), (yr, xr.grad), tol=1e-6, names=("y", "dx"))


# ---------------------------------------------------------------------------------------------------- 3. whole tape
def _decoder_case(model):
    from oracle import decoder as od
    g = torch.Generator().manual_seed(12)
    N = 1500
    pcd = torch.randn(N, 128, generator=g) * 0.7
    xyz = torch.rand(N, 3, generator=g) * 4.0
    sd = {k: v.detach().cpu().double().clone() for k, v in model.state_dict().items() if v.is_floating_point()}
    pos = od.fourier_pos_enc(xyz.double(), sd["pos_enc.gauss_B"], xyz.double().min(0)[0], xyz.double().max(0)[0])
    ci = {"0": [7], "1": [10, 400], "2": [33], "3": [900, 1200, 77]}
    ct = {"0": [6], "1": [0, 3], "2": [1], "3": [2, 4, 5]}
    R = [torch.randn(N, 4, generator=g) / 8 for _ in range(3)]
    return pcd, xyz, sd, pos, ci, ct, R


def test_decoder_tape_with_dropout_matches_autograd():
    """The three decoder passes at p = 0.1 against float64 autograd through oracle/decoder.py with its dropout hook at
    attention_block.py's sites (pinned on the reference's own modules by tests/golden/make_decoder_train_goldens.py), the
    masks taken from a3d_dropout_mask (and the ReLU and attention masks from the tape, as in
    test_decoder_training_step_matches_autograd)."""
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_decoder import DecoderTape
    from oracle import decoder as od
    p, seed = 0.1, 0x0123_4567_89ab_cdef
    torch.manual_seed(11)
    model = build_model(default_args(dropout=p)).cuda().train()
    pcd, xyz, sd, pos, ci, ct, R = _decoder_case(model)
    tape = DecoderTape(model, pcd.cuda(), pos.float().cuda(), ci, ct, dropout=p, seed=seed)
    state = {"d": -1}

    def dropout(d, s, x):
        state["d"] = max(state["d"], d)
        heads, rows, cols = x.shape if x.dim() == 3 else (1,) + tuple(x.shape)
        return x * zmat(seed, 0, 8 * d + s, p, heads, rows, cols).reshape(x.shape)

    n_fg = 6
    relu_seq = []
    for l in range(3):
        ffn_m, mlp = tape.relu_masks[2 * l].cpu().double(), tape.relu_masks[2 * l + 1].cpu().double()
        relu_seq += [ffn_m, mlp[:n_fg], mlp[n_fg:]]
    it = iter(relu_seq)
    for k in sd:
        if not k.startswith(("backbone.", "pos_enc.")):
            sd[k].requires_grad_()
    pcd_o = pcd.double().requires_grad_()
    od.RELU = lambda z: z * next(it)
    try:
        outs = od.forward_mask(sd, pcd_o, xyz.double(), pos, ci, ct, grad=True,
                               force_masks=[m.cpu().bool() for m in tape.attn_masks], dropout=dropout)
    finally:
        od.RELU = torch.relu
    assert state["d"] == 2
    for l in range(3):
        err = (tape.logits[l].cpu().double() - outs[l].detach()).abs().max().item()
        assert err <= 2e-4 * max(1.0, outs[l].abs().max().item()), (l, err)
    sum((o * r.double()).sum() for o, r in zip(outs, R)).backward()
    grads, d_pcd = tape.backward([r.cuda() for r in R])
    names = [k for k in sd if sd[k].requires_grad and sd[k].grad is not None]
    assert set(grads) == set(names), set(names) ^ set(grads)
    worst = ("", 0.0)
    for k in names:
        ref, got = sd[k].grad, grads[k].cpu().double()
        rel = (got - ref).abs().max().item() / max(1e-3, ref.abs().max().item())
        worst = max(worst, (k, rel), key=lambda t: t[1])
    rel_pcd = (d_pcd.cpu().double() - pcd_o.grad).abs().max().item() / pcd_o.grad.abs().max().item()
    print(f"decoder tape p = {p}: worst relative gradient error {worst[1]:.2e} ({worst[0]}), d_pcd {rel_pcd:.2e}")
    assert worst[1] <= 2e-3 and rel_pcd <= 2e-3, (worst, rel_pcd)


# ---------------------------------------------------------------------------------------------------- 4. invariance
def test_tape_with_zero_dropout_is_the_tape_without_it():
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_decoder import DecoderTape
    torch.manual_seed(11)
    model = build_model(default_args()).cuda().train()
    pcd, xyz, sd, pos, ci, ct, R = _decoder_case(model)
    rng = torch.get_rng_state()
    a = DecoderTape(model, pcd.cuda(), pos.float().cuda(), ci, ct)
    b = DecoderTape(model, pcd.cuda(), pos.float().cuda(), ci, ct, dropout=0.0, seed=5, sample_base=3)
    assert torch.equal(rng, torch.get_rng_state())          # p = 0 draws nothing
    for l in range(3):
        assert torch.equal(a.logits[l], b.logits[l])
    ga, da = a.backward([r.cuda() for r in R])
    gb, db = b.backward([r.cuda() for r in R])
    assert torch.equal(da, db) and set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_dropout_changes_the_training_forward_only():
    from agile3d_amd import SparseTensor, build_model, default_args
    from agile3d_amd.synthetic import make_clicks
    torch.manual_seed(0)
    m0 = build_model(default_args()).cuda()
    m1 = build_model(default_args(dropout=0.1)).cuda()
    m1.load_state_dict(m0.state_dict())
    sc = make_scene(3000, seed=1)
    ci, ct = make_clicks(sc["labels"], n_objects=3, clicks_per_object=2, n_bg_clicks=1, seed=1)
    outs = {}
    for name, m in (("p0", m0), ("p1", m1)):
        for mode in ("eval", "train"):
            m.train(mode == "train")
            x = SparseTensor(features=torch.from_numpy(sc["feats"]), coordinates=torch.from_numpy(sc["coords"]), device=DEV)
            with torch.no_grad():
                r = m.forward_backbone(x, raw_coordinates=torch.from_numpy(sc["raw_xyz"]).to(DEV))
                torch.manual_seed(3)
                outs[name, mode] = m.forward_mask(*r, click_idx=[ci], click_time_idx=[ct])["pred_masks"][0].clone()
    assert torch.equal(outs["p0", "eval"], outs["p1", "eval"])
    assert not torch.equal(outs["p0", "train"], outs["p1", "train"])


def test_batched_dropout_tape_equals_one_tape_per_sample():
    from agile3d_amd import build_model, default_args
    from agile3d_amd.train_decoder import DecoderTape
    from oracle import decoder as od
    torch.manual_seed(21)
    model = build_model(default_args(dropout=0.1)).cuda().train()
    g = torch.Generator().manual_seed(22)
    sizes = [1700, 2300]
    cis = [{"0": [7], "1": [10, 400], "2": [33], "3": [900, 1200, 77]}, {"0": [3, 4], "1": [600]}]
    cts = [{"0": [6], "1": [0, 3], "2": [1], "3": [2, 4, 5]}, {"0": [1, 2], "1": [0]}]
    pcds, poss, Rs = [], [], []
    for n, ci in zip(sizes, cis):
        xyz = (torch.rand(n, 3, generator=g) * 4.0).double()
        B_ = model.state_dict()["pos_enc.gauss_B"].detach().cpu().double()
        poss.append(od.fourier_pos_enc(xyz, B_, xyz.min(0)[0], xyz.max(0)[0]).float().cuda())
        pcds.append((torch.randn(n, 128, generator=g) * 0.7).cuda())
        Rs.append([(torch.randn(n, len(ci), generator=g) / 8).cuda() for _ in range(3)])
    seed = 4242
    batched = DecoderTape(model, pcds, poss, cis, cts, dropout=0.1, seed=seed)
    singles = [DecoderTape(model, pp, q, ci, ct, dropout=0.1, seed=seed, sample_base=b)
               for b, (pp, q, ci, ct) in enumerate(zip(pcds, poss, cis, cts))]
    for l in range(3):
        for b, t in enumerate(singles):
            assert torch.equal(batched.logits[l][b], t.logits[l]), (l, b)
    gb, dpb = batched.backward([[Rs[b][l] for b in range(2)] for l in range(3)])
    gs, dps = {}, []
    for b, t in enumerate(singles):
        g_, dp = t.backward(Rs[b])
        dps.append(dp)
        for k, v in g_.items():
            gs[k] = v if k not in gs else gs[k] + v
    worst = max((gb[k] - gs[k]).abs().max().item() / max(1e-3, gs[k].abs().max().item()) for k in gs)
    rel_p = (dpb - torch.cat(dps)).abs().max().item() / torch.cat(dps).abs().max().item()
    assert worst <= 2e-5 and rel_p <= 2e-5, (worst, rel_p)


def test_dense_path_with_dropout_matches_flash():
    import agile3d_amd.train_decoder as TD
    from agile3d_amd import build_model, default_args
    torch.manual_seed(11)
    model = build_model(default_args(dropout=0.1)).cuda().train()
    pcd, xyz, sd, pos, ci, ct, R = _decoder_case(model)
    res = {}
    for flash in (True, False):
        TD.FLASH = flash
        try:
            t = TD.DecoderTape(model, pcd.cuda(), pos.float().cuda(), ci, ct, dropout=0.1, seed=99)
            res[flash] = (t.logits, t.backward([r.cuda() for r in R]))
        finally:
            TD.FLASH = True
    for l in range(3):
        a, b = res[True][0][l], res[False][0][l]
        assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item()), l
    ga, gb = res[True][1][0], res[False][1][0]
    worst = max((ga[k] - gb[k]).abs().max().item() / max(1e-3, gb[k].abs().max().item()) for k in gb)
    assert worst <= 1e-3, worst


# ---------------------------------------------------------------------------------------------------- 5. end to end
def _batch():
    from agile3d_amd import batched_coordinates
    scenes = [make_scene(3000, seed=30), make_scene(2500, seed=31)]
    return (batched_coordinates([s["coords"][:, 1:] for s in scenes]),
            torch.from_numpy(np.concatenate([s["raw_xyz"] for s in scenes])),
            torch.from_numpy(np.concatenate([s["feats"] for s in scenes])),
            [torch.from_numpy(s["labels"].astype(np.int64)) for s in scenes], None, None, [{}, {}],
            ("scene0030_00", "scene0031_00"), (0, 0))


def _three_steps(p, seed, batch):
    from agile3d_amd import build_model, default_args
    from agile3d_amd.criterion import build_mask_criterion
    from agile3d_amd.optim import AdamW
    from agile3d_amd.train_step import train_one_step
    args = default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"], dropout=p)
    torch.manual_seed(21)
    model = build_model(args).cuda()
    crit = build_mask_criterion(args)
    opt = AdamW(model.named_parameters(), lr=1e-4, weight_decay=1e-4)
    np.random.seed(seed), torch.manual_seed(seed), random.seed(seed)
    for _ in range(3):
        st = train_one_step(model, crit, opt, batch, DEV, 0.1)
        assert np.isfinite(st["loss"])
    return {k: v.detach().clone() for k, v in model.named_parameters()}


def test_training_with_dropout_is_repeatable():
    batch = _batch()
    a = _three_steps(0.1, 5, batch)
    b = _three_steps(0.1, 5, batch)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = _three_steps(0.1, 6, batch)
    d = _three_steps(0.0, 5, batch)
    dec = [k for k in a if k.startswith(("c2s_", "c2c_", "ffn_", "s2c_"))]
    assert any(not torch.equal(a[k], c[k]) for k in dec)
    assert any(not torch.equal(a[k], d[k]) for k in dec)


def test_reference_training_sequence_with_dropout():
    from agile3d_amd import build_model, default_args
    from agile3d_amd.criterion import build_mask_criterion
    from agile3d_amd.train_step import train_one_step_api
    args = default_args(bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"], dropout=0.1)
    torch.manual_seed(5)
    model = build_model(args).cuda()
    crit = build_mask_criterion(args)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    np.random.seed(7), torch.manual_seed(7), random.seed(7)
    st = train_one_step_api(model, crit, opt, _batch(), DEV, max_norm=0.1)
    assert np.isfinite(st["loss"]) and st["grad_norm"] > 0


def test_fit_with_dropout_lowers_the_loss():
    from agile3d_amd import build_model, default_args
    from agile3d_amd.fit import fit, labelled_scenes
    torch.manual_seed(0)
    model = build_model(default_args(dropout=0.1)).cuda()
    losses = fit(model, labelled_scenes(2, voxels=3000), DEV, iters=40, lr=1e-3)
    print("fit with dropout: losses", [round(x, 3) for x in losses[:3]], "...", [round(x, 3) for x in losses[-3:]])
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses
