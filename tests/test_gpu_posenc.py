"""-m gpu: the position encodings ``sine`` / ``legacy`` and ``normalize_pos_enc=False`` through the public model API
(``eng.decoder_inputs`` -> ``model.forward_mask``, as test_gpu_model.py's golden test), against fixtures produced by the
REFERENCE's own ``get_pos_encs`` + ``forward_mask`` (tests/golden/make_posenc_goldens.py).  Reads tests/golden only.

Bars.  Logits of all three levels <= 1e-3 (north_star's fp32 bound, test_gpu_model.TOL); the fixtures were written only
where the reference's own float32 / float64 gap is <= 2.5e-4 and the smallest top-1 / top-2 margin of levels 0 and 1 is
>= 1e-2, so no label -- hence no intermediate attention mask -- can flip inside the bound.  Encoding: <= 1e-4 for the
normalised configurations and ``legacy`` (the bar the Fourier encoding has in
test_forward_mask_matches_reference_goldens); for the two un-normalised configurations max(1e-4, 4 x pos_enc_fp64_gap)
with the gap read from the fixture -- the factor four covers a different summation order and a fused multiply-add
against torch's ``mm``, each worth about one rounding of the argument."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from agile3d_amd import SparseTensor, build_model, default_args
from agile3d_amd import lib as L
from agile3d_amd.clicks import query_list
from agile3d_amd.synthetic import make_clicks, make_scene
from conftest import GOLDEN, arrays_to_clicks, load_case

pytestmark = pytest.mark.gpu
TOL = 1e-3
CONFIGS = {
    "sine_norm": dict(positional_encoding_type="sine", normalize_pos_enc=True),
    "sine_raw": dict(positional_encoding_type="sine", normalize_pos_enc=False),
    "legacy": dict(positional_encoding_type="legacy", normalize_pos_enc=True),
    "fourier_raw": dict(positional_encoding_type="fourier", normalize_pos_enc=False),
}
ALL_CONFIGS = dict(CONFIGS, fourier_norm=dict(positional_encoding_type="fourier", normalize_pos_enc=True),
                   legacy_flag_off=dict(positional_encoding_type="legacy", normalize_pos_enc=False))
SCENES = ("q27", "q78")


def _model(config, decoder_weights, inv_freq=None, **more):
    """Our model for one configuration with the committed decoder weights (every non-pos_enc entry; gauss_B for Fourier),
    as make_posenc_goldens.py loads them into the reference."""
    args = default_args(**ALL_CONFIGS[config], **more)
    torch.manual_seed(0)
    m = build_model(args).eval()
    fourier = args.positional_encoding_type == "fourier"
    res = m.load_state_dict({k: v for k, v in decoder_weights.items() if fourier or not k.startswith("pos_enc.")}, strict=False)
    assert not res.unexpected_keys
    assert all(k.startswith(("backbone.", "lin_squeeze_head.", "pos_enc.")) for k in res.missing_keys)
    if inv_freq is not None:
        m.load_state_dict({"pos_enc.inv_freq": torch.from_numpy(inv_freq)}, strict=False)
    return m.cuda()


def _fixture(config, scene):
    z = np.load(os.path.join(GOLDEN, f"posenc_case_{config}_{scene}.npz"))
    return {k: z[k] for k in z.files}


def _run(model, c):
    ci, ct = arrays_to_clicks(c["click_rows"], c["click_objs"], c["click_times"], int(c["K"]))
    eng = model._get_engine()
    pcd, aux, coords, pos = eng.decoder_inputs(torch.from_numpy(c["feats128"]), torch.from_numpy(c["xyz"]))
    out = model.forward_mask(pcd, aux, coords, pos, click_idx=[ci], click_time_idx=[ct])
    got = [a["pred_masks"][0].cpu().numpy() for a in out["aux_outputs"]] + [out["pred_masks"][0].cpu().numpy()]
    return pos[4][0][0].cpu().numpy(), got, (ci, ct)


def _attn_mask(logits, clicks, n_bg_learned=10):
    """The attention mask the next decoder layer gets from a level's logits (mask_module, agile3d.py:362-384): the rows
    of an object's queries block every point not labelled with it; a row that would block everything blocks nothing."""
    lab = logits.argmax(1)
    _, _, counts, bg_rows, _ = query_list(*clicks)    # the decoder's query order: objects 1..K, then the background
    rows = []
    for o, c in list(enumerate(counts, start=1)) + [(0, len(bg_rows) + n_bg_learned)]:
        m = lab != o
        if m.all():
            m = np.zeros_like(m)
        rows += [m] * c
    return np.stack(rows)


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("config", list(CONFIGS))
def test_encoding_and_logits_match_the_reference_fixtures(config, scene, decoder_weights):
    c = _fixture(config, scene)
    assert float(c["logits_fp64_gap"]) <= 2.5e-4 and float(c["argmax_margin"]) >= 1e-2      # what the bars rest on
    nq = len(c["click_rows"]) + 10
    assert (nq <= 32) if scene == "q27" else (nq > 64)
    model = _model(config, decoder_weights, inv_freq=c.get("inv_freq"))
    enc, got, clicks = _run(model, c)
    raw = config in ("sine_raw", "fourier_raw")
    bar = max(1e-4, 4.0 * float(c["pos_enc_fp64_gap"])) if raw else 1e-4
    perr = np.abs(enc - c["pos_enc"]).max()
    print(f"{config} {scene}: pos_enc max|diff| = {perr:.3e} (bar {bar:.3e}, reference fp32/fp64 gap {float(c['pos_enc_fp64_gap']):.2e})")
    errs = [np.abs(got[i] - c[f"logits{i}"]).max() for i in range(3)]
    print(f"{config} {scene}: logits max|diff| = " + ", ".join(f"{e:.3e}" for e in errs) + f" (bar {TOL:.0e}, {nq} queries)")
    assert perr <= bar
    assert max(errs) <= TOL, errs
    for i in range(2):
        assert np.array_equal(_attn_mask(got[i], clicks), c[f"attn_mask{i}"]), i


def test_legacy_uses_the_loaded_inv_freq_buffer(decoder_weights):
    """legacy_q78 ran in the reference with inv_freq scaled by 1.5 before the state dict was loaded (the parametrised
    test above passes it with that buffer loaded); the same model with the default buffer must NOT match it -- a kernel
    that recomputed its own frequency table would."""
    c = _fixture("legacy", "q78")
    default = build_model(default_args(positional_encoding_type="legacy")).pos_enc.inv_freq.numpy()
    assert np.abs(c["inv_freq"] / default - 1.5).max() <= 1e-6
    model = _model("legacy", decoder_weights)
    enc, got, _ = _run(model, c)
    perr = np.abs(enc - c["pos_enc"]).max()
    lerr = max(np.abs(got[i] - c[f"logits{i}"]).max() for i in range(3))
    print(f"default inv_freq against the scaled-buffer fixture: pos_enc max|diff| = {perr:.3e}, logits {lerr:.3e}")
    assert perr > 0.1 and lerr > TOL
    # loading the buffer afterwards reaches the device (load_state_dict marks the engine stale)
    model.load_state_dict({"pos_enc.inv_freq": torch.from_numpy(c["inv_freq"])}, strict=False)
    enc, got, _ = _run(model, c)
    assert np.abs(enc - c["pos_enc"]).max() <= 1e-4
    assert max(np.abs(got[i] - c[f"logits{i}"]).max() for i in range(3)) <= TOL


def test_normalize_flag_changes_fourier_and_sine_but_not_legacy(decoder_weights):
    c = _fixture("fourier_raw", "q27")
    xyz = torch.from_numpy(c["xyz"]).cuda()
    enc = {}
    for config in ALL_CONFIGS:
        eng = _model(config, decoder_weights)._get_engine()
        eng.refresh_decoder_if_stale(check_versions=True)
        enc[config], mm = eng._posenc(xyz)
        assert (mm is None) == (config in ("sine_raw", "fourier_raw", "legacy", "legacy_flag_off"))
        if mm is not None:
            assert torch.equal(mm.cpu(), torch.cat([xyz.min(0)[0], xyz.max(0)[0]]).cpu())
    assert (enc["fourier_norm"] - enc["fourier_raw"]).abs().max().item() > 0.5
    assert (enc["sine_norm"] - enc["sine_raw"]).abs().max().item() > 0.5
    assert torch.equal(enc["legacy"], enc["legacy_flag_off"])


@pytest.mark.parametrize("config", list(ALL_CONFIGS))
def test_batched_encoding_equals_per_sample_calls(config, decoder_weights):
    """Mirror of test_batched_position_encoding_equals_per_sample_calls for every configuration: three samples of
    different extents (each normalised by ITS OWN min / max where the encoding normalises) -- the same bits; so are
    the sample-by-sample fall-backs of a gapped layout."""
    eng = _model(config, decoder_weights)._get_engine()
    eng.refresh_decoder_if_stale(check_versions=True)
    g = torch.Generator().manual_seed(78)
    sizes = [37, 5000, 1234]
    extents = [(8.0, 6.0, 2.6), (3.0, 2.0, 2.0), (12.0, 9.0, 3.5)]
    xyz = torch.cat([torch.rand(n, 3, generator=g) * torch.tensor(e) + 1.5 * i for i, (n, e) in enumerate(zip(sizes, extents))]).cuda()
    ranges, s = [], 0
    for n in sizes:
        ranges.append((s, s + n))
        s += n
    pes, mms = eng._posenc_batch(xyz, ranges)
    assert pes[0].data_ptr() + 4 * 128 * sizes[0] == pes[1].data_ptr()          # one matrix: the batched launch ran
    gap_pes, gap_mms = eng._posenc_batch(xyz, [ranges[0], ranges[2]])           # gapped: per-sample calls
    for i, (a, b) in enumerate(ranges):
        ref, rmm = eng._posenc(xyz[a:b])
        assert torch.equal(pes[i], ref), (config, i)
        assert (mms[i] is None and rmm is None) or torch.equal(mms[i], rmm)
        assert torch.isfinite(ref).all() and ref.abs().max().item() <= 1.0
    assert torch.equal(gap_pes[0], pes[0]) and torch.equal(gap_pes[1], pes[2])


def _call(lib, name, *args):
    L.check(getattr(lib, name)(*args), name)


def test_default_fourier_path_is_unchanged(decoder_weights):
    """fourier + normalize_pos_enc=True: the existing golden at its existing bars, through the two entry points the
    default model has always called; and a3d_posenc[_batch](FOURIER, 1) returns the same bits as them."""
    model = _model("fourier_norm", decoder_weights)
    c = load_case("n2048_k3_bg")
    enc, got, _ = _run(model, c)
    perr = np.abs(enc - c["pos_enc"]).max()
    worst = max(np.abs(got[i] - c[f"logits{i}"]).max() for i in range(3))
    print(f"default model, n2048_k3_bg: pos_enc max|diff| = {perr:.3e}, logits max|diff| = {worst:.3e}")
    assert perr <= 1e-4 and worst <= TOL
    lib = L.load()
    eng = model._get_engine()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator().manual_seed(5)
    sizes = [700, 3000, 41]
    xyz = torch.cat([torch.rand(n, 3, generator=g) * (2.0 + i) + i for i, n in enumerate(sizes)]).cuda()
    n = xyz.shape[0]
    starts = (C.c_int64 * 4)(0, 700, 3700, 3741)
    B = eng.decoder.gauss_B_ptr
    assert B == eng.decoder.posenc_table_ptr
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    tmp = torch.empty(max(256 * 6 * 4, lib.a3d_posenc_batch_workspace_bytes(3)), dtype=torch.uint8, device="cuda")
    o_old, o_new, m_old, m_new = new(n, 128), new(n, 128), new(6), new(6)
    _call(lib, "a3d_posenc_fourier", p(xyz), n, B, p(m_old), p(o_old), p(tmp), tmp.numel(), st)
    _call(lib, "a3d_posenc", 0, 1, p(xyz), n, B, p(m_new), p(o_new), p(tmp), tmp.numel(), st)
    assert torch.equal(o_old, o_new) and torch.equal(m_old, m_new)
    b_old, b_new, bm_old, bm_new = new(n, 128), new(n, 128), new(3, 6), new(3, 6)
    _call(lib, "a3d_posenc_fourier_batch", p(xyz), starts, 3, B, p(bm_old), p(b_old), p(tmp), tmp.numel(), st)
    _call(lib, "a3d_posenc_batch", 0, 1, p(xyz), starts, 3, B, p(bm_new), p(b_new), p(tmp), tmp.numel(), st)
    assert torch.equal(b_old, b_new) and torch.equal(bm_old, bm_new)
    assert not torch.equal(b_old, o_old)                                       # per-sample ranges really differ


@pytest.mark.parametrize("config", ["fourier_norm", "sine_norm"])
def test_one_sample_reduction_past_its_block_cap(config, decoder_weights):
    """A one-sample call reduces over min(ceil(n / 256), 256) blocks: at n = 65 836 the 256 x 256 threads cover 65 536
    rows and some take a second sweep.  Every extreme of the sample lies in a row only that sweep reads (the first row
    past the cap, the last row and two in between), so a reduction that stopped at the cap would miss all six.  Its
    min / max is exact, and its rows carry the same bits as the same points as sample 0 of a batched call (16 blocks per
    sample) and as a3d_posenc_batch called with that one sample."""
    eng = _model(config, decoder_weights)._get_engine()
    eng.refresh_decoder_if_stale(check_versions=True)
    n, n1, cap = 65836, 300, 256 * 256
    g = torch.Generator().manual_seed(65836)
    xyz = torch.rand(n + n1, 3, generator=g) * torch.tensor((9.0, 7.0, 3.0)) - 2.0          # x in [-2, 7), y [-2, 5), z [-2, 1)
    xyz[cap] = torch.tensor((-2.5, 0.0, 1.25))         # min x, max z
    xyz[cap + 131] = torch.tensor((7.5, -2.75, 0.0))   # max x, min y
    xyz[n - 2] = torch.tensor((0.0, 5.5, 0.0))         # max y
    xyz[n - 1] = torch.tensor((0.0, 0.0, -3.0))        # min z
    xyz = xyz.cuda()
    one = xyz[:n]
    below = torch.cat([one[:cap].min(0)[0], one[:cap].max(0)[0]])
    assert (below != torch.cat([one.min(0)[0], one.max(0)[0]])).all()       # all six extremes lie past the block cap
    pe, mm = eng._posenc(one)
    assert torch.equal(mm, torch.cat([one.min(0)[0], one.max(0)[0]]))
    pes, mms = eng._posenc_batch(xyz, [(0, n), (n, n + n1)])
    assert pes[0].data_ptr() + 4 * 128 * n == pes[1].data_ptr()                 # one matrix: the batched launch ran
    assert torch.equal(pes[0], pe) and torch.equal(mms[0], mm)
    lib = L.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    kind, table = L.POSENC_KINDS[ALL_CONFIGS[config]["positional_encoding_type"]], eng.decoder.posenc_table_ptr
    out = torch.empty((n, 128), dtype=torch.float32, device="cuda")
    bmm = torch.empty((1, 6), dtype=torch.float32, device="cuda")
    tmp = torch.empty(lib.a3d_posenc_batch_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    _call(lib, "a3d_posenc_batch", kind, 1, p(one), (C.c_int64 * 2)(0, n), 1, table, p(bmm), p(out), p(tmp), tmp.numel(),
          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert torch.equal(out, pe) and torch.equal(bmm[0], mm)
    assert torch.isfinite(pe).all() and pe.abs().max().item() <= 1.0


def test_entry_points_refuse_bad_arguments():
    lib = L.load()
    xyz = torch.rand(64, 3, device="cuda")
    out = torch.empty((64, 128), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.a3d_posenc(7, 1, p(xyz), 64, None, None, p(out), None, 0, st) != 0            # unknown kind
    assert lib.a3d_posenc(2, 0, p(xyz), 64, None, None, p(out), None, 0, st) != 0            # legacy without inv_freq
    assert lib.a3d_posenc(1, 1, p(xyz), 64, None, None, p(out), None, 0, st) != 0            # normalising without min / max
    assert lib.a3d_posenc(1, 0, p(xyz), 64, None, None, C.c_void_p(out.data_ptr() + 4), None, 0, st) != 0     # misaligned rows
    assert lib.a3d_posenc(1, 0, p(xyz), 64, None, None, p(out), None, 0, st) == 0            # raw sine needs neither
    torch.cuda.synchronize()


def _scene_inputs(n, seed):
    sc = make_scene(n, seed=seed)
    x = SparseTensor(features=torch.from_numpy(sc["feats"]), coordinates=torch.from_numpy(sc["coords"]), device="cuda")
    ci, ct = make_clicks(sc["labels"], n_objects=3, clicks_per_object=2, n_bg_clicks=1, seed=seed)
    return sc, x, torch.from_numpy(sc["raw_xyz"]).cuda(), ci, ct


@pytest.mark.parametrize("config", ["sine_norm", "sine_raw", "legacy", "fourier_raw"])
def test_end_to_end_backbone_to_mask(config, decoder_weights):
    """forward_backbone on a synthetic scene -> forward_mask, against decoder_inputs fed with the backbone's own
    features: both paths (batched launch inside forward_backbone, single launch inside decoder_inputs) serve the
    model's encoding."""
    model = _model(config, decoder_weights)
    sc, x, raw, ci, ct = _scene_inputs(3000, 4)
    pcd, aux, coords, pos = model.forward_backbone(x, raw_coordinates=raw)
    a = model.forward_mask(pcd, aux, coords, pos, click_idx=[ci], click_time_idx=[ct])
    eng = model._get_engine()
    pcd2, aux2, coords2, pos2 = eng.decoder_inputs(pcd.F, raw)
    assert torch.equal(pos[4][0][0], pos2[4][0][0])
    b = model.forward_mask(pcd2, aux2, coords2, pos2, click_idx=[ci], click_time_idx=[ct])
    la = [o["pred_masks"][0] for o in a["aux_outputs"]] + [a["pred_masks"][0]]
    lb = [o["pred_masks"][0] for o in b["aux_outputs"]] + [b["pred_masks"][0]]
    err = max((u - v).abs().max().item() for u, v in zip(la, lb))
    print(f"{config}: forward_backbone -> forward_mask against decoder_inputs: max|diff| = {err:.3e}")
    assert err <= 1e-4
    assert torch.isfinite(la[-1]).all() and la[-1].shape == (len(sc["coords"]), 4)


def test_training_mode_with_the_sine_encoding(decoder_weights):
    """model.train(): forward_backbone / forward_mask / criterion / backward with a sine model.  The encodings carry no
    gradient and the training tape takes them as inputs; at dropout 0 its logits agree with the eval-mode kernels'
    within 1e-4 (the bar test_gpu_model.py uses between two of its own paths) and every parameter gets a finite gradient."""
    from agile3d_amd.clicks import cal_click_loss_weights
    from agile3d_amd.criterion import build_mask_criterion
    model = _model("sine_norm", decoder_weights, bce_loss_coef=1.0, dice_loss_coef=2.0, losses=["bce", "dice"])
    crit = build_mask_criterion(model.args)
    sc, x, raw, ci, ct = _scene_inputs(3000, 6)
    labels = torch.from_numpy(sc["labels"].astype(np.int64)).cuda()
    target = torch.zeros(len(labels), device="cuda")
    for o in range(1, 4):
        target[labels == labels[ci[str(o)][0]]] = o
    model.train()
    crit.train()
    r = model.forward_backbone(x, raw_coordinates=raw)
    out = model.forward_mask(*r, click_idx=[ci], click_time_idx=[ct])
    train_logits = [o["pred_masks"][0].detach().clone() for o in out["aux_outputs"]] + [out["pred_masks"][0].detach().clone()]
    weights = cal_click_loss_weights(x.C[:, 0], raw, target, [ci])
    loss_dict = crit(out, [target], weights)
    loss = sum(loss_dict[k] * crit.weight_dict[k] for k in loss_dict if k in crit.weight_dict)
    assert np.isfinite(float(loss.detach()))
    loss.backward()
    missing = [k for k, p_ in model.named_parameters() if p_.grad is None or not torch.isfinite(p_.grad).all()]
    assert not missing, missing
    assert any(p_.grad.abs().max().item() > 0 for p_ in model.parameters())
    model.eval()
    with torch.no_grad():
        ev = model.forward_mask(*r, click_idx=[ci], click_time_idx=[ct])
    eval_logits = [o["pred_masks"][0] for o in ev["aux_outputs"]] + [ev["pred_masks"][0]]
    err = max((u - v).abs().max().item() for u, v in zip(train_logits, eval_logits))
    print(f"sine, training-mode against eval-mode logits on the same features: max|diff| = {err:.3e}")
    assert err <= 1e-4
