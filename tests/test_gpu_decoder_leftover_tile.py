"""The decoder at 17 .. 32 queries: a scene with 17 .. 20 queries runs its second query tile (queries 16 .. 19) on the
4x4x1 build of k_kv_c2s and, while the queries' keys stay in LDS (up to 8 objects at 19 and 20 queries), of k_s2c_out; the
last layer stores only its logits.  By the planner (test_decoder_plan_classes.py) the 17- and 18-query cases and the batch
below run both leftover builds; the 20-query case with its ten objects runs k_kv_c2s<2, LO> next to k_s2c_out<2, 12, KG>,
the two-tile build with the keys in global memory.  forward_mask's pred_masks and every
aux output against (a) the unfused live path (A3D_FUSED_C2S=0 A3D_FUSED_S2C=0, read once per process -> a second
interpreter) at the tolerance of test_one_pass_scene_to_click_half_matches_the_two_kernel_path, and (b) the CPU oracle at
the 1e-3 bar of test_gpu_model.py.  16 and 33 queries are the neighbours on either side (one tile; the wide tier)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from agile3d_amd import SparseTensor, build_model, default_args, randomize_bn_stats
from agile3d_amd.synthetic import make_clicks, make_scene
from oracle import backbone as ob, decoder as od

pytestmark = pytest.mark.gpu

TOL = 1e-3          # test_gpu_model.TOL: per-point mask logits against the oracle
TOL_PATHS = 1e-4    # fused against unfused (test_one_pass_scene_to_click_half_matches_the_two_kernel_path)
QUERY_COUNTS = (16, 17, 18, 20, 24, 28, 32, 33)
N_POINTS = 6000


def _single_case(nq):
    """nq - 10 clicks (the model adds 10 learned background queries) on random decoder inputs; at 20 queries ten objects
    with one click each on 1 000 points, so that some object owns no point of the first and second layer's mask (its
    attention-mask row would be all True and is lifted) while the others block every point they do not own."""
    g = torch.Generator().manual_seed(1006 + nq)
    n_points = 1000 if nq == 20 else N_POINTS
    feats = torch.randn(n_points, 128, generator=g) * 0.5
    xyz = torch.rand(n_points, 3, generator=g) * torch.tensor([8.0, 6.0, 2.6])
    n_clicks = nq - 10
    n_obj = 10 if nq == 20 else min(4, n_clicks - 1)
    rows = torch.randperm(n_points, generator=g)[:n_clicks].tolist()
    order = torch.randperm(n_clicks, generator=g).tolist()
    owner = [1 + (i % n_obj) if i < n_clicks - 1 or nq == 20 else 0 for i in range(n_clicks)]   # the last click is a background click
    ci = {str(o): [r for r, w in zip(rows, owner) if w == o] for o in range(n_obj + 1)}
    ct = {str(o): [t for t, w in zip(order, owner) if w == o] for o in range(n_obj + 1)}
    return feats, xyz, ci, ct


def _batch_case():
    """three scenes of one forward_backbone + forward_mask call with 18, 20 and 12 queries: the first two are consecutive
    samples of one padded query count, so they share ONE launch of the leftover-tile builds with different query counts
    (per-sample score bias, object bytes and zero key rows below the launch's nqr_max); the third is a launch of its own"""
    scs = [make_scene(6000, seed=33, batch_index=0), make_scene(5000, seed=31, batch_index=1), make_scene(7000, seed=32, batch_index=2)]
    cl = [make_clicks(scs[0]["labels"], 4, 2, 0, seed=3), make_clicks(scs[1]["labels"], 5, 2, 0, seed=1),
          make_clicks(scs[2]["labels"], 1, 2, 0, seed=2)]
    return scs, cl


def _outputs(model):
    """every logits array of every case, in a fixed order: per single case the aux outputs then pred_masks; then the batch's
    per-scene aux outputs and pred_masks"""
    outs, pos_encs = [], []
    eng = model._get_engine()
    for nq in QUERY_COUNTS:
        feats, xyz, ci, ct = _single_case(nq)
        pcd, aux, coords, pos = eng.decoder_inputs(feats, xyz)
        o = model.forward_mask(pcd, aux, coords, pos, click_idx=[ci], click_time_idx=[ct])
        assert o["pred_masks"][0].shape[0] == feats.shape[0]
        outs += [a["pred_masks"][0].cpu().numpy() for a in o["aux_outputs"]] + [o["pred_masks"][0].cpu().numpy()]
        pos_encs.append(pos[4][0][0].cpu())
    scs, cl = _batch_case()
    x = SparseTensor(features=torch.from_numpy(np.concatenate([s["feats"] for s in scs])).cuda(),
                     coordinates=torch.from_numpy(np.concatenate([s["coords"] for s in scs])).cuda())
    r = model.forward_backbone(x, raw_coordinates=torch.from_numpy(np.concatenate([s["raw_xyz"] for s in scs])).cuda())
    o = model.forward_mask(*r, click_idx=[c[0] for c in cl], click_time_idx=[c[1] for c in cl])
    for b in range(len(scs)):
        outs += [a["pred_masks"][b].cpu().numpy() for a in o["aux_outputs"]] + [o["pred_masks"][b].cpu().numpy()]
    return outs, pos_encs


_CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_decoder_leftover_tile as t
torch.manual_seed(0)
model = t.randomize_bn_stats(t.build_model(t.default_args())).eval().cuda()
outs, _ = t._outputs(model)
np.savez(sys.argv[2], *outs)
'''


def test_leftover_query_tile_matches_unfused_path_and_oracle(tmp_path):
    torch.manual_seed(0)
    m = randomize_bn_stats(build_model(default_args())).eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    model = m.cuda()
    fused, pos_encs = _outputs(model)
    n_layers = len(fused) // (len(QUERY_COUNTS) + 3)
    assert n_layers * (len(QUERY_COUNTS) + 3) == len(fused) and n_layers >= 2

    # (a) the unfused live path, in its own interpreter
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "unfused.npz")
    env = dict(os.environ, A3D_FUSED_C2S="0", A3D_FUSED_S2C="0")
    subprocess.run([sys.executable, "-c", _CHILD, root, out], check=True, env=env, timeout=900)
    z = np.load(out)
    unfused = [z[k] for k in z.files]
    assert len(unfused) == len(fused)
    names = [f"{nq} queries, layer {i}" for nq in QUERY_COUNTS for i in range(n_layers)] + \
            [f"batch scene {b}, layer {i}" for b in range(3) for i in range(n_layers)]
    for name, a, b in zip(names, fused, unfused):
        scale = max(1.0, float(np.abs(b).max()))
        err = float(np.abs(a - b).max())
        print(f"{name}: fused vs unfused max|diff| = {err:.2e} (scale {scale:.1f})")
        assert a.shape == b.shape and err <= TOL_PATHS * scale, (name, err)

    # (b) the CPU oracle
    blocked_whole_query = False
    for k, nq in enumerate(QUERY_COUNTS):
        feats, xyz, ci, ct = _single_case(nq)
        ref = od.forward_mask(sd, feats, xyz, pos_encs[k], ci, ct)
        for i in range(n_layers):
            got = fused[k * n_layers + i]
            err = float(np.abs(got - ref[i].numpy()).max())
            scale = max(1.0, float(ref[i].abs().max()))
            print(f"{nq} queries, layer {i}: vs oracle max|diff| = {err:.2e} (scale {scale:.1f})")
            assert err <= TOL * scale, (nq, i, err)
        if nq == 20:   # an object without a point in a layer's mask: the next layer lifts its all-True row, the others block
            for i in range(n_layers - 1):
                owned = np.bincount(ref[i].argmax(-1).numpy(), minlength=ref[i].shape[1])
                blocked_whole_query = blocked_whole_query or bool((owned[1:] == 0).any() and (owned[1:] > 0).any())
    assert blocked_whole_query, "the 20-query case no longer has an object without points"
    scs, cl = _batch_case()
    for b, (sc, (ci, ct)) in enumerate(zip(scs, cl)):
        coords = sc["coords"].copy()
        coords[:, 0] = 0
        ref_b = ob.forward_backbone(sd, coords, torch.from_numpy(sc["feats"]), torch.from_numpy(sc["raw_xyz"]))
        ref = od.forward_mask(sd, ref_b["pcd_features"], torch.from_numpy(sc["raw_xyz"]), ref_b["pos_enc"], ci, ct)
        for i in range(n_layers):
            got = fused[(len(QUERY_COUNTS) + b) * n_layers + i]
            err = float(np.abs(got - ref[i].numpy()).max())
            scale = max(1.0, float(ref[i].abs().max()))
            print(f"batch scene {b}, layer {i}: vs oracle max|diff| = {err:.2e} (scale {scale:.1f})")
            assert err <= TOL * scale, (b, i, err)
