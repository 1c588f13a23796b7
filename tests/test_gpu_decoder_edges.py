"""The inference decoder at its build, point-count and object edges, against oracle.decoder.forward_mask in float64.

Every case of decoder_edge_cases.py runs through the public path -- the engine's decoder_inputs + forward_mask on random
features and coordinates, the seed-0 model of the other decoder tests -- and every layer's logits are compared with the
reference at the project's bar (TOL = 1e-3 of max(1, max|reference|) per layer); decoder_edge_cases.compare says how label
near-ties are dealt with.  Which kernel builds a case runs is the planner's statement, held against the table without a GPU
by test_decoder_plan_classes.py:
  * samples of 2, 15, 16, 17, 127, 128 and 129 points (one 16-point group and its neighbours, one 128-point click-to-scene
    chunk and its neighbours; 31 .. 33 in the wide tier) at one tile, the leftover tile, two tiles with the keys out of LDS,
    and the wide tier at 33 and 70 queries;
  * the object count at up to 32 queries: keys in LDS against global memory at 24 queries, twelve waves against eight at 27 /
    28 queries, the last fused shape (32 queries, 22 objects);
  * click placements: an object on one row, a background click on a foreground row, click times 0 and 199, an object that
    owns no point after the first layer;
  * the first-layer cache: three consecutive calls on one scene state (fused first layer, the call that fills the cache, a
    call that reads it), each against the reference, for every cached build;
  * every build of the wide tier on both sides of its tile edge, and 210 queries with 200 objects;
  * four samples of 2, 17, 129 and 4 200 points in one launch (a table on which both workgroup-share clamps act);
  * a model with one learned background query: one tile with its keys out of LDS;
  * A3D_WIDE_FROM=65 (read once per process -> a second interpreter): 33, 48, 49 and 64 queries on k_kv_c2s<3|4>, k_q_s2c,
    k_out_ln_mask."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import decoder_edge_cases as E
from agile3d_amd import build_model, default_args, randomize_bn_stats
from agile3d_amd.lib import A3DError

pytestmark = pytest.mark.gpu

SINGLE = E.single_cases()


def _model(n_bg=E.N_BG):
    torch.manual_seed(0)
    args = default_args()
    assert args.num_bg_queries == E.N_BG
    args.num_bg_queries = n_bg
    m = randomize_bn_stats(build_model(args)).eval()
    sd32 = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda(), sd32


@pytest.fixture(scope="module")
def model_sd():
    model, sd32 = _model()
    return model, E.to_double(sd32), sd32


def _layers(out, b=0):
    return [a["pred_masks"][b].cpu().numpy() for a in out["aux_outputs"]] + [out["pred_masks"][b].cpu().numpy()]


def _run_case(model, name, points, spec, states, n_bg=E.N_BG):
    """the logits of every call of a case: len(states) consecutive forward_mask calls on one scene state"""
    seed = E.case_seed(name)
    feats, xyz = E.inputs(points, seed)
    ci, ct = E.clicks(points, spec, seed, n_bg)
    r = model._get_engine().decoder_inputs(feats, xyz)
    st = r[0]._a3d
    calls = []
    for k, state in enumerate(states):
        assert state == min(k, 2) and (st.kv0 is None) == (k < 2 or len(states) == 1)    # the engine's cache states 0, 1, 2
        out = model.forward_mask(*r, click_idx=[ci], click_time_idx=[ct])
        assert out["pred_masks"][0].shape == (points, spec[1] + 1)
        calls.append(_layers(out))
    if len(states) == 3:
        assert st.kv0 is not None
    return feats, xyz, ci, ct, calls


@pytest.mark.parametrize("name", list(SINGLE))
def test_decoder_edge_case(model_sd, name):
    model, sd64, sd32 = model_sd
    points, spec, states = SINGLE[name]
    if E.DECLARED[(spec[0], spec[1], 0)] == ("unsupported",):      # the planner's word (test_decoder_plan_classes.py)
        with pytest.raises(A3DError):
            _run_case(model, name, points, spec, states)
        return
    feats, xyz, ci, ct, calls = _run_case(model, name, points, spec, states)
    for state, got in zip(states, calls):
        E.compare(f"{name} state {state}", got, sd64, sd32, feats, xyz, ci, ct)
    if name == "placement_no_point":
        ref = E.reference(sd64, feats, xyz, ci, ct)
        owned = np.bincount(ref[0].argmax(1).numpy(), minlength=ref[0].shape[1])
        assert (owned[1:] == 0).any() and (owned[1:] > 0).any(), f"no object without a point after the first layer: {owned}"


def test_one_tile_with_its_keys_out_of_lds():
    """A model with ONE learned background query: 16 queries with 15 one-click objects run k_s2c_out<1, 12, KG> and, on the
    cached first layer, <1, 12, KG, QC> -- builds the ten learned background queries of the other cases never reach (at most
    six objects at one tile).  Three consecutive calls, each against the float64 reference."""
    model, sd32 = _model(E.ONE_BG)
    assert sd32["bg_query_feat.weight"].shape[0] == E.ONE_BG
    name, points, spec, states = E.ONE_BG_CASE
    feats, xyz, ci, ct, calls = _run_case(model, name, points, spec, states, E.ONE_BG)
    for state, got in zip(states, calls):
        E.compare(f"{name} state {state}", got, E.to_double(sd32), sd32, feats, xyz, ci, ct, E.ONE_BG)


def test_mixed_batch_in_one_launch(model_sd):
    """2, 17, 129 and 4 200 points with 18, 20, 18 and 20 queries: one launch group of the leftover builds in which the
    smallest sample's workgroup share is raised to one and the larger samples' shares are cut to what their 16-point groups can
    use.  The small samples against the float64 reference, the large one against its own single-sample run.  What this pins is
    the kernels on such a table: tiny and large samples side by side in one launch.  It does NOT pin the upper clamp itself:
    workgroups beyond a sample's groups find no group to take, so a share that is not cut changes no output (tried:
    every case of this module passes without it); the clamps are held by test_decoder_plan_classes.py::
    test_workgroup_shares_are_held_to_what_a_sample_can_use on the CPU."""
    model, sd64, sd32 = model_sd
    eng = model._get_engine()
    data, ranges, start = [], [], 0
    for b, (points, spec) in enumerate(zip(E.MIXED_POINTS, E.MIXED_SPECS)):
        seed = E.case_seed(f"mixed{b}")
        data.append(E.inputs(points, seed) + E.clicks(points, spec, seed))
        ranges.append((start, start + points))
        start += points
    r = eng.decoder_inputs_batch(torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data]), ranges)
    out = model.forward_mask(*r, click_idx=[d[2] for d in data], click_time_idx=[d[3] for d in data])
    for b, (feats, xyz, ci, ct) in enumerate(data[:-1]):
        E.compare(f"mixed batch sample {b} ({E.MIXED_POINTS[b]} points)", _layers(out, b), sd64, sd32, feats, xyz, ci, ct)
    feats, xyz, ci, ct = data[-1]
    alone = _layers(model.forward_mask(*eng.decoder_inputs(feats, xyz), click_idx=[ci], click_time_idx=[ct]))
    for i, (a, w) in enumerate(zip(_layers(out, len(data) - 1), alone)):
        scale = max(1.0, float(np.abs(w).max()))
        err = float(np.abs(a - w).max())
        print(f"mixed batch sample {len(data) - 1}, layer {i}: batched vs alone max|diff| = {err:.2e} (scale {scale:.1f})")
        assert a.shape == w.shape and err <= E.TOL_PATHS * scale, (i, err)


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_decoder_edges as t
model, _ = t._model()
arrays = {}
for name, (points, spec, states) in t.E.child_cases().items():
    calls = t._run_case(model, name, points, spec, states)[4]
    for state, got in zip(states, calls):
        for i, a in enumerate(got):
            arrays[f"{name}|{state}|{i}"] = a
np.savez(sys.argv[2], **arrays)
'''


def test_33_to_64_queries_below_the_wide_tier(model_sd, tmp_path):
    """A3D_WIDE_FROM=65 in a child interpreter: the classes of DECLARED_WIDE65, three calls each, against the same reference"""
    _, sd64, sd32 = model_sd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "wide_from_65.npz")
    subprocess.run([sys.executable, "-c", _CHILD, root, out], check=True, env=dict(os.environ, A3D_WIDE_FROM="65"), timeout=600)
    z = np.load(out)
    for name, (points, spec, states) in E.child_cases().items():
        seed = E.case_seed(name)
        feats, xyz = E.inputs(points, seed)
        ci, ct = E.clicks(points, spec, seed)
        for state in states:
            got = [z[f"{name}|{state}|{i}"] for i in range(sum(k.startswith(f"{name}|{state}|") for k in z.files))]
            assert len(got) >= 2
            E.compare(f"{name} state {state}", got, sd64, sd32, feats, xyz, ci, ct)
