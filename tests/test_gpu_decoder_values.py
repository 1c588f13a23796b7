"""-m gpu: the inference decoder on wide-range, peaked and drifting attention scores, against oracle.decoder.forward_mask in
float64 at the project's unchanged bar (TOL = 1e-3 of max(1, max|reference|) per layer, decoder_edge_cases.compare).

The other decoder tests run 0.5 randn features through the default initialisation: their click-to-scene scores span about 10
in the log2 domain, so the lazy reference maximum of k_kv_c2s (kRefLazy) and of k_c2s_w (kLazy) hardly ever moves after a
walk's first group, the wide tier hardly ever recomputes a tile against a new -m, the slot merge and k_c2s_combine only meet
partials with nearly equal m, and no group underflows.  The cases of decoder_value_cases.py (q / k in-projections of both
cross attentions times 3, features times 4; one point six times further out; a ramp along the point index) have score
ranges of 150 .. 700; test_decoder_value_cases_host.py holds, without a GPU, that each case reaches that code on the build it
names.  Every case goes through the public path (decoder_inputs + forward_mask), and the 4 200-point wide_range and ramp
inputs also through the unfused kernels (exact running maximum) and through k_kv_c2s<3|4>, each in a fresh interpreter (the
switches are read once per process), against the same reference and against the default path's run.

Measured on an MI355X: the worst error / scale of a case is 1.9e-05 (walk4200_outlier_mid_q28_k5; the others 3e-06 .. 1e-05,
where the float32 oracle itself is); the runs on other kernels agree with the default path to 7e-06 of the scale or better.

Tried on scratch builds, each change confined to the moves AFTER a walk's first one: the rescale of acc skipped in k_c2s_w's
move branch, -m left stale in its mask product; the rescale of l skipped in k_kv_c2s's branch, the sign of its exponent
turned round.  Every walking case here of the tier that was changed fails (9, 9, 15 and 16 of the 29 cases), and so does the
comparison with the other kernels.  The older decoder tests are not blind to these changes -- test_gpu_model's many-click
scenes and a few 127 / 128-point cases of test_gpu_decoder_edges.py do move a reference once in a while, and 7 to 19 of
them fail as well -- but they reach the branch by accident of their random scores; here the host test holds every case to
it, at every plan class and at the depths of walk the planner gives."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import decoder_edge_cases as E
import decoder_value_cases as V

pytestmark = pytest.mark.gpu

CASES = V.cases()
_GPU_MODELS = {}


def _model(factor):
    if factor not in _GPU_MODELS:
        m, sd32 = V.seed0_model(factor)
        _GPU_MODELS[factor] = (m.cuda(), E.to_double(sd32), sd32)
    return _GPU_MODELS[factor]


def _layers(out, b=0):
    return [a["pred_masks"][b].cpu().numpy() for a in out["aux_outputs"]] + [out["pred_masks"][b].cpu().numpy()]


def _run(model, feats, xyz, ci, ct, states=(0,)):
    """the logits of len(states) consecutive forward_mask calls on one scene state (test_gpu_decoder_edges._run_case)"""
    r = model._get_engine().decoder_inputs(feats, xyz)
    st = r[0]._a3d
    calls = []
    for k, state in enumerate(states):
        assert state == min(k, 2) and (st.kv0 is None) == (k < 2 or len(states) == 1)
        out = model.forward_mask(*r, click_idx=[ci], click_time_idx=[ct])
        assert out["pred_masks"][0].shape == (feats.shape[0], len(ci))
        calls.append(_layers(out))
    return calls


@pytest.mark.parametrize("name", list(CASES))
def test_decoder_value_case(name):
    points, spec, states, recipe = CASES[name]
    model, sd64, sd32 = _model(V.qk_scale(name))
    feats, xyz, ci, ct = V.case_inputs(name, points, spec, recipe)
    for state, got in zip(states, _run(model, feats, xyz, ci, ct, states)):
        E.compare(f"{name} state {state}", got, sd64, sd32, feats, xyz, ci, ct)


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_decoder_values as t
model = t._model(t.V.QK_SCALE)[0]
arrays = {}
for run, name, points, spec, recipe in t.V.child_cases():
    if run == int(sys.argv[3]):
        for i, a in enumerate(t._run(model, *t.V.case_inputs(name, points, spec, recipe))[0]):
            arrays[f"{name}|{i}"] = a
np.savez(sys.argv[2], **arrays)
'''


def test_other_kernels_on_the_same_values(tmp_path):
    """The 4 200-point wide_range and ramp inputs with A3D_FUSED_C2S=0 A3D_FUSED_WIDE=0 (18 and 70 queries: k_c2s_attn and
    k_s2c_attn_wide, which keep an exact running maximum) and with A3D_WIDE_FROM=65 (48 and 64 queries: k_kv_c2s<3|4>, two
    groups per slot pair, four per slot at SPW = 2): a fresh interpreter per setting.  Each run against the float64 reference
    and, to TOL_PATHS, against the default path's run of the same inputs."""
    model, sd64, sd32 = _model(V.QK_SCALE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for run, (env, _) in enumerate(V.CHILD_RUNS):
        out = str(tmp_path / f"child{run}.npz")
        subprocess.run([sys.executable, "-c", _CHILD, root, out, str(run)], check=True, env=dict(os.environ, **env), timeout=600)
        z = np.load(out)
        mine = [c for c in V.child_cases() if c[0] == run]
        assert mine and len(z.files) == 3 * len(mine)
        for _, name, points, spec, recipe in mine:
            feats, xyz, ci, ct = V.case_inputs(name, points, spec, recipe)
            got = [z[f"{name}|{i}"] for i in range(3)]
            E.compare(f"{name} {env}", got, sd64, sd32, feats, xyz, ci, ct)
            default = _run(model, feats, xyz, ci, ct)[0]
            for i, (a, w) in enumerate(zip(got, default)):
                scale = max(1.0, float(np.abs(w).max()))
                err = float(np.abs(a - w).max())
                print(f"{name} {env} layer {i}: against the default path max|diff| = {err:.2e} (scale {scale:.1f})")
                assert a.shape == w.shape and err <= E.TOL_PATHS * scale, (name, env, i, err)
