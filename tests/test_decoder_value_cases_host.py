"""The value cases of test_gpu_decoder_values.py reach the code they are there for (CPU, float64 scores; no GPU).

Per case: (a) the planner puts it on the click-to-scene build it names; (b) the lazy reference maximum, replayed over the
float64 scores in the order one slot or workgroup visits its groups (decoder_value_cases.py states that order and the kernel
lines it mirrors), moves after the first open group in at least a quarter of the walks of every layer -- at 129 points,
where a walk is one group or two: the partials of at least a quarter of the (head, query) pairs differ in m by more than 24;
(c) the float32 oracle stays within TOL / 4 of the float64 one on every layer, so that the inputs are not beyond what an fp32
implementation can be held to at the unchanged bar.  (b) and (c) are conditions on the inputs, not measurements of the
kernels: a case that falls short gets another seed or amplitude, never a lower condition."""
import numpy as np
import pytest

import decoder_edge_cases as E
import decoder_value_cases as V

CASES = V.cases()


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return E.build_planner(str(tmp_path_factory.mktemp("decoder_plan_values")))


def _weights(name):
    _, sd32 = V.seed0_model(V.qk_scale(name))
    return E.to_double(sd32), sd32


def test_the_recipe_scales_only_q_and_k_of_the_cross_attentions():
    from agile3d_amd import build_model, default_args
    sd = build_model(default_args()).state_dict()
    got = V.scale_weights(sd)
    changed = sorted(k for k in sd if not bool((sd[k] == got[k]).all()))
    assert changed == sorted(f"{s}.{d}.0.multihead_attn.{leaf}" for s in ("c2s_attention", "s2c_attention") for d in range(3)
                             for leaf in ("in_proj_weight", "in_proj_bias") if bool(sd[f"{s}.{d}.0.multihead_attn.{leaf}"][:256].any()))
    w = "c2s_attention.1.0.multihead_attn.in_proj_weight"
    assert bool((got[w][:256] == sd[w][:256] * V.QK_SCALE).all()) and bool((got[w][256:] == sd[w][256:]).all())


@pytest.mark.parametrize("name", list(CASES))
def test_plan_class(planner, name):
    """(a): every cache state of the case plans to its declared class, and that class runs the build the case is named for"""
    _, (nq, k), states, _ = CASES[name]
    plans = E.run_planner(planner, [[(nq, k, st)] for st in states], E.DEFAULT)
    for st, p in zip(states, plans):
        assert E.plan_class(p) == E.DECLARED[(nq, k, st)], (name, st, E.plan_class(p))
    cls = E.plan_class(plans[0])
    assert cls[0] == cls[3] == V.C2S_BUILD[(nq, k)], (name, cls)
    if (nq, k) in V.S2C_WAVES:
        assert cls[1] == V.S2C_WAVES[(nq, k)], (name, cls)
    if len(states) == 3:
        assert all(E.plan_class(p)[0].startswith("k_c2s_attn_b<") and "QC" in E.plan_class(p)[1] for p in plans[1:]), name


def test_child_runs_plan_to_the_unfused_and_the_below_wide_kernels(planner):
    unfused, wide65 = (tuple(int(env.get(k, d)) for k, d in zip(("A3D_FUSED_C2S", "A3D_FUSED_WIDE", "A3D_FUSED_S2O", "A3D_FUSED_S2C",
                                                                "A3D_WIDE_FROM"), E.DEFAULT)) for env, _ in V.CHILD_RUNS)
    assert wide65 == E.WIDE65
    for nq, k in V.CHILD_RUNS[0][1]:
        cls = E.plan_class(E.run_planner(planner, [[(nq, k, 0)]], unfused)[0])
        assert cls[0].startswith("k_c2s_attn<") and cls[3].startswith("k_c2s_attn<"), cls
        assert cls[1].startswith("k_s2c_attn_wide<") and cls[4].startswith("k_s2c_attn_wide<"), cls
    for (nq, k), build in zip(V.CHILD_RUNS[1][1], ("k_kv_c2s<3>", "k_kv_c2s<4>")):
        cls = E.plan_class(E.run_planner(planner, [[(nq, k, 0)]], wide65)[0])
        assert cls == E.DECLARED_WIDE65[(nq, k, 0)] and cls[0] == cls[3] == build, cls


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_the_lazy_code(planner, name):
    sd64, sd32 = _weights(name)
    points, spec, _, recipe = CASES[name]
    feats, xyz, ci, ct = V.case_inputs(name, points, spec, recipe)
    ref64, ref32, scores = V.references(name, sd64, sd32, feats, xyz, ci, ct)
    build = V.C2S_BUILD[spec]
    wide = build.startswith("k_c2s_w<")
    grid, shares = E.run_shares(planner, [points], 1 if wide else 0)
    nwg = shares[0][1] - shares[0][0]
    assert grid == nwg
    nslots, _ = V.slots_of(build, nwg)
    ngroups = (points + 15) // 16
    assert len(scores) == len(ref64) == 3
    fails = []
    for layer, s in enumerate(scores):
        assert s.shape == (8, spec[0], points)
        # (c) the float32 oracle against float64
        scale = max(1.0, float(ref64[layer].abs().max()))
        e32 = float((ref32[layer].double() - ref64[layer]).abs().max()) / scale
        rmax, rmed = V.column_range(s)
        r = V.replay(s, nslots, wide)
        if points == V.MERGE_POINTS:
            # the partials of a (head, query): one per slot that met an open point
            m = r["m"]
            hi, lo = np.where(np.isfinite(m), m, -np.inf).max(-1), np.where(np.isfinite(m), m, np.inf).min(-1)
            several = np.isfinite(m).sum(-1) >= 2
            share = float(((hi - lo > V.MERGE_GAP) & several).mean())
            print(f"VALUE {name} layer {layer}: range {rmax:.0f} / {rmed:.0f}, {nslots} partials, share of (head, query) whose "
                  f"partials' m differ by > {V.MERGE_GAP:.0f}: {share:.2f}, fp32 oracle {e32:.1e}")
            if share < V.MERGE_SHARE:
                fails.append((layer, "merge share", share))
        else:
            walks = r["groups"] >= 2
            assert walks.any(), name
            share = float(r["moved"][walks].mean())
            share_last, share_own = float(r["last"][walks].mean()), float(r["own"][walks].mean())
            print(f"VALUE {name} layer {layer}: range {rmax:.0f} / {rmed:.0f}, {int(walks[0, 0].sum())} of {nslots} walks of "
                  f"{int(r['groups'].max())} groups, share that moves the reference {share:.2f} (in the last group {share_last:.2f}, by its own column {share_own:.2f}),"
                  f" fp32 oracle {e32:.1e}")
            if share < V.WALK_SHARE:
                fails.append((layer, "walk share", share))
            if recipe == "outlier_last" and layer == 0:        # the walk that ends on the last group moves there (the later
                # layers' keys have been through a LayerNorm, which undoes the point's scale: it is an outlier of layer 0)
                slot = (ngroups - 1) % nslots
                assert r["groups"][0, 0, slot] >= 2 and (ngroups - 1) // nslots == r["groups"][0, 0, slot] - 1
                own = float(r["last"][:, :, slot].mean())
                print(f"VALUE {name} layer {layer}: (head, query) of slot {slot} that move on the last group {own:.2f}")
                if own < V.WALK_SHARE:
                    fails.append((layer, "last group", own))
            if recipe == "outlier_mid":
                grp = V.mid_point(points) // 16
                assert nslots <= grp < min(2 * nslots, ngroups - 1), (grp, nslots)
        if recipe == "ramp" and layer == 0:
            trend = V.ramp_trend(s)
            print(f"VALUE {name} layer 0: end-to-end trend of the columns {trend.min():.0f} .. {trend.max():.0f}")
            assert 150.0 <= rmed <= 300.0, (name, rmed)
            assert trend.max() > V.RAMP_TREND and trend.min() < -V.RAMP_TREND, (name, trend.min(), trend.max())
        if e32 > E.TOL / 4:
            fails.append((layer, "fp32 oracle", e32))
    assert not fails, (name, fails)
