"""The VALUE cases of the inference decoder (not collected): inputs on which the click-to-scene attention is peaked, so that
the lazy reference maximum of k_kv_c2s and k_c2s_w moves along a walk, partials with far-apart maxima meet in the slot merge
and in k_c2s_combine, and whole groups underflow.  test_decoder_value_cases_host.py proves on the CPU, with float64 scores,
that each case reaches that code; test_gpu_decoder_values.py runs the cases on the GPU.

THE VISITING ORDER the replay restates (a kernel that deals its 16-point groups differently must fail the host test):
  * k_c2s_w (decoder_wide.h): ``int grp = lb; ... for (int it = 0; grp < ngroups; ++it, grp += nwg)`` -- workgroup lb of the
    sample's nwg takes the groups lb, lb + nwg, ...; a wave is a head; one reference maximum per (head, query), moved for all
    16 queries of a tile when ``it == 0 || ballot(mx4 > kLazy)``: m += max(column maximum - m, 0).
  * k_kv_c2s (decoder.hip): ``slot = lb * SPW + wave / WPG, nslots = nwg * SPW`` and
    ``for (int grp = slot; grp < ngroups; grp += nslots)`` with ``HW = QT <= 2 ? 4 : 2, WPG = H / HW, SPW = 8 / WPG``: SPW = 4
    for one and two query tiles, 2 for three and four.  The reference moves for the 16 queries of a tile when
    ``ballot(mx4 - m > kRefLazy)``: m = max(m, column maximum); the SPW slots of a workgroup are merged at the end, the
    workgroups' records by k_c2s_combine.
  * nwg is dec_wg_shares' (the planner program): a workgroup per group in the wide tier, ceil(groups / 8) at most otherwise.
Scores are oracle.decoder.mha's, times log2(e) (the kernels' domain), -inf where the reference's own mask blocks."""
import math

import numpy as np
import torch

import decoder_edge_cases as E
from oracle import decoder as od

K_LAZY = 8.0                 # kLazy (decoder_wide.h) and kRefLazy (decoder.hip)
QK_SCALE = 3.0               # wide_range: the q and k rows of the in-projections of both cross attentions
FEAT_SCALE = 4.0             # ... and the features
OUTLIER_SCALE = 6.0          # outlier_*: one point's features, on top
QK_OF = {"merge_q11_k1": 4.0}   # a case with its own factor: at 3, layers 1 and 2 of this one fell short of MERGE_SHARE (0.18, 0.16)
RAMP_A = 16.0                # ramp: r(i) in [-A, A] along a fixed unit vector: the median (head, query) column of layer 0 has a
                             # score range of 150 .. 300 and columns climb and fall by more than RAMP_TREND end to end (asserted)
RAMP_TREND = 3 * K_LAZY
MOVE_MIN = 1.0               # a move counts when the reference rises by more than this (l and acc shrink to less than half)
WALK_SHARE = 0.25            # walks of every layer that must move the reference after their first open group
MERGE_SHARE, MERGE_GAP = 0.25, 24.0     # 129 points: (head, query) pairs whose partials' maxima differ by more than 24
SEED_SHIFT = {"merge_q18_k4": 5}    # a case whose first seed met a condition of the host test with little room (0.28, 0.26)
RECIPES = ("wide_range", "ramp", "outlier_last", "outlier_first", "outlier_mid")
LOG2E = math.log2(math.e)


def qk_scale(name):
    return QK_OF.get(name, QK_SCALE)


_MODELS = {}


def seed0_model(factor=QK_SCALE, n_bg=E.N_BG):
    """the seed-0 model of the other decoder tests (CPU) with the wide_range weights loaded, and that fp32 state dict; one per
    factor and process"""
    if (factor, n_bg) not in _MODELS:
        _MODELS[(factor, n_bg)] = _seed0_model(factor, n_bg)
    return _MODELS[(factor, n_bg)]


def _seed0_model(factor, n_bg):
    from agile3d_amd import build_model, default_args, randomize_bn_stats
    torch.manual_seed(0)
    args = default_args()
    args.num_bg_queries = n_bg
    m = randomize_bn_stats(build_model(args)).eval()
    sd32 = scale_weights({k: v.clone() for k, v in m.state_dict().items()}, factor)
    m.load_state_dict(sd32)
    return m, sd32


def scale_weights(sd, factor=QK_SCALE, layers=3):
    """rows [:256] (q and k) of in_proj_weight / in_proj_bias of both cross attentions of every layer times ``factor``"""
    sd = dict(sd)
    for side in ("c2s_attention", "s2c_attention"):
        for d in range(layers):
            for leaf in ("in_proj_weight", "in_proj_bias"):
                key = f"{side}.{d}.0.multihead_attn.{leaf}"
                t = sd[key].clone()
                t[:256] *= factor
                sd[key] = t
    return sd


def mid_point(points):
    """outlier_mid's point: in a group that is the SECOND one of its walk in both tiers and not the last group"""
    return (((points + 15) // 16) - 5) * 16 + 5


def features(recipe, feats):
    """the recipe applied to decoder_edge_cases.inputs' features"""
    n = feats.shape[0]
    f = feats * FEAT_SCALE
    if recipe == "ramp":
        u = torch.randn(128, generator=torch.Generator().manual_seed(12345))
        f = f + torch.linspace(-RAMP_A, RAMP_A, n)[:, None] * (u / u.norm())[None]
    elif recipe.startswith("outlier_"):
        row = {"outlier_last": n - 1, "outlier_first": 0, "outlier_mid": mid_point(n)}[recipe]
        f = f.clone()
        f[row] *= OUTLIER_SCALE
    else:
        assert recipe == "wide_range", recipe
    return f


# ---- the cases: name -> (points, (queries, objects), kv0 states, recipe) ------------------------------------------------
MERGE_POINTS = 129
MERGE_SPECS = ((11, 1), (18, 4), (28, 5), (28, 18), (70, 3), (128, 3), (210, 3), (210, 200))
MERGE_CACHED = ((18, 4), (70, 3))                     # three calls: k_c2s_attn_b and the QC builds on the same values
# the click-to-scene build of a case's plan class (cache state 0), as the issue names them
C2S_BUILD = {(11, 1): "k_kv_c2s<1>", (18, 4): "k_kv_c2s<2,LO>", (28, 5): "k_kv_c2s<2>", (28, 18): "k_kv_c2s<2>",
             (70, 3): "k_c2s_w<5>", (128, 3): "k_c2s_w<8>", (210, 3): "k_c2s_w<14>", (210, 200): "k_c2s_w<14>",
             (129, 3): "k_c2s_w<10>", (20, 10): "k_kv_c2s<2,LO>"}
S2C_WAVES = {(28, 5): "k_s2c_out<2,12,KG>", (28, 18): "k_s2c_out<2,8,KG>"}      # twelve waves against eight
WALK_4200 = ((18, 4), (28, 5), (70, 3))
WALK_12000 = ((70, 3), (129, 3))
WALK_40000 = ((20, 10),)
# one child interpreter of test_gpu_decoder_values.py: (switch environment, specs), each on wide_range and ramp at 4 200 points
CHILD_RUNS = (({"A3D_FUSED_C2S": "0", "A3D_FUSED_WIDE": "0"}, ((18, 4), (70, 3))), ({"A3D_WIDE_FROM": "65"}, ((48, 3), (64, 3))))
CHILD_POINTS, CHILD_RECIPES = 4200, ("wide_range", "ramp")


def cases():
    c = {}
    for nq, k in MERGE_SPECS:
        c[f"merge_q{nq}_k{k}"] = (MERGE_POINTS, (nq, k), (0, 1, 2) if (nq, k) in MERGE_CACHED else (0,), "wide_range")
    for recipe in RECIPES:
        for nq, k in WALK_4200:
            c[f"walk4200_{recipe}_q{nq}_k{k}"] = (4200, (nq, k), (0,), recipe)
    for recipe in ("wide_range", "ramp"):
        for nq, k in WALK_12000:
            c[f"walk12000_{recipe}_q{nq}_k{k}"] = (12000, (nq, k), (0,), recipe)
        for nq, k in WALK_40000:
            c[f"walk40000_{recipe}_q{nq}_k{k}"] = (40000, (nq, k), (0,), recipe)
    return c


def child_cases():
    """[(index into CHILD_RUNS, name, points, spec, recipe)]; the name (hence the inputs) is the one of the default-path case"""
    return [(i, f"walk{CHILD_POINTS}_{recipe}_q{nq}_k{k}", CHILD_POINTS, (nq, k), recipe)
            for i, (_, specs) in enumerate(CHILD_RUNS) for nq, k in specs for recipe in CHILD_RECIPES]


def case_inputs(name, points, spec, recipe):
    """features (recipe applied), coordinates and clicks of a case; the seed is the name's, as in decoder_edge_cases"""
    seed = E.case_seed(name) + SEED_SHIFT.get(name, 0)
    feats, xyz = E.inputs(points, seed)
    ci, ct = E.clicks(points, spec, seed)
    return features(recipe, feats), xyz, ci, ct


_REFS = {}


def ramp_trend(s):
    """mean score of the last tenth of the points minus that of the first tenth, per (head, query)"""
    t = max(1, s.shape[-1] // 10)
    return s[:, :, -t:].mean(-1) - s[:, :, :t].mean(-1)


def references(name, sd64, sd32, feats, xyz, ci, ct):
    """(float64 logits, float32 oracle's logits, float64 click-to-scene scores) of a case, computed once.  The float32
    oracle runs on the attention masks of the float64 one (force_masks): what it is asked is what float32 arithmetic costs on
    these values, and a label near-tie that sends the two down different branches of the later layers -- which
    decoder_edge_cases.compare deals with in the same way -- says nothing about that (seen: 4e-6 on one machine, 3e-4 on
    another, for the same case)."""
    if name not in _REFS:
        scores = []
        inner = od.mha

        def spy(sd, prefix, query, key, value, attn_mask=None, **kw):
            if prefix.startswith("c2s_attention."):
                scores.append(c2s_scores(sd, prefix, query, key, attn_mask))
            return inner(sd, prefix, query, key, value, attn_mask, **kw)
        od.mha = spy
        try:
            ref64 = E.reference(sd64, feats, xyz, ci, ct)
        finally:
            od.mha = inner
        masks = [E.masks_from_logits(r, ci) for r in ref64]
        _REFS[name] = (ref64, E.reference(sd32, feats, xyz, ci, ct, force_masks=masks), scores)
    return _REFS[name]


def c2s_scores(sd, prefix, query, key, attn_mask, nhead=8):
    """oracle.decoder.mha's scores [heads, queries, points] times log2(e), -inf where ``attn_mask`` blocks (numpy)"""
    e = query.shape[-1]
    w, b = sd[prefix + "in_proj_weight"], sd[prefix + "in_proj_bias"]
    dh = e // nhead
    q = (query @ w[:e].T + b[:e]).reshape(-1, nhead, dh).transpose(0, 1) * (1.0 / math.sqrt(dh))
    k = (key @ w[e:2 * e].T + b[e:2 * e]).reshape(-1, nhead, dh).transpose(0, 1)
    s = q @ k.transpose(1, 2) * LOG2E
    if attn_mask is not None:
        s = s.masked_fill(attn_mask.unsqueeze(0), float("-inf"))
    assert s.dtype == torch.float64
    return s.numpy()


def column_range(s):
    """max and median over the (head, query) columns of the range of their open scores"""
    hi = np.where(np.isfinite(s), s, -np.inf).max(-1)
    lo = np.where(np.isfinite(s), s, np.inf).min(-1)
    r = (hi - lo)[np.isfinite(hi)]
    return float(r.max()), float(np.median(r))


# ---- the lazy rule, replayed ------------------------------------------------------------------------------------------------
def slots_of(build, nwg):
    """(walks of the sample, wide tier?) of a click-to-scene build on nwg workgroups"""
    if build.startswith("k_c2s_w<"):
        return nwg, True
    assert build.startswith("k_kv_c2s<"), build
    qt = int(build[len("k_kv_c2s<")])
    return nwg * (4 if qt <= 2 else 2), False


def replay(s, nslots, wide):
    """The lazy reference maximum over the walks of every slot (fused tier) or workgroup (wide tier).  s: [heads, queries,
    points] log2-domain scores, -inf = blocked.  Returns a dictionary of [heads, queries, nslots] arrays:
      groups   how many groups the walk has (the same for every head and query)
      m        the reference when the walk ends (-inf: the column met no open point)
      moved    AFTER its first open group the walk took the kernel's branch (some column of the query tile met a score more
               than K_LAZY above its reference) on a group whose maximum in THIS column is more than MOVE_MIN above the
               column's reference: m rises, l and acc are rescaled by less than 2^-MOVE_MIN
      last     ... in the last group of the walk (walks of two groups and more)
      own      as moved, by a score of this column itself more than K_LAZY above its reference"""
    h, nq, n = s.shape
    ng = (n + 15) // 16
    steps = -(-ng // nslots)
    pad = np.full((h, nq, steps * nslots * 16), -np.inf)
    pad[:, :, :n] = s
    gmax = pad.reshape(h, nq, steps, nslots, 16).max(-1)          # group k * nslots + slot -> [k][slot]
    present = (np.arange(steps)[:, None] * nslots + np.arange(nslots)[None]) < ng
    groups = present.sum(0)
    m = np.full((h, nq, nslots), -np.inf)
    opened = np.zeros((h, nq, nslots), bool)
    moved, last, own = opened.copy(), opened.copy(), opened.copy()
    tile = np.arange(nq) // 16
    for k in range(steps):
        g = gmax[:, :, k, :]
        with np.errstate(invalid="ignore"):
            over = np.where(np.isfinite(g), g - m > K_LAZY, False)         # (from m = -inf: the first open group)
        trig = np.zeros_like(over)
        for t in range(tile.max() + 1):                                    # wave-uniform: the 16 queries of a tile move together
            trig[:, tile == t, :] = over[:, tile == t, :].any(1, keepdims=True)
        if wide and k == 0:
            trig[:] = True
        with np.errstate(invalid="ignore"):
            step = trig & opened & np.where(np.isfinite(g), g - m > MOVE_MIN, False)
        moved |= step
        own |= over & opened
        last = np.where((groups == k + 1)[None, None] & (k > 0), step, last)
        m = np.where(trig & (g > m), g, m)
        opened |= np.isfinite(g)
    return {"groups": np.broadcast_to(groups[None, None], m.shape), "m": m, "moved": moved, "last": last, "own": own}
