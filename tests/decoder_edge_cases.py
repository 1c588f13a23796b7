"""The case table of test_gpu_decoder_edges.py and the host-side planner sweep that test_decoder_plan_classes.py holds it against.

A PLAN CLASS is what plan_decoder (csrc/decoder.hip, between its two marker lines) decides for a launch group, reduced to what
selects code: the builds of the click-to-scene kernel, the scene-to-click kernel and the output half ("-": the kernel before it
does that work) of the first layer, then of the other layers, and whether the pass fills the first-layer cache first:
    ("k_kv_c2s<2,LO>", "k_s2c_out<2,12,LO>", "-", "k_kv_c2s<2,LO>", "k_s2c_out<2,12,LO>", "-", 0)
The build names are decoder_plan_main.cpp's.  Nothing in the planner half needs a GPU; the second half (inputs, the float64
reference, the comparison) is shared by the GPU module and its child interpreter."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import torch

from oracle import decoder as od

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODER = os.path.join(ROOT, "agile3d_amd", "csrc", "decoder.hip")
PLAN_MAIN = os.path.join(ROOT, "tests", "decoder_plan_main.cpp")
BLOCK_BEGIN, BLOCK_END = "// ---- planning:", "// ---- end of planning"
N_BG = 10                    # learned background queries of the model (default_args)
A3D_ERR_UNSUPPORTED = -6
DEFAULT = (1, 1, 1, 1, 33)   # A3D_FUSED_C2S, A3D_FUSED_WIDE, A3D_FUSED_S2O, A3D_FUSED_S2C, A3D_WIDE_FROM
WIDE65 = (1, 1, 1, 1, 65)


# ---- the planner as a host program ---------------------------------------------------------------------------------
def planning_block():
    text = open(DECODER).read()
    assert text.count(BLOCK_BEGIN) == 1 and text.count(BLOCK_END) == 1
    a, b = text.index(BLOCK_BEGIN), text.index(BLOCK_END)
    assert 0 <= a < b
    return text[a:b]


def host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    raise RuntimeError("no host C++ compiler (the build needs one)")


def build_planner(workdir):
    """compiles decoder_plan_main.cpp around the planning block cut from decoder.hip; returns the program's path"""
    with open(os.path.join(workdir, "decoder_planning_block.inc"), "w") as f:
        f.write(planning_block())
    exe = os.path.join(workdir, "decoder_plan")
    subprocess.run([host_compiler(), "-O2", "-std=c++17", "-I", workdir, "-I", os.path.join(ROOT, "include"), PLAN_MAIN, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


_FLAGS = ("rc", "grouped", "wide", "qt", "nblk", "leftover", "fuse_c2s", "fuse_s2c", "fuse_out", "fuse_all", "s2c_kg", "fits12",
          "cached0", "fill0")


def run_planner(exe, queries, switches=DEFAULT, n_bg=N_BG):
    """plans (dicts of _FLAGS, "builds": six names, "lds": six byte counts) of a list of groups; a group is a list of
    (queries, objects, kv0_state) samples of a model with n_bg learned background queries"""
    head = "plan " + " ".join(str(int(v)) for v in switches) + f" {n_bg} "
    text = "".join(head + f"{len(g)} " + " ".join(f"{nq} {k} {st}" for nq, k, st in g) + "\n" for g in queries)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    plans = []
    for line in out[:len(queries)]:
        parts = line.split()
        p = {k: int(v) for k, v in zip(_FLAGS, parts)}
        rest = parts[len(_FLAGS):]
        p["builds"], p["lds"] = tuple(rest[0::2]), tuple(int(v) for v in rest[1::2])
        plans.append(p)
    assert len(plans) == len(queries)
    return plans


def run_shares(exe, points, wg_per_group):
    """dec_wg_shares of a launch group whose samples have ``points`` points: (grid, [(wg_begin, wg_end)])"""
    text = f"shares {int(wg_per_group)} {len(points)} " + " ".join(str(int(n)) for n in points) + "\n"
    out = [int(v) for v in subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()]
    assert len(out) == 1 + 2 * len(points)
    return out[0], list(zip(out[1::2], out[2::2]))


def plan_class(plan):
    """the class tuple of the module docstring; ("unsupported",) for a refused group"""
    if plan["rc"] == A3D_ERR_UNSUPPORTED:
        return ("unsupported",)
    assert plan["rc"] == 0
    return plan["builds"] + (plan["fill0"],)


def sweep_groups():
    """11 .. 210 queries, 1 .. (clicks) objects, the three cache states: every single sample, and pairs (one or (clicks)
    objects each, both in the state the engine gives a call's samples) -- the planner says which pairs share a group"""
    singles = [[(nq, k, st)] for nq in range(11, 211) for k in range(1, nq - N_BG + 1) for st in (0, 1, 2)]
    pairs = [[(a, ka, st), (b, kb, st)] for a in range(11, 211) for b in range(a, 211) for st in (0, 1, 2)
             for ka in {1, a - N_BG} for kb in {1, b - N_BG}]
    return singles + pairs


_REACH = {}


def reachable_classes(exe, switches):
    if (exe, switches) not in _REACH:
        _REACH[(exe, switches)] = {plan_class(p) for p in run_planner(exe, sweep_groups(), switches) if p["grouped"]}
    return _REACH[(exe, switches)]


# The builds of k_s2c_out the library instantiates (s2c_out_kernel, decoder.hip): what the plans name over every switch setting
# and every number of learned background queries.  Left out: <QT, 8> without KG (keys that stay in LDS imply that twelve waves
# fit) and <1, 8, KG> (with the keys out of LDS twelve waves fit up to 25 objects; one tile has at most 16).
S2C_OUT_BUILDS = {"k_s2c_out<1,12>", "k_s2c_out<1,12,QC>", "k_s2c_out<1,12,KG>", "k_s2c_out<1,12,KG,QC>",
                  "k_s2c_out<2,12>", "k_s2c_out<2,12,QC>", "k_s2c_out<2,12,KG>", "k_s2c_out<2,12,KG,QC>",
                  "k_s2c_out<2,12,LO>", "k_s2c_out<2,12,QC,LO>", "k_s2c_out<2,8,KG>"}


def fused_tier_groups(n_bg):
    """every launch group of up to 32 queries of a model with n_bg learned background queries: single samples with 1 ..
    (clicks) objects, and pairs of one padded query count with one or (clicks) objects each; cache states 0 and 2"""
    lo = max(n_bg + 1, 1)
    singles = [[(nq, k, st)] for nq in range(lo, 33) for k in range(1, nq - n_bg + 1) for st in (0, 2)]
    pairs = [[(a, ka, st), (b, kb, st)] for a in range(lo, 33) for b in range(a, 33) for st in (0, 2)
             for ka in {1, a - n_bg} for kb in {1, b - n_bg}]
    return singles + pairs


# ---- the cases ------------------------------------------------------------------------------------------------------
# A case: name -> (points, spec).  spec is what clicks() turns into click dictionaries: (queries, objects) or
# (queries, objects, variant).  Every case's (queries, objects, kv0_state) and the class it is there for stand in the tables
# below; test_decoder_plan_classes.py asserts that each plans to its class and that no class the sweep reaches lacks a case.
POINT_EDGES = (2, 15, 16, 17, 127, 128, 129)
WIDE_POINT_EDGES = POINT_EDGES + (31, 32, 33)          # one workgroup iteration of the wide tier takes 32 points
POINT_GROUPS = ((11, 1), (18, 4), (28, 5), (33, 3), (70, 3))
OBJECT_EDGES = ((21, 11), (24, 2), (24, 5), (27, 17), (28, 18), (32, 22), (32, 2))
WIDE_TILE_EDGES = (33, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 160, 161, 192, 193, 210)
PLACEMENTS = ("one_row", "bg_on_fg", "times", "no_point")
# three consecutive calls on one scene state (kv0 states 0, 1, 2): one tile, the leftover tile, its click-to-scene build next
# to keys in global memory, two tiles with keys in LDS, KG, the 8-wave build (which recomputes the queries), and every build
# of the wide tier with each k_c2s_attn_b build it pairs with
CACHE_SETS = ((11, 1), (16, 3), (18, 4), (20, 10), (24, 2), (28, 5), (28, 18), (33, 3), (64, 3), (70, 3), (96, 3), (112, 3), (128, 3),
              (160, 3), (192, 3), (210, 3))
CHILD_QUERIES = (33, 48, 49, 64)                      # under A3D_WIDE_FROM=65, at 17 and 129 points, three calls each
CHILD_POINTS = (17, 129)
MIXED_POINTS = (2, 17, 129, 4200)                      # one call; 18, 20, 18 and 20 queries: one launch of the leftover builds
MIXED_SPECS = ((18, 4), (20, 5), (18, 3), (20, 4))
EDGE_POINTS = 129


def single_cases():
    """name -> (points, spec, kv0 states the case runs through)"""
    cases = {}
    for nq, k in POINT_GROUPS:
        for n in (WIDE_POINT_EDGES if nq >= 33 else POINT_EDGES):
            cases[f"points{n}_q{nq}_k{k}"] = (n, (nq, k), (0,))
    for nq, k in OBJECT_EDGES:
        cases[f"objects_q{nq}_k{k}"] = (EDGE_POINTS, (nq, k), (0,))
    for v in PLACEMENTS:
        cases[f"placement_{v}"] = (EDGE_POINTS, PLACEMENT_SPECS[v], (0,))
    for nq, k in CACHE_SETS:
        cases[f"cache_q{nq}_k{k}"] = (EDGE_POINTS, (nq, k), (0, 1, 2))
    for nq in WIDE_TILE_EDGES:
        cases[f"wide_q{nq}_k3"] = (EDGE_POINTS, (nq, 3), (0,))
    cases["wide_q210_k200"] = (EDGE_POINTS, (210, 200), (0,))
    return cases


# click placements: an object whose clicks all sit on one row; a background click on the row of a foreground click; click
# times 0 and 199; at one tile, an object that owns no point after the first layer (six objects on 129 points; the GPU test
# asserts on the reference that it happens)
PLACEMENT_SPECS = {"one_row": (18, 3, "one_row"), "bg_on_fg": (14, 2, "bg_on_fg"), "times": (16, 2, "times"),
                   "no_point": (16, 6, "no_point")}


# One tile with its keys out of LDS: 16 queries from 15 objects on, which a model with ten learned background queries never
# has.  A model with ONE learned background query and 15 one-click objects, three calls: k_s2c_out<1,12,KG> and <1,12,KG,QC>.
ONE_BG = 1
ONE_BG_CASE = ("one_bg_q16_k15", EDGE_POINTS, (16, 15), (0, 1, 2))


def child_cases():
    return {f"child_points{n}_q{nq}_k3": (n, (nq, 3), (0, 1, 2)) for nq in CHILD_QUERIES for n in CHILD_POINTS}


def case_groups(cases):
    """the planner queries of a case dictionary: one single-sample group per kv0 state"""
    return [(name, [(spec[0], spec[1], st)]) for name, (_, spec, states) in cases.items() for st in states]



# ---- inputs, the float64 reference and the comparison (shared by test_gpu_decoder_edges.py and its child interpreter) ------
TOL = 1e-3          # test_gpu_model.TOL: per-point mask logits, relative to max(1, max|reference|) of the layer
TOL_PATHS = 1e-4    # two runs of the implementation on different launch geometry (test_gpu_decoder_leftover_tile.TOL_PATHS)
SEED_SHIFT = {"placement_no_point": 1}      # (see test_gpu_decoder_edges: the case asserts what the seed is there for)


def case_seed(name):
    return (zlib.crc32(name.encode()) + SEED_SHIFT.get(name, 0)) % (1 << 31)


def inputs(points, seed):
    """random decoder inputs: features [points, 128] and coordinates in a room-sized box"""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(points, 128, generator=g) * 0.5
    xyz = torch.rand(points, 3, generator=g) * torch.tensor([8.0, 6.0, 2.6])
    return feats, xyz


def clicks(points, spec, seed, n_bg=N_BG):
    """click dictionaries of (queries, objects[, variant]): queries - n_bg clicks on random rows (repeating once the rows
    run out) at distinct random times, dealt to the objects in turn; with more clicks than objects the last is a background
    click"""
    nq, k = spec[:2]
    variant = spec[2] if len(spec) > 2 else None
    g = torch.Generator().manual_seed(seed + 1)
    n_clicks = nq - n_bg
    assert 1 <= k <= n_clicks <= 200
    perm = torch.randperm(points, generator=g).tolist()
    rows = [perm[i % points] for i in range(n_clicks)]
    times = torch.randperm(200, generator=g)[:n_clicks].tolist()
    n_fg = n_clicks if n_clicks == k else n_clicks - 1
    owner = [1 + i % k for i in range(n_fg)] + [0] * (n_clicks - n_fg)
    if variant == "one_row":          # every click of object 1 on one row
        rows = [rows[0] if w == 1 else r for r, w in zip(rows, owner)]
        assert sum(w == 1 for w in owner) >= 2
    elif variant == "bg_on_fg":       # the background click on the row of a foreground click
        assert owner[-1] == 0 and owner[0] == 1
        rows[-1] = rows[0]
    elif variant == "times":          # the ends of the time table
        times[0], times[1] = 0, 199
    ci = {str(o): [r for r, w in zip(rows, owner) if w == o] for o in range(k + 1)}
    ct = {str(o): [t for t, w in zip(times, owner) if w == o] for o in range(k + 1)}
    return ci, ct


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def reference(sd, feats, xyz, ci, ct, force_masks=None):
    """oracle.decoder.forward_mask in the precision of ``sd``, position encoding included: the layers' logits"""
    dt = sd["pos_enc.gauss_B"].dtype
    x, f = xyz.to(dt), feats.to(dt)
    pe = od.fourier_pos_enc(x, sd["pos_enc.gauss_B"], x.min(0)[0], x.max(0)[0]).to(dt)
    out = od.forward_mask(sd, f, x, pe, ci, ct, force_masks=force_masks)
    assert all(o.dtype == dt for o in out)
    return out


def masks_from_logits(logits, ci, n_bg=N_BG):
    """mask_module's attention mask [queries, points] (True = blocked) from a layer's logits [points, 1 + objects]: a row
    that would be all True is lifted"""
    labels = logits.argmax(1)
    k = logits.shape[1] - 1
    rows = []
    for obj in list(range(1, k + 1)) + [0]:
        m = labels != obj
        if bool(m.all()):
            m = torch.zeros_like(m)
        rows.append(m.unsqueeze(0).repeat(len(ci[str(obj)]) + (n_bg if obj == 0 else 0), 1))
    return torch.cat(rows, 0)


def compare(name, got, sd64, sd32, feats, xyz, ci, ct, n_bg=N_BG):
    """The implementation's logits of every layer (``got``: list of [points, 1 + objects] arrays) against the float64
    reference.  Each layer's attention mask comes from the argmax of the previous layer's logits, so a near-tie forks the
    computation: the reference is run with the masks derived from the implementation's own logits (force_masks), and every
    layer must meet the bar against that run.  Separately, wherever the implementation's label differs from the label of the
    reference left to itself, the reference's top-two margin there must be below 2 TOL scale -- up to and including the
    first layer with such a flip (past it the free reference follows another branch).  Prints and returns the figures:
    (worst error / scale over the layers, flips, the float32 oracle's own worst distance / scale from float64)."""
    got = [torch.from_numpy(np.asarray(g)).double() for g in got]
    n_layers = len(got)
    masks = [masks_from_logits(g, ci, n_bg) for g in got]
    forced = reference(sd64, feats, xyz, ci, ct, force_masks=masks)
    free = reference(sd64, feats, xyz, ci, ct)
    f32 = reference(sd32, feats, xyz, ci, ct)
    assert len(forced) == n_layers
    worst, worst32, flips, forked = 0.0, 0.0, 0, False
    for i in range(n_layers):
        assert got[i].shape == forced[i].shape, (name, i, got[i].shape, forced[i].shape)
        assert bool(torch.isfinite(got[i]).all()), (name, i)
        scale = max(1.0, float(forced[i].abs().max()))
        err = float((got[i] - forced[i]).abs().max()) / scale
        worst = max(worst, err)
        worst32 = max(worst32, float((f32[i].double() - free[i]).abs().max()) / max(1.0, float(free[i].abs().max())))
        n_flip = 0
        if not forked:
            differ = got[i].argmax(1) != free[i].argmax(1)
            n_flip = int(differ.sum())
            if n_flip:
                top2 = free[i].topk(min(2, free[i].shape[1]), dim=1)[0]
                margin = float((top2[:, 0] - top2[:, -1])[differ].max())
                fscale = max(1.0, float(free[i].abs().max()))
                assert margin < 2 * TOL * fscale, (name, i, n_flip, margin, fscale)
                forked = True
            flips += n_flip
        print(f"{name}: layer {i} max|diff| / scale = {err:.2e} (scale {scale:.1f}), flips {n_flip}")
        assert err <= TOL, (name, i, err)
    print(f"EDGE {name} err {worst:.3e} flips {flips} f32 {worst32:.3e}")
    return worst, flips, worst32

# the class every (queries, objects, kv0 state) of the tables above is there for: the planner's answer at the time of writing
DECLARED = {
    (11, 1, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (11, 1, 1): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 1),
    (11, 1, 2): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (14, 2, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (16, 2, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (16, 3, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (16, 3, 1): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 1),
    (16, 3, 2): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (16, 6, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12>', '-', 0),
    (18, 3, 0): ('k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 0),
    (18, 4, 0): ('k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 0),
    (18, 4, 1): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,QC,LO>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 1),
    (18, 4, 2): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,QC,LO>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 0),
    (20, 10, 0): ('k_kv_c2s<2,LO>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,KG>', '-', 0),
    (20, 10, 1): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,KG,QC>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,KG>', '-', 1),
    (20, 10, 2): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,KG,QC>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,KG>', '-', 0),
    (21, 11, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (24, 2, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12>', '-', 0),
    (24, 2, 1): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,QC>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12>', '-', 1),
    (24, 2, 2): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,QC>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12>', '-', 0),
    (24, 5, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (27, 17, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (28, 5, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (28, 5, 1): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,KG,QC>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 1),
    (28, 5, 2): ('k_c2s_attn_b<2>', 'k_s2c_out<2,12,KG,QC>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (28, 18, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 0),
    (28, 18, 1): ('k_c2s_attn_b<2>', 'k_s2c_out<2,8,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 1),
    (28, 18, 2): ('k_c2s_attn_b<2>', 'k_s2c_out<2,8,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 0),
    (32, 2, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,12,KG>', '-', 0),
    (32, 22, 0): ('k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 'k_kv_c2s<2>', 'k_s2c_out<2,8,KG>', '-', 0),
    (33, 3, 0): ('k_c2s_w<5>', 'k_s2o_w<5>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (33, 3, 1): ('k_c2s_attn_b<3>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 1),
    (33, 3, 2): ('k_c2s_attn_b<3>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (64, 3, 0): ('k_c2s_w<5>', 'k_s2o_w<5>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (64, 3, 1): ('k_c2s_attn_b<4>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 1),
    (64, 3, 2): ('k_c2s_attn_b<4>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (65, 3, 0): ('k_c2s_w<5>', 'k_s2o_w<5>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (70, 3, 0): ('k_c2s_w<5>', 'k_s2o_w<5>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (70, 3, 1): ('k_c2s_attn_b<5>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 1),
    (70, 3, 2): ('k_c2s_attn_b<5>', 'k_s2o_w<5,QC>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (80, 3, 0): ('k_c2s_w<5>', 'k_s2o_w<5>', '-', 'k_c2s_w<5>', 'k_s2o_w<5>', '-', 0),
    (81, 3, 0): ('k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 'k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 0),
    (96, 3, 0): ('k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 'k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 0),
    (96, 3, 1): ('k_c2s_attn_b<6>', 'k_s2c_w<6,QC>', 'k_out_w<6>', 'k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 1),
    (96, 3, 2): ('k_c2s_attn_b<6>', 'k_s2c_w<6,QC>', 'k_out_w<6>', 'k_c2s_w<6>', 'k_s2c_w<6>', 'k_out_w<6>', 0),
    (97, 3, 0): ('k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 'k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 0),
    (112, 3, 0): ('k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 'k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 0),
    (112, 3, 1): ('k_c2s_attn_b<7>', 'k_s2c_w<7,QC>', 'k_out_w<7>', 'k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 1),
    (112, 3, 2): ('k_c2s_attn_b<7>', 'k_s2c_w<7,QC>', 'k_out_w<7>', 'k_c2s_w<7>', 'k_s2c_w<7>', 'k_out_w<7>', 0),
    (113, 3, 0): ('k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 'k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 0),
    (128, 3, 0): ('k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 'k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 0),
    (128, 3, 1): ('k_c2s_attn_b<8>', 'k_s2c_w<8,QC>', 'k_out_w<8>', 'k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 1),
    (128, 3, 2): ('k_c2s_attn_b<8>', 'k_s2c_w<8,QC>', 'k_out_w<8>', 'k_c2s_w<8>', 'k_s2c_w<8>', 'k_out_w<8>', 0),
    (129, 3, 0): ('k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 'k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 0),
    (160, 3, 0): ('k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 'k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 0),
    (160, 3, 1): ('k_c2s_attn_b<10>', 'k_s2c_w<10,QC>', 'k_out_w<10>', 'k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 1),
    (160, 3, 2): ('k_c2s_attn_b<10>', 'k_s2c_w<10,QC>', 'k_out_w<10>', 'k_c2s_w<10>', 'k_s2c_w<10>', 'k_out_w<10>', 0),
    (161, 3, 0): ('k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 'k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 0),
    (192, 3, 0): ('k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 'k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 0),
    (192, 3, 1): ('k_c2s_attn_b<12>', 'k_s2c_w<12,QC>', 'k_out_w<12>', 'k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 1),
    (192, 3, 2): ('k_c2s_attn_b<12>', 'k_s2c_w<12,QC>', 'k_out_w<12>', 'k_c2s_w<12>', 'k_s2c_w<12>', 'k_out_w<12>', 0),
    (193, 3, 0): ('k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 'k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 0),
    (210, 3, 0): ('k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 'k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 0),
    (210, 3, 1): ('k_c2s_attn_b<14>', 'k_s2c_w<14,QC>', 'k_out_w<14>', 'k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 1),
    (210, 3, 2): ('k_c2s_attn_b<14>', 'k_s2c_w<14,QC>', 'k_out_w<14>', 'k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 0),
    (210, 200, 0): ('k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 'k_c2s_w<14>', 'k_s2c_w<14>', 'k_out_w<14>', 0),
}
# the four samples of the mixed batch share one launch group
DECLARED_MIXED = ('k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 'k_kv_c2s<2,LO>', 'k_s2c_out<2,12,LO>', '-', 0)
# A3D_WIDE_FROM=65: the classes of 33 .. 64 queries, which the child run of test_gpu_decoder_edges.py reaches
DECLARED_WIDE65 = {
    (33, 3, 0): ('k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 0),
    (33, 3, 1): ('k_c2s_attn_b<3>', 'k_q_s2c<3,QC>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 1),
    (33, 3, 2): ('k_c2s_attn_b<3>', 'k_q_s2c<3,QC>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 0),
    (48, 3, 0): ('k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 0),
    (48, 3, 1): ('k_c2s_attn_b<3>', 'k_q_s2c<3,QC>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 1),
    (48, 3, 2): ('k_c2s_attn_b<3>', 'k_q_s2c<3,QC>', 'k_out_ln_mask<3>', 'k_kv_c2s<3>', 'k_q_s2c<3>', 'k_out_ln_mask<3>', 0),
    (49, 3, 0): ('k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 0),
    (49, 3, 1): ('k_c2s_attn_b<4>', 'k_q_s2c<4,QC>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 1),
    (49, 3, 2): ('k_c2s_attn_b<4>', 'k_q_s2c<4,QC>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 0),
    (64, 3, 0): ('k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 0),
    (64, 3, 1): ('k_c2s_attn_b<4>', 'k_q_s2c<4,QC>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 1),
    (64, 3, 2): ('k_c2s_attn_b<4>', 'k_q_s2c<4,QC>', 'k_out_ln_mask<4>', 'k_kv_c2s<4>', 'k_q_s2c<4>', 'k_out_ln_mask<4>', 0),
}
# the model with one learned background query (ONE_BG_CASE)
DECLARED_ONE_BG = {
    (16, 15, 0): ('k_kv_c2s<1>', 'k_s2c_out<1,12,KG>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12,KG>', '-', 0),
    (16, 15, 1): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,KG,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12,KG>', '-', 1),
    (16, 15, 2): ('k_c2s_attn_b<1>', 'k_s2c_out<1,12,KG,QC>', '-', 'k_kv_c2s<1>', 'k_s2c_out<1,12,KG>', '-', 0),
}
# classes that only the A3D_WIDE_FROM=65 sweep reaches and no child case runs -> the existing test that covers each
CITED_WIDE65 = {}
