"""The case table of test_gpu_conv_edges.py and the host-side planner sweep that test_conv_plan_classes.py holds it against.

A PLAN CLASS is what plan_conv (csrc/spconv.hip) decides for an op, reduced to what selects code:
    ("wl", K)                                                           k_conv_wl
    ("sk", K, bn, ch, pair, handoff, gcap, pass2)                       k_conv_sk: the build, shares cut inside tiles or not,
                                                                        G at the resident-workgroup cap, a cout % 128 == 0
                                                                        layer run with 64 columns
    ("deep", K, bn, ch, D, P > 1, G > 256)                              k_conv_deep
and, for an op with a fused projection or head, one more field: fused_ok / head_ok.
Nothing here needs a GPU."""
import os
import shutil
import subprocess

from conv_kit import KVOL, SCENE_LEVELS, SCENES, level_out  # noqa: F401  (the tables' users read them from here too)
from oracle import backbone as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPCONV = os.path.join(ROOT, "agile3d_amd", "csrc", "spconv.hip")
PLAN_MAIN = os.path.join(ROOT, "tests", "conv_plan_main.cpp")
BLOCK_BEGIN, BLOCK_END = "// ---- planning:", "// ---- end of planning"

WIDTHS_IN = [32, 64, 96, 128, 192, 256, 384]      # test_gpu_conv.py's _WIDTHS_IN x _WIDTHS_OUT
WIDTHS_OUT = [32, 64, 96, 128, 256]
KIND_LEVELS = [(kind, lvl) for kind in ("conv3", "down", "up") for lvl in range(5)
               if not (kind == "down" and lvl == 4) and not (kind == "up" and lvl == 0)]

SMALL_SCENES = ["one", "line37", "box63", "box64", "box65", "box128", "outlier", "two_batch", "s1500"]
LARGE_SCENES = ["box8191", "box8192", "g1024", "g1025", "s20000"]

# fused projection: the network's six (cin, cout, cin2); 96 -> 64 (+64), whose 96-channel stages do not divide the projection's
# input: the planner reruns it with 32-channel stages, which have a fused build; and 96 -> 64 (+96), which keeps the 96-channel
# stages and has none: the program runs it as two launches
PROJ_SHAPES = [(64, 64, 32), (128, 128, 64), (256, 256, 128), (256, 256, 384), (128, 128, 192), (96, 96, 128), (96, 64, 64),
               (96, 64, 96)]
PROJ_SMALL_SCENES = ["one", "line37", "box65", "two_batch"]       # every level
PROJ_LARGE_SCENES = ["box8191", "box8192", "s20000"]              # level 0 (other levels: rows of LARGE_CASES)
HEAD_SHAPES = [(96, 96, 128), (128, 96, 128)]      # (cin, cout, head columns), level 0
HEAD_SCENES = ["one", "line37", "box65", "two_batch", "box8192", "s20000"]
WL_SCENES = ["one", "line37", "box64", "g1024", "g1025", "g2047", "g2048"]      # 32 -> 32 conv3 and down at level 0


_LEVELS = {}


def oracle_levels(name):
    """rows per level of a named scene, from the CPU oracle"""
    if name not in _LEVELS:
        lv = ob.SparseLevels(SCENES[name]())
        _LEVELS[name] = [lv.n(i) for i in range(5)]
    return _LEVELS[name]


def op_query(levels, kind, level_in, cin, cout, mode, cin2=0, head=0, stats=0):
    """the planner's view of an op: (n_out, K, cin, cout, cin2, head_cout, up, mode, stats); stats as ConvShape.stats: 0 the
    inference build, 1 a3d_conv_bn_train_forward's, 2 a3d_conv_dgrad_bn's"""
    return (levels[level_out(kind, level_in)], KVOL[kind], cin, cout, cin2, head, int(kind == "up"), mode, stats)


# ---- the planner as a host program ---------------------------------------------------------------------------------
def planning_block():
    text = open(SPCONV).read()
    a, b = text.index(BLOCK_BEGIN), text.index(BLOCK_END)
    assert 0 <= a < b and text.count(BLOCK_BEGIN) == 1 and text.count(BLOCK_END) == 1
    return text[a:b]


def host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    raise RuntimeError("no host C++ compiler (the build needs one)")


def build_planner(workdir):
    """compiles conv_plan_main.cpp around the planning block cut from spconv.hip; returns the program's path"""
    with open(os.path.join(workdir, "conv_planning_block.inc"), "w") as f:
        f.write(planning_block())
    exe = os.path.join(workdir, "conv_plan")
    subprocess.run([host_compiler(), "-O2", "-std=c++17", "-I", workdir, PLAN_MAIN, "-o", exe], check=True, capture_output=True,
                   text=True)
    return exe


_FIELDS = ("family", "K", "bn", "ch", "pair", "handoff", "gcap", "pass2", "D", "P", "G", "fused_ok", "head_ok", "ntile", "n_cblk")


def run_planner(exe, queries):
    """plans (dicts of _FIELDS) of a list of op_query tuples"""
    text = "".join(" ".join(str(int(v)) for v in q) + "\n" for q in queries)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    plans = []
    for line in out[:len(queries)]:
        parts = line.split()
        plans.append({k: (parts[0] if k == "family" else int(v)) for k, v in zip(_FIELDS, parts)})
    assert len(plans) == len(queries)
    return plans


def plan_class(plan, query):
    """the class tuple of the module docstring"""
    f, K = plan["family"], plan["K"]
    if f == "wl":
        cls = ("wl", K)
    elif f == "sk":
        cls = ("sk", K, plan["bn"], plan["ch"], plan["pair"], plan["handoff"], plan["gcap"], plan["pass2"])
    else:
        cls = ("deep", K, plan["bn"], plan["ch"], plan["D"], int(plan["P"] > 1), int(plan["G"] > 256))
    if query[4] > 0:
        cls += ("proj", plan["fused_ok"])
    if query[5] > 0:
        cls += ("head", plan["head_ok"])
    return cls


def full_sweep_queries():
    """kinds x levels x widths over every scene and both modes, plus the fused shapes: what is REACHABLE on these scenes"""
    qs = []
    for name in SMALL_SCENES + LARGE_SCENES:
        lv = oracle_levels(name)
        for mode in (1, 0):
            for kind, level_in in KIND_LEVELS:
                qs += [op_query(lv, kind, level_in, ci, co, mode) for ci in WIDTHS_IN for co in WIDTHS_OUT]
            for level in range(5):
                qs += [op_query(lv, "conv3", level, ci, co, mode, cin2=c2) for ci, co, c2 in PROJ_SHAPES]
            qs += [op_query(lv, "conv3", 0, ci, co, mode, head=h) for ci, co, h in HEAD_SHAPES]
    for name in ("g2047", "g2048"):
        lv = oracle_levels(name)
        qs += [op_query(lv, kind, 0, 32, 32, mode) for kind in ("conv3", "down") for mode in (1, 0) if kind == "conv3" or len(lv) > 1]
    return qs


# ---- the cases ------------------------------------------------------------------------------------------------------
# A row: ((scene, kind, level_in, cin, cout, cin2, mode), the plan class it is there for).  mode: a3d_conv_deep_mode.
# test_conv_plan_classes.py asserts that every row plans to its class and that, with the sweeps below, no class reachable
# on these scenes is without a case.  The trailing comments (workgroups, parts per tile, 64-row tiles) are the planner's at
# the time of writing.
LARGE_CASES = [
    (("box8191", "conv3", 0, 32, 128, 0, 0), ("sk", 27, 128, 32, 0, 1, 0, 0)),   # G 256 P 0 tiles 128
    (("box8191", "conv3", 0, 128, 256, 0, 1), ("sk", 27, 128, 32, 0, 1, 1, 0)),   # G 512 P 0 tiles 128
    (("box8191", "conv3", 0, 256, 64, 0, 1), ("sk", 27, 64, 64, 0, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("box8191", "conv3", 0, 256, 64, 0, 0), ("sk", 27, 64, 64, 0, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("box8191", "conv3", 0, 384, 64, 0, 1), ("sk", 27, 64, 96, 0, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("box8191", "conv3", 0, 384, 64, 0, 0), ("sk", 27, 64, 96, 0, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("box8191", "up", 1, 256, 96, 0, 0), ("sk", 8, 96, 32, 1, 1, 1, 0)),   # G 1020 P 0 tiles 128
    (("box8192", "conv3", 0, 32, 128, 0, 0), ("sk", 27, 128, 32, 1, 1, 0, 0)),   # G 256 P 0 tiles 128
    (("box8192", "conv3", 0, 128, 256, 0, 1), ("sk", 27, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("box8192", "conv3", 1, 32, 96, 0, 1), ("deep", 27, 32, 32, 3, 0, 1)),   # G 297 P 1 tiles 99
    (("box8192", "conv3", 1, 256, 64, 0, 1), ("sk", 27, 64, 64, 0, 1, 0, 0)),   # G 668 P 0 tiles 99
    (("box8192", "down", 0, 32, 256, 0, 0), ("sk", 8, 128, 32, 0, 0, 0, 0)),   # G 198 P 0 tiles 99
    (("box8192", "down", 0, 192, 256, 0, 1), ("sk", 8, 128, 32, 0, 0, 0, 0)),   # G 198 P 0 tiles 99
    (("box8192", "down", 0, 384, 96, 0, 1), ("sk", 8, 96, 32, 1, 1, 1, 0)),   # G 1020 P 0 tiles 99
    (("box8192", "up", 1, 32, 128, 0, 0), ("sk", 8, 128, 32, 1, 1, 0, 0)),   # G 256 P 0 tiles 128
    (("box8192", "up", 1, 32, 256, 0, 0), ("sk", 8, 128, 32, 1, 0, 0, 0)),   # G 256 P 0 tiles 128
    (("box8192", "up", 1, 192, 128, 0, 0), ("sk", 8, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 128
    (("g1024", "conv3", 0, 32, 96, 0, 1), ("sk", 27, 96, 32, 1, 1, 0, 0)),   # G 512 P 0 tiles 256
    (("g1024", "conv3", 0, 256, 32, 0, 1), ("sk", 27, 32, 64, 0, 1, 1, 0)),   # G 1020 P 0 tiles 256
    (("g1024", "conv3", 1, 96, 128, 0, 1), ("sk", 27, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 157
    (("g1024", "conv3", 1, 96, 128, 0, 0), ("sk", 27, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 157
    (("g1024", "conv3", 1, 128, 96, 0, 1), ("sk", 27, 96, 32, 1, 1, 1, 0)),   # G 1020 P 0 tiles 157
    (("g1024", "conv3", 1, 128, 96, 0, 0), ("sk", 27, 96, 32, 1, 1, 1, 0)),   # G 1020 P 0 tiles 157
    (("g1024", "conv3", 1, 256, 32, 0, 0), ("sk", 27, 32, 64, 0, 1, 1, 0)),   # G 1020 P 0 tiles 157
    (("g1024", "conv3", 1, 384, 32, 0, 1), ("sk", 27, 32, 96, 0, 1, 1, 0)),   # G 1020 P 0 tiles 157
    (("g1024", "conv3", 1, 384, 32, 0, 0), ("sk", 27, 32, 96, 0, 1, 1, 0)),   # G 1020 P 0 tiles 157
    (("g1024", "down", 0, 192, 128, 0, 1), ("sk", 8, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 157
    (("g1024", "down", 0, 384, 64, 0, 1), ("sk", 8, 64, 96, 0, 1, 0, 0)),   # G 667 P 0 tiles 157
    (("g1024", "up", 1, 32, 64, 0, 0), ("sk", 8, 64, 32, 0, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 32, 96, 0, 1), ("sk", 8, 96, 32, 1, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 32, 96, 0, 0), ("sk", 8, 96, 32, 1, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 64, 32, 0, 0), ("sk", 8, 32, 64, 0, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 64, 64, 0, 0), ("sk", 8, 64, 64, 0, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 96, 32, 0, 0), ("sk", 8, 32, 96, 0, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1024", "up", 1, 96, 64, 0, 0), ("sk", 8, 64, 96, 0, 0, 0, 0)),   # G 256 P 0 tiles 256
    (("g1025", "conv3", 0, 32, 64, 0, 1), ("deep", 27, 64, 32, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "conv3", 0, 32, 128, 0, 1), ("deep", 27, 128, 32, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "conv3", 0, 64, 32, 0, 1), ("deep", 27, 32, 64, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "conv3", 0, 64, 64, 0, 1), ("deep", 27, 64, 64, 2, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "up", 1, 32, 64, 0, 1), ("deep", 8, 64, 32, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "up", 1, 32, 128, 0, 1), ("deep", 8, 128, 32, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "up", 1, 32, 256, 0, 1), ("sk", 8, 128, 32, 1, 0, 0, 0)),   # G 514 P 0 tiles 257
    (("g1025", "up", 1, 64, 32, 0, 1), ("deep", 8, 32, 64, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("g1025", "up", 1, 64, 64, 0, 1), ("deep", 8, 64, 64, 2, 0, 1)),   # G 257 P 1 tiles 257
    (("s20000", "conv3", 0, 128, 96, 0, 0), ("sk", 27, 96, 32, 1, 1, 1, 0)),   # G 1020 P 0 tiles 315
    (("s20000", "conv3", 0, 384, 256, 0, 1), ("sk", 27, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 315
    (("s20000", "conv3", 0, 384, 256, 0, 0), ("sk", 27, 128, 32, 1, 1, 1, 0)),   # G 768 P 0 tiles 315
    (("s20000", "conv3", 1, 32, 64, 0, 1), ("deep", 27, 32, 32, 3, 1, 1)),   # G 408 P 3 tiles 68
    (("s20000", "conv3", 1, 32, 256, 0, 1), ("deep", 27, 128, 32, 3, 1, 1)),   # G 408 P 3 tiles 68
    (("s20000", "conv3", 1, 384, 64, 0, 1), ("sk", 27, 64, 96, 0, 1, 0, 0)),   # G 459 P 0 tiles 68
    (("s20000", "conv3", 3, 32, 128, 0, 0), ("sk", 27, 64, 32, 0, 1, 0, 1)),   # G 24 P 0 tiles 3
    (("s20000", "down", 0, 32, 64, 0, 0), ("sk", 8, 64, 32, 0, 1, 0, 0)),   # G 187 P 0 tiles 68
    (("s20000", "down", 0, 64, 256, 0, 1), ("deep", 8, 128, 32, 3, 1, 1)),   # G 408 P 3 tiles 68
    (("s20000", "down", 0, 256, 256, 0, 1), ("sk", 8, 128, 32, 0, 1, 1, 0)),   # G 512 P 0 tiles 68
    (("s20000", "up", 1, 96, 96, 0, 0), ("sk", 8, 96, 32, 1, 0, 0, 0)),   # G 315 P 0 tiles 315
    (("s20000", "up", 2, 32, 128, 0, 1), ("deep", 8, 32, 32, 3, 0, 1)),   # G 272 P 1 tiles 68
    (("s20000", "up", 4, 64, 256, 0, 0), ("sk", 8, 64, 64, 0, 1, 0, 1)),   # G 30 P 0 tiles 3
]

# epilogues (scale, shift, residual, ReLU, padded column slices) and in-place accumulation: every reachable build of
# k_conv_sk and k_conv_deep on a small and on a large scene where both exist (the low-register 128-column builds need 8192
# rows, the 32-column stream-K build with 32-channel stages is k_conv_wl's shape), and k_conv_wl
EPI_CASES = [
    (("two_batch", "conv3", 0, 64, 32, 0, 0), ("sk", 27, 32, 64, 0, 1, 0, 0)),   # G 116 P 0 tiles 29
    (("s20000", "down", 1, 64, 32, 0, 0), ("sk", 8, 32, 64, 0, 1, 0, 0)),   # G 41 P 0 tiles 15
    (("two_batch", "conv3", 0, 96, 32, 0, 0), ("sk", 27, 32, 96, 0, 1, 0, 0)),   # G 116 P 0 tiles 29
    (("s20000", "down", 1, 96, 32, 0, 0), ("sk", 8, 32, 96, 0, 1, 0, 0)),   # G 41 P 0 tiles 15
    (("two_batch", "conv3", 0, 32, 64, 0, 0), ("sk", 27, 64, 32, 0, 1, 0, 0)),   # G 116 P 0 tiles 29
    (("s20000", "down", 1, 32, 64, 0, 0), ("sk", 8, 64, 32, 0, 1, 0, 0)),   # G 41 P 0 tiles 15
    (("two_batch", "conv3", 0, 64, 64, 0, 0), ("sk", 27, 64, 64, 0, 1, 0, 0)),   # G 108 P 0 tiles 29
    (("s20000", "down", 1, 64, 64, 0, 0), ("sk", 8, 64, 64, 0, 1, 0, 0)),   # G 37 P 0 tiles 15
    (("two_batch", "conv3", 0, 96, 64, 0, 0), ("sk", 27, 64, 96, 0, 1, 0, 0)),   # G 108 P 0 tiles 29
    (("s20000", "down", 1, 96, 64, 0, 0), ("sk", 8, 64, 96, 0, 1, 0, 0)),   # G 37 P 0 tiles 15
    (("two_batch", "conv3", 0, 32, 96, 0, 0), ("sk", 27, 96, 32, 1, 1, 0, 0)),   # G 116 P 0 tiles 29
    (("s20000", "down", 1, 32, 96, 0, 0), ("sk", 8, 96, 32, 1, 1, 0, 0)),   # G 41 P 0 tiles 15
    (("two_batch", "conv3", 0, 96, 128, 0, 0), ("sk", 27, 128, 32, 0, 1, 0, 0)),   # G 256 P 0 tiles 29
    (("box8191", "up", 1, 32, 128, 0, 0), ("sk", 8, 128, 32, 0, 1, 0, 0)),   # G 256 P 0 tiles 128
    (("box8192", "up", 1, 32, 128, 0, 0), ("sk", 8, 128, 32, 1, 1, 0, 0)),   # G 256 P 0 tiles 128
    (("g1025", "up", 1, 32, 128, 0, 1), ("deep", 8, 128, 32, 3, 0, 1)),   # G 257 P 1 tiles 257
    (("two_batch", "conv3", 0, 128, 256, 0, 1), ("deep", 27, 64, 64, 2, 1, 1)),   # G 464 P 4 tiles 29
    (("s20000", "down", 0, 64, 128, 0, 1), ("deep", 8, 64, 64, 2, 1, 1)),   # G 408 P 3 tiles 68
    (("two_batch", "conv3", 0, 96, 128, 0, 1), ("deep", 27, 64, 32, 3, 1, 1)),   # G 464 P 8 tiles 29
    (("s20000", "down", 0, 32, 128, 0, 1), ("deep", 8, 64, 32, 3, 1, 1)),   # G 408 P 3 tiles 68
    (("two_batch", "conv3", 0, 64, 32, 0, 1), ("deep", 27, 32, 64, 3, 1, 0)),   # G 232 P 8 tiles 29
    (("s20000", "down", 1, 64, 32, 0, 1), ("deep", 8, 32, 64, 3, 1, 0)),   # G 60 P 4 tiles 15
    (("two_batch", "conv3", 0, 32, 64, 0, 1), ("deep", 27, 32, 32, 3, 1, 0)),   # G 232 P 4 tiles 29
    (("s20000", "down", 1, 32, 64, 0, 1), ("deep", 8, 32, 32, 3, 1, 0)),   # G 120 P 4 tiles 15
    (("box64", "conv3", 0, 32, 32, 0, 0), ("wl", 27)),
    (("g1025", "conv3", 0, 32, 32, 0, 1), ("wl", 27)),
]


# ---- rows of the training builds alone (test_gpu_conv_train_edges.py; plan_conv reads ConvShape.stats only to add LDS and to
# forbid the fused head -- test_conv_plan_classes.py holds that -- so the tables above serve STATS = 1 and 2 as they stand)
# 1x1 layers (A3D_OP_LINEAR, K = 1; the training path runs them with statistics): whole tiles, no hand-off, no kernel map
LINEAR_CASES = [
    (("box65", "linear", 0, 128, 96, 0, 1), ("sk", 1, 96, 32, 1, 0, 0, 0)),   # G 2 P 0 tiles 2
    (("box65", "linear", 0, 128, 96, 0, 0), ("sk", 1, 96, 32, 1, 0, 0, 0)),
    (("two_batch", "linear", 3, 384, 256, 0, 1), ("sk", 1, 128, 32, 0, 0, 0, 0)),   # G 14 P 0 tiles 7
    (("two_batch", "linear", 3, 384, 256, 0, 0), ("sk", 1, 128, 32, 0, 0, 0, 0)),
    (("s20000", "linear", 2, 32, 64, 0, 1), ("sk", 1, 64, 32, 0, 0, 0, 0)),   # G 15 P 0 tiles 15
    (("s20000", "linear", 2, 32, 64, 0, 0), ("sk", 1, 64, 32, 0, 0, 0, 0)),
    # k_conv_sk<32, 32, 0>: with a kernel map 32 -> 32 is k_conv_wl's, so only a 1x1 layer runs this build
    (("box65", "linear", 0, 32, 32, 0, 1), ("sk", 1, 32, 32, 0, 0, 0, 0)),   # G 2 P 0 tiles 2
    (("box65", "linear", 0, 32, 32, 0, 0), ("sk", 1, 32, 32, 0, 0, 0, 0)),
    (("s20000", "linear", 0, 32, 32, 0, 1), ("sk", 1, 32, 32, 0, 0, 0, 0)),   # G 315 P 0 tiles 315
    (("s20000", "linear", 0, 32, 32, 0, 0), ("sk", 1, 32, 32, 0, 0, 0, 0)),
]
# 63 / 64 per-block partials: below 64 blocks bn_sums_from_partials folds them with k_col_final<16, 1>, from 64 on with
# k_col_final<256, 4> (bnorm.hip: 16 or 256 block lanes per column).  64-row tiles of k_conv_sk / k_conv_deep on box4032 / box4096, 16-row groups of k_conv_wl
# on box1008 / box1024; level 0 only, not part of SMALL_SCENES / LARGE_SCENES (the reachability sweep keeps its meaning)
TRAIN_BOX_CASES = [
    (("box1008", "conv3", 0, 32, 32, 0, 1), ("wl", 27)),
    (("box1008", "conv3", 0, 32, 32, 0, 0), ("wl", 27)),
    (("box1024", "conv3", 0, 32, 32, 0, 1), ("wl", 27)),
    (("box1024", "conv3", 0, 32, 32, 0, 0), ("wl", 27)),
    (("box4032", "conv3", 0, 32, 64, 0, 1), ("deep", 27, 32, 32, 3, 1, 1)),   # G 504 P 4 tiles 63
    (("box4032", "conv3", 0, 32, 64, 0, 0), ("sk", 27, 64, 32, 0, 1, 0, 0)),   # G 252 P 0 tiles 63
    (("box4032", "conv3", 0, 96, 96, 0, 1), ("deep", 27, 32, 32, 3, 1, 1)),   # G 378 P 2 tiles 63
    (("box4032", "conv3", 0, 96, 96, 0, 0), ("sk", 27, 96, 32, 1, 1, 0, 0)),   # G 330 P 0 tiles 63
    (("box4096", "conv3", 0, 32, 64, 0, 1), ("deep", 27, 32, 32, 3, 1, 1)),   # G 512 P 4 tiles 64
    (("box4096", "conv3", 0, 32, 64, 0, 0), ("sk", 27, 64, 32, 0, 1, 0, 0)),   # G 256 P 0 tiles 64
    (("box4096", "conv3", 0, 96, 96, 0, 1), ("deep", 27, 32, 32, 3, 1, 1)),   # G 384 P 2 tiles 64
    (("box4096", "conv3", 0, 96, 96, 0, 0), ("sk", 27, 96, 32, 1, 1, 0, 0)),   # G 336 P 0 tiles 64
]
TRAIN_CASES = LINEAR_CASES + TRAIN_BOX_CASES


def small_sweep_rows():
    """(scene, kind, level_in, cin, cout, 0, mode): the full width sets on every small scene"""
    return [(name, kind, lvl, ci, co, 0, mode) for name in SMALL_SCENES for mode in (1, 0) for kind, lvl in KIND_LEVELS
            for ci in WIDTHS_IN for co in WIDTHS_OUT]


def wl_rows():
    return [(name, kind, 0, 32, 32, 0, mode) for name in WL_SCENES for mode in (1, 0) for kind in ("conv3", "down")]


def proj_rows():
    rows = [(name, "conv3", lvl, ci, co, c2, mode) for name in PROJ_SMALL_SCENES for lvl in range(5) for mode in (1, 0)
            for ci, co, c2 in PROJ_SHAPES]
    return rows + [(name, "conv3", 0, ci, co, c2, mode) for name in PROJ_LARGE_SCENES for mode in (1, 0) for ci, co, c2 in PROJ_SHAPES]


def head_rows():
    """(row, head columns)"""
    return [((name, "conv3", 0, ci, co, 0, mode), h) for name in HEAD_SCENES for mode in (1, 0) for ci, co, h in HEAD_SHAPES]


def row_query(row, head=0, stats=0):
    name, kind, level_in, cin, cout, cin2, mode = row
    return op_query(oracle_levels(name), kind, level_in, cin, cout, mode, cin2, head, stats)


def all_case_queries():
    """the planner queries of every case test_gpu_conv_edges.py runs"""
    qs = [row_query(r) for r in small_sweep_rows() + wl_rows() + proj_rows()]
    qs += [row_query(r, h) for r, h in head_rows()]
    return qs + [row_query(r) for r, _ in LARGE_CASES + EPI_CASES]
