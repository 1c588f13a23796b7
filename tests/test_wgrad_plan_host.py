"""The planner of the weight gradient (csrc/wgrad.hip) on the CPU (no GPU).

The planning block of wgrad.hip (between its two marker lines) is plain C++; it is compiled here around
tests/wgrad_plan_main.cpp with the host compiler and asked for the plans of a seeded sweep: every (cin, cout) of the multiples
of 32 up to 1024, K in {1, 8, 27}, 1 .. 65536 groups, random per-offset counts with an empty offset, and the forced segment
lengths 1 and 3 of A3D_WGRAD_SEG.  Every plan must name a build of A3D_WGRAD_BUILDS, its tables must be the consistent cut of
its counts, and k_wgrad's own decoding of (XCD, item) must reach every segment exactly once.  The (cin, cout) -> build table
that the GPU modules rely on (test_gpu_train_primitives.py, test_gpu_wgrad_edges.py) is pinned here."""
import os
import re
import subprocess

import numpy as np
import pytest

from conv_edge_cases import BLOCK_BEGIN, BLOCK_END, ROOT, host_compiler

WGRAD = os.path.join(ROOT, "agile3d_amd", "csrc", "wgrad.hip")
PLAN_MAIN = os.path.join(ROOT, "tests", "wgrad_plan_main.cpp")
GROUPS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 100, 255, 256, 257, 1000, 1259, 4096, 5000, 20000, 65535, 65536]
N_HEAD = 8                                                   # ok cx cy nblocks seg_len slots grid_items part_bytes


def planning_block():
    text = open(WGRAD).read()
    assert text.count(BLOCK_BEGIN) == 1 and text.count(BLOCK_END) == 1
    a, b = text.index(BLOCK_BEGIN), text.index(BLOCK_END)
    assert 0 <= a < b
    return text[a:b]


def builds():
    """the (cx, cy) of A3D_WGRAD_BUILDS, read from wgrad.hip"""
    line = re.search(r"#define A3D_WGRAD_BUILDS\(V\)(.*)\n", open(WGRAD).read()).group(1)
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"V\(([^)]*)\)", line)]


def build_planner(workdir, extra=()):
    """compiles wgrad_plan_main.cpp around the planning block cut from wgrad.hip; returns the program's path"""
    with open(os.path.join(workdir, "wgrad_planning_block.inc"), "w") as f:
        f.write(planning_block())
    exe = os.path.join(workdir, "wgrad_plan")
    subprocess.run([host_compiler(), "-O2", "-std=c++17", *extra, "-I", workdir, "-I", os.path.join(ROOT, "include"), PLAN_MAIN, "-o", exe],
                   check=True, capture_output=True, text=True)
    return exe


def sweep_queries():
    """(cin, cout, K, ngroups, seg, counts or None): K = 1 without counts (every group: the linear entry points and 1x1
    maps), K = 8 / 27 with counts in 0 .. ngroups of which one is 0 and one is ngroups."""
    rng = np.random.default_rng(20240607)
    widths = list(range(32, 1025, 32))

    def one(cin, cout, K, ng, seg):
        if K == 1:
            return (cin, cout, K, ng, seg, None)
        c = np.zeros(27, np.int64)
        c[:K] = rng.integers(0, ng + 1, K)
        full, empty = rng.choice(K, 2, replace=False)
        c[full], c[empty] = ng, 0
        return (cin, cout, K, ng, seg, tuple(int(v) for v in c))
    q = []
    for cin in widths:
        for cout in widths:
            for K in (1, 8, 27):
                for ng in rng.choice(GROUPS, 3, replace=False):
                    q.append(one(cin, cout, K, int(ng), 0))
    for cin in (32, 64, 96, 128, 256, 1024):                 # A3D_WGRAD_SEG = 1, 3: segments of one group, and of three
        for cout in (32, 64, 96, 128, 256, 1024):
            for K in (1, 8, 27):
                for ng in (1, 2, 5, 17, 100, 1259):
                    for seg in (1, 3):
                        q.append(one(cin, cout, K, ng, seg))
    return q


def query_text(queries):
    return "".join(f"plan {ci} {co} {K} {ng} {seg} " + ("0" if c is None else "1 " + " ".join(map(str, c))) + "\n"
                   for ci, co, K, ng, seg, c in queries)


def run_planner(exe, queries):
    """-> list of None (refused) or dict(cx, cy, nblocks, seg_len, slots, grid_items, part_bytes, cnt[27], base[28],
    xbase[8, 28], seg_lo[27, 9])"""
    out = subprocess.run([exe], input=query_text(queries), capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= len(queries)
    plans = []
    for line in out[:len(queries)]:
        if not line.startswith("1 "):
            plans.append(None)
            continue
        v = np.array(line.split(), dtype=np.int64)
        assert len(v) == N_HEAD + 27 + 28 + 8 * 28 + 27 * 9
        p = dict(zip(("cx", "cy", "nblocks", "seg_len", "slots", "grid_items", "part_bytes"), (int(x) for x in v[1:N_HEAD])))
        t = v[N_HEAD:]
        p["cnt"], p["base"], p["xbase"], p["seg_lo"] = t[:27], t[27:55], t[55:55 + 224].reshape(8, 28), t[55 + 224:].reshape(27, 9)
        plans.append(p)
    return plans


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(str(tmp_path_factory.mktemp("wgrad_plan")))


@pytest.fixture(scope="module")
def sweep(planner):
    q = sweep_queries()
    return q, run_planner(planner, q)


def test_the_sweep_is_as_wide_as_it_says(sweep):
    q, plans = sweep
    assert len(q) >= 8484 and all(p is not None for p in plans), "a plan of the sweep was refused"
    assert {x[0] for x in q} == set(range(32, 1025, 32)) == {x[1] for x in q} and {x[2] for x in q} == {1, 8, 27}
    assert {x[3] for x in q} >= {1, 65536} and {x[4] for x in q} == {0, 1, 3}
    assert all(0 in x[5][:x[2]] for x in q if x[5] is not None)


def test_every_plan_names_a_build_and_every_build_is_reached(sweep):
    b = builds()
    assert len(b) == 13 and len(set(b)) == 13
    q, plans = sweep
    reached = {(p["cx"], p["cy"]) for p in plans}
    assert reached == set(b), (sorted(reached - set(b)), sorted(set(b) - reached))
    for (cin, cout, *_), p in zip(q, plans):
        assert cin % (16 * p["cx"]) == 0 and cout % (16 * p["cy"]) == 0
        assert p["nblocks"] == (cin // (16 * p["cx"])) * (cout // (16 * p["cy"]))


def test_the_tables_are_the_cut_of_the_counts(sweep):
    """per offset: seg_lo[k][0] = 0, seg_lo[k][8] = base[k + 1] - base[k] = ceil(cnt[k] / seg_len), the eighths do not
    decrease; the XCDs' item counts sum to base[27] and grid_items is the largest; part_bytes = slots * cin * cout * 4"""
    q, plans = sweep
    most_slots = 0
    for (cin, cout, K, ng, seg, counts), p in zip(q, plans):
        where = (cin, cout, K, ng, seg)
        want = np.zeros(27, np.int64)
        want[:K] = ng if counts is None else counts[:K]
        assert np.array_equal(p["cnt"], want), where
        L = p["seg_len"]
        assert L >= 1 and (seg == 0 or L == min(seg, max(1, int(want.max())))), where
        nseg = -(-want // L)
        assert p["base"][0] == 0 and np.array_equal(np.diff(p["base"]), nseg), where
        assert not p["seg_lo"][:, 0].any() and np.array_equal(p["seg_lo"][:, 8], nseg), where
        assert (np.diff(p["seg_lo"], axis=1) >= 0).all(), where
        assert not p["xbase"][:, 0].any() and np.array_equal(np.diff(p["xbase"], axis=1), np.diff(p["seg_lo"], axis=1).T), where
        assert p["xbase"][:, 27].sum() == p["base"][27] and p["grid_items"] == p["xbase"][:, 27].max(), where
        assert p["slots"] == max(1, int(p["base"][27])) and p["part_bytes"] == p["slots"] * cin * cout * 4, where
        if seg == 0:
            most_slots = max(most_slots, p["slots"])
    assert most_slots <= 2048, most_slots                       # kMaxSlots of the search (or every list as one segment: <= 27)
    print(f"{len(plans)} plans, at most {most_slots} partial slots without a forced segment length")


def test_the_kernel_s_decoding_reaches_every_segment_once(sweep):
    """The first lines of k_wgrad: workgroup b is item b / 8 of XCD b % 8, leaves if item >= xbase[x][27], else
    k = #{kk in 1 .. 26: item >= xbase[x][kk]}, seg = seg_lo[k][x] + item - xbase[x][k], slot = base[k] + seg."""
    q, plans = sweep
    for query, p in zip(q, plans):
        slots = []
        for x in range(8):
            item = np.arange(p["grid_items"])
            item = item[item < p["xbase"][x, 27]]
            k = (item[:, None] >= p["xbase"][x, 1:27][None, :]).sum(1)
            seg = p["seg_lo"][k, x] + item - p["xbase"][x, k]
            assert ((seg >= 0) & (seg < p["base"][k + 1] - p["base"][k])).all(), (query[:5], x)
            assert (seg * p["seg_len"] < p["cnt"][k]).all(), (query[:5], x, "a segment past the end of its list")
            slots.append(p["base"][k] + seg)
        slots = np.sort(np.concatenate(slots))
        assert np.array_equal(slots, np.arange(p["base"][27])), query[:5]


# cin -> cout -> (channels per lane of x, of dy, channel blocks)
BUILD_TABLE = {
    32: {32: (2, 2, 1), 64: (2, 4, 1), 96: (2, 6, 1), 128: (2, 8, 1)},
    64: {32: (4, 2, 1), 64: (4, 4, 1), 96: (4, 6, 1), 128: (4, 8, 1)},
    96: {32: (6, 2, 1), 64: (6, 4, 1), 96: (6, 6, 1), 128: (6, 4, 2)},
    128: {32: (8, 2, 1), 64: (8, 4, 1), 96: (4, 6, 2), 128: (8, 4, 2)},
}


def test_the_build_table_of_the_gpu_modules(planner):
    """{32, 64, 96, 128}^2 -> (cx, cy, channel blocks), whatever the map: thirteen pairs select the thirteen builds, (96, 128),
    (128, 96) and (128, 128) repeat 6x4, 4x6 and 8x4 with two channel blocks; the FFN shapes run 8x4 with sixteen."""
    pairs = [(ci, co) for ci in BUILD_TABLE for co in BUILD_TABLE[ci]]
    for K, ng, seg in ((1, 63, 0), (27, 1259, 0), (8, 5, 3)):
        counts = None if K == 1 else tuple([ng] * K + [0] * (27 - K))
        plans = run_planner(planner, [(ci, co, K, ng, seg, counts) for ci, co in pairs])
        got = {pr: (p["cx"], p["cy"], p["nblocks"]) for pr, p in zip(pairs, plans)}
        assert got == {(ci, co): BUILD_TABLE[ci][co] for ci, co in pairs}, (K, ng, seg)
    single = [pr for pr in pairs if BUILD_TABLE[pr[0]][pr[1]][2] == 1]
    assert sorted(BUILD_TABLE[ci][co][:2] for ci, co in single) == sorted(builds())
    ffn = run_planner(planner, [(128, 1024, 1, 63, 0, None), (1024, 128, 1, 63, 0, None)])
    assert [(p["cx"], p["cy"], p["nblocks"]) for p in ffn] == [(8, 4, 16), (8, 4, 16)]


def test_what_the_planner_refuses(planner):
    refused = [(48, 32, 1, 4, 0, None), (32, 16, 1, 4, 0, None), (0, 32, 1, 4, 0, None), (32, 32, 1, 0, 0, None), (32, 32, 28, 4, 0, None)]
    assert run_planner(planner, refused) == [None] * len(refused)


def test_the_map_table(planner):
    """13 rows in the order engine.Scene.wgrad_lists walks (its loop is the independent statement of the layout): the 3^3
    maps of five levels, the stride-2 maps of four with positions on the level above, the transposed maps of four."""
    v = [int(x) for x in subprocess.run([planner], input="maps\n", capture_output=True, text=True, check=True).stdout.split()]
    rows, jobs = [tuple(v[5 * i:5 * i + 5]) for i in range(len(v) // 5)], v[-1]
    want, before = [], 0
    for list_kind, levels, K in ((0, 5, 27), (1, 4, 8), (2, 4, 8)):
        for level in range(levels):
            want.append((list_kind, level, K, int(list_kind == 1), before))
            before += K
    assert rows == want and jobs == before == 199
