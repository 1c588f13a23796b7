"""The case table of test_gpu_conv_edges.py against the planner of the sparse-convolution forward kernels (no GPU).

The planning block of csrc/spconv.hip (between its two marker lines) is plain C++; it is compiled here around
tests/conv_plan_main.cpp with the host compiler and asked, with level sizes from the CPU oracle, what every case of the GPU
module and every op of the full sweep (kinds x levels x width sets, the fused shapes, both a3d_conv_deep_mode settings, over
the module's scenes) would run on.  A planner change that moves a case off its class, or opens a class no case reaches,
fails here and names it."""
import pytest

import conv_edge_cases as E


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return E.build_planner(str(tmp_path_factory.mktemp("conv_plan")))


def _classes(planner, queries):
    return [(q[7],) + E.plan_class(p, q) for q, p in zip(queries, E.run_planner(planner, queries))]


def test_scene_level_sizes():
    for name, want in E.SCENE_LEVELS.items():
        assert E.oracle_levels(name)[:len(want)] == want, name


def test_every_table_row_plans_to_its_declared_class(planner):
    rows = E.LARGE_CASES + E.EPI_CASES + E.TRAIN_CASES
    got = _classes(planner, [E.row_query(r) for r, _ in rows])
    wrong = [(r, declared, g[1:]) for (r, declared), g in zip(rows, got) if g[1:] != declared]
    assert not wrong, "\n".join(f"{r}: declared {d}, the planner says {g}" for r, d, g in wrong)


def test_statistics_do_not_move_a_plan_class(planner):
    """plan_conv reads ConvShape.stats only to add LDS for the epilogue's meeting place and to forbid the fused head: every
    printed field of the plan -- family, build, hand-off, workgroups, parts, tiles -- is the same for the inference build
    (stats 0), a3d_conv_bn_train_forward's (1) and a3d_conv_dgrad_bn's (2).  This is what lets test_gpu_conv_train_edges.py
    take LARGE_CASES / EPI_CASES, declared for the inference kernels, as the class table of the training builds."""
    base = [q for q in E.full_sweep_queries() if q[4] == 0 and q[5] == 0] + [E.row_query(r) for r, _ in E.TRAIN_CASES]
    assert len(base) > 9000 and all(q[8] == 0 for q in base)
    plain = E.run_planner(planner, base)
    for stats in (1, 2):
        with_stats = E.run_planner(planner, [q[:8] + (stats,) for q in base])
        moved = [(q, a, b) for q, a, b in zip(base, plain, with_stats) if a != b]
        assert not moved, f"stats = {stats} moves {len(moved)} plans, the first: {moved[0]}"


def test_the_training_rows_hold_their_partial_counts():
    """63 / 64 per-block partials on the box scenes (64-row tiles, 16-row groups), and 1x1 rows on a scene of two tiles with
    one row in the second, on a coarse level and on a large scene"""
    n = {name: E.SCENE_LEVELS[name][0] for name in ("box4032", "box4096", "box1008", "box1024")}
    assert [(n["box4032"] + 63) // 64, (n["box4096"] + 63) // 64] == [63, 64] and n["box4032"] % 64 == 0
    assert [(n["box1008"] + 15) // 16, (n["box1024"] + 15) // 16] == [63, 64] and n["box1008"] % 16 == 0
    for name in n:
        assert name not in E.SMALL_SCENES + E.LARGE_SCENES
    assert {(r[0], r[2]) for r, _ in E.LINEAR_CASES} == {("box65", 0), ("two_batch", 3), ("s20000", 2), ("s20000", 0)}
    assert all(r[1] == "linear" and c[1] == 1 and c[5] == 0 for r, c in E.LINEAR_CASES)
    for rows in (E.LINEAR_CASES, E.TRAIN_BOX_CASES):                      # every row under both a3d_conv_deep_mode settings
        assert {r[:6] + (1 - r[6],) for r, _ in rows} == {r for r, _ in rows}


def test_every_build_has_a_table_row_on_a_small_and_a_large_scene():
    """Every (BN, CH, PAIR) of A3D_SK_BUILDS and every (BN, CH) of A3D_DEEP_BUILDS, read from spconv.hip, is the declared
    class of a table row -- rows whose launch the GPU modules hold to the class through its profile entry -- on a scene
    below 4096 level-0 voxels and on one from 4096 on; the low-register 128-column builds need 8192 rows and exist on
    large scenes only.  <32, 32, 0> has a kernel-map twin in k_conv_wl: only the 1x1 rows reach it."""
    import re
    text = open(E.SPCONV).read()

    def builds(macro):
        line = re.search(r"#define " + macro + r"\(V\)((?:.*\\\n)*.*)\n", text).group(1)
        return {tuple(int(v) for v in m.split(",")) for m in re.findall(r"V\(([^)]*)\)", line)}
    sk, deep = builds("A3D_SK_BUILDS"), builds("A3D_DEEP_BUILDS")
    assert len(sk) == 9 and len(deep) == 5
    seen = {}
    for row, cls in E.EPI_CASES + E.LARGE_CASES + E.TRAIN_CASES:
        size = "small" if E.SCENE_LEVELS[row[0]][0] < 4096 else "large"
        key = ("sk",) + cls[2:5] if cls[0] == "sk" else ("deep",) + cls[2:4] if cls[0] == "deep" else ("wl",)
        seen.setdefault(key, set()).add(size)
    large_only = {("sk", 128, 32, 1), ("deep", 128, 32)}
    for key in [("sk",) + b for b in sorted(sk)] + [("deep",) + b for b in sorted(deep)] + [("wl",)]:
        assert seen.get(key) == ({"large"} if key in large_only else {"small", "large"}), (key, seen.get(key))


def test_no_reachable_class_is_without_a_case(planner):
    """(mode, class) sets: the union over all cases equals what the full sweep reaches on these scenes."""
    reach = set(_classes(planner, E.full_sweep_queries()))
    cases = set(_classes(planner, E.all_case_queries()))
    missing, beyond = sorted(reach - cases, key=str), sorted(cases - reach, key=str)
    assert not missing, f"{len(missing)} reachable classes without a case: {missing}"
    assert not beyond, f"cases outside the sweep (extend full_sweep_queries): {beyond}"
    families = {c[1] for c in reach}
    assert families == {"wl", "sk", "deep"}
    print(f"{len(reach)} (mode, class) pairs: {sum(1 for c in reach if c[0] == 1)} with the small-level kernel on, "
          f"{sum(1 for c in reach if c[0] == 0)} with it off")


def test_the_issue_s_edges_are_in_the_table(planner):
    """What the table must hold whatever else it holds: 2^3 layers without hand-offs and a G-clamped row for every
    reachable stream-K build, <128,32,0> on 8191 rows against <128,32,1> on 8192 at the same widths, k_conv_deep beyond 256
    workgroups with two and three ring slots, whole and cut tiles, and the 64-column second pass."""
    rows = E.LARGE_CASES
    cls = {c for _, c in rows}
    sweep_q = E.full_sweep_queries()
    reach = {c[1:] for c in _classes(planner, sweep_q)}
    sk = [c for c in reach if c[0] == "sk" and len(c) == 8]
    for want in [c for c in sk if c[1] == 8 and c[5] == 0] + [c for c in sk if c[6] == 1]:
        assert want in cls, want
    a = [r for r, c in rows if r[0] == "box8191" and c[:5] == ("sk", 27, 128, 32, 0)]
    b = [r for r, c in rows if r[0] == "box8192" and c[:5] == ("sk", 27, 128, 32, 1)]
    assert {r[1:] for r in a} & {r[1:] for r in b}
    deep = [c for c in cls if c[0] == "deep" and c[6] == 1]
    assert {c[4] for c in deep} == {2, 3} and {c[5] for c in deep} == {0, 1}
    assert any(c[0] == "sk" and c[7] == 1 for c in cls)
