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
    rows = E.LARGE_CASES + E.EPI_CASES
    got = _classes(planner, [E.row_query(r) for r, _ in rows])
    wrong = [(r, declared, g[1:]) for (r, declared), g in zip(rows, got) if g[1:] != declared]
    assert not wrong, "\n".join(f"{r}: declared {d}, the planner says {g}" for r, d, g in wrong)


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
