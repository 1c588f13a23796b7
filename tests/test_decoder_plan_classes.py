"""The case table of test_gpu_decoder_edges.py against the launch planner of the inference decoder (no GPU).

The planning block of csrc/decoder.hip (between its two marker lines) is plain C++; it is compiled here around
tests/decoder_plan_main.cpp with the host compiler and asked what every case of the GPU module, and every launch group of a
sweep (11 .. 210 queries, 1 .. (clicks) objects, the three states of the first-layer cache; single samples and pairs), would
run on.  A planner change that moves a case off its class, or opens a class no case reaches, fails here and names it."""
import pytest

import decoder_edge_cases as E


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return E.build_planner(str(tmp_path_factory.mktemp("decoder_plan")))


def _case_classes(planner, cases, switches):
    groups = E.case_groups(cases)
    return [(name, g[0], E.plan_class(p)) for (name, g), p in zip(groups, E.run_planner(planner, [g for _, g in groups], switches))]


def test_every_table_row_plans_to_its_declared_class(planner):
    rows = [(n, key, got, E.DECLARED.get(key)) for n, key, got in _case_classes(planner, E.single_cases(), E.DEFAULT)]
    rows += [(n, key, got, E.DECLARED_WIDE65.get(key)) for n, key, got in _case_classes(planner, E.child_cases(), E.WIDE65)]
    mixed = E.run_planner(planner, [[(nq, k, 0) for nq, k in E.MIXED_SPECS]], E.DEFAULT)[0]
    assert mixed["grouped"] == 1, "the mixed batch's samples no longer share a launch group"
    rows.append(("mixed batch", tuple(E.MIXED_SPECS), E.plan_class(mixed), E.DECLARED_MIXED))
    name, _, spec, states = E.ONE_BG_CASE
    one_bg = E.run_planner(planner, [[(spec[0], spec[1], st)] for st in states], E.DEFAULT, n_bg=E.ONE_BG)
    rows += [(name, spec + (st,), E.plan_class(p), E.DECLARED_ONE_BG.get(spec + (st,))) for st, p in zip(states, one_bg)]
    wrong = [r for r in rows if r[2] != r[3]]
    assert not wrong, "\n".join(f"{n} {key}: declared {d}, the planner says {g}" for n, key, g, d in wrong)
    # what the table must hold whatever else it holds
    cls = {c: E.DECLARED[c][1] for c in E.DECLARED}
    assert cls[(24, 2, 0)] == "k_s2c_out<2,12>" and cls[(24, 5, 0)] == "k_s2c_out<2,12,KG>"          # KG off and on at one query count
    assert cls[(27, 17, 0)] == "k_s2c_out<2,12,KG>" and cls[(28, 18, 0)] == "k_s2c_out<2,8,KG>"      # twelve waves against eight
    assert cls[(32, 22, 0)] == "k_s2c_out<2,8,KG>" and cls[(28, 18, 2)] == "k_s2c_out<2,8,KG>"       # the fallback under a cache
    assert cls[(11, 1, 2)] == cls[(16, 3, 2)] == "k_s2c_out<1,12,QC>" and cls[(18, 4, 2)] == "k_s2c_out<2,12,QC,LO>"
    assert cls[(28, 5, 2)] == "k_s2c_out<2,12,KG,QC>"
    assert E.DECLARED[(210, 200, 0)] != ("unsupported",)


def test_no_class_of_the_default_sweep_is_without_a_case(planner):
    reach = E.reachable_classes(planner, E.DEFAULT)
    cases = {c for _, _, c in _case_classes(planner, E.single_cases(), E.DEFAULT)} | {E.DECLARED_MIXED}
    missing, beyond = sorted(reach - cases, key=str), sorted(cases - reach, key=str)
    assert not missing, f"{len(missing)} reachable classes without a case: {missing}"
    assert not beyond, f"cases outside the sweep (extend sweep_groups): {beyond}"
    print(f"{len(reach)} classes under the default switches")


def test_no_class_of_the_wide_from_65_sweep_is_without_a_case(planner):
    """A3D_WIDE_FROM=65 keeps 33 .. 64 queries on k_kv_c2s<3|4>, k_q_s2c and k_out_ln_mask: every class that only this setting
    reaches is run by the child interpreter of test_gpu_decoder_edges.py or covered by a cited test; the others are the
    default sweep's."""
    reach = E.reachable_classes(planner, E.WIDE65)
    only65 = reach - E.reachable_classes(planner, E.DEFAULT)
    child = {c for _, _, c in _case_classes(planner, E.child_cases(), E.WIDE65)}
    assert all(isinstance(v, str) and "::" in v for v in E.CITED_WIDE65.values())
    missing = sorted(only65 - child - set(E.CITED_WIDE65), key=str)
    beyond = sorted((child | set(E.CITED_WIDE65)) - reach, key=str)
    assert not missing, f"{len(missing)} classes reachable under A3D_WIDE_FROM=65 without a case or a cited test: {missing}"
    assert not beyond, f"child cases or citations outside the sweep: {beyond}"
    assert only65 and all(c[0].startswith(("k_kv_c2s<3>", "k_kv_c2s<4>", "k_c2s_attn_b<3>", "k_c2s_attn_b<4>")) for c in only65)
    print(f"{len(reach)} classes under A3D_WIDE_FROM=65, {len(only65)} of them its own")


def test_every_k_s2c_out_build_a_plan_names_is_instantiated(planner):
    """The number of learned background queries is the model's (a3d_decoder_weights::n_bg_queries), not the library's: with
    fewer of them a sample of up to 16 queries has up to 16 objects, and one tile moves its keys out of LDS from 15 on.  Over
    0, 1 and 10 learned background queries and every setting of the switches, the k_s2c_out builds the plans name are the
    ones s2c_out_kernel holds -- with no learned background query all of them, with ten the one-tile KG builds drop out -- and
    the model with one, which ONE_BG_CASE runs on the GPU, reaches both of those."""
    import itertools
    reached = {}
    for n_bg in (0, E.ONE_BG, E.N_BG):
        groups = E.fused_tier_groups(n_bg)
        reached[n_bg] = set()
        for sw in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (17, 33, 65)):
            for p in E.run_planner(planner, groups, sw, n_bg=n_bg):
                assert p["rc"] == 0
                if p["grouped"]:
                    reached[n_bg] |= {b for b in p["builds"] if b.startswith("k_s2c_out<")}
        assert reached[n_bg] <= E.S2C_OUT_BUILDS, (n_bg, sorted(reached[n_bg] - E.S2C_OUT_BUILDS))
    one_tile_kg = {"k_s2c_out<1,12,KG>", "k_s2c_out<1,12,KG,QC>"}
    assert reached[0] == E.S2C_OUT_BUILDS
    assert reached[E.N_BG] == E.S2C_OUT_BUILDS - one_tile_kg
    assert one_tile_kg <= reached[E.ONE_BG] and one_tile_kg == {c[1] for c in E.DECLARED_ONE_BG.values()}


@pytest.mark.parametrize("wg_per_group", (0, 1))
def test_workgroup_shares_are_held_to_what_a_sample_can_use(planner, wg_per_group):
    """256 workgroups in proportion to the samples' 16-point groups, each share in [1, ceil(groups / 8)] (a wave per group)
    or [1, groups] (a workgroup per group).  In the mixed batch of test_gpu_decoder_edges.py the 2-point sample's share is
    raised to one and the others are cut; a sample alone gets exactly what it can use."""
    def want(points):
        groups = [(n + 15) // 16 for n in points]
        shares = [min(max(256 * g // sum(groups), 1), g if wg_per_group else (g + 7) // 8) for g in groups]
        ends = [sum(shares[:i + 1]) for i in range(len(shares))]
        return sum(shares), [(e - s, e) for s, e in zip(shares, ends)]

    for points in [E.MIXED_POINTS] + [(n,) for n in E.WIDE_POINT_EDGES] + [(2, 80000), (129, 129, 129), (4200, 17)]:
        assert E.run_shares(planner, points, wg_per_group) == want(points), points
    groups = [(n + 15) // 16 for n in E.MIXED_POINTS]
    raw = [256 * g // sum(groups) for g in groups]
    assert raw[0] < 1, "the mixed batch no longer raises its smallest sample's share"
    # (the batch runs the <= 32-query kernels: a wave per group)
    assert all(r > (g + 7) // 8 for r, g in zip(raw[2:], groups[2:])), "the mixed batch no longer cuts its larger samples' shares"
