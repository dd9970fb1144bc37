"""filter_cases.py held to the oracle and to what it promises, on a machine without a GPU: the per-id answer in Python is the oracle's for
every id of the table, every operator and every literal; every layout holds the edges test_gpu_filter_edges.py runs it for; the expected
rows of a cut of every layout are the oracle's rows of the same filter over the same rows, in order."""
import numpy as np
import pytest

from rdf_fusion_amd.plan import PlanBuilder
import filter_cases as fc
import minmax_cases as mc


@pytest.mark.parametrize("lit", fc.LITERALS, ids=[l.name for l in fc.LITERALS])
def test_verdict_is_the_oracles(lit):
    os_ = fc.oracle_store()
    ids = np.arange(fc.N_TABLE + 2, dtype=np.uint32)                  # the null id, the whole table, two ids beyond it
    for op in fc.OPS:
        kept = os_.eval_bool(fc.predicate(0, op, lit), [ids]) == 1
        table = fc.keep_mask(ids, op, lit)
        np.testing.assert_array_equal(table, kept, err_msg=f"{op} {lit.name}")
        some = list(range(fc.EXT0 + 40)) + [fc.EXT0 + 499, fc.EXT0 + 500, fc.EXT0 + 1443, fc.N_TABLE - 1, fc.BEYOND, fc.BEYOND + 1]
        assert [fc.verdict(i, op, lit) for i in some] == kept[some].tolist(), (op, lit.name)


def test_every_operator_has_ids_on_all_three_sides():
    """below, equal and above every literal but the two that are there for their lack of an equal: so each operator keeps some ids and drops
    others, and EQ / GEQ / LEQ differ from NEQ / GT / LT on some id"""
    for lit in fc.LITERALS[:-2]:
        sides = {mc.partial_cmp(fc.value(i), fc.lit_value(lit)) for i in range(1, fc.EXT0) if fc.value(i)[0] in mc.KINDS}
        assert sides == {-1, 0, 1, None}, lit.name
    assert not fc.verdict_table("EQ", fc.LIT["double 0.3"]).any()
    numeric = [i for i in range(1, fc.EXT0) if fc.value(i)[0] in mc.KINDS]
    assert not any(fc.verdict_table(op, fc.LIT["double NaN"])[numeric].any() for op in fc.OPS)
    # 2^53 + 1 is above the integer 2^53 and equal to the double 2^53
    i = fc.IDS["i2^53+1"]
    assert fc.verdict(i, "GT", fc.LIT["integer 2^53"]) and fc.verdict(i, "EQ", fc.LIT["double 2^53"]) and not fc.verdict(i, "GT", fc.LIT["double 2^53"])


def facts(name, head):
    layout = fc.LAYOUTS[name](head)
    return layout, {(op, ln): fc.layout_facts(layout, op, fc.LIT[ln]) for op, ln in fc.CASES[name]}


@pytest.mark.parametrize("head", fc.HEADS)
def test_layout_facts(head):
    # A: 2^20 rows, run copy eligible, every run 10^4 rows or more, no survivor and every row reached; whole waves of xsd:integer ids and
    # whole waves of other kinds (a wave of the streamed form reads 4 x 256 consecutive rows: a run of 10^4 rows holds whole waves)
    a, fa = facts("long_runs", head)
    assert fc.rows_of(a) == fc.ROWS and len(a.ids) == 64 and a.counts.min() >= 10_000 and fc.span_of(a) * 1024 <= fc.ROWS
    assert {f["survivors"] for f in fa.values()} >= {0, fc.ROWS}
    tags = {fc.value(i)[0] for i in a.ids}
    assert tags == set(mc.KINDS)
    assert all(f["qualifying_runs"] >= 2 for k, f in fa.items() if k[1] in fc.A_KIND_LITERALS and k[0] != "EQ")
    for ln in fc.A_KIND_LITERALS:                                      # an id equal to the literal: GEQ / LEQ / EQ differ from GT / LT / NEQ
        assert fa[("GEQ", ln)]["survivors"] > fa[("GT", ln)]["survivors"] and fa[("LEQ", ln)]["survivors"] > fa[("LT", ln)]["survivors"]
        assert 0 < fa[("EQ", ln)]["survivors"] == fc.ROWS - fa[("NEQ", ln)]["survivors"]
    # B: the inclusive bound, runs of 1 .. 5 rows, absent ids, every output phase, a run that ends on a chunk boundary and one that
    # crosses one, qualifying runs between runs that do not qualify
    b, fb = facts("short_runs", head)
    assert fc.rows_of(b) == fc.ROWS and fc.span_of(b) == 1024 and fc.span_of(b) * 1024 == fc.ROWS
    assert {1, 2, 3, 4, 5} <= set(b.counts.tolist()) and (b.counts <= 5).sum() >= 300 and b.counts.max() > 2000
    f = fb[("GT", "integer 0")]
    assert f["absent_ids"] >= 100 and f["start_phases"] == {0, 1, 2, 3} and f["ends_on_chunk"] and f["crosses_chunk"]
    assert f["alternations"] >= 300 and f["short_qualifying_runs"] >= 100 and f["last_id_kept"]
    assert fb[("LEQ", "integer 0")]["start_phases"] == {0, 1, 2, 3} and fb[("LEQ", "integer 0")]["alternations"] >= 300
    assert fb[("EQ", "double NaN")]["survivors"] == 0
    not_kept = {int(i) for i in b.ids[~fc.keep_mask(b.ids, "NEQ", fc.LIT["double 0.5"])]}
    assert not_kept == {fc.IDS["fNaN"], fc.IDS["gNaN"], fc.IDS["g0.5"]} | {i for i in fc.NOT_NUMERIC_IDS if not fc.verdict(i, "NEQ", fc.LIT["double 0.5"])}
    # C: two ids per lane of the scan; one more id is past the bound of the run copy and inside that of the verdict bits
    c, fcs = facts("span_1025", head)
    assert fc.span_of(c) == 1025 and fc.rows_of(c) == 1025 * 1024
    c1 = fc.with_one_more_id(c)
    assert fc.span_of(c1) * 1024 > fc.rows_of(c1) == fc.rows_of(c) + 1 and fc.span_of(c1) * 4 <= fc.rows_of(c1)
    assert fcs[("GT", "integer 0")]["alternations"] >= 1000 and fcs[("GT", "integer 0")]["start_phases"] == {0, 1, 2, 3}
    assert fcs[("NEQ", "double NaN")]["survivors"] == 0 and fcs[("GEQ", "integer -2^63")]["survivors"] == fc.rows_of(c)
    assert fcs[("EQ", "integer 0")]["qualifying_runs"] == 1
    # D: the verdict bits, a last ballot of 48 ids, groups whose ids lie in three or more verdict words at every phase, the last id kept
    d, fd = facts("sparse_singles", head)
    assert fc.rows_of(d) == fc.ROWS and fc.span_of(d) * 4 <= fc.ROWS and fc.span_of(d) % 64 != 0 and int(d.ids[0]) == 1
    assert all(f["groups_of_three_words"] >= 1 and f["places_33_apart"] >= 64 for f in fd.values())
    assert any(f["last_id_kept"] for f in fd.values()) and any(not f["last_id_kept"] for f in fd.values())
    assert set(range(1001, fc.EXT0)) <= set(d.ids.tolist())          # every edge id, the NaNs and the ids that are not numeric included
    # E: the inclusive bound of the verdict bits; one more id (beyond the table) is past it
    e, fe = facts("wide_span", head)
    assert fc.rows_of(e) == fc.ROWS and fc.span_of(e) * 4 == fc.ROWS
    e1 = fc.with_one_more_id(e)
    assert fc.span_of(e1) * 4 > fc.rows_of(e1) and int(e1.ids[-1]) == fc.BEYOND
    assert fe[("GEQ", "integer 0")]["survivors"] > fe[("GT", "integer 0")]["survivors"] > 0 and fe[("EQ", "integer 0")]["survivors"] > 0
    assert fe[("GT", "integer 0")]["alternations"] >= 100_000 and fe[("GT", "integer 0")]["absent_ids"] == fc.N_EXT // 8
    # F: one run, every row or none
    f_, ff = facts("one_run", head)
    assert fc.span_of(f_) == 1 and fc.rows_of(f_) == fc.ROWS + 1
    assert sorted(f["survivors"] for f in ff.values()) == [0, 0, fc.ROWS + 1, fc.ROWS + 1]


def test_wide_span_reaches_an_id_equal_to_its_literal():
    """(the period of the run lengths and the period of the values leave ids of value 0 with rows)"""
    e = fc.wide_span(0)
    zero = e.ids[fc.ext_value(e.ids) == 0]
    assert len(zero) > 0
    f = {k: fc.layout_facts(e, k, fc.LIT["integer 0"]) for k in ("GT", "GEQ", "EQ")}
    assert f["GEQ"]["survivors"] == f["GT"]["survivors"] + f["EQ"]["survivors"] and f["EQ"]["survivors"] > 0


def cut_of(rows, n=5000):
    """n rows of a slice, in order: its first and last rows and two windows in between"""
    m, q = len(rows[0]), n // 4
    idx = np.concatenate([np.arange(q), m // 3 + np.arange(q), 2 * m // 3 + np.arange(q), np.arange(m - q, m)])
    return [c[idx] for c in rows]


@pytest.mark.parametrize("name", list(fc.LAYOUTS))
def test_expected_is_the_oracles_rows_in_order(name):
    os_ = fc.oracle_store()
    layout = fc.LAYOUTS[name](1)
    rows = fc.slice_rows(layout)
    assert np.all(np.diff(rows[1].astype(np.int64)) >= 0) and len(np.unique(rows[0])) == len(rows[0])
    same = np.diff(rows[1].astype(np.int64)) == 0
    assert np.all(np.diff(rows[0].astype(np.int64))[same] > 0)        # GPOS: by object, then by subject
    if name == "short_runs":
        cut = [c[-5000:] for c in rows]                               # the short runs and the last edge ids
    else:
        cut = cut_of(rows)
    for op, ln in fc.CASES[name][:12]:
        for projection in ([0], [1, 0]):
            pb = PlanBuilder()
            desc = pb.build(pb.filter(pb.table(0, 2), fc.predicate(1, op, fc.LIT[ln]), projection=projection))
            got, n_got, _ = os_.execute(desc, [cut])
            exp, n_exp = fc.expected(cut, 1, op, fc.LIT[ln], projection)
            assert n_got == n_exp, (name, op, ln)
            for g, e in zip(got, exp):
                np.testing.assert_array_equal(np.asarray(g)[:n_got], e, err_msg=f"{name} {op} {ln}")
