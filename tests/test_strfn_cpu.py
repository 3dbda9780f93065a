"""String functions evaluated per row (lcase, ucase, ltrim, rtrim, substring, concat,
to_string of integers / bools) as group keys, WHERE operands and inside aggregate
arguments: what can be said without a GPU.

  * the fixtures tests/golden/ref_csql_strfn.json / ref_csql_strfnlsm.json (the reference's
    own engine over the cases of tests/strfn_cases.py) against plan.py and the C oracle,
    like test_ref_csql_cpu.py / test_lsm_partition.py for their suites;
  * every shape compiles for gfx950, the refusals that stay keep their messages;
  * literals: a substring position is a kernel argument, a string literal is text;
  * the generated kernels use no scratch memory and spill no VGPR.
"""
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, DumpedPlan, Call, If, Lit, col, count, sum_, dump_of_plan
import oracle_lib as O
import refcases
import strfn_cases  # noqa: F401  (registers the suites "strfn" and "strfnlsm")
from test_literal_pool_cpu import objects, kernel_facts
from test_lsm_partition import oracle_filters, scan_order_images
from test_ref_csql_cpu import (load, fixture_case, case_plan, strip_dump, check_result,
                               check_partial, all_lowerable, run_oracle)

SUITES = ["strfn", "strfnlsm"]


def make_plan(c, **extra):
    return Plan(refcases.table_schema(c["table"]), scan_mode=c["scan_mode"], **dict(c["kw"], **extra))


@pytest.mark.parametrize("suite", SUITES)
def test_fixture_matches_case_list(suite):
    fx = load(suite)
    cases = refcases.SUITES[suite]()
    assert len(cases) == (60 if suite == "strfn" else 12)
    assert [c["id"] for c in fx["cases"]] == sorted(c["id"] for c in cases)
    by_id = {c["id"]: c for c in cases}
    for c in fx["cases"]:
        assert c["sql"] == by_id[c["id"]]["sql"], c["id"]
        # the reference ran every case and its programs were dumped
        assert c["result"]["ok"] is True and c["partial"]["ok"] is True, c["id"]
        assert "programs" in c and all_lowerable(c["programs"]), c["id"]


@pytest.mark.parametrize("suite", SUITES)
def test_plan_py_emits_the_reference_compilers_bytecode(suite):
    for fx in load(suite)["cases"]:
        assert fx["programs"]["symbols_agree"], fx["id"]
        c = case_plan(suite, fx["id"])
        assert dump_of_plan(make_plan(c)) == strip_dump(fx["programs"]), (fx["id"], fx["sql"])


def _ids(suite):
    return [c["id"] for c in load(suite)["cases"]]


@pytest.mark.parametrize("cid", _ids("strfn"))
def test_oracle_reproduces_the_reference(cid):
    fx = fixture_case("strfn", cid)
    c = case_plan("strfn", cid)
    img, _, _ = refcases.table_image(c["table"])
    r = run_oracle(img, make_plan(c))
    check_result(fx["result"], r if isinstance(r, str) else (r.types, r.rows()))
    r2 = run_oracle(img, DumpedPlan(fx["programs"], scan_mode=c["scan_mode"]))
    check_result(fx["result"], r2 if isinstance(r2, str) else (r2.types, r2.rows()))
    rp = O.oracle_run(img, make_plan(c, mode=K.MODE_PARTIAL))
    check_partial(fx["partial"], [rp.keys[20 * i:20 * i + 20] for i in range(rp.nrows)], rp.columns[0])


@pytest.mark.parametrize("cid", _ids("strfnlsm"))
def test_oracle_reproduces_the_partition_cursor(cid):
    fx = fixture_case("strfnlsm", cid)
    c = case_plan("strfnlsm", cid)
    pname = c["table"][4:]
    imgs, filters = scan_order_images(pname), oracle_filters(pname)
    r = O.oracle_run_chain(imgs, filters, make_plan(c))
    check_result(fx["result"], (r.types, r.rows()))
    r2 = O.oracle_run_chain(imgs, filters, DumpedPlan(fx["programs"], scan_mode=c["scan_mode"]))
    check_result(fx["result"], (r2.types, r2.rows()))
    rp = O.oracle_run_chain(imgs, filters, make_plan(c, mode=K.MODE_PARTIAL))
    check_partial(fx["partial"], [rp.keys[20 * i:20 * i + 20] for i in range(rp.nrows)], rp.columns[0])


# ---------------------------------------------------------------------------------------
# the planner and the generated kernels
# ---------------------------------------------------------------------------------------
S = dict(k=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64, s=K.T_STRING, ns=K.T_STRING)
COLUMNS = [dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
           dict(name="a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
           dict(name="v", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
           dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
           dict(name="ns", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1)]
k, a, v, s, ns = [col(x) for x in ("k", "a", "v", "s", "ns")]


def f(name, *args):
    return Call(name, *args)


def keyed(key, **kw):
    return Plan(S, select=[key, count(1), sum_(a)], group_by=[key], **kw)


def sum_if(cond, **kw):
    return Plan(S, select=[k, sum_(If(cond, a, 0))], group_by=[k], groups_hint=1000, **kw)


# concat / substring / rtrim nested three deep, with a position computed from the row
DEEP = f("concat", f("substring", f("rtrim", s), k % 3 - 2), f("rtrim", f("concat", ns, Lit("x"))))


def test_every_shape_compiles(built, tmp_path):
    """computed key, computed WHERE operand, computed operand inside an aggregate argument,
    bare scan with a computed WHERE -- and PARTIAL mode, an ungrouped plan, two keys"""
    plans = [
        keyed(f("lcase", s), groups_hint=1000),
        Plan(S, select=[count(1)], where=f("substring", s, 8).eq("example.com/")),
        sum_if(f("startswith", f("lcase", ns), Lit("mozilla"))),
        Plan(S, scan_select=[k, s], where=f("endswith", f("rtrim", ns), Lit("7"))),
        keyed(f("concat", s, f("to_string", k % 3)), mode=K.MODE_PARTIAL),
        Plan(S, select=[k, f("ucase", s), count(1)], group_by=[k, f("ucase", s)]),
        keyed(f("to_string", k > 3)),
    ]
    assert len(objects(tmp_path, plans, COLUMNS)) == len(plans)


def refusal(plan, columns=COLUMNS):
    with pytest.raises(E.EvqlError) as ei:
        E.compile_only(plan, columns)
    assert ei.value.code == K.EVQL_ENOTSUP, ei.value
    return ei.value.msg


def test_what_stays_refused(built):
    assert "IF over strings" in refusal(Plan(S, select=[count(1)], where=If(k > 1, s, ns).eq("x")))
    assert "IF over strings" in refusal(keyed(f("lcase", If(k > 1, s, ns))))
    assert "to_string of a float64" in refusal(keyed(f("concat", s, f("to_string", v))))
    assert "string aggregates" in refusal(Plan(S, select=[k, count(f("lcase", s))], group_by=[k]))
    assert "bare scan's select list" in refusal(Plan(S, scan_select=[f("lcase", s)]))
    # a tree of more string-typed nodes than the planner's limit (32): 33 columns, 32 concats
    wide = s
    for _ in range(32):
        wide = f("concat", wide, s)
    assert "nodes" in refusal(keyed(wide))
    # nested scans
    NS = {"id": K.T_UINT64, "items.name": K.T_STRING}
    ncols = [dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
             dict(name="items.name", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN,
                  rlevel_max=1, dlevel_max=1)]
    name = col("items.name")
    for kw in (dict(select=[f("lcase", name), count(1)], group_by=[f("lcase", name)]),
               dict(select=[count(1)], where=f("ucase", name).eq("X"))):
        msg = refusal(Plan(NS, scan_mode=K.SCAN_NESTED, **kw), ncols)
        assert msg.endswith("string functions in a nested scan are not lowered"), msg


def test_the_limit_admits_every_generated_tree(built):
    """RefStrGen.strx nests three deep: at most 8 leaves under 7 functions"""
    E.compile_only(keyed(f("concat", f("concat", f("concat", s, ns), f("concat", ns, s)),
                           f("concat", f("concat", s, s), f("concat", ns, ns)))), COLUMNS)


def test_position_is_an_argument_and_a_string_literal_is_text(built, tmp_path):
    where = lambda pos, lit: Plan(S, select=[count(1)], where=f("substring", s, pos).eq(lit))  # noqa: E731
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    assert len(objects(tmp_path / "a", [where(2, "x"), where(9, "x")], COLUMNS)) == 1
    assert len(objects(tmp_path / "b", [where(2, "x"), where(2, "y")], COLUMNS)) == 2


CLEAN = {
    "lcase-key-lds": (lambda: keyed(f("lcase", s), groups_hint=1000), ["evql_scan_agg"]),
    "deep-key-partitioned": (lambda: keyed(DEEP, groups_hint=400000),
                             ["evql_scan_agg", "evql_part_count", "evql_part_scatter",
                              "evql_part_refine", "evql_part_aggregate"]),
    "two-trees-in-sum-if": (lambda: sum_if(f("lt", f("ucase", s), f("concat", ns, f("to_string", k % 3)))),
                            ["evql_scan_agg"]),
}


@pytest.mark.parametrize("case", sorted(CLEAN))
def test_kernels_use_no_scratch_memory(built, tmp_path, case):
    plan, kernels = CLEAN[case]
    objs = objects(tmp_path, [plan()], COLUMNS)
    assert len(objs) == 1
    facts = kernel_facts(objs[0])
    for kernel in kernels:
        spilled, scratch, _ = facts[kernel]
        assert (spilled, scratch) == (0, 0), (case, kernel, facts[kernel])
