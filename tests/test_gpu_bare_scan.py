"""Bare scans (SELECT .. WHERE without GROUP BY / aggregate) on the device against the C
oracle's restatement of FastCSTableScan::nextBatch / CSTableScan NO_AGGREGATION.

Rows are compared IN ORDER with `==` and the packed SVector bytes of every column are
compared as bytes: projections are per row and floating-point contraction is off, so
there is nothing a device could legitimately reorder or round differently.  Every plan
listed here must lower: no test returns early on ENOTSUP."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import If, Order, Plan, col
import lsm_nested_tables as LN
import lsm_tables
import nested_tables as N
import oracle_lib as O
import refcases
import tables as T
from test_lsm_partition import (case_plan, fixture_case, make_plan, oracle_filters,
                                scan_order_images)
from test_ref_csql_cpu import check_result

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "oracle", "_ref", "csql_probe")

k, a, b, v, n, s, ns = [col(x) for x in ("k", "a", "b", "v", "n", "s", "ns")]
nv, nb, f, t_, w, k10, p = [col(x) for x in ("nv", "nb", "f", "t", "w", "k10", "p")]

W25 = (a > 30000) & (b < 30000)        # ~24.9 % of the rows
W001 = (a > 65000) & (b < 1000)        # ~0.01 %
MIXED_ROWS = 300_000


def third_filter(nrows):
    return np.arange(nrows) % 3 != 0


@pytest.fixture(scope="module")
def mixed(ctx):
    img, c = T.mixed_table()
    t = ctx.open_image(img)
    yield t, img, c
    t.close()


@pytest.fixture(scope="module")
def survey(ctx):
    img, c = T.survey_table()
    t = ctx.open_image(img)
    yield t, img, c
    t.close()


def run_query(q, batch=1024):
    q.execute()
    return q.fetch_all(batch)


def check_against_oracle(t, img, plan, order=None):
    exp = O.oracle_run(img, plan, order=order)
    q = t.query(plan)
    try:
        assert q.column_count() == len(exp.types)
        assert [q.column_type(i) for i in range(q.column_count())] == list(exp.types)
        if order is not None:
            q.set_order(order)
        got = run_query(q)
        assert got.nrows == exp.nrows
        assert got.rows() == exp.rows()
        assert got.raw == exp.raw
        st = q.stats()
        if order is None:
            assert st["rows_passed"] == exp.rows_passed
            assert st["rows_scanned"] == exp.rows_scanned
        assert st["num_groups"] == 0
    finally:
        q.close()
    return exp


MIXED_PLANS = {
    "where-0pct": dict(scan_select=[a], where=a > 10**9),
    "where-100pct": dict(scan_select=[a, b], where=a < 70000),
    "arith-if": dict(scan_select=[a + b, v * 2.0, If(a > 5000, n, b), a % 7, If(b > 0, a / b, b),
                                  (a * 3 - b) > 1000],
                     where=b > 10),
    "strings": dict(scan_select=[k, s, ns, n, s < "g5"], where=(s < "g5") & ns.neq("s3") & (a > 20000)),
    "nullable-numerics": dict(scan_select=[n, nv, nb, If(a > 30000, nv, v)], where=a > 20000),
    "bool-timestamp-wide": dict(scan_select=[f, t_, w, k10, p], where=a > 40000),
    "filter-and-where": dict(scan_select=[a, s], where=a > 1000, row_filter=third_filter(MIXED_ROWS)),
    "filter-only": dict(scan_select=[k, b], row_filter=third_filter(MIXED_ROWS)),
    "row-end": dict(scan_select=[a, ns], where=a > 1000, row_end=123_457),
}

SURVEY_PLANS = {
    "no-where": dict(scan_select=[k, a]),
    "where-0.01pct": dict(scan_select=[k, b, v, s], where=W001),
    "where-25pct": dict(scan_select=[k, v], where=W25),
}


@pytest.mark.parametrize("name", sorted(MIXED_PLANS))
def test_flat_parity_mixed(mixed, name):
    t, img, _ = mixed
    exp = check_against_oracle(t, img, Plan(T.MIXED_SCHEMA, **MIXED_PLANS[name]))
    assert (exp.nrows == 0) == (name == "where-0pct")


@pytest.mark.parametrize("name", sorted(SURVEY_PLANS))
def test_flat_parity_survey(survey, name):
    t, img, c = survey
    exp = check_against_oracle(t, img, Plan(T.SURVEY_SCHEMA, **SURVEY_PLANS[name]))
    if name == "where-25pct":
        m = (c["a"] > 30000) & (c["b"] < 30000)
        assert exp.nrows == int(m.sum())
        assert [r[0] for r in exp.rows()] == c["k"][m].tolist()


def test_row_begin_splits_the_scan(mixed):
    """the oracle has no row_begin: scan[0, m) + scan[m, N) == scan[0, N) for an m inside
    a tile, and the rows are numpy's"""
    t, img, c = mixed
    m = 100_001
    kw = dict(scan_select=[a, v, ns], where=a > 30000)
    out = []
    for rb, re_ in ((0, m), (m, MIXED_ROWS), (0, 0)):
        q = t.query(Plan(T.MIXED_SCHEMA, row_begin=rb, row_end=re_, **kw))
        out.append(run_query(q))
        q.close()
    assert out[0].nrows > 0 and out[1].nrows > 0
    assert out[0].rows() + out[1].rows() == out[2].rows()
    assert [x + y for x, y in zip(out[0].raw, out[1].raw)] == out[2].raw
    mask = c["a"] > 30000
    assert [r[0] for r in out[2].rows()] == c["a"][mask].tolist()
    assert [r[1] for r in out[1].rows()] == c["v"][m:][mask[m:]].tolist()
    assert out[0].nrows == int(mask[:m].sum())


@pytest.mark.parametrize("cid", ["lsm-single_plain-scan", "lsm-single_skip-scan"])
def test_reference_fixture_scans(ctx, cid):
    """`select rid from t;` over the single-file partitions: the rows of the reference
    engine (tests/golden/ref_csql_lsm.json), in the oracle's order"""
    fx = fixture_case(cid)
    c = case_plan(cid)
    pname = c["table"][4:]
    files = lsm_tables.partition(pname)
    assert len(files) == 1
    tabs = [ctx.open_image(fl[1]) for fl in reversed(files)]
    ch = E.LsmChain(ctx)
    for tb, fl in zip(tabs, reversed(files)):
        ch.add(tb, has_skiplist=fl[2], has_updates=fl[3])
    ch.build()
    try:
        q = ch.query(make_plan(c))
        got = run_query(q)
        q.close()
        check_result(fx["result"], (got.types, got.rows()))
        exp = O.oracle_run_chain(scan_order_images(pname), oracle_filters(pname), make_plan(c))
        assert got.rows() == exp.rows()
        assert got.raw == exp.raw
    finally:
        ch.close()
        for tb in tabs:
            tb.close()


def test_windows_and_batches(mixed, monkeypatch):
    """the same bytes whatever the window (EVQL_SCAN_WINDOW_ROWS, read when the query is
    created) and whatever next_batch's max_rows; execute twice; two queries drained in turn"""
    t, img, _ = mixed
    kw = dict(scan_select=[k, s, ns, v], where=W25, row_end=50_001)
    exp = O.oracle_run(img, Plan(T.MIXED_SCHEMA, **kw))
    assert exp.nrows > 5000
    for window in ("1", "5000", None):
        if window is None:
            monkeypatch.delenv("EVQL_SCAN_WINDOW_ROWS", raising=False)
        else:
            monkeypatch.setenv("EVQL_SCAN_WINDOW_ROWS", window)
        q = t.query(Plan(T.MIXED_SCHEMA, **kw))
        for batch in (1, 1000, 1 << 20):
            got = run_query(q, batch)  # (also: execute again on the same query)
            assert got.nrows == exp.nrows, (window, batch)
            assert got.raw == exp.raw, (window, batch)
        q.close()
    # two queries on one table, drained alternately
    monkeypatch.setenv("EVQL_SCAN_WINDOW_ROWS", "3000")
    kw2 = dict(scan_select=[a, ns], where=a > 1000, row_end=123_457)
    exp2 = O.oracle_run(img, Plan(T.MIXED_SCHEMA, **kw2))
    q1, q2 = t.query(Plan(T.MIXED_SCHEMA, **kw)), t.query(Plan(T.MIXED_SCHEMA, **kw2))
    q1.execute()
    q2.execute()
    raws = {1: [b""] * 4, 2: [b""] * 2}
    live = {1: q1, 2: q2}
    while live:
        for i in sorted(live):
            cnt, raw = live[i].next_batch(777 if i == 1 else 4096)
            if cnt == 0:
                del live[i]
                continue
            raws[i] = [x + y for x, y in zip(raws[i], raw)]
    assert raws[1] == exp.raw
    assert raws[2] == exp2.raw
    q1.close()
    q2.close()


def test_heartbeat_covers_the_windows(mixed, monkeypatch):
    """the heartbeat given to execute is beaten by next_batch's window kernels too (once
    per window at least); a beat that asks to stop fails the next window"""
    t, img, _ = mixed
    monkeypatch.setenv("EVQL_SCAN_WINDOW_ROWS", "5000")
    kw = dict(scan_select=[k, s, ns, v], where=W25, row_end=50_001)
    exp = O.oracle_run(img, Plan(T.MIXED_SCHEMA, **kw))
    windows = -(-exp.nrows // 5000)
    assert windows >= 3
    q = t.query(Plan(T.MIXED_SCHEMA, **kw))
    beats = []
    q.execute(heartbeat=lambda: beats.append(1) or 0)
    during_execute = len(beats)
    assert during_execute >= 2
    got = q.fetch_all(1000)
    assert got.raw == exp.raw
    assert len(beats) - during_execute >= windows
    stop = []
    q.execute(heartbeat=lambda: 1 if stop else 0)
    stop.append(1)
    with pytest.raises(E.EvqlError) as ei:
        q.next_batch(100)
    assert ei.value.code == K.EVQL_ERUNTIME and "aborted" in ei.value.msg
    q.close()


def test_limit_and_offset(survey):
    t, img, _ = survey
    plan = Plan(T.SURVEY_SCHEMA, scan_select=[k, a, v], where=W25)
    passing = O.oracle_run(img, plan).nrows
    assert passing > 200_000
    for limit, offset in ((10, 0), (7, 12345), (0, 0), (5, passing - 2)):
        exp = check_against_oracle(t, img, plan, order=Order(plan, [], limit, offset))
        assert exp.nrows == min(limit, passing - offset)
    q = t.query(plan)
    with pytest.raises(E.EvqlError) as ei:
        q.set_order(Order(plan, [(0, False)], limit=5))
    assert ei.value.code == K.EVQL_ENOTSUP and "ORDER BY over a bare scan" in ei.value.msg
    q.close()


def test_errors_only_for_passing_rows(mixed):
    t, img, _ = mixed
    quiet = Plan(T.MIXED_SCHEMA, scan_select=[a / (b - b)], where=a > 10**9)
    exp = check_against_oracle(t, img, quiet)
    assert exp.nrows == 0
    for kw in (dict(scan_select=[a / (b - b)], where=a > 1000),
               dict(scan_select=[a], where=(a % (b - b)) > 1)):
        plan = Plan(T.MIXED_SCHEMA, **kw)
        with pytest.raises(RuntimeError) as oi:
            O.oracle_run(img, plan)
        assert "zero" in str(oi.value)
        q = t.query(plan)
        with pytest.raises(E.EvqlError) as ei:
            run_query(q)
        assert ei.value.code == K.EVQL_ERUNTIME and "zero" in ei.value.msg
        q.close()


def test_nested_scans(ctx):
    img, _ = N.items_table(100_000)
    t = ctx.open_image(img)
    rid, pos, price = col("id"), col("items.position"), col("items.price")
    flt = np.random.default_rng(17).random(100_000) < 0.5
    for where in (None, price > 5):
        plan = Plan(N.ITEMS_SCHEMA, scan_select=[rid, pos, price + 1], where=where,
                    scan_mode=K.SCAN_NESTED, row_filter=flt)
        exp = check_against_oracle(t, img, plan)
        assert exp.nrows > 10_000
    t.close()
    # columns of sibling repeated groups, zipped level by level
    path = os.path.join(T.GOLDEN, "testtbl.cst")
    t = ctx.open_file(path)
    plan = Plan(N.SIBLING_SCHEMA,
                scan_select=[col("time"), col("event.cart_items.quantity"),
                             col("event.search_query.result_items.position"),
                             col("event.page_view.time")],
                scan_mode=K.SCAN_NESTED)
    exp = check_against_oracle(t, path, plan)
    assert exp.nrows > 213
    t.close()


def test_refusals(mixed, ctx):
    t, _, _ = mixed
    q = t.query(Plan(T.MIXED_SCHEMA, **MIXED_PLANS["where-100pct"]))
    q.execute()
    with pytest.raises(E.EvqlError) as ei:
        q.export_groups(None, 16)
    assert ei.value.code == K.EVQL_EARG
    q.close()
    # a bare scan over a chain of several files
    files = LN.partition("quiet")
    assert len(files) > 1
    tabs = [ctx.open_image(fl[1]) for fl in reversed(files)]
    ch = E.LsmChain(ctx)
    for tb, fl in zip(tabs, reversed(files)):
        ch.add(tb, has_skiplist=fl[2], has_updates=fl[3])
    ch.build()
    with pytest.raises(E.EvqlError) as ei:
        ch.query(Plan(LN.NESTED_LSM_SCHEMA, scan_select=[col("id")]))
    assert ei.value.code == K.EVQL_ENOTSUP and "chain" in ei.value.msg
    ch.close()
    for tb in tabs:
        tb.close()


@pytest.mark.skipif(not os.path.exists(PROBE), reason="oracle/_ref/csql_probe not built "
                    "(needs the reference sources at build time)")
def test_reference_engine_with_lowered_scans():
    """the reference's own engine with `MODE gpuscan strict` (opts.lower_scans): the
    sequential scan -- and a LIMIT directly above it -- run on the device; same rows in
    the same order as `MODE cpu`"""
    img, _, kind = refcases.table_image("survey")
    queries = ["select k, a from t where a > 60000;",
               "select a + b, v from t where a > 30000 and b < 30000 limit 50 offset 20;",
               "select k from t where a > 70000;"]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t.cst")
        with open(path, "wb") as fh:
            fh.write(img)
        res = {}
        for mode in ("cpu", "gpuscan strict"):
            cmds = ["TABLE t %s %s" % (path, kind), "ROWS on", "MODE " + mode] + ["SQL " + x for x in queries]
            pr = subprocess.run([PROBE], input="\n".join(cmds) + "\n", capture_output=True,
                                text=True, timeout=600)
            assert pr.returncode == 0, pr.stderr[-2000:]
            res[mode] = [json.loads(l) for l in pr.stdout.splitlines() if l.strip()]
    for x, c, g in zip(queries, res["cpu"], res["gpuscan strict"]):
        assert c["ok"] and g["ok"], (x, c.get("error"), g.get("error"))
        assert g["types"] == c["types"], x
        assert g["rows"] == c["rows"], x
        d = {y["node"]: y["lowered"] for y in g["decisions"]}
        assert d.get("seqscan") is True, (x, g["decisions"])
    assert len(res["cpu"][0]["rows"]) > 10_000
    assert res["cpu"][2]["rows"] == []
