"""Nested (EVQL_SCAN_NESTED) and record (EVQL_SCAN_NESTED_WITHIN_RECORD) scans under row
filters and over partition file chains, HIP path against the C oracle.

The row filter of a nested scan holds one bit per RECORD (CSTableScan::setFilter,
sql/CSTableScan.cc:203-204, 426, 545, 642-645): k_filter_expand turns it into one bit
per flattened row, the fused kernels then run as under a flat scan's filter.  Every
expectation comes from the oracle (tests/test_nested_filter_cpu.py pins the identities
used): a single file is `oracle_run` of the plan with its filter, a chain is
`oracle_partial_frame` per file in scan order, each under its filter, + `oracle_merge`.

The filter is data, not code: every filter of a directed case reuses the code object of
its plan shape."""
import random

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import (Plan, Agg, CompileError, If, Lit, Order, col, count, lit, max_,
                              min_, out, sum_)
import lsm_nested_tables as LN
import nested_tables as N
import oracle_lib as O
import tables as T
import test_gpu_fuzz as F

pytestmark = pytest.mark.gpu

WR = K.SCAN_NESTED_WITHIN_RECORD
NESTED = K.SCAN_NESTED
NREC = 100_000

FILTERS = ["ones", "zeros", "p01", "p50", "p99", "single", "first", "last", "short"]


def make_filter(name, nrec, seed=17):
    rng = np.random.default_rng(seed)
    f = np.zeros(nrec, bool)
    if name == "ones":
        f[:] = True
    elif name in ("p01", "p50", "p99"):
        f = rng.random(nrec) < {"p01": 0.01, "p50": 0.5, "p99": 0.99}[name]
    elif name == "single":
        f[nrec * 2 // 3] = True
    elif name == "first":
        f[0] = True
    elif name == "last":
        f[nrec - 1] = True
    elif name == "short":  # row_filter_len < records: the records behind it are dropped
        f = rng.random(nrec * 3 // 5) < 0.5
    return f


def cd(x):
    return Agg("count_distinct", x)


def partial_rows(r):
    return {r.keys[20 * i:20 * i + 20]: r.columns[0][i] for i in range(r.nrows)}


def check_single(t, img, schema, kw, f, order=None):
    """one operator over one file under the record filter `f` against the oracle: rows
    (integers, strings, NULL tags bit-exact, float sums within 1e-6 relative),
    rows_scanned and rows_passed"""
    plan = Plan(schema, row_filter=f, **kw)
    exp = O.oracle_run(img, plan, order=order)
    q = t.query(plan)
    try:
        if order is not None:
            q.set_order(order)
        got = q.run()
        assert got.nrows == exp.nrows
        if kw.get("mode") == K.MODE_PARTIAL:
            assert dict(got.rows()) == partial_rows(exp)
        elif order is not None:
            assert got.rows() == exp.rows()
        else:
            T.compare_results(got.rows(), exp.rows(), exp.types,
                              key_cols=len(kw.get("group_by", [])), rel=1e-6)
        st = q.stats()
        assert st["rows_passed"] == exp.rows_passed
        assert st["rows_scanned"] == exp.rows_scanned
    finally:
        q.close()


# ---------------------------------------------------------------------------------------
# single files
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def items(ctx):
    img, st = N.items_table(NREC)
    t = ctx.open_image(img)
    yield t, img, st
    t.close()


@pytest.fixture(scope="module")
def testtbl(ctx):
    img = N.testtbl_v2()
    t = ctx.open_image(img)
    yield t, img
    t.close()


rid, pos, price, score = col("id"), col("items.position"), col("items.price"), col("score")


def items_plans():
    return {
        # GROUP BY a leaf column
        "leaf": dict(select=[pos, count(1), sum_(price), min_(price), max_(price)], group_by=[pos],
                     scan_mode=NESTED),
        # GROUP BY a parent expression, first-row values of leaf and parent, float sums
        "parent": dict(select=[rid % 97, pos, price, score, count(1), sum_(score)],
                       group_by=[rid % 97], scan_mode=NESTED),
        "global": dict(select=[count(1), sum_(price), sum_(pos), sum_(score), count(score)],
                       scan_mode=NESTED),
        "where": dict(select=[pos, count(1), sum_(price)], group_by=[pos], where=price > 50000,
                      scan_mode=NESTED),
        # WHERE over columns of different repetition depth (apply_where_resets)
        "mixed": dict(select=[pos, count(1), sum_(rid), sum_(price)], group_by=[pos],
                      where=(pos > 2) & ((rid % 3).eq(0)), scan_mode=NESTED),
        "distinct": dict(select=[pos, cd(price % 100), count(1)], group_by=[pos], scan_mode=NESTED),
        "partial": dict(select=[pos, count(1), sum_(price), max_(rid)], group_by=[pos],
                        mode=K.MODE_PARTIAL, scan_mode=NESTED),
        # fetchNextWithoutColumns: one row per kept record
        "no-columns": dict(select=[count(1)], scan_mode=NESTED),
        # a leaf that is not repeated: rows are records, the caller's bits are used directly
        "flat-leaf": dict(select=[rid % 10, count(1), sum_(score)], group_by=[rid % 10],
                          scan_mode=NESTED),
        "wr-group": dict(scan_select=[count(pos), sum_(price), sum_(rid)],
                         select=[out(0), count(1), sum_(out(1)), max_(out(2))], group_by=[out(0)],
                         scan_mode=WR),
        "wr-global": dict(scan_select=[count(price), sum_(price), count(1)],
                          select=[sum_(out(0)), sum_(out(1)), sum_(out(2)), count(1)], scan_mode=WR),
        "wr-first": dict(scan_select=[count(pos), sum_(price), sum_(rid)],
                         select=[out(0), out(1), out(2) + 1, count(1)], group_by=[out(0)],
                         scan_mode=WR),
        "wr-partial": dict(scan_select=[count(pos), sum_(price)],
                           select=[out(0), count(1), sum_(out(1))], group_by=[out(0)],
                           mode=K.MODE_PARTIAL, scan_mode=WR),
    }


@pytest.mark.parametrize("fname", FILTERS)
def test_items_table_under_a_record_filter(items, fname):
    t, img, _ = items
    f = make_filter(fname, NREC)
    for name, kw in items_plans().items():
        try:
            check_single(t, img, N.ITEMS_SCHEMA, kw, f)
        except AssertionError as e:
            raise AssertionError("plan %s, filter %s: %s" % (name, fname, e))


@pytest.mark.parametrize("fname", ["p50", "short", "single"])
def test_items_table_order_by_limit(items, fname):
    """ORDER BY + LIMIT over the groups of a filtered nested / record scan"""
    t, img, _ = items
    f = make_filter(fname, NREC)
    for name in ("leaf", "wr-group"):
        kw = items_plans()[name]
        p = Plan(N.ITEMS_SCHEMA, **kw)
        order = Order(p, [(1, True), (0, False)], limit=4, offset=1)
        check_single(t, img, N.ITEMS_SCHEMA, kw, f, order=order)


def test_filter_expansion_matches_the_record_layout(items):
    """the expansion itself, against numpy: grouping the flattened rows by record id under
    a filter returns exactly the kept records with their own row counts and sums (records
    of 0..8 items, ~120 tiles of 2048 slots)"""
    t, img, st = items
    f = make_filter("p50", NREC)
    plan = Plan(N.ITEMS_SCHEMA, select=[rid, count(1), sum_(pos)], group_by=[rid], scan_mode=NESTED,
                row_filter=f, groups_hint=NREC)
    q = t.query(plan)
    got = sorted(q.run().rows())
    assert q.stats()["rows_scanned"] == st["total"]
    q.close()
    cnt = st["cnt"]
    # (a record without items has one undefined slot, which reads 0)
    exp = [(int(r) * 7, int(max(cnt[r], 1)), int(cnt[r] * (cnt[r] + 1) // 2))
           for r in np.flatnonzero(f)]
    assert got == exp


def fixture_plans():
    tm = col("time")
    sq_time = col("event.search_query.time")
    nitems = col("event.search_query.num_result_items")
    tpos = col("event.search_query.result_items.position")
    clicked = col("event.search_query.result_items.clicked")
    sid, qs = col("session_id"), col("event.search_query.query_string")
    item = col("event.search_query.result_items.item_id")
    return {
        "leaf": dict(select=[tpos, count(1), sum_(nitems), max_(tm)], group_by=[tpos],
                     scan_mode=NESTED),
        # GROUP BY a parent column, first-row strings of every depth
        "parent-strings": dict(select=[nitems, sid, qs, item, count(1), sum_(tpos)],
                               group_by=[nitems], scan_mode=NESTED),
        "string-key": dict(select=[qs, count(1), sum_(tpos)], group_by=[qs], scan_mode=NESTED),
        "global": dict(select=[count(tm), count(sq_time), sum_(nitems), count(tpos)],
                       scan_mode=NESTED),
        "mixed": dict(select=[nitems, count(1), sum_(tpos), sum_(tm)], group_by=[nitems],
                      where=(tpos > 3) & (nitems > 10), scan_mode=NESTED),
        # a string predicate on the leaf's own depth
        "string-where": dict(select=[tpos, count(1), sum_(If(clicked, 1, 0))], group_by=[tpos],
                             where=item >= "p~6", scan_mode=NESTED),
        "distinct": dict(select=[nitems, cd(tpos), count(1)], group_by=[nitems], scan_mode=NESTED),
        "partial": dict(select=[tpos, count(1), sum_(nitems)], group_by=[tpos], mode=K.MODE_PARTIAL,
                        scan_mode=NESTED),
        "no-columns": dict(select=[count(1)], scan_mode=NESTED),
        "wr-group": dict(scan_select=[count(tpos), sum_(nitems), sum_(tpos), count(clicked)],
                         select=[out(0), count(1), sum_(out(1)), max_(out(2)), min_(out(3))],
                         group_by=[out(0)], scan_mode=WR),
        "wr-global": dict(scan_select=[count(sq_time), sum_(nitems), count(tpos), count(1)],
                          select=[sum_(out(0)), sum_(out(1)), sum_(out(2)), sum_(out(3)), count(1)],
                          scan_mode=WR),
        "wr-lit": dict(scan_select=[count(sq_time), sum_(tm), sum_(lit(2))],
                       select=[out(0), count(1), sum_(out(1)), sum_(out(2))], group_by=[out(0)],
                       scan_mode=WR),
    }


@pytest.mark.parametrize("fname", FILTERS)
def test_testtbl_under_a_record_filter(testtbl, fname):
    """the reference's fixture (213 records, two repetition depths, strings at each)"""
    t, img = testtbl
    f = make_filter(fname, 213)
    for name, kw in fixture_plans().items():
        try:
            check_single(t, img, N.NESTED_SCHEMA, kw, f)
        except AssertionError as e:
            raise AssertionError("plan %s, filter %s: %s" % (name, fname, e))
    kw = fixture_plans()["leaf"]
    order = Order(Plan(N.NESTED_SCHEMA, **kw), [(1, True), (0, False)], limit=5, offset=2)
    check_single(t, img, N.NESTED_SCHEMA, kw, f, order=order)


def test_sibling_groups_under_a_filter_are_refused(ctx):
    """columns of sibling repeated groups are zipped per record (materialize_nested_zip);
    the rows of a record then come from k_zip_rows' row offsets, from which the record
    mask is not expanded: refused by name, and lowered as before without a filter"""
    import os
    path = os.path.join(T.GOLDEN, "testtbl.cst")
    t = ctx.open_file(path)
    S = N.SIBLING_SCHEMA
    kw = dict(select=[count(1), sum_(col("event.cart_items.quantity")),
                      sum_(col("event.search_query.result_items.position"))], scan_mode=NESTED)
    plain = Plan(S, **kw)
    q = t.query(plain)
    exp = O.oracle_run(path, plain)
    assert q.run().rows() == exp.rows()
    q.close()
    with pytest.raises(E.EvqlError) as ei:
        t.query(Plan(S, row_filter=make_filter("p50", 213), **kw))
    assert ei.value.code == K.EVQL_ENOTSUP and "sibling" in ei.value.msg
    t.close()


def test_still_refused(items, ctx):
    t, _, _ = items
    kw = items_plans()["leaf"]
    for extra in (dict(row_end=10), dict(row_begin=3, row_end=10),
                  dict(row_end=10, row_filter=make_filter("p50", NREC))):
        with pytest.raises(E.EvqlError) as ei:
            t.query(Plan(N.ITEMS_SCHEMA, **dict(kw, **extra)))
        assert ei.value.code == K.EVQL_ENOTSUP and "row range" in ei.value.msg
    # a bare scan over a multi-file chain
    files = LN.partition("quiet")
    tabs = [ctx.open_image(f[1]) for f in reversed(files)]
    ch = E.LsmChain(ctx)
    for tb, f in zip(tabs, reversed(files)):
        ch.add(tb, has_skiplist=f[2], has_updates=f[3])
    ch.build()
    with pytest.raises(E.EvqlError) as ei:
        ch.query(Plan(LN.NESTED_LSM_SCHEMA, scan_select=[col("id")]))
    assert ei.value.code == K.EVQL_ENOTSUP
    ch.close()
    for tb in tabs:
        tb.close()


# ---------------------------------------------------------------------------------------
# chains: one operator over the files of a partition
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nested_chain(ctx):
    chains = {}

    def get(pname):
        if pname not in chains:
            files = LN.partition(pname)
            tabs = [ctx.open_image(f[1]) for f in reversed(files)]
            ch = E.LsmChain(ctx)
            for t, f in zip(tabs, reversed(files)):
                ch.add(t, has_skiplist=f[2], has_updates=f[3])
            ch.build()
            chains[pname] = (ch, tabs)
        return chains[pname]
    yield get
    for ch, tabs in chains.values():
        ch.close()
        for t in tabs:
            t.close()


_filters = {}


def oracle_filters(pname):
    if pname not in _filters:
        _filters[pname] = O.oracle_partition_filters(LN.partition(pname))
    return _filters[pname]


def chain_plans():
    k, s, lid = col("k"), col("s"), col("id")
    lpos, lprice = col("items.position"), col("items.price")
    return {
        "leaf": dict(select=[lpos, count(1), sum_(lprice), max_(lid)], group_by=[lpos],
                     scan_mode=NESTED),
        # first rows across files: (file << 44 | flattened row), newest file first; string
        # bytes of nested first rows
        "parent-first": dict(select=[k, lid, s, lpos, lprice, count(1), sum_(lprice)], group_by=[k],
                             scan_mode=NESTED),
        "string-key": dict(select=[s, count(1), sum_(lpos)], group_by=[s], scan_mode=NESTED),
        "global": dict(select=[count(1), sum_(lprice), count(lprice), min_(lid)], scan_mode=NESTED),
        "mixed": dict(select=[k, count(1), sum_(lprice)], group_by=[k],
                      where=(lpos < 4) & (k > 7), scan_mode=NESTED),
        "distinct": dict(select=[k, cd(lpos), count(1)], group_by=[k], scan_mode=NESTED),
        "no-columns": dict(select=[count(1)], scan_mode=NESTED),
        "wr-group": dict(scan_select=[count(lpos), sum_(lprice), sum_(k)],
                         select=[out(2), count(1), sum_(out(0)), sum_(out(1))], group_by=[out(2)],
                         scan_mode=WR),
        "wr-global": dict(scan_select=[count(lprice), sum_(lprice), count(1)],
                          select=[sum_(out(0)), sum_(out(1)), sum_(out(2)), count(1)], scan_mode=WR),
    }


def oracle_chain(pname, kw):
    """(expected result, rows scanned, rows passed) of `kw` over the partition: the partial
    aggregates of every file (scan order, newest first, each under its filter), merged.
    PartitionCursor feeds ONE GroupByExpression, so a non-aggregate select expression keeps
    the group's first row in scan order (groupby.cc:161-172), while GroupByMergeExpression
    keeps the row it decodes LAST (groupby.cc:577-612, oracle/csql_merge.inc): the frames are
    handed to the merge oldest file first, which states exactly that first row; aggregates
    do not depend on the order.  test_first_rows_of_a_chain_against_numpy checks the first
    rows without the oracle."""
    files = list(reversed(LN.partition(pname)))
    S = LN.NESTED_LSM_SCHEMA
    frames, scanned, passed = [], 0, 0
    for f, flt in zip(files, oracle_filters(pname)):
        p = Plan(S, mode=K.MODE_PARTIAL, row_filter=flt, **kw)
        r = O.oracle_run(f[1], p)
        keys = [r.keys[20 * i:20 * i + 20] for i in range(r.nrows)]
        frames.append(O.partial_frame(keys, r.columns[0]))
        scanned += r.rows_scanned
        passed += r.rows_passed
    return O.oracle_merge(Plan(S, **kw), frames[::-1]), scanned, passed


@pytest.mark.parametrize("pname", sorted(LN.PARTITIONS))
def test_device_filters_of_nested_partitions(nested_chain, pname):
    ch, _ = nested_chain(pname)
    files = list(reversed(LN.partition(pname)))
    for i, e in enumerate(oracle_filters(pname)):
        f, kept = ch.filter(i)
        if e is None:
            assert f is None and kept == len(files[i][4]["ids"])
        else:
            assert f is not None and (f == e).all() and kept == int(e.sum())


@pytest.mark.parametrize("pname", sorted(LN.PARTITIONS))
def test_nested_scans_over_a_chain(nested_chain, pname):
    ch, _ = nested_chain(pname)
    S = LN.NESTED_LSM_SCHEMA
    for name, kw in chain_plans().items():
        exp, scanned, passed = oracle_chain(pname, kw)
        q = ch.query(Plan(S, **kw))
        try:
            first = None
            for _ in range(2):  # executing twice gives the same rows
                q.execute()
                got = q.fetch_all()
                assert got.nrows == exp.nrows, name
                T.compare_results(got.rows(), exp.rows(), exp.types,
                                  key_cols=len(kw.get("group_by", [])), rel=1e-6)
                rows = sorted(got.rows(), key=repr)
                assert first is None or rows == first, name
                first = rows
            st = q.stats()
            assert (st["rows_scanned"], st["rows_passed"]) == (scanned, passed), name
        except AssertionError as e:
            raise AssertionError("plan %s over %s: %s" % (name, pname, e))
        finally:
            q.close()


@pytest.mark.parametrize("pname", ["basic", "edges", "quiet"])
def test_first_rows_of_a_chain_against_numpy(nested_chain, pname):
    """non-aggregate select expressions over a chain keep the group's first flattened row in
    scan order -- newest file first, inside a file the first kept record's first slot
    ((file << 44 | flattened row) in chain_merge) -- computed here from the columns the
    files were written from: id, the string s, and the first slot's position / price (an
    undefined slot reads 0)"""
    ch, _ = nested_chain(pname)
    files = list(reversed(LN.partition(pname)))
    exp = {}
    for f, flt in zip(files, oracle_filters(pname)):
        c = f[4]
        keep = np.ones(len(c["ids"]), bool) if flt is None else flt
        for r in np.flatnonzero(keep):
            k = int(c["k"][r])
            slot = int(c["starts"][r])
            rows = int(max(c["cnt"][r], 1))
            if k not in exp:
                d = bool(c["defined"][slot])
                exp[k] = [k, int(c["id"][r]), c["s"][r], int(c["pos"][slot]) if d else 0,
                          int(c["price"][slot]) if d else 0, 0]
            exp[k][5] += rows
    kw = chain_plans()["parent-first"]
    kw = dict(kw, select=kw["select"][:6])
    q = ch.query(Plan(LN.NESTED_LSM_SCHEMA, **kw))
    got = sorted(q.run().rows())
    q.close()
    assert got == sorted(tuple(v) for v in exp.values())


def test_chain_partial_mode_and_order_by(nested_chain):
    """EVQL_MODE_PARTIAL over a chain: the (key, state) bytes of the merged groups, read as
    one more partial frame, merge to the expected rows; ORDER BY + LIMIT on the merged table"""
    S = LN.NESTED_LSM_SCHEMA
    for pname in ("basic", "edges"):
        ch, _ = nested_chain(pname)
        for name in ("leaf", "wr-group", "distinct"):
            kw = chain_plans()[name]
            exp, _, _ = oracle_chain(pname, kw)
            q = ch.query(Plan(S, mode=K.MODE_PARTIAL, **kw))
            rows = q.run().rows()
            q.close()
            merged = O.oracle_merge(Plan(S, **kw), [O.partial_frame([r[0] for r in rows],
                                                                    [r[1] for r in rows])])
            assert sorted(merged.rows()) == sorted(exp.rows()), (pname, name)
        kw = chain_plans()["leaf"]
        p = Plan(S, **kw)
        exp, _, _ = oracle_chain(pname, kw)
        q = ch.query(p)
        q.set_order(Order(p, [(1, True), (0, False)], limit=3, offset=1))
        assert q.run().rows() == sorted(exp.rows(), key=lambda r: (-r[1], r[0]))[1:4]
        q.close()


def test_one_file_chain_without_a_filter_is_the_plain_query(nested_chain):
    ch, tabs = nested_chain("single_plain")
    assert ch.filter(0)[0] is None
    S = LN.NESTED_LSM_SCHEMA
    for name, kw in chain_plans().items():
        q = ch.query(Plan(S, **kw))
        a = sorted(q.run().rows(), key=repr)
        sa = q.stats()
        q.close()
        q = tabs[0].query(Plan(S, **kw))
        b = sorted(q.run().rows(), key=repr)
        sb = q.stats()
        q.close()
        assert a == b, name
        assert (sa["rows_scanned"], sa["rows_passed"]) == (sb["rows_scanned"], sb["rows_passed"])


# ---------------------------------------------------------------------------------------
# seeded fuzz
# ---------------------------------------------------------------------------------------
FUZZ_SEEDS = range(60)
FUZZ_CAP = 6


def nested_fuzz_case(seed):
    """test_gpu_fuzz.test_random_nested_plan's draw for `seed`: (0 items / 1 testtbl, kw)"""
    _, items_cols, fixture_cols = F._nested_gens()
    which = seed % 2
    g = F.NestedGen(2000 + seed, **(items_cols if which == 0 else fixture_cols))
    g.two_level_hints = True
    if which == 0:
        g.leaf_uint, g.leaf_bool = ["items.position", "items.price"], []
    else:
        g.leaf_uint = ["event.search_query.result_items.position"]
        g.leaf_bool = ["event.search_query.result_items.clicked"]
    kw = g.plan_kwargs([1])
    kw.pop("row_end", None)
    kw["scan_mode"] = NESTED
    return which, kw


def within_fuzz_case(seed):
    """test_gpu_fuzz.test_random_within_record_plan's draw for `seed`"""
    _, items_cols, fixture_cols = F._nested_gens()
    which = seed % 2
    cols = items_cols if which == 0 else fixture_cols
    r = random.Random(7000 + seed)
    inner = []
    for _ in range(r.randint(1, 5)):
        c = col(r.choice(cols["uint_cols"]))
        inner.append(r.choice([lambda: count(c), lambda: sum_(c), lambda: count(1),
                               lambda: sum_(lit(r.choice([1, 3, 1000]))),
                               lambda: count(col(r.choice(cols["uint_cols"] + cols["bool_cols"])))
                               ])())
    inner.append(count(col(r.choice(cols["uint_cols"]))))
    outs = ["$%d" % i for i in range(len(inner))]
    g = F.Gen(8000 + seed, uint_cols=outs, float_cols=[], bool_cols=[], key_cols=outs,
              first_cols=outs, lits=[0, 1, 2, 5, 9, 40, 1000])
    g.flt = lambda depth=0: Lit(g.r.choice([0.0, 1.5, -2.25, 100.0]))
    kw = g.plan_kwargs([1])
    kw.pop("row_end", None)
    kw.pop("where", None)
    kw["scan_select"] = inner
    kw["scan_mode"] = WR
    return which, kw


def run_fuzz(draw, items, testtbl):
    """every seed under the record filter default_rng(seed).random(nrec) < 0.5.  A seed may
    end without a comparison only when Plan() raises CompileError, the oracle rejects the
    plan, or the library answers EVQL_ENOTSUP with the message it also gives for the SAME
    plan without the filter (the unfiltered path is the parent commit's); at most FUZZ_CAP
    of the seeds may end that way"""
    uncompared, failures = [], []
    for seed in FUZZ_SEEDS:
        which, kw = draw(seed)
        t, img, schema, nrec = ((items[0], items[1], N.ITEMS_SCHEMA, NREC) if which == 0 else
                                (testtbl[0], testtbl[1], N.NESTED_SCHEMA, 213))
        f = np.random.default_rng(seed).random(nrec) < 0.5
        try:
            plan = Plan(schema, row_filter=f, **kw)
        except CompileError:
            uncompared.append((seed, "CompileError"))
            continue
        try:
            exp, exp_err = O.oracle_run(img, plan), None
        except RuntimeError as e:
            exp, exp_err = None, str(e)
        try:
            q = t.query(plan)
        except E.EvqlError as e:
            if e.code != K.EVQL_ENOTSUP or "row filter on a nested scan" in e.msg or \
                    "nested scan over a chain" in e.msg:
                failures.append((seed, "refused: %s" % e.msg))
                continue
            try:
                t.query(Plan(schema, **kw)).close()
                failures.append((seed, "refused only under the filter: %s" % e.msg))
            except E.EvqlError as e2:
                if (e2.code, e2.msg) == (e.code, e.msg):
                    uncompared.append((seed, e.msg))
                else:
                    failures.append((seed, "refusals differ: %s / %s" % (e.msg, e2.msg)))
            continue
        try:
            if exp_err is not None:
                uncompared.append((seed, "oracle: " + exp_err))
                with pytest.raises(E.EvqlError) as ei:
                    q.run()
                assert ("zero" in exp_err) == ("zero" in ei.value.msg)
                continue
            got = q.run()
            assert got.nrows == exp.nrows
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=len(kw["group_by"]),
                              rel=1e-6, abs_tol=1e-3)
            assert q.stats()["rows_passed"] == exp.rows_passed
        except AssertionError as e:
            failures.append((seed, str(e)[:300]))
        finally:
            q.close()
    assert not failures, failures
    assert len(uncompared) <= FUZZ_CAP, uncompared
    return uncompared


def test_fuzz_nested_plans_under_a_record_filter(items, testtbl):
    """seeds 0..59 of test_random_nested_plan (even: items table, odd: testtbl_v2).
    Counted on the CPU: 0 of the 60 raise CompileError, 0 are rejected by the oracle under
    the filter, 0 are refused by the planner without the filter (compile_only, both
    tables); what materialize_nested refuses at run time is only seen here."""
    run_fuzz(nested_fuzz_case, items, testtbl)


def test_fuzz_within_record_plans_under_a_record_filter(items, testtbl):
    """seeds 0..59 of test_random_within_record_plan (restated in within_fuzz_case).
    Counted on the CPU: 0 of the 60 raise CompileError, 0 are rejected by the oracle under
    the filter, 0 are refused by the planner without the filter."""
    run_fuzz(within_fuzz_case, items, testtbl)
