"""Result materialisation on the device (Query.to_table / evql_table_from_query): the groups of
an executed GROUP BY become a resident cstable.  What the table holds is compared with the
oracle's rows of the inner plan (read back through a bare scan of the downloaded image on the
oracle); what its bytes are, with the image E.Writer makes of those rows."""
import ctypes as C
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Call, Order, Plan, col, count, lit, max_, mean, min_, sum_
import lsm_tables
import materialize_model as M
import nested_tables
import oracle_lib as O
import partial_emit_model as PM

pytestmark = pytest.mark.gpu


def materialised_rows(tab, specs):
    """(rows in table order, types) of a materialised table, read by the oracle"""
    res = M.scan_image(tab.download_image(), specs)
    return res.rows(), res.types


def check_stats(st, rows, sorted_by=None):
    assert st["rows"] == rows
    assert st["n_host_waits"] <= 3
    assert st["encode_ms"] >= 0 and st["sort_ms"] >= 0
    if rows:
        assert st["gather_ms"] > 0 and st["n_kernel_launches"] >= 1
    if sorted_by is None:
        assert st["presorted"] == 0 and st["passes"] == 0


# ---- 1. cell classes ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cells(ctx):
    img, c = M.cell_table()
    exp = O.oracle_run(img, M.cell_plan())
    t = ctx.open_image(img)
    yield t, exp
    t.close()


@pytest.mark.parametrize("sort_by", [None, "n", "t"])
def test_every_cell_class(cells, sort_by):
    t, exp = cells
    assert exp.nrows == M.CELL_GROUPS
    keys = [r[0] for r in exp.rows()]
    assert None in keys and M.M64 in keys  # record kinds 2 and 1
    by_key = {r[0]: r for r in exp.rows()}
    no_value = by_key[M.NO_VALUE_GROUP * 3 + 1]
    assert no_value[5] is None and no_value[6] is None and no_value[7] is None
    lens = {len(r[11]) for r in exp.rows()}
    assert {0, 1, 128} <= lens and sum(len(r[11]) for r in exp.rows()) > M.STRING_PAGE
    assert any(r[12] is None for r in exp.rows()) and any(r[13] is None for r in exp.rows())
    q = t.query(M.cell_plan(groups_hint=1000))
    q.execute()
    tab = q.to_table(M.CELL_SPECS, sort_by=sort_by)
    try:
        st = q.materialize_stats
        check_stats(st, M.CELL_GROUPS, sort_by)
        assert st["string_bytes"] == sum(len(r[11] or b"") + len(r[12] or b"") for r in exp.rows())
        assert tab.num_rows == M.CELL_GROUPS
        info = {c["name"]: c for c in tab.columns()}
        assert info["s"]["n_data_pages"] >= 2  # the heap spans two STRING_PLAIN pages
        got, types = materialised_rows(tab, M.CELL_SPECS)
        assert types == exp.types
        M.assert_rows_equal(got, exp.rows(), exp.types)
        if sort_by == "n":
            assert st["presorted"] == 1 and st["passes"] == 0  # every count is 10
        if sort_by == "t":
            ts = [r[14] for r in got]
            assert ts == sorted(ts)
    finally:
        tab.close()
        q.close()


# ---- 2. byte identity ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ids(ctx):
    img, c = M.id_table()
    exp = sorted(O.oracle_run(img, M.id_plan()).rows())
    t = ctx.open_image(img)
    q = t.query(M.id_plan(groups_hint=5000))
    q.execute()
    yield q, exp
    q.close()
    t.close()


@pytest.mark.parametrize("page_order", [K.PAGE_ORDER_COLUMNS, K.PAGE_ORDER_ROWS])
@pytest.mark.parametrize("enc", sorted(M.ID_SPECS))
def test_sorted_image_is_the_writers(ids, enc, page_order):
    q, exp = ids
    specs = M.ID_SPECS[enc]
    assert len(exp) == M.ID_GROUPS and any(r[3] is None for r in exp) and any(r[7] is None for r in exp)
    tab = q.to_table(specs, sort_by="k", page_order=page_order)
    try:
        got = tab.download_image()
        check_stats(q.materialize_stats, M.ID_GROUPS, "k")
        assert q.materialize_stats["string_bytes"] == sum(len(r[6]) + len(r[7] or b"") for r in exp)
    finally:
        tab.close()
    want = M.writer_image(specs, exp)
    assert len(got) == len(want) and got == want


# ---- 3. sizes at the borders --------------------------------------------------------------------
def run_key_case(ctx, groups, hint, where=None):
    img, c, rows = PM.key_table(max(groups, 1))
    kw = dict(groups_hint=hint)
    if where is not None:
        kw["where"] = where
    exp = sorted(O.oracle_run(img, M.key_plan(**({"where": where} if where is not None else {}))).rows())
    assert len(exp) == groups
    t = ctx.open_image(img)
    q = t.query(M.key_plan(**kw))
    try:
        q.execute()
        tab = q.to_table(M.KEY_SPECS, sort_by="k")
        try:
            st = q.materialize_stats
            check_stats(st, groups, "k")
            assert st["string_bytes"] == 0
            assert tab.num_rows == groups
            assert tab.download_image() == M.writer_image(M.KEY_SPECS, exp)
        finally:
            tab.close()
        tab = q.to_table(M.KEY_SPECS)
        try:
            check_stats(q.materialize_stats, groups)
            got, types = materialised_rows(tab, M.KEY_SPECS)
            assert sorted(got) == exp
        finally:
            tab.close()
    finally:
        q.close()
        t.close()


@pytest.mark.parametrize("groups", [1, M.SORT_TILE - 1, M.SORT_TILE, M.SORT_TILE + 1])
def test_sizes_around_the_sort_tile(ctx, groups):
    run_key_case(ctx, groups, 0)


def test_no_groups(ctx):
    run_key_case(ctx, 0, 0, where=col("k") > lit(10 ** 15))


@pytest.mark.parametrize("hint", [1000, 200_000, 0])
def test_seventy_thousand_groups(ctx, hint):
    """groups compacted from the HBM table, dense records of the partitioned path, the probe"""
    run_key_case(ctx, 70_001, hint)


def sorted_case(ctx, groups, stride, sort_by):
    img, c = M.sort_table(groups, stride)
    exp = O.oracle_run(img, M.sort_plan()).rows()
    ci = [s["name"] for s in M.SORT_SPECS].index(sort_by)
    t = ctx.open_image(img)
    q = t.query(M.sort_plan(groups_hint=2 * groups))
    try:
        q.execute()
        tab = q.to_table(M.SORT_SPECS, sort_by=sort_by)
        try:
            st = dict(q.materialize_stats)
            check_stats(st, groups, sort_by)
            got, types = materialised_rows(tab, M.SORT_SPECS)
        finally:
            tab.close()
    finally:
        q.close()
        t.close()
    vals = [r[ci] for r in got]
    assert vals == sorted(vals)
    assert sorted(got) == sorted(exp)
    return st


def test_presorted_keys_run_no_pass(ctx):
    # every count is 2: non-descending whatever the order of the records
    st = sorted_case(ctx, M.SORT_TILE + 1, 2, "n")
    assert st["presorted"] == 1 and st["passes"] == 0


def test_one_digit_pass(ctx):
    st = sorted_case(ctx, M.SORT_TILE + 1, 2, "b")  # 0 .. 199
    assert st["presorted"] == 0 and st["passes"] == 1


@pytest.mark.parametrize("sort_by", ["k", "r"])
def test_three_digit_passes(ctx, sort_by):
    # key range 64 * 2048 = 2^17: three digits; r = 2^40 - k mirrors the order of k
    st = sorted_case(ctx, M.SORT_TILE + 1, 64, sort_by)
    assert st["presorted"] == 0 and st["passes"] == 3


def test_reverse_sorted_keys(ctx):
    """two groups: the records lie in one of two orders, and r = 2^40 - k descends where k
    ascends -- one of the two sort columns meets reverse-sorted input, the other presorted.
    The same mirror pair at 3 * 2048 + 1 groups: every ascent of one column is a descent of
    the other."""
    by_k = sorted_case(ctx, 2, 2, "k")
    by_r = sorted_case(ctx, 2, 2, "r")
    assert sorted([by_k["presorted"], by_r["presorted"]]) == [0, 1]
    assert sorted([by_k["passes"], by_r["passes"]]) == [0, 1]
    for sort_by in ("k", "r"):
        st = sorted_case(ctx, 3 * M.SORT_TILE + 1, 2, sort_by)
        assert st["presorted"] == 0 and st["passes"] == 2  # range 2 * 6144: 14 bits


# ---- 4. other record sources --------------------------------------------------------------------
def test_chain_of_two_files(ctx):
    files = lsm_tables.partition("basic")[:2]
    filters = O.oracle_partition_filters(files)
    scan = list(reversed(files))
    S = lsm_tables.LSM_SCHEMA
    kw = dict(select=[col("a"), count(1), sum_(col("rid")), max_(col("k"))], group_by=[col("a")])
    specs = [M.U64("a"), M.LEB("n"), M.U64("sum_rid"), M.BP("max_k")]
    exp = sorted(O.oracle_run_chain([f[1] for f in scan], filters, Plan(S, **kw)).rows())
    assert len(exp) > M.SORT_TILE
    tabs = [ctx.open_image(f[1]) for f in scan]
    ch = E.LsmChain(ctx)
    for t, f in zip(tabs, scan):
        ch.add(t, has_skiplist=f[2], has_updates=f[3])
    ch.build()
    q = ch.query(Plan(S, groups_hint=10_000, **kw))
    try:
        q.execute()
        tab = q.to_table(specs, sort_by="a")
        try:
            check_stats(q.materialize_stats, len(exp), "a")
            assert tab.download_image() == M.writer_image(specs, exp)
        finally:
            tab.close()
        # first-row columns do not come out of merged records
        q2 = ch.query(Plan(S, select=[col("a"), count(1), col("s")], group_by=[col("a")],
                           groups_hint=10_000))
        try:
            q2.execute()
            with pytest.raises(E.EvqlError) as ei:
                q2.to_table([M.U64("a"), M.LEB("n"), M.STR("s")])
            assert ei.value.code == K.EVQL_ENOTSUP and "merged" in ei.value.msg
            assert q2.fetch_all().nrows == len(exp)
        finally:
            q2.close()
    finally:
        q.close()
        ch.close()
        for t in tabs:
            t.close()


def test_two_rank_hub_exchange(ctx):
    """every rank ends with all groups in its merged table and materialises them"""
    parts = [PM.key_table(M.SORT_TILE + 1), PM.key_table(M.SORT_TILE - 1)]
    w = E.Writer(PM.KEY_COLUMNS)
    for name in ("k", "a"):
        w.put(name, np.concatenate([p[1][name] for p in parts]))
    w.commit(sum(p[2] for p in parts))
    whole = w.image()
    w.close()
    exp = sorted(O.oracle_run(whole, M.key_plan()).rows())
    assert len(exp) == M.SORT_TILE + 1
    want = M.writer_image(M.KEY_SPECS, exp)
    first_row_plan = dict(select=[col("k"), count(1), col("a")], group_by=[col("k")])
    hub = E.Hub(2)
    out, errs = [None, None], []

    def work(r):
        try:
            c = E.Context(0)
            t = c.open_image(parts[r][0])
            x = E.Exchange.hub(c, hub, r)
            q = t.query(M.key_plan())
            q.execute()
            q.exchange(x, K.EXCHANGE_GATHER_ALL)
            tab = q.to_table(M.KEY_SPECS, sort_by="k")
            img = tab.download_image()
            st = q.materialize_stats
            tab.close()
            rows = sorted(q.fetch_all().rows())
            q.close()
            # the same merged query with a first-row column
            q = t.query(Plan(PM.KEY_SCHEMA, **first_row_plan))
            q.execute()
            q.exchange(x, K.EXCHANGE_GATHER_ALL)
            refusal = None
            try:
                q.to_table([M.U64("k"), M.LEB("n"), M.U64("a")]).close()
            except E.EvqlError as e:
                refusal = (e.code, e.msg)
            nrows = q.fetch_all().nrows
            q.close()
            out[r] = (img, st, rows, refusal, nrows)
            x.close()
            t.close()
            c.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    assert not errs, errs
    hub.close()
    for img, st, rows, refusal, nrows in out:
        check_stats(st, len(exp), "k")
        assert img == want
        assert rows == exp
        assert refusal is not None and refusal[0] == K.EVQL_ENOTSUP and "merged" in refusal[1]
        assert nrows == len(exp)


# ---- 5. it is a table ---------------------------------------------------------------------------
def test_outer_group_by_over_the_materialised_table(ctx):
    """a histogram of the inner counts; the table still answers after the query is closed"""
    img, c, rows = PM.key_table(70_001)
    inner = dict(select=[col("a"), count(1), sum_(col("k"))], group_by=[col("a")])
    specs = [M.BP("a"), M.LEB("n"), M.U64("sum_k")]
    inner_rows = sorted(O.oracle_run(img, Plan(PM.KEY_SCHEMA, **inner)).rows())
    assert len(inner_rows) == 977
    S2 = M.schema_of(specs)
    outer = dict(select=[col("n"), count(1), sum_(col("sum_k")), max_(col("a"))], group_by=[col("n")])
    exp = O.oracle_run(M.writer_image(specs, inner_rows), Plan(S2, **outer))
    assert exp.nrows >= 2
    t = ctx.open_image(img)
    q = t.query(Plan(PM.KEY_SCHEMA, groups_hint=1000, **inner))
    q.execute()
    tab = q.to_table(specs)
    q.close()
    t.close()
    try:
        assert tab.schema() == S2
        q2 = tab.query(Plan(S2, **outer))
        got = q2.run()
        q2.close()
        assert sorted(got.rows()) == sorted(exp.rows())
    finally:
        tab.close()


def test_zone_maps_prune_a_sorted_table(ctx):
    groups = 3 * M.SORT_TILE + 1
    img, c = M.sort_table(groups, 2)
    inner_rows = sorted(O.oracle_run(img, M.sort_plan()).rows())
    t = ctx.open_image(img)
    q = t.query(M.sort_plan(groups_hint=2 * groups))
    q.execute()
    tab = q.to_table(M.SORT_SPECS, sort_by="k")
    q.close()
    t.close()
    try:
        zmin, zmax = tab.zone_map("k")
        assert len(zmin) == 4 and (zmax[:-1] < zmin[1:]).all()
        bound = inner_rows[2 * groups // 3][0]
        S2 = M.schema_of(M.SORT_SPECS)
        kw = dict(select=[count(1), sum_(col("r")), max_(col("k"))], where=col("k") >= lit(bound))
        exp = O.oracle_run(M.writer_image(M.SORT_SPECS, inner_rows), Plan(S2, **kw))
        q2 = tab.query(Plan(S2, **kw))
        got = q2.run()
        zs = q2.zone_stats()
        q2.close()
        assert got.rows() == exp.rows() and got.rows()[0][0] == groups - 2 * groups // 3
        assert zs["tiles_skipped"] > 0 and zs["zones_excluded"] >= 2
    finally:
        tab.close()


# ---- 6. the query is untouched ------------------------------------------------------------------
@pytest.mark.parametrize("when", ["before_fetch", "after_fetch"])
def test_query_is_untouched(ctx, when):
    img, c = M.id_table()
    specs = M.ID_SPECS["leb128"]
    t = ctx.open_image(img)
    try:
        fresh = t.query(M.id_plan(groups_hint=5000))
        want = sorted(fresh.run().rows())
        fresh.close()
        q = t.query(M.id_plan(groups_hint=5000))
        q.execute()
        first = None
        if when == "after_fetch":
            n, raw = q.next_batch(1024)
            assert n == 1024
            first = raw
        tab = q.to_table(specs, sort_by="k")
        img1 = tab.download_image()
        st1 = dict(q.materialize_stats)
        tab.close()
        tab = q.to_table(specs, sort_by="k")
        img2 = tab.download_image()
        tab.close()
        assert img1 == img2
        check_stats(st1, M.ID_GROUPS, "k")
        assert st1["string_bytes"] == sum(len(r[6]) + len(r[7] or b"") for r in want)
        rest = q.fetch_all()
        if when == "before_fetch":
            assert sorted(rest.rows()) == want
        else:
            assert rest.nrows == M.ID_GROUPS - 1024
            whole = [a + b for a, b in zip(first, rest.raw)]
            from eventql_amd.plan import unpack_svector
            cols = [unpack_svector(ty, r) for ty, r in zip(rest.types, whole)]
            assert sorted(zip(*cols)) == want
        q.close()
    finally:
        t.close()


# ---- 7. refusals --------------------------------------------------------------------------------
def refused(q, specs, code, text, **kw):
    with pytest.raises(E.EvqlError) as ei:
        q.to_table(specs, **kw).close()
    assert ei.value.code == code, (ei.value.code, ei.value.msg)
    assert text in ei.value.msg, ei.value.msg


def test_refusals(ctx):
    img, c = M.id_table()
    S = M.ID_SCHEMA
    k, a, nb, fv, s = col("k"), col("a"), col("nb"), col("fv"), col("s")
    base = [M.U64("k"), M.U64("x")]
    t = ctx.open_image(img)

    def run(select, group_by=(k,), execute=True, **kw):
        q = t.query(Plan(S, select=select, group_by=list(group_by), groups_hint=5000, **kw))
        if execute:
            q.execute()
        return q

    try:
        NS, AR = K.EVQL_ENOTSUP, K.EVQL_EARG
        cases = [
            (run([k, sum_(a) + 1]), base, NS, "post-aggregate", {}),
            (run([k, sum_(fv)], float_sum_mode=K.FLOAT_SUM_EXACT, float_sum_bound=1e6),
             [M.U64("k"), M.F64("x")], NS, "exact float sum", {}),
            (run([k, sum_(Call("add", a, lit(-5)))]), base, NS, "INT64", {}),
            (run([k, Call("to_nil", a), count(1)]), base + [M.U64("n")], NS, "NIL", {}),
            (run([Call("add", a, lit(1)), count(1)], group_by=[Call("add", a, lit(1))]), base, NS,
             "computed key", {}),
            (run([k, Call("add", a, lit(1)), count(1)]), base + [M.U64("n")], NS, "not a first-row bare column", {}),
            (run([k] * 32 + [count(1)]), [M.U64("c%d" % i) for i in range(33)], NS, "more than 32", {}),
            (run([k, min_(nb)]), [M.U64("k"), M.U64("m", dlevel_max=1)], NS, "optional", dict(sort_by="m")),
            (run([k, fv]), [M.U64("k"), M.F64("fv")], NS, "not an unsigned-integer", dict(sort_by="fv")),
            (run([k, count(1)], execute=False), base, AR, "not executed", {}),
            (run([k, count(1)], mode=K.MODE_PARTIAL), base, AR, "PARTIAL", {}),
            (run([k, count(1)]), base + [M.U64("y")], AR, "3 column specs for 2", {}),
            (run([k, count(1)]), [M.U64("k"), M.U64("x", rlevel_max=1)], AR, "repeated / nested", {}),
            (run([k, count(1)]), [M.U64("k"), M.U64("x", dlevel_max=2)], AR, "repeated / nested", {}),
            (run([k, count(1)]), base, AR, "page order", dict(page_order=7)),
            (run([k, count(1)]), [M.U64("k"), M.F64("x")], AR, "type", {}),
            (run([k, mean(a)]), base, AR, "type", {}),
            (run([k, s]), [M.U64("k"), M.U64("s")], AR, "type", {}),
        ]
        for q, specs, code, text, kw in cases:
            try:
                refused(q, specs, code, text, **kw)
            finally:
                q.close()
        # ORDER BY / LIMIT set
        plan = Plan(S, select=[k, count(1)], group_by=[k], groups_hint=5000)
        q = t.query(plan)
        q.set_order(Order(plan, [(0, False)], limit=5))
        q.execute()
        refused(q, base, NS, "ORDER BY / LIMIT")
        q.close()
        # a bare scan
        q = t.query(Plan(S, scan_select=[k, a]))
        q.execute()
        refused(q, base, NS, "bare scan")
        q.close()
        # a sort column outside the columns (the python layer checks names: the C call itself)
        q = run([k, count(1)])
        cs, _keep = E.LsmChain._column_specs(base)
        tab = C.c_void_p()
        for sc in (2, -2):
            rc = E.lib().evql_table_from_query(q.h, cs, 2, sc, K.PAGE_ORDER_COLUMNS, C.byref(tab), None)
            assert rc == K.EVQL_EARG and "sort column" in E.last_error() and not tab.value
        assert E.lib().evql_table_from_query(q.h, cs, 2, -1, K.PAGE_ORDER_COLUMNS, None, None) == K.EVQL_EARG
        with pytest.raises(E.EvqlError) as ei:
            q.to_table(base, sort_by="nope")
        assert ei.value.code == K.EVQL_EARG
        # ... and the query still materialises
        tab2 = q.to_table(base, sort_by="k")
        assert tab2.num_rows == M.ID_GROUPS
        tab2.close()
        q.close()
    finally:
        t.close()


def test_first_row_columns_of_a_nested_scan_are_refused(ctx):
    S = nested_tables.ITEMS_SCHEMA
    t = ctx.open_image(nested_tables.items_table(2000)[0])
    try:
        sel = [col("id"), col("items.position"), count(1)]
        q = t.query(Plan(S, select=sel, group_by=[col("id"), col("items.position")],
                         scan_mode=K.SCAN_NESTED, groups_hint=20_000))
        q.execute()
        refused(q, [M.U64("id"), M.U64("p", dlevel_max=1), M.U64("n")], K.EVQL_ENOTSUP, "nested scan")
        assert q.fetch_all().nrows > 2000
        q.close()
    finally:
        t.close()


def test_null_in_a_required_column(ctx):
    img, c = M.cell_table()
    exp = O.oracle_run(img, M.cell_plan())
    t = ctx.open_image(img)
    q = t.query(M.cell_plan(groups_hint=1000))
    try:
        q.execute()
        for name in ("nk", "min_nb", "mean_nb", "ns", "nu"):
            specs = [dict(sp, dlevel_max=0) if sp["name"] == name else sp for sp in M.CELL_SPECS]
            refused(q, specs, K.EVQL_ERUNTIME, "NULL in required column " + name)
        # ... and the query stays usable
        tab = q.to_table(M.CELL_SPECS)
        got, types = materialised_rows(tab, M.CELL_SPECS)
        tab.close()
        M.assert_rows_equal(got, exp.rows(), exp.types)
        M.assert_rows_equal(q.fetch_all().rows(), exp.rows(), exp.types)
    finally:
        q.close()
        t.close()
