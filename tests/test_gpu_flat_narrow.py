"""Narrow copies as flat arrays and page-table entries read through the
constant address space: every plan runs over a table opened with EVQL_NARROW_PLAIN=1 and over
the same image opened with 0, both are compared with the oracle and with each other.  Row
counts sit around every border of the layout: one pair, one wave, one tile (8192 / 16384
rows), a 65,536-value page of the file, a 131,072-value unit of the copy."""
import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K, synth
from eventql_amd.plan import Plan, col, count, max_, min_, out, sum_
import oracle_lib as O
import tables as T
from test_gpu_narrow_plain import FLOAT, UINT, check, lsm_file, open_table, write

pytestmark = pytest.mark.gpu

k, a, b, v = col("k"), col("a"), col("b"), col("v")
CONFIG3 = dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k],
               where=(a > 30000) & (b < 30000), groups_hint=1000)
CONFIG2 = dict(select=[k, sum_(v), count(1)], group_by=[k], groups_hint=1000)
UNGROUPED = dict(select=[count(1), sum_(a), min_(b), max_(b), sum_(v)], where=a > 30000)
FIRST_ROW = dict(select=[k, a, b, v, count(1)], group_by=[k], groups_hint=1000)
BARE = dict(scan_select=[k, b + 1, v * 2.0, a], where=(a > 30000) & (b < 30000))

ROWS = [1, 127, 129, 8191, 8193, 16385, 65536 + 3, 131072 + 5, 3 * 131072 + 8191]


def flat(i, bits):
    """the page-less overload of the width's accessor: (base, row, ...), no `.pages`"""
    return "evql_bitpacked_x2<%d>(A.col[%d].base, r, " % (bits, i)


def check_bare(tn, tp, img, schema, **kw):
    plan = Plan(schema, **kw)
    exp = O.oracle_run(img, plan)
    for t in (tn, tp):
        q = t.query(plan)
        try:
            got = q.run()
            assert got.nrows == exp.nrows
            assert got.rows() == exp.rows() and got.raw == exp.raw
            assert q.stats()["rows_passed"] == exp.rows_passed
        finally:
            q.close()


@pytest.mark.parametrize("n", ROWS)
def test_every_plan_at_every_border(ctx, n):
    c = synth.table_columns(n)
    img = write([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        sn, sp = check(tn, tp, img, B.SCHEMA, **CONFIG3)
        # a, b < 65536 from a few hundred rows on; the switch off reads the file's pages
        wa = 8 if int(c["a"].max()) < 256 else 16
        assert flat(0, wa) in sn and "evql_bitpacked_x2<" not in sp
        assert "evql_plain64_x2(A.col[0].base, A.col[0].pages" in sp
        check(tn, tp, img, B.SCHEMA, **CONFIG2)
        check(tn, tp, img, B.SCHEMA, key_cols=0, **UNGROUPED)
        check(tn, tp, img, B.SCHEMA, **FIRST_ROW)
        check_bare(tn, tp, img, B.SCHEMA, **BARE)
        lo, hi = (n // 3) | 1, n - n // 5 - (n > 4)  # an odd first row, an end short of n
        if lo < hi:
            check(tn, tp, img, B.SCHEMA, row_begin=lo, row_end=hi, **CONFIG3)
            check(tn, tp, img, B.SCHEMA, key_cols=0, row_begin=lo, **UNGROUPED)
    finally:
        tn.close()
        tp.close()


@pytest.mark.parametrize("top,bits", [(255, 8), (256, 16), (65535, 16), (65536, 32),
                                      ((1 << 32) - 1, 32), (1 << 32, 0)])
def test_maxima_at_each_width(ctx, top, bits):
    """x takes its maximum in its LAST row, behind a unit border of the copy: the value that
    sets the width is the one nearest the zero fill"""
    n = 131072 + 5
    rng = np.random.default_rng(top % 1000003)
    x = rng.integers(0, top, n, dtype=np.uint64)
    x[n - 1] = top
    c = dict(g=rng.integers(0, 41, n, dtype=np.uint64), x=x,
             y=rng.integers(0, 1 << 63, n, dtype=np.uint64))
    S = dict(g=K.T_UINT64, x=K.T_UINT64, y=K.T_UINT64)
    img = write([UINT("g"), UINT("x"), UINT("y")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        g, xx, y = col("g"), col("x"), col("y")
        sn, _ = check(tn, tp, img, S, select=[g, sum_(xx), max_(xx), min_(xx), count(1), sum_(y)],
                      group_by=[g], where=xx > top // 3, groups_hint=64)
        # scan columns in order of first use: x (WHERE), g, y
        assert (flat(0, bits) if bits else "evql_plain64_x2(A.col[0].") in sn
        assert flat(1, 8) in sn and "evql_plain64_x2(A.col[2]." in sn
        check(tn, tp, img, S, key_cols=0, select=[max_(xx), sum_(xx), count(1)], where=xx >= top)
        check(tn, tp, img, S, select=[g, xx, count(1)], group_by=[g], row_begin=n - 1, groups_hint=64)
    finally:
        tn.close()
        tp.close()


def test_partitioned_path_with_a_narrowed_key(ctx):
    n = 3 * 131072 + 8191
    c = synth.table_columns(n)
    c["u"] = c["x"] % np.uint64(200_000)
    img = write([UINT("u"), UINT("a"), FLOAT("v")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        u = col("u")
        sn, sp = check(tn, tp, img, B.SCHEMA, select=[u, sum_(a), count(1), sum_(v)], group_by=[u],
                       groups_hint=200_000)
        assert "evql_part_scatter" in sn and "evql_part_scatter" in sp
        assert flat(0, 32) in sn and flat(1, 16) in sn
    finally:
        tn.close()
        tp.close()


def test_zone_map_query_over_a_narrowed_column(ctx):
    """an ascending 16-bit column: its zone map is read from the flat copy (k_zone_minmax's
    8-values-per-thread branch), the query skips tiles and still matches the oracle"""
    n = 3 * 131072 + 8191
    c = synth.table_columns(n)
    c["s"] = np.arange(n, dtype=np.uint64) // np.uint64(7)
    S = dict(B.SCHEMA, s=K.T_UINT64)
    img = write([UINT("s"), UINT("k"), UINT("b"), FLOAT("v")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        s = col("s")
        kw = dict(select=[k, count(1), sum_(b), sum_(v)], group_by=[k],
                  where=(s >= 20011) & (s < 41003), groups_hint=1000)
        sn, _ = check(tn, tp, img, S, **kw)
        assert flat(0, 16) in sn
        for t in (tn, tp):
            q = t.query(Plan(S, **kw))
            q.run()
            assert q.zone_stats()["tiles_skipped"] > 0
            q.close()
        want_min = c["s"][::2048]
        want_max = np.append(c["s"][2047::2048], c["s"][-1])[:len(want_min)]
        for t in (tn, tp):
            zmin, zmax = t.zone_map("s")
            assert zmin.tolist() == want_min.tolist() and zmax.tolist() == want_max.tolist()
        # a zone that ends inside a thread's 8 values: n is no multiple of 8
        zmin, zmax = tn.zone_map("b")
        bb = c["b"]
        assert zmin[-1] == bb[(n // 2048) * 2048:].min() and zmax[-1] == bb[(n // 2048) * 2048:].max()
        assert zmax[3] == bb[3 * 2048:4 * 2048].max()
    finally:
        tn.close()
        tp.close()


def test_leb128_table(ctx):
    """required LEB128 columns narrow whatever the switch says: both tables read flat arrays"""
    n = 131072 + 5
    c = synth.table_columns(n)
    leb = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT,  # noqa: E731
                            storage_type=K.ENC_UINT64_LEB128)
    img = write([leb("k"), leb("a"), leb("b"), FLOAT("v")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        sn, sp = check(tn, tp, img, B.SCHEMA, **CONFIG3)
        assert flat(0, 16) in sn and flat(0, 16) in sp
        check(tn, tp, img, B.SCHEMA, **FIRST_ROW)
        check(tn, tp, img, B.SCHEMA, row_begin=8191, row_end=131073, **CONFIG3)
        check_bare(tn, tp, img, B.SCHEMA, **BARE)
    finally:
        tn.close()
        tp.close()


def test_nested_table_through_the_packed_flattened_columns(ctx):
    """the config 5 / 5w shapes: the flattened columns are packed into flat arrays"""
    import nested_tables as N
    img, _ = N.items_table(20_000)
    pos, price = col("items.position"), col("items.price")
    plans = [Plan(N.ITEMS_SCHEMA, select=[pos, count(1), sum_(price)], group_by=[pos],
                  scan_mode=K.SCAN_NESTED, groups_hint=16),
             Plan(N.ITEMS_SCHEMA, select=[pos, price, count(1)], group_by=[pos], where=price > 7,
                  scan_mode=K.SCAN_NESTED, groups_hint=16),
             Plan(N.ITEMS_SCHEMA, scan_select=[count(pos), sum_(price)],
                  select=[out(0), count(1), sum_(out(1))], group_by=[out(0)],
                  scan_mode=K.SCAN_NESTED_WITHIN_RECORD, groups_hint=16)]
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        for i, plan in enumerate(plans):
            exp = O.oracle_run(img, plan)
            rows = []
            for t in (tn, tp):
                q = t.query(plan)
                try:
                    got = q.run()
                    assert got.nrows == exp.nrows
                    T.compare_results(got.rows(), exp.rows(), exp.types)
                    rows.append(sorted(map(repr, got.rows())))
                    if i == 0:
                        assert "evql_bitpacked_x2<" in q.kernel_source()
                        assert ".pages, r" not in q.kernel_source()
                finally:
                    q.close()
            assert rows[0] == rows[1]
    finally:
        tn.close()
        tp.close()


def test_chain_of_two_files_of_different_widths(ctx):
    """k fits 8 bits in the older file and 16 in the newer; a 16 / 32; rid 16 / not at all"""
    rng = np.random.default_rng(11)
    S = dict(rid=K.T_UINT64, k=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64)
    shape = [(16_385, 0, 1, 200, 60_000, 0), (131_072 + 5, 1, 1, 50_000, 1 << 20, 1 << 33)]
    total = sum(f[0] for f in shape)
    files = []
    for fi, (n, skl, upd, kt, at, rb) in enumerate(shape):
        img, c = lsm_file(rng, fi, n, bool(skl), total // 2, kt, at, rb)
        files.append(("f%d" % fi, img, bool(skl), bool(upd), c))
    filters = O.oracle_partition_filters(files)
    scan = list(reversed(files))
    imgs = [f[1] for f in scan]
    rid, kk, aa, vv = col("rid"), col("k"), col("a"), col("v")
    kw = dict(select=[kk, rid, count(1), sum_(aa), max_(aa), sum_(vv)], group_by=[kk],
              where=aa > 1000, groups_hint=1000)
    exp = O.oracle_run_chain(imgs, filters, Plan(S, **kw))
    results = {}
    for narrow in (1, 0):
        tabs = [open_table(ctx, img, narrow) for img in imgs]
        ch = E.LsmChain(ctx)
        for t, f in zip(tabs, scan):
            ch.add(t, has_skiplist=f[2], has_updates=f[3])
        ch.build()
        q = ch.query(Plan(S, **kw))
        try:
            got = q.run()
            assert got.nrows == exp.nrows
            T.compare_results(got.rows(), exp.rows(), exp.types)
            assert q.stats()["rows_passed"] == exp.rows_passed
            results[narrow] = got.rows()
        finally:
            q.close()
        if narrow:  # scan columns: a, k, rid; newest file first
            srcs = []
            for t in tabs:
                pq = t.query(Plan(S, **kw))
                srcs.append(pq.kernel_source())
                pq.close()
            assert flat(0, 32) in srcs[0] and flat(1, 16) in srcs[0]
            assert "evql_plain64_x2(A.col[2]." in srcs[0]
            assert flat(0, 16) in srcs[1] and flat(1, 8) in srcs[1] and flat(2, 16) in srcs[1]
        ch.close()
        for t in tabs:
            t.close()
    assert sorted(r[:5] for r in results[1]) == sorted(r[:5] for r in results[0])
