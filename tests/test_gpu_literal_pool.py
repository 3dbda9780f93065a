"""Numeric literals travel in the kernel arguments (EvqlArgs::lit): every kernel family
reads the values of ITS launch, and a query that differs from an earlier one only in such
values runs without a compile.  HIP path against the C oracle (exact-mode float sums
against the quantum rule restated in float_edges.py, as test_gpu_float_edges.py does).

The module runs on a context and an on-disk kernel cache of its own, both empty at the
start, so that `kernel_cache_stats().compiles` counts exactly the hiprtc compiles of the
plans below.  The rule every sweep checks: the first literal of a shape may compile (its
plan, and what the table needs once -- the dictionary-build plan, the exact-offset twin of
a partitioned plan whose buckets overflow, one plan per file of a chain); no later literal
compiles anything.

Not covered: a hint-less plan over >= 8 Mi rows (the cardinality probe).  No fixture of the
suite has such a table below the 2e5 rows these tests stay under; the probe launches through
the same fill_host_args as every launch checked here."""
import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import If, Plan, col, count, count_distinct, lit, sum_
import float_edges as F
import lsm_nested_tables as LN
import nested_tables as N
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

ROWS = 100_000
NREC = 20_000
S = T.MIXED_SCHEMA
k, a, b, v, s = [col(x) for x in "kabvs"]
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def pctx(built, tmp_path_factory):
    """a context without modules over an empty kernel cache directory"""
    E.lib().evql_set_kernel_cache_dir(str(tmp_path_factory.mktemp("kcache")).encode())
    c = E.Context(0)
    yield c
    c.close()
    E.lib().evql_set_kernel_cache_dir(E.KERNEL_CACHE_DIR.encode())


@pytest.fixture(scope="module")
def mixed(pctx):
    img, c = T.mixed_table(ROWS)
    t = pctx.open_image(img)
    yield t, img, c
    t.close()


def compiles(ctx):
    return ctx.kernel_cache_stats().compiles


def run_plan(t, img, plan, key_cols, raw=False, expect_source=()):
    """one query against the oracle; returns (rows passed, result rows)"""
    exp = O.oracle_run(img, plan)
    q = t.query(plan)
    try:
        src = q.kernel_source()
        for word, present in expect_source:
            assert (word in src) == present, word
        got = q.run()
        assert got.nrows == exp.nrows, (got.nrows, exp.nrows)
        if raw:
            assert got.raw == exp.raw
        else:
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=key_cols, rel=1e-6)
        st = q.stats()
        assert st["rows_passed"] == exp.rows_passed
        return exp.rows_passed, got.rows()
    finally:
        q.close()


def sweep(ctx, t, img, schema, make_kw, lits, key_cols, **kw):
    """every literal against the oracle; only the first one may compile"""
    passed, after_first = [], None
    for L in lits:
        before = compiles(ctx)
        try:
            p, _ = run_plan(t, img, Plan(schema, **make_kw(L)), key_cols, **kw)
        except AssertionError as e:
            raise AssertionError("literal %r: %s" % (L, e))
        passed.append(p)
        if after_first is None:
            assert compiles(ctx) >= before + 1, "the shape was compiled before this sweep"
            after_first = compiles(ctx)
        assert compiles(ctx) == after_first, "literal %r was compiled" % (L,)
    return passed


EDGES = [0, 1, 65535, 1 << 31, 1 << 32, 1 << 63, (1 << 64) - 1]


def test_sweep_on_one_context(pctx, mixed):
    """select k, sum(a), count(1) where a > L1 and b < L2 group by k over 8 x 8 literals
    (a, b in [0, 65535]; a is read from bit-packed pages, b from 8-byte words): every
    result is the oracle's, and the whole sweep costs ONE compile"""
    t, img, _ = mixed
    l1s, l2s = EDGES + [30000], EDGES + [41000]
    before = compiles(pctx)
    hits = pctx.kernel_cache_stats().memory_hits
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(select=[k, sum_(a), count(1)], group_by=[k],
                                  where=(a > L[0]) & (b < L[1]), groups_hint=1000),
                   [(x, y) for x in l1s for y in l2s], 1)
    st = pctx.kernel_cache_stats()
    assert st.compiles == before + 1
    assert st.memory_hits == hits + 63
    assert len(set(passed)) >= 4 and 0 in passed and max(passed) > ROWS * 0.9, sorted(set(passed))


def test_ungrouped(pctx, mixed):
    t, img, _ = mixed
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(select=[count(1), sum_(a + L[1])], where=b > L[0]),
                   [(30000, 0), (0, 1 << 40), (65535, 7), (12345, (1 << 64) - 1)], 0)
    assert len(set(passed)) == 4


@pytest.mark.parametrize("shape", ["one-level", "two-level", "overflow"])
def test_partitioned_path(pctx, mixed, shape):
    """groups_hint beyond the LDS table: count / scatter / (refine) / aggregate.  `overflow`:
    three keys under a hint of 3e6 groups put every tuple into three coarse buckets, which
    outgrow their slack -- the launch is void and runs again with exact offsets from
    evql_part_count, literals and all.

    The sum's argument b + L travels in the tuple, as 32 bits while its bound (the maximum
    of b, 65535, plus L) stays below 2^32 - 1 (value_bounds.cc choose_tuple_widths).  The
    first sweep keeps every L below that, 2^31 included; L = 2^33 is another tuple layout,
    so another shape: it compiles, once, and a second wide L does not"""
    t, img, _ = mixed
    key, hint = {"one-level": (a, 100_000), "two-level": (a, 3_000_000),
                 "overflow": (k % 3 + 17, 3_000_000)}[shape]
    src = [("evql_part_scatter", True), ("evql_part_refine", shape != "one-level")]
    mk = lambda L: dict(select=[key, count(1), sum_(b + L[1])], group_by=[key],  # noqa: E731
                        where=b > L[0], groups_hint=hint)
    passed = sweep(pctx, t, img, S, mk,
                   [(100, 5), (30000, 1 << 31), (0, 0), (60000, 9)], 1, expect_source=src)
    assert len(set(passed)) == 4 and max(passed) > ROWS * 0.9
    wide = sweep(pctx, t, img, S, mk, [(30000, 1 << 33), (100, 1 << 40), (60000, (1 << 50) + 1)],
                 1, expect_source=src)
    assert wide == [passed[1], passed[0], passed[3]]


def test_count_distinct(pctx, mixed):
    """count_distinct((a + L) / 4096): 16 values per group for L = 0, 17 for L = 2048"""
    t, img, _ = mixed
    sweep(pctx, t, img, S,
          lambda L: dict(select=[k % 10, count_distinct((a + L) / 4096), count(1)],
                         group_by=[k % 10]),
          [0, 2048, 1 << 20, 4095], 1)


def test_exact_float_sum_follows_the_literal(pctx):
    """EVQL_FLOAT_SUM_EXACT with sum(xp * L): the bound of the argument, and with it the
    quantum, is derived per query from L; the kernel is the same.  Bit-equal to the terms
    rounded to that quantum and added exactly"""
    img, c = F.exact_table(100_003)
    t = pctx.open_image(img)
    try:
        after_first = None
        exps = set()
        for L in (1.0, 3.0, -0.001, 1e200):
            q = t.query(Plan(F.EXACT_SCHEMA, select=[col("g"), sum_(col("xp") * L)],
                             group_by=[col("g")], float_sum_mode=K.FLOAT_SUM_EXACT))
            rows = q.run().rows()
            q.close()
            terms = c["xp"] * np.float64(L)
            e = F.exact_quantum_exp(float(np.max(np.abs(c["xp"]))) * abs(L))
            exps.add(e)
            exp = [(g, F.exact_mode_sum(terms[c["g"] == np.uint64(g)].tolist(), e))
                   for g in range(3)]
            F.check_same_bits(rows, exp, where="L = %r" % L)
            after_first = compiles(pctx) if after_first is None else after_first
            assert compiles(pctx) == after_first, L
        assert len(exps) == 4
    finally:
        t.close()


def test_bare_scan_in_two_windows(pctx, mixed, monkeypatch):
    """evql_scan_count + evql_scan_emit, a literal in WHERE and one in the select list, the
    result staged in windows of 5000 rows: the same bytes as the oracle's"""
    t, img, _ = mixed
    monkeypatch.setenv("EVQL_SCAN_WINDOW_ROWS", "5000")
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(scan_select=[k, b + L[1], v], where=a > L[0], row_end=50_001),
                   [(30000, 1), (50000, 1 << 35), (65000, 0), (65535, 3)], 0, raw=True)
    assert passed[0] > 10_000 and passed[3] == 0 and len(set(passed)) == 4


rid, pos, price = col("id"), col("items.position"), col("items.price")


def test_nested_mixed_depth_where_under_a_record_filter(pctx):
    """evql_where_rows (WHERE over columns of different repetition depth) and the fused
    kernel behind it read the same pool"""
    img, _ = N.items_table(NREC)
    f = np.random.default_rng(5).random(NREC) < 0.6
    t = pctx.open_image(img)
    try:
        passed = sweep(pctx, t, img, N.ITEMS_SCHEMA,
                       lambda L: dict(select=[pos, count(1), sum_(rid), sum_(price + L[2])],
                                      group_by=[pos], where=(pos > L[0]) & ((rid % 3).eq(L[1])),
                                      scan_mode=K.SCAN_NESTED, row_filter=f),
                       [(2, 0, 1), (0, 1, 1 << 50), (3, 2, 0), (1, 7, 3)], 1,
                       expect_source=[("evql_where_rows", True)])
        assert passed[3] == 0 and len(set(passed)) >= 3
    finally:
        t.close()


def test_two_file_chain(pctx):
    """evql_query_create_chain over the two files of partition `quiet`: one operator per
    file, each with the pool of its own plan; expectation: the partial aggregates of every
    file, merged (test_gpu_nested_filter.py oracle_chain)"""
    files = list(reversed(LN.partition("quiet")))
    SN = LN.NESTED_LSM_SCHEMA
    tabs = [pctx.open_image(f[1]) for f in files]
    ch = E.LsmChain(pctx)
    for tb, f in zip(tabs, files):
        ch.add(tb, has_skiplist=f[2], has_updates=f[3])
    ch.build()
    filters = O.oracle_partition_filters(LN.partition("quiet"))
    lk, lpos, lprice = col("k"), col("items.position"), col("items.price")
    try:
        after_first, seen = None, []
        for L in [(4, 7, 0), (2, 0, 1 << 44), (9, 20, 5), (0, 0, 1)]:
            kw = dict(select=[lk, count(1), sum_(lprice + L[2])], group_by=[lk],
                      where=(lpos < L[0]) & (lk > L[1]), scan_mode=K.SCAN_NESTED)
            frames, passed = [], 0
            for f, flt in zip(files, filters):
                r = O.oracle_run(f[1], Plan(SN, mode=K.MODE_PARTIAL, row_filter=flt, **kw))
                frames.append(O.partial_frame([r.keys[20 * i:20 * i + 20] for i in range(r.nrows)],
                                              r.columns[0]))
                passed += r.rows_passed
            exp = O.oracle_merge(Plan(SN, **kw), frames[::-1])
            q = ch.query(Plan(SN, **kw))
            got = q.run()
            assert got.nrows == exp.nrows, L
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1, rel=1e-6)
            assert q.stats()["rows_passed"] == passed, L
            q.close()
            seen.append(passed)
            after_first = compiles(pctx) if after_first is None else after_first
            assert compiles(pctx) == after_first, L
        assert seen[3] == 0 and len(set(seen)) == 4
    finally:
        ch.close()
        for tb in tabs:
            tb.close()


def test_string_key_on_the_dictionary(pctx, mixed):
    """a STRING key that is only grouped by runs on the table's dictionary codes; the
    numeric WHERE literals sit in the same kernel"""
    t, img, _ = mixed
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(select=[s, count(1), sum_(a)], group_by=[s],
                                  where=(a > L[0]) & (b < L[1])),
                   [(30000, 30000), (0, 1 << 32), (65000, 65535), (1 << 32, 5)], 1,
                   expect_source=[("evql_ident_add", False)])
    assert passed[3] == 0 and len(set(passed)) == 4


def test_float_literal_bits(pctx, mixed):
    """v > L and the literal itself as a select value (IF's branch that is always taken):
    -0.0, the smallest subnormal and -1e300 arrive bit for bit"""
    t, img, _ = mixed
    floats = [-0.0, 0.0, 5e-324, 1.5, -1e300]
    sweep(pctx, t, img, S,
          lambda L: dict(scan_select=[a, If(a > 100_000, v, L), v * L], where=a < 3000),
          floats, 0, raw=True)
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(select=[k % 7, count(1), sum_(v)], group_by=[k % 7], where=v > L),
                   floats + [8000000.0], 1)
    assert passed[4] == ROWS and passed[5] < ROWS // 2 and passed[0] == passed[1]


def test_signed_literal_bits(pctx, mixed):
    """an INT64 projection (a - 40000, in [-40000, 25535]) against -1, INT64_MIN and
    INT64_MAX"""
    t, img, _ = mixed
    x = a + (-40000)
    ints = [-1, INT64_MIN, INT64_MAX, 0]
    passed = sweep(pctx, t, img, S,
                   lambda L: dict(select=[k % 7, count(1), sum_(x)], group_by=[k % 7],
                                  where=x > lit(L, K.T_INT64)), ints, 1)
    assert passed[1] == ROWS and passed[2] == 0 and 0 < passed[3] < passed[0] < ROWS
    sweep(pctx, t, img, S,
          lambda L: dict(scan_select=[a, If(a > 100_000, x, lit(L, K.T_INT64))], where=a < 3000),
          ints, 0, raw=True)


def test_two_live_queries_of_one_shape(pctx, mixed):
    """q1 and q2 share one module; their launches overlap (launch, launch, finish, finish).
    A pool kept in module memory would give both the literals of the later launch"""
    t, img, _ = mixed
    mk = lambda L: Plan(S, select=[k, sum_(a + L), count(1)], group_by=[k], where=b > L,  # noqa: E731
                        groups_hint=1000)
    p1, p2 = mk(20000), mk(50000)
    e1, e2 = O.oracle_run(img, p1), O.oracle_run(img, p2)
    q1 = t.query(p1)
    before = compiles(pctx)
    q2 = t.query(p2)
    assert compiles(pctx) == before
    try:
        q1.launch()
        q2.launch()
        q2.finish()
        q1.finish()
        r2, r1 = q2.fetch_all().rows(), q1.fetch_all().rows()
        T.compare_results(r1, e1.rows(), e1.types, key_cols=1)
        T.compare_results(r2, e2.rows(), e2.types, key_cols=1)
        assert q1.stats()["rows_passed"] == e1.rows_passed != e2.rows_passed
        assert sorted(r1) != sorted(r2)
        q1.execute()
        assert sorted(q1.fetch_all().rows()) == sorted(r1)
        assert q1.stats()["rows_passed"] == e1.rows_passed
    finally:
        q1.close()
        q2.close()


def plan40(lits):
    """tests/test_literal_pool_cpu.py plan40: lits[0] in WHERE, lits[1:] in the sum"""
    arg = a
    for x in lits[1:]:
        arg = arg + x
    return dict(select=[k, sum_(arg), count(1)], group_by=[k], where=a > lits[0], groups_hint=1000)


def test_pool_overflow(pctx, mixed):
    """40 literals: 32 from the pool, 8 from the text.  Changing pooled ones compiles
    nothing, changing one beyond the pool does"""
    t, img, _ = mixed
    base = [1000 + 7 * i for i in range(40)]
    inside = [x * 3 + (1 << 34) if i in (0, 5, 31) else x for i, x in enumerate(base)]
    sweep(pctx, t, img, S, plan40, [base, inside], 1)
    beyond = list(base)
    beyond[35] = 999_999
    before = compiles(pctx)
    run_plan(t, img, Plan(S, **plan40(beyond)), 1)
    assert compiles(pctx) == before + 1


def test_zero_divisor_still_raises(pctx, mixed):
    """a / (b - L): with L = the b of a passing row the query fails as the reference does;
    with an L no row holds, the same code object gives the oracle's rows"""
    t, img, c = mixed
    mk = lambda L: dict(select=[k % 5, count(1), sum_(a / (b - L))], group_by=[k % 5],  # noqa: E731
                        where=a > 100)
    row = int(np.flatnonzero(c["a"] > 100)[0])
    run_plan(t, img, Plan(S, **mk(70000)), 1)
    before = compiles(pctx)
    bad = Plan(S, **mk(int(c["b"][row])))
    with pytest.raises(RuntimeError) as oi:
        O.oracle_run(img, bad)
    assert "zero" in str(oi.value)
    q = t.query(bad)
    with pytest.raises(E.EvqlError) as ei:
        q.run()
    q.close()
    assert ei.value.code == K.EVQL_ERUNTIME and "zero" in ei.value.msg
    run_plan(t, img, Plan(S, **mk(70001)), 1)
    assert compiles(pctx) == before
