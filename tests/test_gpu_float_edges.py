"""Float and 64-bit aggregates on IEEE edge values (float_edges.py) through every
aggregation path of the device, against the exact reference with the strict comparator:
register accumulators (no GROUP BY), the lane-private accumulator cache, the LDS table
sizes, the partitioned path with and without refine, device- and host-packed emission,
the exchange merges and PARTIAL rows into the host merge.  Every case checks that it took
the path it names (kernel source markers, the emission condition).  Then
EVQL_FLOAT_SUM_EXACT at the edges of its quantum rule, bit for bit."""
import re
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, sum_
import oracle_lib as O
import float_edges as F

pytestmark = pytest.mark.gpu
S = F.SCHEMA
G = [col("g")]
_REF = {}


def ref(name, c, aggs, where=False, key="g"):
    """the reference of a table's rows (cached: both layouts hold the same groups)"""
    k = (name, aggs, where, key)
    if k not in _REF:
        _REF[k] = F.reference(c, aggs, F.where_mask(c) if where else None, key=key)
    return _REF[k]


def define(src, name):
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


def run(t, schema=S, **kw):
    q = t.query(Plan(schema, **kw))
    try:
        rows = q.run().rows()
        return rows, q.kernel_source(), q.stats()
    finally:
        q.close()


def run_ranks(img, cuts, kw, schema=S):
    """one hub rank per row range [cuts[r], cuts[r+1]), EXCHANGE_GATHER_ALL -> rows per rank"""
    nr = len(cuts) - 1
    hub = E.Hub(nr)
    out, errs = [None] * nr, []

    def work(r):
        try:
            cx = E.Context(0)
            tt = cx.open_image(img)
            qq = tt.query(Plan(schema, row_begin=cuts[r], row_end=cuts[r + 1], **kw))
            x = E.Exchange.hub(cx, hub, r)
            qq.execute()
            qq.exchange(x, K.EXCHANGE_GATHER_ALL)
            out[r] = qq.fetch_all().rows()
            qq.close(); x.close(); tt.close(); cx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(r,)) for r in range(nr)]
    [x.start() for x in th]
    [x.join(timeout=300) for x in th]
    hub.close()
    assert not errs, errs
    return out


@pytest.fixture(scope="module")
def main(ctx):
    out = {}
    for layout in ("contiguous", "strided"):
        img, c = F.main_table(layout)
        out[layout] = (ctx.open_image(img), img, c)
    yield out
    for t, _, _ in out.values():
        t.close()


@pytest.fixture(scope="module")
def wide(ctx):
    img, c = F.wide_table()
    t = ctx.open_image(img)
    yield t, img, c
    t.close()


@pytest.mark.parametrize("name", F.NAMES)
def test_global_aggregates(ctx, name):
    """no GROUP BY: register accumulators, shuffle and block reduction, one global atomic
    per word and workgroup -- every class alone, with and without WHERE"""
    d = F.by_class(F.main_columns(), [name])
    t = ctx.open_image(F.image_of(d))
    try:
        for where in (False, True):
            rows, src, _ = run(t, select=F.select(F.FLOAT_AGGS, key=None),
                               where=F.WHERE if where else None)
            assert "__shared__ u64 red[" in src and "evql_part_scatter" not in src
            F.check_strict(rows, F.reference(d, F.FLOAT_AGGS, F.where_mask(d) if where else None,
                                             key=None), key_cols=0, where="%s where=%s" % (name, where))
    finally:
        t.close()


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_lane_cache(ctx, layout):
    """three classes at a time, one group each: with groups_hint 4 every lane keeps the
    groups it meets in its four-entry accumulator cache (strided: all three in turn)"""
    c = F.main_columns()
    for i in range(0, F.NCLASS, 3):
        names = F.NAMES[i:i + 3]
        d = F.by_class(c, names)
        if layout == "strided":
            d = F.strided(d)
        t = ctx.open_image(F.image_of(d))
        try:
            exp = F.reference(d, F.FLOAT_AGGS)
            for hint in (len(names) + 1, 0):
                rows, src, _ = run(t, select=F.select(F.FLOAT_AGGS), group_by=G, groups_hint=hint)
                assert "evql_part_scatter" not in src and define(src, "EVQL_LDS_SLOTS") > 0
                if hint:
                    assert define(src, "EVQL_LCACHE") == 4
                F.check_strict(rows, exp, where="%s %s hint %d" % (layout, names, hint))
        finally:
            t.close()


@pytest.mark.parametrize("hint", [10, 1000, 5000, 100_000])
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_group_table_variants(main, layout, hint):
    """~1000 groups: LDS tables of 1024 and more slots (a full table sends rows on to the
    HBM table); a hint beyond the LDS slots partitions"""
    t, _, c = main[layout]
    rows, src, st = run(t, select=F.select(F.FLOAT_AGGS), group_by=G, groups_hint=hint)
    slots = define(src, "EVQL_LDS_SLOTS")
    if hint == 10:
        assert slots == 1024 and "evql_part_scatter" not in src
    elif hint == 1000:
        assert slots >= 1024 and "evql_part_scatter" not in src
    elif hint == 100_000:
        assert "evql_part_scatter" in src and "evql_part_refine" not in src
    else:  # partitioned exactly when the hint is beyond the table's slots
        assert ("evql_part_scatter" in src) == (hint > slots)
    F.check_strict(rows, ref("main", c, F.FLOAT_AGGS), where="%s hint %d" % (layout, hint))
    if hint == 1000:
        rows, src, _ = run(t, select=F.select(F.FLOAT_AGGS), group_by=G, where=F.WHERE,
                           groups_hint=hint)
        assert "evql_part_scatter" not in src
        F.check_strict(rows, ref("main", c, F.FLOAT_AGGS, where=True), where="%s WHERE" % layout)


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_hbm_only_table(main, layout):
    """a plan with count_distinct does not partition: far beyond the LDS slots it
    aggregates straight into the HBM table (global FP64 atomics for every row)"""
    t, _, c = main[layout]
    aggs = F.FLOAT_AGGS + (("count_distinct", "u"),)
    rows, src, _ = run(t, select=F.select(aggs), group_by=G, groups_hint=300_000)
    assert define(src, "EVQL_LDS_SLOTS") == 0 and "evql_part_scatter" not in src
    F.check_strict(rows, ref("main", c, aggs), where=layout)


@pytest.mark.parametrize("hint", [100_000, 300_000, 3_000_000])
def test_partitioned(main, wide, hint):
    """radix partitions, ~1000 and 75,600 groups: one level (100k: this select list's 15
    state words leave about 1000 LDS slots, so 300k already takes the refine pass) and
    with refine"""
    for name, (t, _, c) in (("main", main["strided"]), ("wide", wide)):
        rows, src, _ = run(t, select=F.select(F.FLOAT_AGGS), group_by=G, groups_hint=hint)
        assert "evql_part_scatter" in src
        assert ("evql_part_refine" in src) == (hint > 100_000)
        F.check_strict(rows, ref(name, c, F.FLOAT_AGGS), where="%s hint %d" % (name, hint))


def test_integer_edges(main):
    """uint64 sums modulo 2^64, to_int64 sums / min / max at INT64_MIN / MAX, uint64 min / max
    at 0 and 2^64 - 1 (the EMPTY marker), means near 2^64, count_distinct over 2^64 - 1 and
    2^64 - 2: no GROUP BY, LDS table, HBM table; partitioned without count_distinct (a
    plan with it does not partition)"""
    t, _, c = main["strided"]
    rows, src, _ = run(t, select=F.select(F.INT_AGGS, key=None))
    assert "__shared__ u64 red[" in src
    F.check_strict(rows, ref("main", c, F.INT_AGGS, key=None), key_cols=0, where="global")
    part = tuple(a for a in F.INT_AGGS if a[0] != "count_distinct")
    for aggs, hint in ((F.INT_AGGS, 1000), (F.INT_AGGS, 300_000), (part, 300_000)):
        rows, src, _ = run(t, select=F.select(aggs), group_by=G, where=F.WHERE, groups_hint=hint)
        if hint == 1000:
            assert define(src, "EVQL_LDS_SLOTS") > 0 and "evql_part_scatter" not in src
        elif aggs is F.INT_AGGS:
            assert define(src, "EVQL_LDS_SLOTS") == 0 and "evql_part_scatter" not in src
        else:
            assert "evql_part_scatter" in src
        F.check_strict(rows, ref("main", c, aggs, where=True), where="hint %d" % hint)


def test_device_and_host_emission(wide):
    """>= 2^16 groups of a FINAL plan without ORDER BY / LIMIT, key + bare aggregates: the
    rows are packed on the device (k_emit_fixed computes the min / max NULLs and the means);
    a LIMIT above the group count keeps the host packer.  Both against the reference, and
    the order-free columns of the two bit for bit"""
    t, _, c = wide
    exp = ref("wide", c, F.FLOAT_AGGS)
    assert len(exp) >= 1 << 16
    plan = Plan(S, select=F.select(F.FLOAT_AGGS), group_by=G)
    q = t.query(plan)
    dev = q.run().rows()
    assert q.stats()["num_groups"] >= 1 << 16
    q.close()
    F.check_strict(dev, exp, where="device emission")
    q = t.query(plan)
    q.set_order(Order(plan, limit=len(exp) + 1))
    host = q.run().rows()
    q.close()
    F.check_strict(host, exp, where="host emission")
    free = [0] + [i + 1 for i, (fn, _) in enumerate(F.FLOAT_AGGS) if fn in ("min", "max", "count")]
    F.check_same_bits(dev, host, columns=free, where="device vs host")
    for a, b in zip(sorted(dev, key=lambda r: r[0]), sorted(host, key=lambda r: r[0])):
        assert [v is None for v in a] == [v is None for v in b], (a, b)   # NULL tags


@pytest.mark.parametrize("nranks", [2, 3])
def test_exchange_merges(main, nranks):
    """row ranges over 2 / 3 hub ranks, every rank gathers all groups"""
    _, img, c = main["strided"]
    n = len(c["g"])
    cuts = [0, 400_001, n] if nranks == 2 else [0, 1, 654_321, n]
    for rows in run_ranks(img, cuts, dict(select=F.select(F.FLOAT_AGGS), group_by=G)):
        F.check_strict(rows, ref("main", c, F.FLOAT_AGGS), where="%d ranks" % nranks)


@pytest.mark.parametrize("aggs", [F.FLOAT_AGGS, F.INT_AGGS], ids=["float", "int"])
def test_partial_rows_into_the_host_merge(main, aggs):
    """PARTIAL rows of three row ranges -> E.Merge: against the reference, and bit for bit
    against the oracle's merge of the same frames"""
    t, img, c = main["strided"]
    n = len(c["g"])
    kw = dict(select=F.select(aggs), group_by=G, where=F.WHERE)
    whole = Plan(S, **kw)
    m = E.Merge(whole)
    frames = []
    for lo, hi in ((0, 333_334), (333_334, 700_001), (700_001, n)):
        q = t.query(Plan(S, mode=K.MODE_PARTIAL, row_begin=lo, row_end=hi, **kw))
        q.execute()
        keys, datas = [], []
        while True:
            k, raw = q.next_batch(1024)
            if k == 0:
                break
            m.add_rows(raw[0], raw[1], k)
            keys += E.plan.unpack_svector(K.T_STRING, raw[0])
            datas += E.plan.unpack_svector(K.T_STRING, raw[1])
        frames.append(O.partial_frame(keys, datas))
        q.close()
    got = m.fetch_all().rows()
    m.close()
    F.check_strict(got, ref("main", c, aggs, where=True), where="merge")
    F.check_same_bits(got, O.oracle_merge(whole, frames).rows(), where="oracle merge")


def test_group_by_float_keys(ctx):
    """a single float key is identified by its bits: -0.0 / +0.0 and three NaNs (one of them
    all ones, the table's EMPTY marker) are distinct groups, as in the oracle"""
    img, c = F.float_key_table()
    t = ctx.open_image(img)
    try:
        plan = Plan(F.FKEY_SCHEMA, select=[col("fk"), count(1), sum_(col("v"))], group_by=[col("fk")])
        q = t.query(plan)
        rows = q.run().rows()
        q.close()
        F.check_same_bits(rows, O.oracle_run(img, plan).rows(), where="oracle")
        F.check_strict(rows, F.float_key_reference(c))
    finally:
        t.close()


# ---- EVQL_FLOAT_SUM_EXACT -------------------------------------------------------------------
EX_COLS = ("xs", "xt", "xp", "xc")


def exact_select(names):
    return [col("g")] + [sum_(col(nm)) for nm in names]


@pytest.mark.parametrize("hint", [4, 1000, 3_000_000])
def test_exact_sums_at_the_edges(ctx, hint):
    """derived bounds: subnormals only (bound < 2^-1022), |x| < 1e-300, full mantissas in
    +-1000, exact cancellation (+0.0); lane cache, LDS table, partitioned -- bit-equal to
    the terms rounded to the documented quantum and added exactly"""
    img, c = F.exact_table()
    t = ctx.open_image(img)
    try:
        rows, src, _ = run(t, schema=F.EXACT_SCHEMA, select=exact_select(EX_COLS), group_by=G,
                           groups_hint=hint, float_sum_mode=K.FLOAT_SUM_EXACT)
        if hint == 4:
            assert define(src, "EVQL_LCACHE") == 4 and "evql_part_scatter" not in src
        elif hint == 1000:
            assert define(src, "EVQL_LDS_SLOTS") > 0 and "evql_part_scatter" not in src
        else:
            assert "evql_part_refine" in src
        exp = F.exact_reference(c, EX_COLS)
        F.check_same_bits(rows, [k + tuple(v) for k, v in exp.items()], where="hint %d" % hint)
        assert F.bits(dict((r[0], r[4]) for r in rows)[0]) == 0   # x + (-x): exactly +0.0
    finally:
        t.close()


@pytest.mark.parametrize("names,bound", [
    (("xs", "xt"), 1e-300),
    (("xp", "xc"), float(np.nextafter(1024.0, 0.0))),   # just below 2^10
    (("xp", "xc"), 1024.0),
    (("xp", "xc"), float(np.nextafter(1024.0, 2048.0)))])
def test_exact_sums_explicit_bounds_and_splits(ctx, names, bound):
    """explicit bounds, and the same bits for the rows split over 1, 2 and 3 hub ranks"""
    img, c = F.exact_table()
    n = len(c["g"])
    kw = dict(select=exact_select(names), group_by=G, float_sum_mode=K.FLOAT_SUM_EXACT,
              float_sum_bound=bound)
    exp = [k + tuple(v) for k, v in F.exact_reference(c, names, bound).items()]
    t = ctx.open_image(img)
    try:
        rows, _, _ = run(t, schema=F.EXACT_SCHEMA, **kw)
    finally:
        t.close()
    F.check_same_bits(rows, exp, where="one rank")
    for cuts in ([0, 100_001, n], [0, 77_777, 155_555, n]):
        for r, got in enumerate(run_ranks(img, cuts, kw, schema=F.EXACT_SCHEMA)):
            F.check_same_bits(got, exp, where="rank %d of %d" % (r, len(cuts) - 1))


def test_exact_sum_bounds_refused(main):
    """a non-finite bound is refused when the query is created; a NaN or an infinity in a
    passing row fails the query even under an explicit bound"""
    t = main["contiguous"][0]
    for bad in (F.INF, F.NAN, -1.0):
        with pytest.raises(E.EvqlError) as ei:
            t.query(Plan(S, select=[sum_(col("x"))], float_sum_mode=K.FLOAT_SUM_EXACT,
                         float_sum_bound=bad))
        assert ei.value.code == K.EVQL_EARG, bad
    for name in ("nan_only", "pinf", "ninf"):
        q = t.query(Plan(S, select=[sum_(col("x"))], where=col("g").eq(F.CLASS_INDEX[name]),
                         float_sum_mode=K.FLOAT_SUM_EXACT, float_sum_bound=1e300))
        try:
            with pytest.raises(E.EvqlError) as ei:
                q.run()
            assert ei.value.code == K.EVQL_ERUNTIME and "bound" in ei.value.msg, name
        finally:
            q.close()
