"""The eager step tail against the lazy one: every case runs the same plan
with the epilogue's pinned block (the default) and with EVQL_EAGER_TAIL=0 in one process and
asserts byte-equal next_batch columns and equal num_groups / rows_passed, then checks the
rows against the oracle.  Float columns hold small integers: every summation order gives the
same bits, so the comparisons are exact."""
import os

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, Order, Call, col, count, lit, max_, mean, min_, sum_
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

N = 60_000
BLOCK_WORDS = (256 << 10) // 8   # the pinned block; 16 header words, then the records
SCHEMA = dict(k=K.T_UINT64, e=K.T_UINT64, g=K.T_UINT64, a=K.T_UINT64, af=K.T_FLOAT64,
              v=K.T_FLOAT64, nv=K.T_FLOAT64, na=K.T_UINT64, f=K.T_BOOL, s=K.T_STRING)


def eager_records(q):
    """E: how many records of this operator the epilogue may leave in the block"""
    return min(4096, (BLOCK_WORDS - 16) // q.record_words())


def build_table():
    i = np.arange(N, dtype=np.uint64)
    uint = lambda name, **kw: dict(name=name, logical_type=K.COL_UNSIGNED_INT,  # noqa: E731
                                   storage_type=K.ENC_UINT64_PLAIN, **kw)
    flt = lambda name, **kw: dict(name=name, logical_type=K.COL_FLOAT,  # noqa: E731
                                  storage_type=K.ENC_FLOAT_IEEE754, **kw)
    w = E.Writer([uint("k"), uint("e"), uint("g", dlevel_max=1), uint("a"), uint("af"), flt("v"),
                  flt("nv", dlevel_max=1), uint("na", dlevel_max=1),
                  dict(name="f", logical_type=K.COL_BOOLEAN, storage_type=K.ENC_BOOLEAN_BITPACKED),
                  dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN)])
    k = (i * np.uint64(2654435761) >> np.uint64(5)) % np.uint64(1000)
    a = (i * np.uint64(40503)) % np.uint64(65521)
    w.put("k", k)
    w.put("e", i % np.uint64(5000))
    # a key column with NULLs and with the table's EMPTY marker 2^64 - 1 among its values
    g = np.where(i % np.uint64(4) == 0, np.uint64(2**64 - 1), i % np.uint64(4))
    w.put("g", g, present=(i % np.uint64(7) != 3).astype(np.uint8))
    w.put("a", a)
    w.put("af", a % np.uint64(977))
    w.put("v", ((i * np.uint64(7919)) % np.uint64(4096)).astype(np.float64) - 2048.0)
    # groups k < 100 see only NULLs in nv / na
    w.put("nv", (a % np.uint64(513)).astype(np.float64) - 256.0,
          present=((k >= 100) & (i % np.uint64(3) != 0)).astype(np.uint8))
    w.put("na", a % np.uint64(4099), present=((k >= 100) & (i % np.uint64(5) != 1)).astype(np.uint8))
    w.put("f", a & np.uint64(1))
    w.put("s", [b"row-%d" % (int(x) % 321) for x in a])
    w.commit(N)
    img = w.image()
    w.close()
    return img


@pytest.fixture(scope="module")
def tab(ctx):
    img = build_table()
    t = ctx.open_image(img)
    yield t, img
    t.close()


def make_query(t, plan, eager):
    """EVQL_EAGER_TAIL is read when the operator is created"""
    old = os.environ.pop("EVQL_EAGER_TAIL", None)
    if not eager:
        os.environ["EVQL_EAGER_TAIL"] = "0"
    try:
        return t.query(plan)
    finally:
        os.environ.pop("EVQL_EAGER_TAIL", None)
        if old is not None:
            os.environ["EVQL_EAGER_TAIL"] = old


def drain(q, batch=1024):
    nc = q.column_count()
    chunks = [[] for _ in range(nc)]
    total = 0
    while True:
        n, raw = q.next_batch(batch)
        if n == 0:
            break
        total += n
        for c, r in zip(chunks, raw):
            c.append(r)
    return total, [b"".join(c) for c in chunks]


def rows_of(q, raws):
    types = [q.column_type(i) for i in range(q.column_count())]
    cols = [E.unpack_svector(t, r) for t, r in zip(types, raws)]
    return list(zip(*cols)) if cols else [], types


def ab(t, img, key_cols=1, order=None, batch=1024, schema=None, oracle=True, **kw):
    """eager and lazy tail of one plan: equal bytes and stats; the rows against the oracle"""
    out = {}
    for eager in (True, False):
        plan = Plan(schema or SCHEMA, **kw)
        q = make_query(t, plan, eager)
        try:
            if order is not None:
                q.set_order(Order(plan, *order))
            q.execute()
            n, raws = drain(q, batch)
            st = q.stats()
            out[eager] = (n, raws, st["num_groups"], st["rows_passed"])
            if eager:
                rows, types = rows_of(q, raws)
                launches = st["n_kernel_launches"]
        finally:
            q.close()
    assert out[True][0] == out[False][0]
    assert out[True][1] == out[False][1], "eager and lazy tail deliver different bytes"
    assert out[True][2:] == out[False][2:]
    if oracle:
        plan = Plan(schema or SCHEMA, **kw)
        exp = O.oracle_run(img, plan, order=Order(plan, *order) if order is not None else None)
        assert out[True][0] == exp.nrows
        if kw.get("mode") == K.MODE_PARTIAL:
            # (SHA1 group key, saved states): the oracle keeps the keys beside its one column
            assert types == [K.T_STRING, K.T_STRING]
            want = {exp.keys[20 * i:20 * i + 20]: exp.columns[0][i] for i in range(exp.nrows)}
            assert len(rows) == len(want) and dict(rows) == want
            assert out[True][3] == exp.rows_passed
            return out[True], launches
        assert types == exp.types
        if order is not None:
            assert rows == exp.rows()
        else:
            T.compare_results(rows, exp.rows(), exp.types, key_cols=key_cols, rel=0.0)
        assert out[True][3] == exp.rows_passed
    return out[True], launches


CONFIG3 = dict(select=[col("k"), sum_(col("v")), count(1), sum_(col("a"))], group_by=[col("k")],
               where=(col("a") > 30000) & (col("e") < 3500), groups_hint=1000)


# ---- group count ------------------------------------------------------------------------
def test_config3_shape_is_three_launches(tab):
    t, img = tab
    (n, _, groups, _), launches = ab(t, img, **CONFIG3)
    assert n == groups == 1000
    assert launches == 3   # prologue, scan, epilogue


def test_no_group_passes_where(tab):
    t, img = tab
    (n, _, groups, passed), _ = ab(t, img, **dict(CONFIG3, where=col("a") > 70000))
    assert (n, groups, passed) == (0, 0, 0)


def test_zero_row_table_and_empty_row_range(ctx, tab):
    """no scan kernel is launched; the epilogue still reports 0 groups"""
    w = E.Writer([dict(name=n, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
                  for n in "ka"])
    w.put("k", np.zeros(0, np.uint64))
    w.put("a", np.zeros(0, np.uint64))
    w.commit(0)
    img0 = w.image()
    w.close()
    t0 = ctx.open_image(img0)
    try:
        (n, _, groups, _), launches = ab(t0, img0, schema=dict(k=K.T_UINT64, a=K.T_UINT64),
                                         select=[col("k"), count(1), sum_(col("a"))],
                                         group_by=[col("k")], groups_hint=10)
        assert (n, groups, launches) == (0, 0, 2)
    finally:
        t0.close()
    t, img = tab
    # (the oracle takes no row_begin: an empty range has no rows to compare)
    (n, _, groups, passed), launches = ab(t, img, oracle=False, **dict(CONFIG3, row_begin=N))
    assert (n, groups, passed, launches) == (0, 0, 0, 2)


def test_one_group(tab):
    t, img = tab
    (n, _, _, _), _ = ab(t, img, **dict(CONFIG3, where=col("k").eq(7)))
    assert n == 1
    # no GROUP BY at all: the one slot of an ungrouped aggregate
    (n, _, _, _), _ = ab(t, img, key_cols=0, select=[count(1), sum_(col("a")), min_(col("v"))],
                         where=col("a") > 30000)
    assert n == 1


def test_null_key_and_empty_marker_key(tab):
    """NULL and 2^64 - 1 land in the two slots behind the table (gcap, gcap + 1)"""
    t, img = tab
    (n, raws, _, _), _ = ab(t, img, select=[col("g"), count(1), sum_(col("a")), max_(col("v"))],
                            group_by=[col("g")], groups_hint=8)
    assert n == 5   # NULL, 2^64 - 1, 1, 2, 3
    keys = E.unpack_svector(K.T_UINT64, raws[0])
    assert None in keys and 2**64 - 1 in keys


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_E_groups_and_one_more(tab, extra):
    """E groups fit the block; E + 1 fall back to the lazy compaction"""
    t, img = tab
    kw = dict(select=[col("e"), count(1), sum_(col("a"))], group_by=[col("e")], groups_hint=5000)
    q = t.query(Plan(SCHEMA, **kw))
    e_rec = eager_records(q)
    q.close()
    assert e_rec == 4096
    (n, _, groups, _), _ = ab(t, img, where=col("e") < lit(e_rec + extra), **kw)
    assert n == groups == e_rec + extra


def test_wide_records_lower_E(tab):
    """24 state words per slot: E follows the block size, and more groups than that go lazy"""
    t, img = tab
    sel = [col("k")] + [f(col(c)) for c in ("a", "v", "na", "nv") for f in (min_, max_, mean)]
    q = t.query(Plan(SCHEMA, select=sel, group_by=[col("k")], groups_hint=1000))
    e_rec = eager_records(q)
    q.close()
    assert 1000 <= e_rec < 4096
    ab(t, img, select=sel, group_by=[col("k")], groups_hint=1000)
    sel_e = [col("e")] + sel[1:]
    ab(t, img, select=sel_e, group_by=[col("e")], groups_hint=5000)   # 5000 > E: lazy


# ---- table growth -----------------------------------------------------------------------
def test_grown_table_relaunches_prologue_scan_epilogue(ctx):
    """70,000 distinct keys, groups_hint=1: status 2 -> grow and relaunch; the next execute of
    the same operator starts from the grown table"""
    n = 200_000
    i = np.arange(n, dtype=np.uint64)
    w = E.Writer([dict(name=c, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
                  for c in ("x", "a")])
    w.put("x", (i * np.uint64(2654435761)) % np.uint64(70_000))
    w.put("a", i % np.uint64(1013))
    w.commit(n)
    img = w.image()
    w.close()
    S = dict(x=K.T_UINT64, a=K.T_UINT64)
    kw = dict(select=[col("x"), count(1), sum_(col("a"))], group_by=[col("x")], groups_hint=1)
    t = ctx.open_image(img)
    try:
        exp = O.oracle_run(img, Plan(S, **kw))
        assert exp.nrows == 70_000
        res = {}
        for eager in (True, False):
            q = make_query(t, Plan(S, **kw), eager)
            try:
                for rep in range(2):
                    q.execute()
                    nrows, raws = drain(q)
                    assert nrows == q.stats()["num_groups"] == 70_000
                    rows, types = rows_of(q, raws)
                    T.compare_results(rows, exp.rows(), exp.types, rel=0.0)
                    res[eager, rep] = sorted(rows)
            finally:
                q.close()
        assert res[True, 0] == res[False, 0] == res[True, 1] == res[False, 1]
    finally:
        t.close()


# ---- first rows (gathered on the lazy path) -----------------------------------------------
def test_two_key_group_by_with_a_non_key_column(tab):
    t, img = tab
    ab(t, img, key_cols=2, select=[col("k"), col("f"), col("a"), count(1), sum_(col("v"))],
       group_by=[col("k"), col("f")], groups_hint=2000)


def test_first_row_null_uint_as_float_and_string(tab):
    t, img = tab
    # an optional column whose first-row value is NULL for a good part of the groups
    ab(t, img, select=[col("k"), col("na"), col("nv"), count(1)], group_by=[col("k")],
       groups_hint=1000)
    # readFloat on an unsigned column
    ab(t, img, select=[col("k"), col("af"), sum_(col("af"))], group_by=[col("k")],
       groups_hint=1000)
    # string bytes come through the lazy string copy
    ab(t, img, select=[col("k"), col("s"), count(1)], group_by=[col("k")], groups_hint=1000)
    ab(t, img, select=[col("s"), count(1), sum_(col("a"))], group_by=[col("s")])


# ---- above the operator -------------------------------------------------------------------
def test_order_by_with_and_without_limit(tab):
    t, img = tab
    ab(t, img, order=([(0, False)],), **CONFIG3)
    ab(t, img, order=([(2, True), (0, False)],), **CONFIG3)
    ab(t, img, order=([(0, True)], 10, 3), **CONFIG3)
    ab(t, img, order=([(2, True), (0, False)], 25), **CONFIG3)
    ab(t, img, order=([], 17, 5), oracle=False, **CONFIG3)   # LIMIT alone: which rows is unspecified


def test_partial_mode(tab):
    t, img = tab
    ab(t, img, mode=K.MODE_PARTIAL, **CONFIG3)
    ab(t, img, mode=K.MODE_PARTIAL, select=[col("g"), count(1), min_(col("nv")), mean(col("v"))],
       group_by=[col("g")], groups_hint=8)


# ---- life cycle ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 7, 1024])
def test_batch_sizes(tab, batch):
    t, img = tab
    ab(t, img, batch=batch, **dict(CONFIG3, where=col("k") < 50))


def test_executes_drains_and_close(tab):
    t, img = tab
    exp = O.oracle_run(img, Plan(SCHEMA, **CONFIG3))
    ref = None
    for eager in (True, False):
        q = make_query(t, Plan(SCHEMA, **CONFIG3), eager)
        try:
            seen = []
            for _ in range(3):                 # three executes, drained after each
                q.execute()
                seen.append(drain(q))
            q.execute()                        # two executes with no drain between them
            q.execute()
            seen.append(drain(q))
            assert q.next_batch(1024)[0] == 0  # again after exhaustion
            assert q.next_batch(1024)[0] == 0
            q.launch()                         # launch / finish as the benchmark drives it
            q.finish()
            seen.append(drain(q))
            assert all(s == seen[0] for s in seen)
            assert seen[0][0] == exp.nrows == 1000
            if ref is None:
                ref = seen[0]
                rows, types = rows_of(q, seen[0][1])
                T.compare_results(rows, exp.rows(), exp.types, rel=0.0)
            assert seen[0] == ref
            q.execute()                        # close without a drain
        finally:
            q.close()
    # closed between launch and finish: the block goes back only once the device is idle
    q = make_query(t, Plan(SCHEMA, **CONFIG3), True)
    q.launch()
    q.close()
    ab(t, img, **CONFIG3)


def test_operator_per_step_reuses_the_pinned_block(tab):
    """config 5w builds an operator per step: blocks come from the context's free list"""
    t, img = tab
    first = None
    for _ in range(20):
        q = t.query(Plan(SCHEMA, **CONFIG3))
        q.launch()
        q.finish()
        got = drain(q)
        q.close()
        first = first or got
        assert got == first


# ---- invalidation -------------------------------------------------------------------------
def test_import_and_recount_behind_finish(tab):
    """groups imported after execute: next_batch must not serve the block of the scan"""
    import torch
    t, img = tab
    kw = dict(select=[col("k"), count(1), sum_(col("a")), min_(col("v")), max_(col("af"))],
              group_by=[col("k")], where=col("a") > 5000, groups_hint=1000)
    m = 23_457
    exp = O.oracle_run(img, Plan(SCHEMA, **kw))
    res = {}
    for eager in (True, False):
        qa = make_query(t, Plan(SCHEMA, row_end=m, **kw), eager)
        qb = make_query(t, Plan(SCHEMA, row_begin=m, **kw), eager)
        try:
            qa.execute()
            qb.execute()
            buf = torch.zeros(4096 * qb.record_words(), dtype=torch.int64, device="cuda")
            cnt = qb.export_groups(buf.data_ptr(), 4096)
            qa.import_groups(buf.data_ptr(), cnt)
            n, raws = drain(qa)
            rows, types = rows_of(qa, raws)
            T.compare_results(rows, exp.rows(), exp.types, rel=0.0)
            res[eager] = (n, raws, qa.stats()["num_groups"])
            # the exporter's own result is untouched by the export
            nb, _ = drain(qb)
            assert nb == cnt
        finally:
            qa.close()
            qb.close()
    assert res[True] == res[False]


# ---- direct packing of simple result columns ------------------------------------------------
def test_direct_packing_every_aggregate_and_type(tab):
    """sum / count / min / max / mean over uint64, int64 and float64; groups k < 100 see only
    NULLs in na / nv (min, max and mean are NULL there); a bool key"""
    t, img = tab
    ia = Call("to_int64", col("a")) - 40000
    dense = [count(1), sum_(col("a")), min_(col("a")), max_(col("a")), mean(col("a")),
             sum_(ia), min_(ia), max_(ia), mean(ia),
             sum_(col("v")), min_(col("v")), max_(col("v")), mean(col("v"))]
    aggs = [min_(col("na")), max_(col("na")), mean(col("na")), sum_(col("na")),
            min_(col("nv")), max_(col("nv")), mean(col("nv")), count(col("nv"))]
    ab(t, img, select=[col("k")] + dense, group_by=[col("k")], groups_hint=1000)
    (n, raws, _, _), _ = ab(t, img, select=[col("k")] + aggs, group_by=[col("k")],
                            groups_hint=1000)
    assert n == 1000
    nulls = E.unpack_svector(K.T_FLOAT64, raws[-2]).count(None)
    assert nulls >= 100
    ab(t, img, select=[col("f")] + dense, group_by=[col("f")], groups_hint=2)
    ab(t, img, select=[col("f")] + aggs, group_by=[col("f")], groups_hint=2)
    # the interpreter keeps what the packer does not claim: arithmetic above an aggregate
    ab(t, img, select=[col("k"), sum_(col("a")) + 1, count(1)], group_by=[col("k")],
       groups_hint=1000)
    # the eager block with the row interpreter (EVQL_EAGER_TAIL=records) packs the same bytes
    os.environ["EVQL_EAGER_TAIL"] = "records"
    try:
        q = t.query(Plan(SCHEMA, select=[col("k")] + aggs, group_by=[col("k")], groups_hint=1000))
    finally:
        del os.environ["EVQL_EAGER_TAIL"]
    q.execute()
    assert drain(q) == (n, raws)
    q.close()
