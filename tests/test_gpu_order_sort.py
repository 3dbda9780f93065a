"""ORDER BY over a large GROUP BY result sorted on the device: the rows, their
order -- ties included -- and the bytes of every column equal what the host path
(EVQL_ORDER_DEVICE_SORT=0: records_to_host, sort_host_records, order_fetched) produces.  Where
the specs form a total order the rows are also the plain Python model's (order_edges.Model)
or the oracle's.  No tie order is pinned that the host path does not itself produce: ties are
only ever compared between the two paths.

One query per (table, plan, switch): set_order, execute, fetch for every order (set_order
belongs before execute; the switch is read when the query is created)."""
import os
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, out, sum_
import oracle_lib as O
import order_edges as X
import partial_emit_model as M

pytestmark = pytest.mark.gpu

G = X.DENSE_G
MIN = K.DEVICE_EMIT_MIN_GROUPS
# the dense table's plan with an unsigned sum in front: one-row groups, so sum(u) is the
# product i * 0x9E3779B97F4A7C15 wrapped to 64 bits, spread over the whole unsigned range
AGGS = (("key", "g"), ("sum", "u"), ("sum", "x"), ("imin", "u"), ("isum", "t"))
FIRST_KEYS = {"usum": 1, "fsum": 2, "imin": 3, "isum_t": 4}


def make_query(table, plan, device):
    """the switch is read when the query is created"""
    old = os.environ.get("EVQL_ORDER_DEVICE_SORT")
    os.environ["EVQL_ORDER_DEVICE_SORT"] = "1" if device else "0"
    try:
        return table.query(plan)
    finally:
        if old is None:
            del os.environ["EVQL_ORDER_DEVICE_SORT"]
        else:
            os.environ["EVQL_ORDER_DEVICE_SORT"] = old


def fetch(q, plan, specs, limit=None, offset=0):
    q.set_order(Order(plan, list(specs), limit=limit, offset=offset))
    res = q.run()
    return res, q.order_stats(), q.emit_stats(), q.stats()


def rows_sig(res):
    return [X.sig(r) for r in res.rows()]


def same(dev, host, where):
    """rows in order with ==, and the raw bytes of every column"""
    assert dev.nrows == host.nrows, (where, dev.nrows, host.nrows)
    a, b = rows_sig(dev), rows_sig(host)
    if a != b:
        i = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y)
        raise AssertionError((where, "row %d of %d" % (i, len(a)), dev.rows()[i], host.rows()[i]))
    assert dev.rows() == host.rows() or any(v != v for r in host.rows() for v in r
                                            if isinstance(v, float)), where
    assert dev.raw == host.raw, (where, "column bytes")


def expected_rows(n, limit, offset):
    if limit is None:
        return n
    lo = min(offset, n)
    return 0 if limit == 0 else min(n, offset + limit) - lo


@pytest.fixture(scope="module")
def dense(ctx):
    img, rows = X.dense_table()
    t = ctx.open_image(img)
    yield t
    t.close()


@pytest.fixture(scope="module")
def dense_model():
    _, rows = X.dense_table()
    return X.Model(rows, ("g", "u", "x", "t"), AGGS)


@pytest.fixture(scope="module")
def dense_queries(dense):
    """(hint, device) -> query, made on demand"""
    made = {}

    def get(hint, device):
        if (hint, device) not in made:
            plan = X.make_plan(X.DENSE_SCHEMA, AGGS, groups_hint=hint)
            made[hint, device] = (make_query(dense, plan, device), plan)
        return made[hint, device]
    yield get
    for q, _ in made.values():
        q.close()


# ---- 1. full order, no LIMIT --------------------------------------------------------------------
@pytest.mark.parametrize("hint", [1000, 100_000, 3_000_000])
@pytest.mark.parametrize("first", sorted(FIRST_KEYS))
def test_full_order(dense_queries, dense_model, hint, first):
    """ascending and descending, alone and followed by the key.  isum(t) has 16 values of
    ~4,375 ties each: alone, its tie runs come in the host path's order exactly (stability and
    the base order)"""
    qd, plan = dense_queries(hint, True)
    qh, _ = dense_queries(hint, False)
    src = qd.kernel_source()
    assert ("evql_part_scatter" in src) == (hint >= 100_000)
    assert ("evql_part_refine" in src) == (hint > 100_000)
    c = FIRST_KEYS[first]
    for desc in (False, True):
        for specs in (((c, desc),), ((c, desc), (0, False))):
            where = "hint %d order by %s" % (hint, specs)
            dev, os_, es, st = fetch(qd, plan, specs)
            host, hs, _, _ = fetch(qh, plan, specs)
            assert os_["sorted_on_device"] == 1 and os_["decision"] == K.OSORT_DEVICE, (where, os_)
            assert os_["records"] == G and os_["rows"] == G and os_["n_keys"] == len(specs) + 2
            assert es["device_packed"] == 1 and es["rows"] == G
            assert hs["sorted_on_device"] == 0 and hs["decision"] == K.OSORT_SWITCHED_OFF
            assert st["num_groups"] == G and dev.nrows == G
            same(dev, host, where)
            dense_model.check(dev.rows(), specs, None, 0, where)
    if first == "isum_t":
        # (the model cannot say where a tie goes; the host path can)
        t = [r[4] for r in dev.rows()]
        assert t == sorted(t, reverse=True) and len(set(t)) == 16


def test_three_specs_mixed_directions(dense_queries, dense_model):
    qd, plan = dense_queries(100_000, True)
    qh, _ = dense_queries(100_000, False)
    for specs in (((4, True), (3, False), (0, True)), ((4, False), (2, True), (1, False))):
        dev, os_, _, _ = fetch(qd, plan, specs)
        host, _, _, _ = fetch(qh, plan, specs)
        assert os_["sorted_on_device"] == 1 and os_["n_keys"] == 5
        same(dev, host, specs)
        dense_model.check(dev.rows(), specs, None, 0, "three specs")


# ---- 2. LIMIT / OFFSET ----------------------------------------------------------------------------
# limit 0 with offset 0 never reaches the sort: the top-k selection in front of it (want = 0)
# leaves no record.  With offset = G every record enters it and the slice is empty.
LIMITS = [(None, 0, 1), (G + 5, 0, 1), (0, G, 1), (66_000, 1_000, 1), (100, G - 101, 1),
          (100, 35_000, 0), (0, 0, 0)]


@pytest.mark.parametrize("limit,offset,on_device", LIMITS)
def test_limit_offset(dense_queries, dense_model, limit, offset, on_device):
    qd, plan = dense_queries(100_000, True)
    qh, _ = dense_queries(100_000, False)
    for specs in (((1, True), (0, False)), ((4, False), (0, True))):
        where = "order by %s limit %s offset %s" % (specs, limit, offset)
        dev, os_, _, st = fetch(qd, plan, specs, limit, offset)
        host, _, _, _ = fetch(qh, plan, specs, limit, offset)
        assert os_["sorted_on_device"] == on_device, (where, os_)
        if on_device:
            assert os_["decision"] == K.OSORT_DEVICE and os_["records"] >= MIN
        else:
            assert os_["decision"] == K.OSORT_FEW_RECORDS and os_["records"] < MIN
        assert os_["rows"] == expected_rows(os_["records"], limit, offset) == dev.nrows
        assert dev.nrows == expected_rows(G, limit, offset)
        assert st["num_groups"] == G, where
        same(dev, host, where)
        dense_model.check(dev.rows(), specs, limit, offset, where)


# ---- 3. the threshold --------------------------------------------------------------------------------
def key_plan(**kw):
    return Plan(M.KEY_SCHEMA, select=[col("k"), count(1), sum_(col("a"))], group_by=[col("k")], **kw)


@pytest.mark.parametrize("groups,on_device", [(MIN - 1, 0), (MIN, 1), (MIN + 1, 1)])
def test_threshold(ctx, groups, on_device):
    img, _, _ = M.key_table(groups)
    plan = key_plan()
    specs = [(1, True), (0, False)]
    exp = O.oracle_run(img, plan, order=Order(plan, specs)).rows()
    t = ctx.open_image(img)
    try:
        qd, qh = make_query(t, plan, True), make_query(t, plan, False)
        dev, os_, _, st = fetch(qd, plan, specs)
        host, hs, _, _ = fetch(qh, plan, specs)
        assert os_["sorted_on_device"] == on_device and os_["records"] == groups == st["num_groups"]
        assert os_["decision"] == (K.OSORT_DEVICE if on_device else K.OSORT_FEW_RECORDS)
        assert hs["sorted_on_device"] == 0
        assert hs["decision"] == (K.OSORT_SWITCHED_OFF if on_device else K.OSORT_FEW_RECORDS)
        same(dev, host, groups)
        assert dev.rows() == exp
        qd.close()
        qh.close()
    finally:
        t.close()


# ---- 4. keys that need no pass -------------------------------------------------------------------
def test_equal_keys_and_ascending_keys_run_no_pass(dense):
    """ORDER BY count(1) over one-row groups: every key equal, the output is the base order.
    ORDER BY the key: ascending already once the base order (by identity) stands.  Neither
    spec runs a digit pass.  What remains are the passes of the base order itself: the kind
    word (all equal: none) and the identity, 0 .. 70,000 = 17 bits: at most 3"""
    plan = Plan(X.DENSE_SCHEMA, select=[col("g"), count(1), sum_(col("u"))], group_by=[col("g")],
                groups_hint=100_000)
    t = dense
    q1, q0 = make_query(t, plan, True), make_query(t, plan, False)
    try:
        base, _, _, _ = fetch(q0, plan, [(0, False)])
        assert [r[0] for r in base.rows()] == list(range(G))
        seen = []
        for specs in ([(1, False)], [(1, True)], [(0, False)]):
            dev, os_, _, _ = fetch(q1, plan, specs)
            host, _, _, _ = fetch(q0, plan, specs)
            assert os_["sorted_on_device"] == 1 and os_["n_keys"] == 3
            assert os_["n_sort_passes"] <= 3 and os_["n_passes_skipped"] >= 8 + 8 + 5
            assert os_["n_sort_passes"] + os_["n_passes_skipped"] == 24
            seen.append(os_["n_sort_passes"])
            same(dev, host, specs)
            assert dev.raw == base.raw
        assert len(set(seen)) == 1        # the spec added nothing to the base order's passes
        dev, os_, _, _ = fetch(q1, plan, [(2, False)])
        assert os_["n_sort_passes"] == seen[0] + 8     # sum(u) spans all 64 bits
    finally:
        q1.close()
        q0.close()


# ---- 5. key edges at size ------------------------------------------------------------------------
NK_SCHEMA = dict(nk=K.T_UINT64, a=K.T_UINT64)
NK_COLUMNS = [dict(name="nk", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN,
                   dlevel_max=1),
              dict(name="a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)]


@pytest.fixture(scope="module")
def nk_table(ctx):
    """66,000 one-row groups: the keys 0 .. 65,997 shuffled, 2^64 - 1, and one NULL key"""
    n = 66_000
    i = np.arange(n, dtype=np.uint64)
    nk = (i * np.uint64(40_503)) % np.uint64(n - 2)      # (40,503 is coprime to 65,998)
    assert len(set(nk[:n - 2].tolist())) == n - 2
    nk[n - 2] = np.uint64(X.M64)
    present = np.ones(n, np.uint8)
    null_at = 12_345
    displaced = int(nk[null_at])
    nk[n - 1], nk[null_at], present[null_at] = displaced, 0, 0
    w = E.Writer(NK_COLUMNS)
    w.put("nk", nk, present=present)
    w.put("a", i + np.uint64(1))
    w.commit(n)
    img = w.image()
    w.close()
    t = ctx.open_image(img)
    yield t, n
    t.close()


def test_null_key_and_largest_key(nk_table):
    """the NULL key reads 0 and ties with the key 0: the base order decides between them"""
    t, n = nk_table
    plan = Plan(NK_SCHEMA, select=[col("nk"), count(1), sum_(col("a"))], group_by=[col("nk")])
    qd, qh = make_query(t, plan, True), make_query(t, plan, False)
    try:
        for specs in ([(0, False)], [(0, True)], [(0, False), (2, True)], [(1, False), (0, True)]):
            dev, os_, _, st = fetch(qd, plan, specs)
            host, _, _, _ = fetch(qh, plan, specs)
            assert os_["sorted_on_device"] == 1 and os_["records"] == n == st["num_groups"]
            same(dev, host, specs)
            keys = [r[0] for r in dev.rows()]
            assert keys.count(None) == 1 and keys.count(X.M64) == 1 and keys.count(0) == 1
            if specs[0] == (0, False):
                assert set(keys[:2]) == {None, 0} and keys[-1] == X.M64
                assert keys[2:-1] == list(range(1, n - 2))
            elif specs[0] == (0, True):
                assert set(keys[-2:]) == {None, 0} and keys[0] == X.M64
    finally:
        qd.close()
        qh.close()


# ---- 6. select lists ------------------------------------------------------------------------------
S_SCHEMA = dict(g=K.T_UINT64, a=K.T_UINT64, s=K.T_STRING)
S_COLUMNS = [dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
             dict(name="a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
             dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN)]
S_GROUPS = 66_001


@pytest.fixture(scope="module")
def s_table(ctx):
    """66,001 groups of one or two rows; s depends on the group alone, 0 to 40 bytes"""
    rows = S_GROUPS + 3_000
    i = np.arange(rows, dtype=np.uint64)
    g = (i * np.uint64(7_919)) % np.uint64(S_GROUPS)       # (7,919 is coprime to 66,001)
    a = i % np.uint64(1_013)
    s = [(b"s%d-" % v) * (v % 5) + b"x" * (v % 9) for v in g.tolist()]
    w = E.Writer(S_COLUMNS)
    w.put("g", g)
    w.put("a", a)
    w.put("s", s)
    w.commit(rows)
    img = w.image()
    w.close()
    t = ctx.open_image(img)
    yield t, img
    t.close()


def test_first_row_string_column_is_packed_in_order(s_table):
    t, img = s_table
    plan = Plan(S_SCHEMA, select=[col("g"), count(1), col("s"), sum_(col("a"))], group_by=[col("g")])
    qd, qh = make_query(t, plan, True), make_query(t, plan, False)
    try:
        for specs in ([(1, True), (0, False)], [(3, False)], [(1, False), (3, True)]):
            dev, os_, es, _ = fetch(qd, plan, specs)
            host, _, hes, _ = fetch(qh, plan, specs)
            assert os_["sorted_on_device"] == 1 and es["device_packed"] == 1
            assert hes["device_packed"] == 0
            same(dev, host, specs)
            for r in dev.rows()[::997]:
                assert r[2] == (b"s%d-" % r[0]) * (r[0] % 5) + b"x" * (r[0] % 9)
        exp = O.oracle_run(img, plan, order=Order(plan, [(1, True), (0, False)]))
        dev, _, _, _ = fetch(qd, plan, [(1, True), (0, False)])
        assert dev.rows() == exp.rows()
    finally:
        qd.close()
        qh.close()


def test_post_aggregate_arithmetic_is_emitted_by_the_host_in_device_order(s_table):
    t, img = s_table
    plan = Plan(S_SCHEMA, select=[col("g"), count(1), sum_(col("a")), sum_(col("a")) + 1],
                group_by=[col("g")])
    qd, qh = make_query(t, plan, True), make_query(t, plan, False)
    try:
        for specs, limit, offset in (([(1, True), (2, False), (0, True)], None, 0),
                                     ([(2, True), (0, False)], 200, 65_800)):
            dev, os_, es, _ = fetch(qd, plan, specs, limit, offset)
            host, _, _, _ = fetch(qh, plan, specs, limit, offset)
            assert os_["sorted_on_device"] == 1 and es["device_packed"] == 0
            same(dev, host, specs)
            assert all(r[3] == r[2] + 1 for r in dev.rows())
        exp = O.oracle_run(img, plan, order=Order(plan, [(1, True), (2, False), (0, True)]))
        dev, _, _, _ = fetch(qd, plan, [(1, True), (2, False), (0, True)])
        assert dev.rows() == exp.rows()
    finally:
        qd.close()
        qh.close()


# ---- 7. fallbacks keep the host path ---------------------------------------------------------------
def test_fallbacks_keep_the_host_path(s_table):
    t, _ = s_table
    plan = Plan(S_SCHEMA, select=[col("g"), count(1), col("s"), sum_(col("a"))], group_by=[col("g")])
    qd, qh = make_query(t, plan, True), make_query(t, plan, False)
    try:
        for specs, decision in (([(1, True), (2, False)], K.OSORT_UNREADABLE),
                                ([(1, True), (out(0) + out(3), False)], K.OSORT_EXPRESSION)):
            dev, os_, _, _ = fetch(qd, plan, specs)
            host, hs, _, _ = fetch(qh, plan, specs)
            assert os_["sorted_on_device"] == 0 and os_["decision"] == decision, os_
            assert os_["n_kernel_launches"] == 0 and os_["records"] == S_GROUPS
            same(dev, host, specs)
        assert hs["sorted_on_device"] == 0 and hs["decision"] == K.OSORT_SWITCHED_OFF
    finally:
        qd.close()
        qh.close()


def test_a_nan_sort_key_falls_back(ctx):
    """a group holding +inf and -inf sums to NaN: value_cmp has no order for it, the device
    sort is abandoned and the host orders as it always did"""
    n = 66_000
    i = np.arange(n + 1, dtype=np.uint64)
    g = i % np.uint64(n)                                  # group 0 has two rows
    x = (i.astype(np.float64) - 30_000.0) / 8.0
    x[0], x[n] = np.inf, -np.inf
    schema = dict(g=K.T_UINT64, x=K.T_FLOAT64)
    columns = [dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
               dict(name="x", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)]
    w = E.Writer(columns)
    w.put("g", g)
    w.put("x", x)
    w.commit(n + 1)
    img = w.image()
    w.close()
    plan = Plan(schema, select=[col("g"), sum_(col("x")), count(1)], group_by=[col("g")])
    t = ctx.open_image(img)
    qd, qh = make_query(t, plan, True), make_query(t, plan, False)
    try:
        for specs in ([(1, False), (0, False)], [(2, True), (1, True)]):
            dev, os_, _, _ = fetch(qd, plan, specs)
            host, _, _, _ = fetch(qh, plan, specs)
            assert os_["sorted_on_device"] == 0 and os_["decision"] == K.OSORT_NAN_KEY, os_
            nan_rows = [r for r in dev.rows() if r[1] != r[1]]
            assert len(nan_rows) == 1 and nan_rows[0][0] == 0
            same(dev, host, specs)
        # without the float key in the specs the NaN is a value like any other
        dev, os_, _, _ = fetch(qd, plan, [(2, True), (0, False)])
        host, _, _, _ = fetch(qh, plan, [(2, True), (0, False)])
        assert os_["sorted_on_device"] == 1
        same(dev, host, "count, key")
        assert dev.rows()[0][0] == 0 and dev.rows()[0][2] == 2
    finally:
        qd.close()
        qh.close()
        t.close()


# ---- 8. a merged result ------------------------------------------------------------------------------
def test_merged_result_is_sorted_on_the_device(ctx):
    """the hub exchange of two ranks: every rank ends with all groups in its merged table,
    ordered by count descending, then key"""
    parts = [M.key_table(70_001), M.key_table(MIN + 1)]
    w = E.Writer(M.KEY_COLUMNS)
    for name in ("k", "a"):
        w.put(name, np.concatenate([p[1][name] for p in parts]))
    w.commit(sum(p[2] for p in parts))
    whole = w.image()
    w.close()
    plan = key_plan()
    specs = [(1, True), (0, False)]
    t = ctx.open_image(whole)
    q = make_query(t, plan, False)
    single, _, _, _ = fetch(q, plan, specs)
    q.close()
    t.close()
    assert single.nrows == 70_001
    assert single.rows() == O.oracle_run(whole, plan, order=Order(plan, specs)).rows()

    def exchange_run(device):
        hub = E.Hub(2)
        res, errs = [None, None], []

        def work(r):
            try:
                c = E.Context(0)
                tr = c.open_image(parts[r][0])
                qr = tr.query(plan)
                x = E.Exchange.hub(c, hub, r)
                qr.set_order(Order(plan, specs))
                qr.execute()
                qr.exchange(x, K.EXCHANGE_GATHER_ALL)
                got = qr.fetch_all()
                res[r] = (got, qr.order_stats(), qr.emit_stats(), qr.stats())
                qr.close()
                x.close()
                tr.close()
                c.close()
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                raise

        # (the switch is read when a query is created: it is set around both ranks' lives)
        old = os.environ.get("EVQL_ORDER_DEVICE_SORT")
        os.environ["EVQL_ORDER_DEVICE_SORT"] = "1" if device else "0"
        try:
            th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
            for x in th:
                x.start()
            for x in th:
                x.join(timeout=300)
        finally:
            if old is None:
                del os.environ["EVQL_ORDER_DEVICE_SORT"]
            else:
                os.environ["EVQL_ORDER_DEVICE_SORT"] = old
        assert not any(x.is_alive() for x in th), "a rank hangs"
        assert not errs, errs
        hub.close()
        return res

    on, off = exchange_run(True), exchange_run(False)
    for (dev, os_, es, st), (host, hs, _, _) in zip(on, off):
        assert os_["sorted_on_device"] == 1 and os_["records"] == 70_001 and es["device_packed"] == 1
        assert hs["sorted_on_device"] == 0 and st["num_groups"] == 70_001
        same(dev, host, "merged")
        same(dev, single, "merged against the single table")
