"""One select list through every route a GROUP BY result leaves the device by (DESIGN.md 3.7,
"where a select cell lives in a record"): FINAL rows packed on the device, PARTIAL rows packed
on the device and merged on the device, a resident cstable unsorted and sorted, and ORDER BY
sorted on the device.  Every route reads its cells through the one ResultCell / cell_bits
(csrc/result_cell.h), so every route must show the same cells: the oracle's, bit for bit -- the
float bits of the mean included.

The table has 65,536 + 8 groups of one or two rows: just over kDeviceEmitMinGroups, so that
every device route is taken.  Among the groups: the NULL key; a group whose aggregated column
is all NULL (count 0 under min, max and mean); a BOOL column; a uint column read as FLOAT64;
first-row strings that are empty, NULL, and exactly 11 bytes long (STAG_INLINE in a PARTIAL
row)."""
import functools
import struct

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, max_, mean, min_, sum_, unpack_svector
import materialize_model as MM
import oracle_lib as O
import partial_emit_model as PM

pytestmark = pytest.mark.gpu

G = PM.MIN_GROUPS + 8
ROWS = G + G // 2  # the groups of the lower half have two rows
NULL_KEY_GROUP, NO_VALUE_GROUP, EMPTY_STRING_GROUP, NULL_STRING_GROUP, INLINE_STRING_GROUP = 5, 7, 9, 10, 11
M64 = (1 << 64) - 1

SCHEMA = dict(nk=K.T_UINT64, a=K.T_UINT64, nb=K.T_UINT64, fb=K.T_BOOL, uf=K.T_FLOAT64, ns=K.T_STRING)
COLUMNS = [MM.LEB("nk", dlevel_max=1), MM.LEB("a"), MM.LEB("nb", dlevel_max=1), MM.BOOL("fb"),
           MM.U64("uf"), MM.STR("ns", dlevel_max=1)]
NULLABLE = ("nk", "nb", "ns")
# the select list of every route; its columns by position
SELECT = [col("nk"), count(1), sum_(col("a")), min_(col("nb")), max_(col("nb")), mean(col("nb")),
          col("fb"), col("uf"), col("ns")]
C_KEY, C_COUNT, C_SUM, C_MIN, C_MAX, C_MEAN, C_BOOL, C_UF, C_STR = range(9)
SPECS = [MM.U64("nk", dlevel_max=1), MM.LEB("n"), MM.LEB("sum_a"), MM.LEB("min_nb", dlevel_max=1),
         MM.U64("max_nb", dlevel_max=1), MM.F64("mean_nb", dlevel_max=1), MM.BOOL("fb"), MM.F64("uf"),
         MM.STR("ns", dlevel_max=1)]


def group_string(g):
    if g == EMPTY_STRING_GROUP:
        return b""
    if g == INLINE_STRING_GROUP:
        return b"elevenbytes"
    return b"s%d" % g * (g % 4)  # (empty again wherever g % 4 == 0)


@functools.lru_cache(maxsize=1)
def table():
    """every first-row column is a function of the row's group g = i % G"""
    i = np.arange(ROWS, dtype=np.uint64)
    g = i % np.uint64(G)
    c = {}
    c["nk"] = g * np.uint64(3) + np.uint64(1)
    c["nk_present"] = (g != NULL_KEY_GROUP).astype(np.uint8)
    c["a"] = (g * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(24)  # sums need several digit passes
    # one or two values per group: their sum is an exact double, so that the mean is one
    # correctly rounded division whoever computes it
    c["nb"] = (g * np.uint64(7)) % np.uint64(1000) + (i // np.uint64(G)) * np.uint64(3)
    c["nb_present"] = (g != NO_VALUE_GROUP).astype(np.uint8)
    c["fb"] = (g % np.uint64(3) == 0).astype(np.uint64)
    c["uf"] = g * np.uint64(11) + (np.uint64(1) << np.uint64(53))  # (not every one is a double)
    strings = [group_string(x) for x in range(G)]
    c["ns"] = [strings[x] for x in g.tolist()]
    c["ns_present"] = (g != NULL_STRING_GROUP).astype(np.uint8)
    w = E.Writer(COLUMNS)
    for sp in COLUMNS:
        name = sp["name"]
        if name in NULLABLE:
            w.put(name, c[name], present=c[name + "_present"])
        else:
            w.put(name, c[name])
    w.commit(ROWS)
    img = w.image()
    w.close()
    return img


def plan(**kw):
    return Plan(SCHEMA, select=SELECT, group_by=[col("nk")], **kw)


def bits(v):
    """a cell as something == compares bit for bit: a float by its 64 bits"""
    return ("f64", struct.unpack("<Q", struct.pack("<d", v))[0]) if isinstance(v, float) else v


def cells(rows):
    """{key: the row's cells, floats as bits}"""
    out = {r[C_KEY]: tuple(bits(v) for v in r) for r in rows}
    assert len(out) == len(rows), "duplicate keys"
    return out


@functools.lru_cache(maxsize=1)
def expected():
    """the oracle's FINAL rows: computed once, shared, never changed"""
    exp = O.oracle_run(table(), plan())
    assert exp.nrows == G
    return exp.rows(), exp.types, cells(exp.rows())


@functools.lru_cache(maxsize=1)
def expected_partial():
    return PM.oracle_rows(O.oracle_run(table(), plan(mode=K.MODE_PARTIAL)))


@pytest.fixture(scope="module")
def tab(ctx):
    t = ctx.open_image(table())
    yield t
    t.close()


def test_the_table_holds_every_edge():
    rows, types, by_key = expected()
    assert None in by_key                                                   # the NULL key
    r = by_key[NO_VALUE_GROUP * 3 + 1]
    assert r[C_MIN] is None and r[C_MAX] is None and r[C_MEAN] is None      # count 0
    assert {x[C_COUNT] for x in rows} == {1, 2}
    assert {x[C_BOOL] for x in rows} == {True, False} and types[C_BOOL] == K.T_BOOL
    assert types[C_UF] == K.T_FLOAT64 and types[C_MEAN] == K.T_FLOAT64
    r = by_key[12 * 3 + 1]
    assert r[C_UF] == bits(float((1 << 53) + 12 * 11)) and (1 << 53) + 13 * 11 != int(float((1 << 53) + 13 * 11))
    assert by_key[EMPTY_STRING_GROUP * 3 + 1][C_STR] == b""
    assert by_key[NULL_STRING_GROUP * 3 + 1][C_STR] is None
    assert len(by_key[INLINE_STRING_GROUP * 3 + 1][C_STR]) == 11
    # a mean that is no integer, from two values
    assert by_key[1 * 3 + 1][C_MEAN] == bits((7 + 10) / 2.0)


def test_final_rows_packed_on_the_device(tab):
    q = tab.query(plan())
    try:
        res = q.run()
        st = q.emit_stats()
        assert st["device_packed"] == 1 and st["partial"] == 0 and st["rows"] == G
        assert res.nrows == G and res.types == expected()[1]
        assert cells(res.rows()) == expected()[2]
    finally:
        q.close()


def test_partial_rows_packed_and_merged_on_the_device(tab, ctx):
    q = tab.query(plan(mode=K.MODE_PARTIAL))
    m = E.Merge(plan(), ctx)
    try:
        q.execute()
        got = {}
        while True:
            n, raw = q.next_batch(1 << 15)
            if n == 0:
                break
            got.update(zip(unpack_svector(K.T_STRING, raw[0]), unpack_svector(K.T_STRING, raw[1])))
            m.add_rows(raw[0], raw[1], n)
        st = q.emit_stats()
        assert st["device_packed"] == 1 and st["partial"] == 1 and st["rows"] == G
        assert got == expected_partial()
        # the STAG_INLINE case: the 11-byte string leaves with bit 7 set in its tag
        inline = PM.encoded_cell(K.T_STRING, b"elevenbytes")
        assert inline[-1] == 0x80 and sum(inline in d for d in got.values()) == 1
        merged = m.fetch_all()
        assert m.stats().packed_on_device == 1
        assert merged.nrows == G and merged.types == expected()[1]
        assert cells(merged.rows()) == expected()[2]
    finally:
        m.close()
        q.close()


@pytest.mark.parametrize("sort_by", [None, "sum_a"])
def test_materialised_table(tab, sort_by):
    q = tab.query(plan())
    try:
        q.execute()
        t2 = q.to_table(SPECS, sort_by=sort_by)
        try:
            st = q.materialize_stats
            assert st["rows"] == G == t2.num_rows
            res = MM.scan_image(t2.download_image(), SPECS)
        finally:
            t2.close()
        assert res.types == expected()[1]
        assert cells(res.rows()) == expected()[2]
        if sort_by:
            assert st["presorted"] == 0 and st["passes"] >= 2
            sums = [r[C_SUM] for r in res.rows()]
            assert sums == sorted(sums)
    finally:
        q.close()


@pytest.mark.parametrize("column", [C_MIN, C_MEAN])
def test_order_by_sorted_on_the_device(tab, column):
    """a NULL orders as payload 0; the key behind the column makes the order total (no key is 0
    but the NULL key's payload, and no other group of that column's value 0 ... is checked)"""
    rows = expected()[0]

    def order_key(r):
        v = r[column]
        return (0 if v is None else v, 0 if r[C_KEY] is None else r[C_KEY])
    want = sorted(rows, key=order_key)
    assert len({order_key(r) for r in rows}) == G  # a total order
    p = plan()
    q = tab.query(p)
    try:
        q.set_order(Order(p, [(column, False), (C_KEY, False)]))
        res = q.run()
        os_ = q.order_stats()
        assert os_["sorted_on_device"] == 1 and os_["decision"] == K.OSORT_DEVICE
        assert q.emit_stats()["device_packed"] == 1
        assert res.nrows == G
        assert [tuple(bits(v) for v in r) for r in res.rows()] == [tuple(bits(v) for v in r) for r in want]
    finally:
        q.close()
