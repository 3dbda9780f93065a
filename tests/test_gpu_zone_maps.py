"""Zone maps on the device: per-column minimum / maximum of every 2048 rows
(k_zone_minmax), the per-query bitmap of excluded zones (k_zone_select) and the tile loops
of the generated kernels that skip what the bitmap excludes.

Every result is compared with the C oracle exactly as test_gpu_parity.py and
test_gpu_bare_scan.py do -- the oracle reads every row, so equal rows mean that no tile
with a passing row was skipped -- and the statistics (zones excluded, tiles skipped) are
compared with numpy's count over the same zones: equal counts mean that every tile that
could be skipped was.  No case returns early on ENOTSUP."""
import functools

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, lit, sum_
import lsm_tables
import oracle_lib as O
import tables as T
from test_lsm_partition import oracle_filters, scan_order_images

pytestmark = pytest.mark.gpu

ZONE = 2048
ROWS = 40_000  # 19 zones and a partial one of 1,088 rows
SORTED0, SORTED_STEP = 1000, 3


def ts(x):
    return lit(int(x), K.T_TIMESTAMP64)


# ---- numpy's side -------------------------------------------------------------------------
def zone_min_max(values):
    values = np.asarray(values, dtype=np.uint64)
    nz = -(-len(values) // ZONE)
    zmin = np.array([values[z * ZONE:(z + 1) * ZONE].min() for z in range(nz)], dtype=np.uint64)
    zmax = np.array([values[z * ZONE:(z + 1) * ZONE].max() for z in range(nz)], dtype=np.uint64)
    return zmin, zmax


def excluded_zones(zmin, zmax, op, L):
    """the rule of the issue, per zone, in python integers"""
    out = []
    for mn, mx in zip(zmin.tolist(), zmax.tolist()):
        out.append({">": mx <= L, ">=": mx < L, "<": mn >= L, "<=": mn > L,
                    "=": L < mn or L > mx}[op])
    return np.array(out, dtype=bool)


def tiles_all_excluded(excl, tile_rows, nrows, row_begin=0, row_end=0):
    """tiles of `tile_rows` rows over [row_begin, row_end) whose zones are all excluded (a
    zone behind the table holds no row)"""
    row_end = min(row_end, nrows) if row_end else nrows
    if row_end <= row_begin:
        return 0, 0
    tile0 = row_begin // tile_rows
    ntiles = -(-row_end // tile_rows) - tile0
    skipped = 0
    for t in range(tile0, tile0 + ntiles):
        z0, z1 = t * tile_rows // ZONE, max((t + 1) * tile_rows // ZONE, t * tile_rows // ZONE + 1)
        skipped += all(z >= len(excl) or excl[z] for z in range(z0, z1))
    return ntiles, skipped


def check_zone_stats(q, excl, nrows, conjuncts, row_begin=0, row_end=0):
    zs = q.zone_stats()
    assert zs["zone_rows"] == ZONE
    assert zs["conjuncts_used"] == conjuncts
    assert zs["zones_total"] == len(excl)
    assert zs["zones_excluded"] == int(excl.sum())
    assert zs["tile_rows"] in (512, 1024, 2048, 4096, 8192, 16384)
    ntiles, skipped = tiles_all_excluded(excl, zs["tile_rows"], nrows, row_begin, row_end)
    assert zs["tiles_total"] == ntiles
    assert zs["tiles_skipped"] == skipped, (zs, skipped)
    return zs


# ---- 1. the statistics kernel ---------------------------------------------------------------
ENC_SPECS = [
    dict(name="p64", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="q64", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="p32", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_PLAIN),
    dict(name="bp17", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_BITPACKED,
         bitpack_max_value=(1 << 17) - 1),
    dict(name="l16", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128),
    dict(name="l40", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128),
    dict(name="dt", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_LEB128),
    dict(name="srt", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128),
    dict(name="nn", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
    dict(name="fv", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
]
ENC_SCHEMA = dict(p64=K.T_UINT64, q64=K.T_UINT64, p32=K.T_UINT64, bp17=K.T_UINT64, l16=K.T_UINT64,
                  l40=K.T_UINT64, dt=K.T_TIMESTAMP64, srt=K.T_UINT64, k=K.T_UINT64, nn=K.T_UINT64,
                  fv=K.T_FLOAT64, s=K.T_STRING)
IN_PLACE = ["p64", "q64", "p32", "bp17", "l16", "l40", "dt"]


@functools.lru_cache(maxsize=1)
def encodings_table():
    """one column per in-place encoding; inside every zone the values are a shuffled ramp
    around a per-zone level, so minimum and maximum sit somewhere in the middle of the zone
    and differ from zone to zone"""
    rng = np.random.default_rng(20250)
    i = np.arange(ROWS, dtype=np.uint64)

    def shuffled(top):
        level = rng.integers(0, top // 2, -(-ROWS // ZONE), dtype=np.uint64)
        out = np.empty(ROWS, dtype=np.uint64)
        for z in range(len(level)):
            n = min(ZONE, ROWS - z * ZONE)
            ramp = level[z] + rng.integers(0, top // 2, n, dtype=np.uint64)
            out[z * ZONE:z * ZONE + n] = rng.permutation(ramp)
        return out

    c = dict(p64=shuffled((1 << 64) - 1), q64=shuffled(1 << 16), p32=shuffled(1 << 32),
             bp17=shuffled(1 << 17), l16=shuffled(1 << 16), l40=shuffled(1 << 40),
             dt=np.uint64(1438055327000000) + shuffled(1 << 36),
             srt=np.uint64(SORTED0) + i * np.uint64(SORTED_STEP), k=i % np.uint64(37),
             nn=i, nn_present=(i % 5 != 0).astype(np.uint8), fv=rng.normal(0, 1e3, ROWS),
             s=[b"s%d" % (x % 11) for x in range(ROWS)])
    w = E.Writer(ENC_SPECS)
    for spec in ENC_SPECS:
        name = spec["name"]
        if name == "nn":
            w.put(name, c[name], present=c["nn_present"])
        else:
            w.put(name, c[name])
    w.commit(ROWS)
    img = w.image()
    w.close()
    return img, c


@pytest.fixture(scope="module")
def enc(ctx):
    img, c = encodings_table()
    t = ctx.open_image(img)
    yield t, img, c
    t.close()


@pytest.mark.parametrize("name", IN_PLACE)
def test_zone_map_of_every_encoding(enc, name):
    """PLAIN64, PLAIN32, 17-bit pages, LEB128 kept as 16-bit pages, LEB128 kept as 8-byte
    SoA, a LEB128 DATETIME: numpy's per-2048-row minimum and maximum, exactly"""
    t, _, c = enc
    before = t.device_bytes()
    zmin, zmax = t.zone_map(name)
    emin, emax = zone_min_max(c[name])
    assert len(zmin) == 20 and ROWS - 19 * ZONE == 1088
    assert zmin.tolist() == emin.tolist()
    assert zmax.tolist() == emax.tolist()
    # minimum and maximum are not at the zones' ends
    assert c[name][0] not in (emin[0], emax[0]) and c[name][ZONE - 1] not in (emin[0], emax[0])
    assert t.device_bytes() >= before
    held = t.device_bytes()
    again = t.zone_map(name)  # (reused: nothing new is allocated)
    assert again[0].tolist() == emin.tolist() and again[1].tolist() == emax.tolist()
    assert t.device_bytes() == held


def test_zone_map_reads_the_narrow_copy(ctx, monkeypatch):
    """EVQL_NARROW_PLAIN=1: the table keeps 16-bit pages of the PLAIN64 column once a query
    has referenced it; the statistics are then read from that copy"""
    img, c = encodings_table()
    monkeypatch.setenv("EVQL_NARROW_PLAIN", "1")
    t = ctx.open_image(img)
    try:
        plan = Plan(ENC_SCHEMA, select=[count(1), sum_(col("q64"))])
        q = t.query(plan)
        assert "evql_bitpacked_x2<16>" in q.kernel_source()  # the copy exists and is read
        assert q.run().rows() == O.oracle_run(img, plan).rows()
        q.close()
        zmin, zmax = t.zone_map("q64")
        emin, emax = zone_min_max(c["q64"])
        assert zmin.tolist() == emin.tolist() and zmax.tolist() == emax.tolist()
    finally:
        t.close()


@pytest.mark.parametrize("name", ["nn", "fv", "s", "nope"])
def test_zone_map_refuses_other_columns(enc, name):
    """nullable, float and string columns (and a missing one) have no zone map"""
    t, _, _ = enc
    with pytest.raises(E.EvqlError) as ei:
        t.zone_map(name)
    assert ei.value.code == K.EVQL_EARG


# ---- 2. boundaries --------------------------------------------------------------------------
srt, kk = col("srt"), col("k")
OPS = {
    ">": lambda L: srt > L, ">=": lambda L: srt >= L, "<": lambda L: srt < L,
    "<=": lambda L: srt <= L, "=": lambda L: srt.eq(L),
    "reversed": lambda L: lit(L) < srt,  # L < c: c > L from the column's side
}


def grouped_on_sorted(where, **kw):
    return Plan(ENC_SCHEMA, select=[kk, count(1), sum_(col("p32"))], group_by=[kk], where=where,
                groups_hint=100, **kw)


def run_against_oracle(t, img, plan, key_cols=1, exp=None):
    exp = O.oracle_run(img, plan) if exp is None else exp
    q = t.query(plan)
    got = q.run()
    assert got.nrows == exp.nrows, (got.nrows, exp.nrows)
    if plan.select:
        T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=key_cols, rel=1e-6)
    else:
        assert got.rows() == exp.rows()
        assert got.raw == exp.raw
    st = q.stats()
    assert st["rows_passed"] == exp.rows_passed
    assert st["rows_scanned"] == exp.rows_scanned
    return q, exp


@pytest.mark.parametrize("op", sorted(OPS))
def test_boundaries_of_a_zone(enc, op):
    """a sorted column and the four literals around zone 7's [min, max]: the oracle's rows,
    numpy's excluded zones, and every tile skipped whose zones are all excluded"""
    t, img, c = enc
    zmin, zmax = zone_min_max(c["srt"])
    j = 7
    some_skipped = 0
    for L in (int(zmin[j]) - 1, int(zmin[j]), int(zmax[j]), int(zmax[j]) + 1):
        q, exp = run_against_oracle(t, img, grouped_on_sorted(OPS[op](L)))
        excl = excluded_zones(zmin, zmax, ">" if op == "reversed" else op, L)
        zs = check_zone_stats(q, excl, ROWS, 1)
        q.close()
        # the passing rows are numpy's too
        cmp_ = {">": c["srt"] > L, ">=": c["srt"] >= L, "<": c["srt"] < L, "<=": c["srt"] <= L,
                "=": c["srt"] == L, "reversed": c["srt"] > L}[op]
        assert exp.rows_passed == int(cmp_.sum())
        assert excl.sum() >= 7, (op, L)
        some_skipped += zs["tiles_skipped"]
    assert some_skipped > 0


def test_nothing_and_everything_skipped(enc):
    t, img, c = enc
    zmin, zmax = zone_min_max(c["srt"])
    below, above = SORTED0 - 1, int(c["srt"][-1]) + 1
    # below every value: nothing is excluded, the kernels get no bitmap
    q, exp = run_against_oracle(t, img, grouped_on_sorted(srt > below))
    zs = check_zone_stats(q, excluded_zones(zmin, zmax, ">", below), ROWS, 1)
    assert zs["zones_excluded"] == 0 and zs["tiles_skipped"] == 0 and exp.rows_passed == ROWS
    q.close()
    # above every value: every zone and every tile, the last partial one included
    q, exp = run_against_oracle(t, img, grouped_on_sorted(srt > above))
    zs = check_zone_stats(q, excluded_zones(zmin, zmax, ">", above), ROWS, 1)
    assert zs["zones_excluded"] == 20 and zs["tiles_skipped"] == zs["tiles_total"] > 0
    assert exp.nrows == 0
    q.close()
    # `select count(1)`: the oracle's answer, which is NO row -- GroupByExpression emits a
    # group only once a row has reached it (groupby.cc:183,192; pinned for the unpruned path
    # by test_gpu_parity.py "zero passing rows => zero result rows")
    plan = Plan(ENC_SCHEMA, select=[count(1)], where=srt > above)
    q, exp = run_against_oracle(t, img, plan, key_cols=0)
    assert exp.rows() == [] and q.stats()["rows_passed"] == 0
    zs = q.zone_stats()
    assert zs["tiles_skipped"] == zs["tiles_total"] > 0
    q.close()
    # a bare scan of nothing
    plan = Plan(ENC_SCHEMA, scan_select=[srt, col("s")], where=srt > above)
    q, exp = run_against_oracle(t, img, plan)
    assert exp.nrows == 0 and q.zone_stats()["tiles_skipped"] == q.zone_stats()["tiles_total"] > 0
    q.close()


# ---- 3. every kernel family -----------------------------------------------------------------
MIXED_ROWS = 300_000
k, a, b, v, s, w, tt, n = [col(x) for x in ("k", "a", "b", "v", "s", "w", "t", "n")]
LO_ROW, HI_ROW = 100_000, 200_500


@pytest.fixture(scope="module")
def mixed(ctx):
    img, c = T.mixed_table()
    t = ctx.open_image(img)
    yield t, img, c
    t.close()


def time_range(c):
    return (tt >= ts(c["t"][LO_ROW])) & (tt < ts(c["t"][HI_ROW]))


def range_excluded(c):
    zmin, zmax = zone_min_max(c["t"])
    return (excluded_zones(zmin, zmax, ">=", int(c["t"][LO_ROW])) |
            excluded_zones(zmin, zmax, "<", int(c["t"][HI_ROW])))


FAMILIES = {
    "lds": dict(select=[k, count(1), sum_(a), sum_(v)], group_by=[k], groups_hint=1000),
    "ungrouped": dict(select=[count(1), sum_(a), sum_(v)]),
    "partitioned": dict(select=[w, count(1), sum_(a)], group_by=[w], groups_hint=400_000),
    "no-hint": dict(select=[k, count(1), sum_(b)], group_by=[k]),
    "bare": dict(scan_select=[a, tt, s, v]),
    "row-filter": dict(select=[k, count(1), sum_(a)], group_by=[k], groups_hint=1000,
                       row_filter=np.arange(MIXED_ROWS) % 3 != 0),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_kernel_family(mixed, family):
    """t >= L1 AND t < L2 over the ascending `t` of the mixed table"""
    t, img, c = mixed
    kw = FAMILIES[family]
    plan = Plan(T.MIXED_SCHEMA, where=time_range(c), **kw)
    q, exp = run_against_oracle(t, img, plan, key_cols=0 if family == "ungrouped" else 1)
    rf = kw.get("row_filter")
    inside = np.zeros(MIXED_ROWS, dtype=bool)
    inside[LO_ROW:HI_ROW] = True
    assert exp.rows_passed == int((inside if rf is None else inside & rf).sum())
    zs = check_zone_stats(q, range_excluded(c), MIXED_ROWS, 2)
    assert zs["tiles_skipped"] > 0 and zs["zones_excluded"] >= 90
    if family == "partitioned":
        assert "evql_part_scatter" in q.kernel_source()
    # the bitmap belongs to the query: a second execute reuses it
    got = q.run()
    assert got.nrows == exp.nrows and q.zone_stats()["tiles_skipped"] == zs["tiles_skipped"]
    q.close()


def test_bare_scan_limit_behind_skipped_tiles(mixed):
    """LIMIT 7 OFFSET 1000: the window starts behind ~12 tiles that were never read"""
    t, img, c = mixed
    plan = Plan(T.MIXED_SCHEMA, scan_select=[tt, a, s], where=time_range(c) & (a > 30000))
    order = Order(plan, limit=7, offset=1000)
    exp = O.oracle_run(img, plan, order=order)
    q = t.query(plan)
    q.set_order(order)
    got = q.run()
    assert got.nrows == exp.nrows == 7
    assert got.rows() == exp.rows() and got.raw == exp.raw
    m = np.zeros(MIXED_ROWS, dtype=bool)
    m[LO_ROW:HI_ROW] = True
    m &= c["a"] > 30000
    assert [r[0] for r in got.rows()] == c["t"][m][1000:1007].tolist()
    # three conjuncts: `a > 30000` prunes as well (it excludes no zone of the random column)
    amin, amax = zone_min_max(c["a"])
    check_zone_stats(q, range_excluded(c) | excluded_zones(amin, amax, ">", 30000), MIXED_ROWS, 3)
    assert q.zone_stats()["tiles_skipped"] > 0
    q.close()


def test_row_range_starts_in_a_skipped_region(mixed):
    """row_begin in the excluded zones in front of L1, row_end in the middle of a tile.  No
    row in front of LO_ROW passes, so the oracle's scan of [0, row_end) has the same rows"""
    t, img, c = mixed
    rb, re_ = 50_001, 150_123
    kw = dict(select=[k, count(1), sum_(a)], group_by=[k], groups_hint=1000, where=time_range(c))
    exp = O.oracle_run(img, Plan(T.MIXED_SCHEMA, row_end=re_, **kw))
    assert exp.rows_passed == re_ - LO_ROW
    q = t.query(Plan(T.MIXED_SCHEMA, row_begin=rb, row_end=re_, **kw))
    got = q.run()
    T.compare_results(got.rows(), exp.rows(), exp.types)
    assert q.stats()["rows_passed"] == exp.rows_passed
    assert q.stats()["rows_scanned"] == re_ - rb
    zs = check_zone_stats(q, range_excluded(c), MIXED_ROWS, 2, row_begin=rb, row_end=re_)
    assert 0 < zs["tiles_skipped"] < zs["tiles_total"]
    q.close()
    # the bare scan over the same range
    kw = dict(scan_select=[tt, a], where=time_range(c))
    exp = O.oracle_run(img, Plan(T.MIXED_SCHEMA, row_end=re_, **kw))
    q = t.query(Plan(T.MIXED_SCHEMA, row_begin=rb, row_end=re_, **kw))
    got = q.run()
    assert got.rows() == exp.rows() and got.raw == exp.raw
    check_zone_stats(q, range_excluded(c), MIXED_ROWS, 2, row_begin=rb, row_end=re_)
    q.close()


# ---- 4. what must not prune -----------------------------------------------------------------
def test_conjuncts_that_do_not_prune(mixed):
    t, img, c = mixed
    above = ts(int(c["t"][-1]) + 1)
    sel = dict(select=[k, count(1), sum_(a)], group_by=[k], groups_hint=1000)
    # a nullable column (ascending where present); a conjunct under OR
    for where in (n > 250_000, (tt > ts(c["t"][250_000])) | (a > 65000)):
        q, exp = run_against_oracle(t, img, Plan(T.MIXED_SCHEMA, where=where, **sel))
        zs = q.zone_stats()
        assert zs["conjuncts_used"] == 0 and zs["tiles_skipped"] == 0 and zs["zones_excluded"] == 0
        assert 0 < exp.rows_passed < MIXED_ROWS
        q.close()
    # logical_and is eager: the division raises on rows that `t > L` rejects, all of them here
    raising = Plan(T.MIXED_SCHEMA, where=(tt > above) & (a / (b - b) > 1), **sel)
    with pytest.raises(RuntimeError) as oe:
        O.oracle_run(img, raising)
    assert "zero" in str(oe.value).lower()
    q = t.query(raising)
    assert q.zone_stats()["conjuncts_used"] == 0
    with pytest.raises(E.EvqlError) as ei:
        q.run()
    assert ei.value.code == K.EVQL_ERUNTIME
    q.close()
    # a constant divisor cannot raise: this one prunes
    L = ts(c["t"][250_000])
    q, exp = run_against_oracle(t, img, Plan(T.MIXED_SCHEMA, where=(tt > L) & (a / 7 > 3), **sel))
    zmin, zmax = zone_min_max(c["t"])
    zs = check_zone_stats(q, excluded_zones(zmin, zmax, ">", int(c["t"][250_000])), MIXED_ROWS, 1)
    assert zs["tiles_skipped"] > 0
    q.close()


# ---- 5. a fresh literal costs no compile ----------------------------------------------------
def test_fresh_literal_no_compile(ctx, mixed):
    t, img, c = mixed
    skipped = []
    for i, row in enumerate((40_000, 260_000)):
        if i == 1:
            before = ctx.kernel_cache_stats().compiles
        plan = Plan(T.MIXED_SCHEMA, select=[k, count(1), sum_(b)], group_by=[k], groups_hint=1000,
                    where=(tt >= ts(c["t"][row])) & (b < 60000))
        q, exp = run_against_oracle(t, img, plan)
        skipped.append(q.zone_stats()["tiles_skipped"])
        q.close()
    assert ctx.kernel_cache_stats().compiles == before
    assert 0 < skipped[0] < skipped[1]


# ---- 6. the off switch ----------------------------------------------------------------------
def test_off_switch(mixed, monkeypatch):
    t, img, c = mixed
    monkeypatch.setenv("EVQL_ZONE_MAPS", "0")
    plan = Plan(T.MIXED_SCHEMA, where=time_range(c), **FAMILIES["lds"])
    q, exp = run_against_oracle(t, img, plan)
    zs = q.zone_stats()
    assert zs["conjuncts_used"] == 0 and zs["tiles_skipped"] == 0 and zs["zones_excluded"] == 0
    assert "evql_zones_excluded" not in q.kernel_source()
    q.close()
    monkeypatch.delenv("EVQL_ZONE_MAPS")
    q, _ = run_against_oracle(t, img, plan, exp=exp)
    assert "evql_zones_excluded" in q.kernel_source()
    assert q.zone_stats()["tiles_skipped"] > 0
    q.close()


# ---- 7. one chain ---------------------------------------------------------------------------
def test_chain_of_files(ctx):
    """GROUP BY over the three files of partition `big` with a range on `rid` (required,
    PLAIN, ascending inside every file): the oldest file is excluded whole, the other two in
    part; every file has a zone map and a bitmap of its own"""
    files = list(reversed(lsm_tables.partition("big")))  # scan order: newest first
    tabs = [ctx.open_image(f[1]) for f in files]
    ch = E.LsmChain(ctx)
    for tb, f in zip(tabs, files):
        ch.add(tb, has_skiplist=f[2], has_updates=f[3])
    ch.build()
    try:
        rid = col("rid")
        lo, hi = 10_000_000 + 30_000, 20_000_000 + 40_000
        plan = Plan(lsm_tables.LSM_SCHEMA, select=[col("k"), count(1), sum_(col("a"))],
                    group_by=[col("k")], where=(rid >= lo) & (rid < hi))
        exp = O.oracle_run_chain(scan_order_images("big"), oracle_filters("big"), plan)
        q = ch.query(plan)
        got = q.run()
        T.compare_results(got.rows(), exp.rows(), exp.types)
        assert got.nrows == exp.nrows > 0
        zs = q.zone_stats()
        excl = 0
        for f in files:
            zmin, zmax = zone_min_max(f[4]["rid"])
            excl += int((excluded_zones(zmin, zmax, ">=", lo) | excluded_zones(zmin, zmax, "<", hi)).sum())
        assert zs["conjuncts_used"] == 2
        assert zs["zones_total"] == sum(-(-len(f[4]["rid"]) // ZONE) for f in files)
        assert zs["zones_excluded"] == excl
        assert 0 < zs["tiles_skipped"] < zs["tiles_total"]
        q.close()
    finally:
        ch.close()
        for tb in tabs:
            tb.close()
