"""Zone maps without a GPU: the two entry points exist, whether a conjunct prunes is a
property of the plan's SHAPE (plans that differ only in the bound share one code object),
and the tile-skip test costs the kernels no spill, no scratch and no FLAT instruction."""
import ctypes as C
import glob
import os
import re

import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K
from eventql_amd.plan import Plan, col, count, lit, sum_
from test_literal_pool_cpu import NARROW_COLUMNS, kernel_facts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEMA = dict(B.SCHEMA, t=K.T_TIMESTAMP64)
COLUMNS = B.PLAIN_COLUMNS + [dict(name="t", logical_type=K.COL_DATETIME,
                                  storage_type=K.ENC_UINT64_LEB128)]
k, a, b, v, t = [col(x) for x in "kabvt"]

T0 = 1438055327000000  # the first value of tests/tables.py's `t`


def ts(x):
    return lit(x, K.T_TIMESTAMP64)


def config3_shaped(where, **kw):
    return Plan(SCHEMA, select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=where,
                groups_hint=1000, **kw)


def objects(tmp_path, plans, columns=COLUMNS):
    for p in plans:
        assert E.compile_only(p, columns, cache_dir=str(tmp_path)) > 4000
    return sorted(glob.glob(str(tmp_path) + "/*.hsaco"))


def test_symbols_exported_and_declared(built):
    L = E.lib()
    for name in ("evql_query_zone_stats", "evql_table_zone_map"):
        assert getattr(L, name) is not None
    with open(os.path.join(ROOT, "include", "evql_gpu.h")) as f:
        header = f.read()
    assert re.search(r"int\s+evql_query_zone_stats\(const evql_query_t\*\s*\w*,\s*evql_zone_stats_t\*", header)
    assert re.search(r"int\s+evql_table_zone_map\(evql_table_t\*", header)
    assert L.evql_query_zone_stats.argtypes[1]._type_ is K.ZoneStats
    # the struct as the header lays it out: two u32, five u64
    assert C.sizeof(K.ZoneStats) == 48
    assert [f[0] for f in K.ZoneStats._fields_] == [
        "conjuncts_used", "zone_rows", "zones_total", "zones_excluded", "tile_rows", "tiles_total",
        "tiles_skipped"]
    assert hasattr(E.Query, "zone_stats") and hasattr(E.Table, "zone_map")


def test_one_object_whatever_the_bound(built, tmp_path):
    """t > L for an L below every value, in the middle and above every value: pruning is
    decided by the shape, the literal is data of k_zone_select"""
    plans = [config3_shaped((t > ts(L)) & (a > 30000)) for L in (0, T0 + 10**11, (1 << 64) - 1)]
    objs = objects(tmp_path, plans)
    assert len(objs) == 1, objs
    # reversed operand order, and the other relations: one object per shape too
    for mk in (lambda L: ts(L) < t, lambda L: t >= ts(L), lambda L: a <= L, lambda L: t.eq(ts(L))):
        d = tmp_path / ("s%d" % len(glob.glob(str(tmp_path) + "/s*")))
        d.mkdir()
        assert len(objects(d, [config3_shaped(mk(L)) for L in (1, T0, 1 << 63)])) == 1


def test_raising_where_compiles_and_differs(built, tmp_path):
    """`t > L AND a / (b - b) > 1` can raise (no pruning); with `a / 7 > 1` it cannot: both
    compile, to different texts"""
    raising = config3_shaped((t > ts(T0)) & (a / (b - b) > 1))
    safe = config3_shaped((t > ts(T0)) & (a / 7 > 1))
    assert len(objects(tmp_path, [raising, safe])) == 2


@pytest.mark.parametrize("case", ["grouped", "grouped-16-bit-pages", "partitioned", "bare",
                                  "bare-16-bit-pages", "ungrouped"])
def test_tile_skip_compiles_clean(built, tmp_path, case):
    """the test of a tile's zones is one scalar load: no spilled VGPR, no scratch, no FLAT"""
    columns = COLUMNS
    if case.endswith("pages"):
        columns = NARROW_COLUMNS + [COLUMNS[-1]]
    w = (t >= ts(T0)) & (t < ts(T0 + 10**9)) & (a > 30000)
    if case.startswith("grouped"):
        plan, kernels = config3_shaped(w), ["evql_scan_agg"]
    elif case == "ungrouped":
        plan, kernels = Plan(SCHEMA, select=[count(1), sum_(a)], where=w), ["evql_scan_agg"]
    elif case == "partitioned":
        plan = Plan(SCHEMA, select=[col("u"), sum_(a), count(1)], group_by=[col("u")], where=w,
                    groups_hint=10_000_000)
        kernels = ["evql_part_scatter"]
    else:
        plan = Plan(SCHEMA, scan_select=[k, b + 1, v * 2.0], where=w)
        kernels = ["evql_scan_count", "evql_scan_emit"]
    objs = objects(tmp_path, [plan], columns)
    assert len(objs) == 1
    facts = kernel_facts(objs[0])
    for kernel in kernels:
        assert facts[kernel] == (0, 0, 0), (case, kernel, facts[kernel])
