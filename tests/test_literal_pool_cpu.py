"""Numeric literals are kernel arguments (EvqlArgs::lit), not text: plans that differ only
in the values of pooled literals share one code object, and everything that still lives in
the text -- divisors, BOOL literals, the literal's type, a WHERE the planner drops, the
literals beyond the pool -- still gives a code object of its own.  No GPU needed: the
plans are compiled for gfx950 into a directory of their own and the objects are counted."""
import glob
import re
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K
from eventql_amd.plan import Plan, col, count, lit, sum_

LLVM = "/opt/rocm/lib/llvm/bin"

S = dict(B.SCHEMA)
k, a, b, v = [col(x) for x in "kabv"]
NARROW_COLUMNS = [dict(c, storage_type=K.ENC_UINT32_BITPACKED, bits=16)
                  if c["name"] in "kab" else c for c in B.PLAIN_COLUMNS]
ITEM_SCHEMA = {"id": K.T_UINT64, "items.position": K.T_UINT64, "items.price": K.T_UINT64}
ITEM_COLUMNS = [
    dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="items.position", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_PLAIN,
         rlevel_max=1, dlevel_max=2),
    dict(name="items.price", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN,
         rlevel_max=1, dlevel_max=2)]
rid, pos, price = col("id"), col("items.position"), col("items.price")


def objects(tmp_path, plans, columns):
    """the code objects `plans` leave in an empty cache directory"""
    for p in plans:
        assert E.compile_only(p, columns, cache_dir=str(tmp_path)) > 4000
    return sorted(glob.glob(str(tmp_path) + "/*.hsaco"))


def config3_with(l1, l2, **kw):
    return Plan(S, select=[k, sum_(v), count(1), sum_(b)], group_by=[k],
                where=(a > l1) & (b < l2), groups_hint=1000, **kw)


def grouped(where=None, key=None, arg=None):
    key = k if key is None else key
    return Plan(S, select=[key, sum_(a if arg is None else arg), count(1)], group_by=[key],
                where=where, groups_hint=1000)


def mixed_depth(l1, l2):
    return Plan(ITEM_SCHEMA, select=[pos, count(1), sum_(rid), sum_(price)], group_by=[pos],
                where=(pos > l1) & ((rid % 3).eq(l2)), scan_mode=K.SCAN_NESTED)


SAME_SHAPE = {
    "config3": (lambda: [B.config3(), config3_with(12345, 54321)], B.PLAIN_COLUMNS),
    "config3-16-bit-pages": (lambda: [B.config3(), config3_with(12345, 54321),
                                      config3_with(1 << 40, (1 << 64) - 1)], NARROW_COLUMNS),
    "float": (lambda: [grouped(where=v > x) for x in (0.0, -0.0, 1.5, -1e300)], B.PLAIN_COLUMNS),
    "negative-int64": (lambda: [grouped(where=a > x) for x in (-5, -7, -(1 << 63))],
                       B.PLAIN_COLUMNS),
    "key-expression": (lambda: [grouped(key=k + x) for x in (1, 2)], B.PLAIN_COLUMNS),
    "aggregate-argument": (lambda: [grouped(arg=a + x) for x in (1, 2)], B.PLAIN_COLUMNS),
    "bare-select-list": (lambda: [Plan(S, scan_select=[k, b + x], where=a > 100 * x)
                                  for x in (1, 2)], B.PLAIN_COLUMNS),
    "nested-where-rows": (lambda: [mixed_depth(2, 0), mixed_depth(3, 1)], ITEM_COLUMNS),
    # the divisor stays in the text, the literal inside the divisor's expression does not
    "inside-a-divisor": (lambda: [grouped(arg=a / (b - x)) for x in (3, 70000)], B.PLAIN_COLUMNS),
}


@pytest.mark.parametrize("name", sorted(SAME_SHAPE))
def test_same_shape_one_object(built, tmp_path, name):
    """plans that differ only in pooled literals compile to ONE code object"""
    plans, columns = SAME_SHAPE[name]
    objs = objects(tmp_path, plans(), columns)
    assert len(objs) == 1, (name, objs)
    if name == "nested-where-rows":
        assert "evql_where_rows" in kernel_facts(objs[0])


DIFFERENT_SHAPE = {
    "mod": (lambda: [grouped(arg=a % 7), grouped(arg=a % 9)], B.PLAIN_COLUMNS),
    "div": (lambda: [grouped(arg=a / 3), grouped(arg=a / 5)], B.PLAIN_COLUMNS),
    "float-div": (lambda: [grouped(arg=v / 3.0), grouped(arg=v / 5.0)], B.PLAIN_COLUMNS),
    "bool": (lambda: [grouped(where=(a > 5) & lit(True)), grouped(where=(a > 5) & lit(False))],
             B.PLAIN_COLUMNS),
    "uint-vs-int64": (lambda: [grouped(where=a > 5), grouped(where=a > -5)], B.PLAIN_COLUMNS),
    # `x >= 0` over an unsigned column is dropped by the planner (and with it the value
    # resets of a nested scan behind rejected rows); `x >= 1` is evaluated
    "dropped-where": (lambda: [Plan(ITEM_SCHEMA, select=[pos, count(1), sum_(price)],
                                    group_by=[pos], where=price >= x, scan_mode=K.SCAN_NESTED)
                               for x in (0, 1)], ITEM_COLUMNS),
}


@pytest.mark.parametrize("name", sorted(DIFFERENT_SHAPE))
def test_different_shape_two_objects(built, tmp_path, name):
    """what decides the text -- a constant divisor, a BOOL literal, a literal's type, a
    WHERE that is always true -- still gives a code object of its own"""
    plans, columns = DIFFERENT_SHAPE[name]
    assert len(objects(tmp_path, plans(), columns)) == 2, name


def plan40(lits):
    """40 numeric literals: lits[0] in WHERE, lits[1:] in the argument of the sum (the
    generator numbers them in this order)"""
    assert len(lits) == 40
    arg = a
    for x in lits[1:]:
        arg = arg + x
    return Plan(S, select=[k, sum_(arg), count(1)], group_by=[k], where=a > lits[0],
                groups_hint=1000)


def test_more_literals_than_the_pool(built, tmp_path):
    """the first 32 literals of a plan are pooled, the others stay in the text"""
    base = [1000 + 7 * i for i in range(40)]
    inside = list(base)
    inside[5] = 999_999
    beyond = list(base)
    beyond[35] = 999_999
    assert len(objects(tmp_path, [plan40(base)], B.PLAIN_COLUMNS)) == 1
    assert len(objects(tmp_path, [plan40(inside)], B.PLAIN_COLUMNS)) == 1
    assert len(objects(tmp_path, [plan40(beyond)], B.PLAIN_COLUMNS)) == 2


def test_process_wide_counters(built, tmp_path):
    """evql_ctx_kernel_cache_stats(NULL, ..): a compile, then the twin read from the disk"""
    s0 = E.kernel_cache_stats()
    E.compile_only(config3_with(777, 888), B.PLAIN_COLUMNS, cache_dir=str(tmp_path))
    s1 = E.kernel_cache_stats()
    assert (s1.compiles, s1.disk_hits) == (s0.compiles + 1, s0.disk_hits)
    assert s1.compile_ms > s0.compile_ms
    E.compile_only(config3_with(999, 111), B.PLAIN_COLUMNS, cache_dir=str(tmp_path))
    s2 = E.kernel_cache_stats()
    assert (s2.compiles, s2.disk_hits) == (s1.compiles, s1.disk_hits + 1)
    assert s2.compile_ms == s1.compile_ms
    assert s2.memory_hits == s0.memory_hits  # (a context's modules: none without a device)


def kernel_facts(code_object):
    """kernel name -> (spilled VGPRs, scratch bytes, FLAT instructions)"""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", code_object], capture_output=True,
                           text=True, check=True).stdout
    asm = subprocess.run([LLVM + "/llvm-objdump", "-d", code_object], capture_output=True,
                         text=True, check=True).stdout
    flat, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = m.group(1)
        elif "\tflat_" in line and cur:
            flat[cur] = flat.get(cur, 0) + 1
    facts = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\w+)", blk).group(1)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))  # noqa: E731
        facts[name] = (g("vgpr_spill_count"), g("private_segment_fixed_size"), flat.get(name, 0))
    return facts


@pytest.mark.parametrize("case", ["config3", "config3-16-bit-pages", "bare", "bare-16-bit-pages"])
def test_pooled_kernels_compile_clean(built, tmp_path, case):
    """reading literals from the kernel arguments costs no spilled VGPR, no scratch memory
    (a pool element addressed dynamically would copy the arguments to private memory) and
    no FLAT instruction"""
    columns = NARROW_COLUMNS if case.endswith("pages") else B.PLAIN_COLUMNS
    if case.startswith("config3"):
        plan, kernels = B.config3(), ["evql_scan_agg"]
    else:
        plan = Plan(S, scan_select=[k, b + 1, v * 2.0], where=(a > 30000) & (b < 30000))
        kernels = ["evql_scan_count", "evql_scan_emit"]
    objs = objects(tmp_path, [plan], columns)
    assert len(objs) == 1
    facts = kernel_facts(objs[0])
    for kernel in kernels:
        assert facts[kernel] == (0, 0, 0), (case, kernel, facts[kernel])
