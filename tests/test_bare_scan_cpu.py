"""Bare scans (SELECT .. WHERE without GROUP BY / aggregate), the parts that need no GPU:
their kernels compile for gfx950 and are clean in the ISA, what stays refused is refused
by name, and the oracle the GPU suite compares against agrees with numpy on row order,
values, NULL tags and the raise-only-for-passing-rows rule."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K
from eventql_amd.plan import If, Plan, col, count, out, sum_
import oracle_lib as O
import tables as T

LLVM = "/opt/rocm/lib/llvm/bin"

STRING_SCHEMA = dict(k=K.T_UINT64, s=K.T_STRING, s2=K.T_STRING, n=K.T_UINT64)
STRING_COLUMNS = [
    dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_BITPACKED, bits=16),
    dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
    dict(name="s2", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1),
    dict(name="n", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1)]
ITEMS_SCHEMA = {"id": K.T_UINT64, "items.position": K.T_UINT64, "items.price": K.T_UINT64}
ITEMS_COLUMNS = [
    dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="items.position", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_BITPACKED,
         rlevel_max=1, dlevel_max=2),
    dict(name="items.price", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128,
         rlevel_max=1, dlevel_max=2)]


def bare_plans():
    S = dict(B.SCHEMA)
    k, a, b, v = [col(x) for x in "kabv"]
    s, s2, n, k2 = col("s"), col("s2"), col("n"), col("k")
    return [
        ("plain", Plan(S, scan_select=[k, v], where=(a > 30000) & (b < 30000)), B.PLAIN_COLUMNS),
        ("no-where", Plan(S, scan_select=[k, a + b, v * 2.0]), B.PLAIN_COLUMNS),
        ("if-and-division", Plan(S, scan_select=[If(a > 5000, a / (b - b), b), k % 7], where=b > 10,
                                 row_filter=np.ones(16, bool)), B.PLAIN_COLUMNS),
        ("strings-nullable-16bit", Plan(STRING_SCHEMA, scan_select=[k2, s, s2, n, s < "g5"],
                                        where=s2.neq("") & (n > 3)), STRING_COLUMNS),
        ("nested", Plan(ITEMS_SCHEMA, scan_select=[col("id"), col("items.position"),
                                                   col("items.price") + 1],
                        where=col("items.price") > 5, scan_mode=K.SCAN_NESTED), ITEMS_COLUMNS),
    ]


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


@pytest.mark.parametrize("idx", range(5))
def test_bare_scan_kernels_compile_clean(built, tmp_path, idx):
    """evql_scan_count and evql_scan_emit of every plan shape: present, no spilled VGPRs,
    no scratch memory, no FLAT instruction (every access has its address space)"""
    name, plan, columns = bare_plans()[idx]
    assert E.compile_only(plan, columns, cache_dir=str(tmp_path)) > 4000, name
    objs = glob.glob(str(tmp_path) + "/*.hsaco")
    assert len(objs) == 1
    facts = kernel_facts(objs[0])
    for kernel in ("evql_scan_count", "evql_scan_emit"):
        assert kernel in facts, (name, sorted(facts))
        assert facts[kernel] == (0, 0, 0), (name, kernel, facts[kernel])
    assert "evql_scan_agg" not in facts


def test_grouped_plans_keep_their_code_objects(built, tmp_path):
    """the bare-scan generator shares the row function, the tile loads and the column
    declarations with the grouped kernels: a grouped plan and its bare twin never share a
    code object, and compiling the bare one leaves the grouped one's digest alone"""
    E.compile_only(B.config3(), B.PLAIN_COLUMNS, cache_dir=str(tmp_path))
    grouped = set(os.listdir(tmp_path))
    E.compile_only(bare_plans()[0][1], B.PLAIN_COLUMNS, cache_dir=str(tmp_path))
    E.compile_only(B.config3(), B.PLAIN_COLUMNS, cache_dir=str(tmp_path))
    assert len(os.listdir(tmp_path)) == 2 and grouped < set(os.listdir(tmp_path))


def test_what_stays_refused(built):
    S = dict(B.SCHEMA)
    k, a = col("k"), col("a")
    with pytest.raises(E.EvqlError) as ei:
        E.compile_only(Plan(S, scan_select=[k, a], mode=K.MODE_PARTIAL), B.PLAIN_COLUMNS)
    assert ei.value.code == K.EVQL_EARG and "partial" in ei.value.msg
    with pytest.raises(E.EvqlError) as ei:
        E.compile_only(Plan(ITEMS_SCHEMA, scan_select=[count(col("items.position")),
                                                       sum_(col("items.price"))],
                            scan_mode=K.SCAN_NESTED_WITHIN_RECORD), ITEMS_COLUMNS)
    assert ei.value.code == K.EVQL_ENOTSUP and "WITHIN RECORD" in ei.value.msg
    # a string-producing select expression
    s, s2 = col("s"), col("s2")
    for e in (If(col("k") > 1, s, s2), s + s2):
        with pytest.raises(E.EvqlError) as ei:
            E.compile_only(Plan(STRING_SCHEMA, scan_select=[e]), STRING_COLUMNS)
        assert ei.value.code == K.EVQL_ENOTSUP and "string" in ei.value.msg
    # a select list above the scan without aggregates or keys is still not a bare scan
    with pytest.raises(E.EvqlError) as ei:
        E.compile_only(Plan(S, scan_select=[k], group_by=[out(0)]), B.PLAIN_COLUMNS)
    assert ei.value.code == K.EVQL_ENOTSUP


def test_oracle_bare_scan_is_numpy(built):
    """the yardstick of tests/test_gpu_bare_scan.py: row order, values, NULL tags, and
    errors raised only for rows that pass the filter and WHERE"""
    n = 20_000
    img, c = T.mixed_table(n)
    S = T.MIXED_SCHEMA
    a, b, s, ns, nn, v, k = [col(x) for x in ("a", "b", "s", "ns", "n", "v", "k")]
    flt = np.arange(n) % 3 != 0
    m = (c["a"] > 30000) & (c["b"] < 40000)
    r = O.oracle_run(img, Plan(S, scan_select=[k, a + b, v * 2.0, s, ns, nn], where=(a > 30000) & (b < 40000)))
    assert r.types == [K.T_UINT64, K.T_UINT64, K.T_FLOAT64, K.T_STRING, K.T_STRING, K.T_UINT64]
    assert r.nrows == int(m.sum()) and r.rows_passed == r.nrows and r.rows_scanned == n
    idx = np.nonzero(m)[0]
    assert r.columns[0] == c["k"][idx].tolist()
    assert r.columns[1] == (c["a"][idx] + c["b"][idx]).tolist()
    assert r.columns[2] == (c["v"][idx] * 2.0).tolist()
    assert r.columns[3] == [c["s"][i] for i in idx]
    assert r.columns[4] == [c["ns"][i] if c["ns_present"][i] else None for i in idx]
    assert r.columns[5] == [int(c["n"][i]) if c["n_present"][i] else None for i in idx]
    # row filter and row_end
    r = O.oracle_run(img, Plan(S, scan_select=[a], where=a > 1000, row_filter=flt))
    assert r.columns[0] == c["a"][(c["a"] > 1000) & flt].tolist()
    r = O.oracle_run(img, Plan(S, scan_select=[a], where=a > 1000, row_end=9000))
    assert r.columns[0] == c["a"][:9000][c["a"][:9000] > 1000].tolist()
    # IF picks per row; the empty result
    r = O.oracle_run(img, Plan(S, scan_select=[If(a > 5000, nn, b)], where=b > 10))
    idx = np.nonzero(c["b"] > 10)[0]
    exp = [(int(c["n"][i]) if c["n_present"][i] else None) if c["a"][i] > 5000 else int(c["b"][i])
           for i in idx]
    assert r.columns[0] == exp
    assert O.oracle_run(img, Plan(S, scan_select=[a], where=a > 10**9)).nrows == 0
    # a zero divisor raises only where a row passes
    assert O.oracle_run(img, Plan(S, scan_select=[a / (b - b)], where=a > 10**9)).nrows == 0
    with pytest.raises(RuntimeError) as ei:
        O.oracle_run(img, Plan(S, scan_select=[a / (b - b)], where=a > 1000))
    assert "zero" in str(ei.value)
    assert O.oracle_run(img, Plan(S, scan_select=[If(b > 70000, a / (b - b), a)])).nrows == n
