"""ORDER BY over a large GROUP BY result sorted on the device, without a GPU:
plan_order_sort decides as the design says (through evql_plan_order_sort, and on its own under
AddressSanitizer + UBSan), the entry points exist through every layer, and the new kernels
compile for gfx950 without scratch memory."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, out, sum_
import order_edges as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
ROCM = os.environ.get("ROCM", "/opt/rocm")
MIN = K.DEVICE_EMIT_MIN_GROUPS

# a schema with a string column: `s` in the select list is a first-row column
S_SCHEMA = dict(g=K.T_UINT64, u=K.T_UINT64, x=K.T_FLOAT64, s=K.T_STRING)
S_COLUMNS = [
    dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="u", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="x", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN)]


def s_plan(**kw):
    return Plan(S_SCHEMA, select=[col("g"), count(1), sum_(col("u")), col("s"), sum_(col("x"))],
                group_by=[col("g")], **kw)


def decide(plan, specs, n=MIN, columns=None, **kw):
    order = None if specs is None else Order(plan, specs, **kw)
    return E.plan_order_sort(plan, columns or X.DENSE_COLUMNS, order, n)


def test_accepted_orders(built, monkeypatch):
    monkeypatch.delenv("EVQL_ORDER_DEVICE_SORT", raising=False)
    plan = X.dense_plan()
    for c in range(len(X.DENSE_AGGS)):          # the key, isum, float sum, imin
        for desc in (False, True):
            assert decide(plan, [(c, desc)]) == K.OSORT_DEVICE
            assert decide(plan, [(c, desc), (0, False)], limit=100, offset=5) == K.OSORT_DEVICE
    assert decide(plan, [(4, True), (2, False), (0, True)], n=10_000_000) == K.OSORT_DEVICE
    main = X.main_plan()                          # min / max / mean, count
    specs = [(c, bool(c & 1)) for c in range(len(X.MAIN_AGGS))]
    assert decide(main, specs[:8], columns=X.COLUMNS) == K.OSORT_DEVICE
    assert decide(main, specs[5:], columns=X.COLUMNS) == K.OSORT_DEVICE


def test_the_threshold(built, monkeypatch):
    monkeypatch.delenv("EVQL_ORDER_DEVICE_SORT", raising=False)
    plan = X.dense_plan()
    assert MIN == 65_536
    assert decide(plan, [(1, True), (0, False)], n=65_535) == K.OSORT_FEW_RECORDS
    assert decide(plan, [(1, True), (0, False)], n=65_536) == K.OSORT_DEVICE
    assert decide(plan, [(1, True)], n=0) == K.OSORT_FEW_RECORDS
    assert decide(plan, [(1, True)], n=(1 << 32) - 1) == K.OSORT_DEVICE
    assert decide(plan, [(1, True)], n=1 << 32) == K.OSORT_TOO_MANY_RECORDS


def test_no_order(built, monkeypatch):
    monkeypatch.delenv("EVQL_ORDER_DEVICE_SORT", raising=False)
    plan = X.dense_plan()
    assert decide(plan, None) == K.OSORT_NO_ORDER
    assert decide(plan, [], limit=10) == K.OSORT_NO_ORDER      # LIMIT alone
    # ORDER BY above a PARTIAL aggregate is refused as evql_query_set_order refuses it
    with pytest.raises(E.EvqlError) as ei:
        decide(X.dense_plan(mode=K.MODE_PARTIAL), [(1, False)])
    assert ei.value.code == K.EVQL_EARG and "partial aggregate" in ei.value.msg


def test_environment_switch(built, monkeypatch):
    plan = X.dense_plan()
    monkeypatch.setenv("EVQL_ORDER_DEVICE_SORT", "0")
    assert decide(plan, [(1, True)]) == K.OSORT_SWITCHED_OFF
    assert decide(plan, [(1, True)], n=MIN - 1) == K.OSORT_FEW_RECORDS
    monkeypatch.setenv("EVQL_ORDER_DEVICE_SORT", "1")
    assert decide(plan, [(1, True)]) == K.OSORT_DEVICE


def test_refused_specs(built, monkeypatch):
    monkeypatch.delenv("EVQL_ORDER_DEVICE_SORT", raising=False)
    plan = s_plan()
    assert decide(plan, [(1, True), (0, False)], columns=S_COLUMNS) == K.OSORT_DEVICE
    # the second spec is a string column (read from the group's first row)
    assert decide(plan, [(1, True), (3, False)], columns=S_COLUMNS) == K.OSORT_UNREADABLE
    # the second spec is out(1) + out(2)
    assert decide(plan, [(1, True), (out(1) + out(2), False)],
                  columns=S_COLUMNS) == K.OSORT_EXPRESSION
    # post-aggregate arithmetic in the select list
    arith = Plan(S_SCHEMA, select=[col("g"), count(1), sum_(col("u")) + 1], group_by=[col("g")])
    assert decide(arith, [(1, True), (2, False)], columns=S_COLUMNS) == K.OSORT_UNREADABLE
    assert decide(arith, [(1, True), (0, False)], columns=S_COLUMNS) == K.OSORT_DEVICE
    # an exact float sum
    exact = s_plan(float_sum_mode=K.FLOAT_SUM_EXACT)
    assert decide(exact, [(1, True), (4, False)], columns=S_COLUMNS) == K.OSORT_UNREADABLE
    assert decide(s_plan(), [(1, True), (4, False)], columns=S_COLUMNS) == K.OSORT_DEVICE
    # a string group key
    skey = Plan(S_SCHEMA, select=[col("s"), count(1)], group_by=[col("s")])
    assert decide(skey, [(1, True), (0, False)], columns=S_COLUMNS) == K.OSORT_UNREADABLE
    # nine specs; eight
    dense = X.dense_plan()
    nine = [(c % 5, False) for c in range(9)]
    assert decide(dense, nine) == K.OSORT_TOO_MANY_SPECS
    assert decide(dense, nine[:8]) == K.OSORT_DEVICE
    assert K.ORDER_SORT_MAX_SPECS == 8
    # what evql_query_set_order refuses for the first spec is refused here the same way
    with pytest.raises(E.EvqlError) as ei:
        decide(plan, [(3, False)], columns=S_COLUMNS)
    assert ei.value.code == K.EVQL_ENOTSUP and "cannot be read from a group record" in ei.value.msg
    with pytest.raises(E.EvqlError) as ei:
        decide(plan, [(out(1) + out(2), False)], columns=S_COLUMNS)
    assert ei.value.code == K.EVQL_ENOTSUP and "not a plain output column" in ei.value.msg
    with pytest.raises(E.EvqlError) as ei:
        decide(exact, [(4, False)], columns=S_COLUMNS)
    assert ei.value.code == K.EVQL_ENOTSUP and "exact float sum" in ei.value.msg


def test_decision_codes():
    assert [K.OSORT_DEVICE, K.OSORT_NO_ORDER, K.OSORT_FEW_RECORDS, K.OSORT_SWITCHED_OFF,
            K.OSORT_EXPRESSION, K.OSORT_UNREADABLE, K.OSORT_TOO_MANY_SPECS,
            K.OSORT_TOO_MANY_RECORDS, K.OSORT_NAN_KEY] == list(range(9))
    hdr = open(os.path.join(CSRC, "order_sort_plan.h")).read()
    for name, v in (("OSORT_DEVICE", 0), ("OSORT_NO_ORDER", 1), ("OSORT_FEW_RECORDS", 2),
                    ("OSORT_SWITCHED_OFF", 3), ("OSORT_EXPRESSION", 4), ("OSORT_UNREADABLE", 5),
                    ("OSORT_TOO_MANY_SPECS", 6), ("OSORT_TOO_MANY_RECORDS", 7),
                    ("OSORT_NAN_KEY", 8)):
        assert re.search(r"\b%s = %d\b" % (name, v), hdr), name


def test_entry_points_through_every_layer(built):
    L = E.lib()
    for name in ("evql_query_order_stats", "evql_plan_order_sort"):
        assert hasattr(L, name)
    assert [f[0] for f in K.OrderStats._fields_] == [
        "sorted_on_device", "decision", "records", "rows", "n_keys", "n_sort_passes",
        "n_passes_skipped", "n_kernel_launches", "n_host_waits", "sort_ms"]
    # the C struct, as the compiler lays it out
    assert C.sizeof(K.OrderStats) == 56
    assert K.OrderStats.records.offset == 8 and K.OrderStats.sort_ms.offset == 48
    assert C.sizeof(K.EmitStats) == 48
    assert callable(getattr(E.Query, "order_stats", None))
    assert callable(getattr(E, "plan_order_sort", None))
    hpp = open(os.path.join(ROOT, "include", "evql_host.hpp")).read()
    assert "orderStats()" in hpp
    h = open(os.path.join(ROOT, "include", "evql_gpu.h")).read()
    assert "evql_order_stats_t" in h and "evql_plan_order_sort" in h


def test_sizeof_order_stats_matches_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evql_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(evql_order_stats_t), '
                   'offsetof(evql_order_stats_t, n_host_waits), sizeof(evql_emit_stats_t)); '
                   'return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert got == [str(C.sizeof(K.OrderStats)), str(K.OrderStats.n_host_waits.offset), "48"]


def test_null_arguments(built):
    """refused before anything touches a device"""
    L = E.lib()
    assert L.evql_query_order_stats(None, None) == K.EVQL_EARG
    st = K.OrderStats()
    assert L.evql_query_order_stats(None, C.byref(st)) == K.EVQL_EARG
    d = C.c_int()
    plan = X.dense_plan()
    infos = E._column_infos(X.DENSE_COLUMNS)
    o = Order(plan, [(1, False)])
    n = len(X.DENSE_COLUMNS)
    assert L.evql_plan_order_sort(None, infos, n, o.specs, 1, MIN, C.byref(d)) == K.EVQL_EARG
    assert L.evql_plan_order_sort(C.byref(plan.desc), None, n, o.specs, 1, MIN,
                                  C.byref(d)) == K.EVQL_EARG
    assert L.evql_plan_order_sort(C.byref(plan.desc), infos, n, None, 1, MIN,
                                  C.byref(d)) == K.EVQL_EARG
    assert L.evql_plan_order_sort(C.byref(plan.desc), infos, n, o.specs, 1, MIN, None) == K.EVQL_EARG
    assert L.evql_plan_order_sort(C.byref(plan.desc), infos, n, o.specs, 1, MIN,
                                  C.byref(d)) == K.EVQL_OK and d.value == K.OSORT_DEVICE


# ---- the host-only plan function under sanitizers ----------------------------------------------
def test_host_only_plan_under_sanitizers(tmp_path):
    """csrc/order_sort_plan.cc as a stand-alone program under AddressSanitizer + UBSan: no
    device, no HIP runtime"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "order_sort_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "order_sort_plan_check.cc"),
                           os.path.join(CSRC, "order_sort_plan.cc"),
                           os.path.join(CSRC, "result_cell.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- the kernels ------------------------------------------------------------------------------
NEW_KERNELS = ("k_ord_key_perm", "k_ord_gather")


def test_kernels_compile_without_scratch(tmp_path):
    out_ = str(tmp_path / "aot_kernels.hsaco")
    # the device half of the Makefile's aot_kernels.o rule, with the resource-usage remarks
    p = subprocess.run([ROCM + "/bin/hipcc", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I" + ROCM + "/include", "-I" + os.path.join(ROOT, "include"),
                        "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", "-ffp-contract=off",
                        "--cuda-device-only", "--no-gpu-bundle-output",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "aot_kernels.hip"), "-o", out_],
                       capture_output=True, text=True, check=True)
    facts = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            facts[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            facts[name][m.group(1).strip()] = int(m.group(2))
    seen = []
    for kernel in NEW_KERNELS + ("k_order_keys",):
        hits = [n for n in facts if kernel in n]
        assert len(hits) == 1, (kernel, hits)
        f = facts[hits[0]]
        print("%-24s vgpr %3d sgpr %3d lds %d scratch %d occupancy %d" % (
            kernel, f["VGPRs"], f["TotalSGPRs"], f["LDS Size"], f["ScratchSize"], f["Occupancy"]))
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (kernel, f)
        seen.append(kernel)
    assert len(seen) == 3
