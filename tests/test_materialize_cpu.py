"""Result materialisation (Query.to_table / evql_table_from_query) without a GPU: the entry
points exist in every layer, evql_plan_materialize decides as DESIGN.md 3.12 says -- through
the C ABI, and plan_materialize on its own under AddressSanitizer + UBSan --, and the new
kernels compile for gfx950 without scratch memory."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Agg, Call, Plan, col, count, lit, max_, mean, min_, sum_
import materialize_model as M
import partial_emit_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_entry_points_through_every_layer(built):
    L = E.lib()
    for name in ("evql_table_from_query", "evql_plan_materialize"):
        assert hasattr(L, name)
    assert [f[0] for f in K.MaterializeStats._fields_] == [
        "rows", "string_bytes", "presorted", "passes", "n_kernel_launches", "n_host_waits",
        "gather_ms", "sort_ms", "encode_ms"]
    assert C.sizeof(K.MaterializeStats) == 48
    assert callable(getattr(E.Query, "to_table", None)) and hasattr(E.Query, "materialize_stats")
    assert callable(E.plan_materialize)
    hpp = open(os.path.join(ROOT, "include", "evql_host.hpp")).read()
    assert "toTable(" in hpp
    # null arguments are refused before anything touches a device
    t = C.c_void_p()
    assert L.evql_table_from_query(None, None, 0, -1, 0, None, None) == K.EVQL_EARG
    assert L.evql_table_from_query(None, None, 1, -1, 0, C.byref(t), None) == K.EVQL_EARG
    d = C.c_int()
    assert L.evql_plan_materialize(None, None, 0, None, 0, -1, 0, C.byref(d)) == K.EVQL_EARG
    plan = M.key_plan()
    assert L.evql_plan_materialize(C.byref(plan.desc), None, 0, None, 0, -1, 0, None) == K.EVQL_EARG


# ---- which plans are materialised -------------------------------------------------------------
def test_accepted_plans(built):
    assert M.decide(M.cell_plan(), M.CELL_COLUMNS, M.CELL_SPECS) == K.MAT_DEVICE
    assert M.decide(M.cell_plan(), M.CELL_COLUMNS, M.CELL_SPECS, sort_by="n") == K.MAT_DEVICE
    assert M.decide(M.cell_plan(), M.CELL_COLUMNS, M.CELL_SPECS, sort_by="t") == K.MAT_DEVICE
    for specs in M.ID_SPECS.values():
        for sort_by in (None, "k", "sum_a", "max_a"):
            assert M.decide(M.id_plan(), M.ID_COLUMNS, specs, sort_by=sort_by) == K.MAT_DEVICE
    assert M.decide(M.key_plan(), PM.KEY_COLUMNS, M.KEY_SPECS, sort_by="k") == K.MAT_DEVICE
    assert M.decide(M.key_plan(), PM.KEY_COLUMNS, M.KEY_SPECS, sort_by="k", merged=True) == K.MAT_DEVICE
    assert M.decide(M.sort_plan(), M.SORT_COLUMNS, M.SORT_SPECS, sort_by="r") == K.MAT_DEVICE
    # a hashed key: its columns are first-row bare columns
    S = M.ID_SCHEMA
    plan = Plan(S, select=[col("k"), col("s"), count(1)], group_by=[col("k"), col("s")])
    specs = [M.U64("k"), M.STR("s"), M.LEB("n")]
    assert M.decide(plan, M.ID_COLUMNS, specs, sort_by="k") == K.MAT_DEVICE
    assert M.decide(plan, M.ID_COLUMNS, specs, merged=True) == K.MAT_FIRST_ROW
    assert "merged" in E.last_error()
    # a global aggregate is one group
    plan = Plan(S, select=[count(1), sum_(col("a"))])
    assert M.decide(plan, M.ID_COLUMNS, [M.U64("n"), M.U64("sum_a")]) == K.MAT_DEVICE


def test_refused_plans(built):
    S, cols = M.ID_SCHEMA, M.ID_COLUMNS
    k, a, nb, fv, s = col("k"), col("a"), col("nb"), col("fv"), col("s")

    def decide(select, specs, group_by=(k,), **kw):
        plan_kw = {x: kw.pop(x) for x in ("mode", "float_sum_mode", "float_sum_bound", "scan_mode")
                   if x in kw}
        return M.decide(Plan(S, select=select, group_by=list(group_by), **plan_kw), cols, specs, **kw)

    base = [M.U64("k"), M.U64("x")]
    # EVQL_ENOTSUP
    assert decide([k, sum_(a) + 1], base) == K.MAT_POST_AGGREGATE
    assert "post-aggregate" in E.last_error()
    assert decide([k, sum_(fv)], [M.U64("k"), M.F64("x")], float_sum_mode=K.FLOAT_SUM_EXACT,
                  float_sum_bound=1e6) == K.MAT_EXACT_SUM
    assert decide([k, sum_(fv)], [M.U64("k"), M.F64("x")]) == K.MAT_DEVICE
    assert decide([k, sum_(Call("add", a, lit(-5)))], base) == K.MAT_INT64
    assert "INT64" in E.last_error()
    assert decide([k, Call("to_int64", a)], base) == K.MAT_INT64
    key = Call("add", a, lit(1))
    assert decide([key, count(1)], base, group_by=[key]) == K.MAT_KEY_EXPR
    assert decide([k, Call("add", a, lit(1)), count(1)], base + [M.U64("n")]) == K.MAT_KEY_EXPR
    assert decide([k, key, count(1)], base + [M.U64("n")], group_by=[k, key]) == K.MAT_KEY_EXPR
    assert decide([k, s, count(1)], [M.U64("k"), M.STR("s"), M.U64("n")], merged=True) == K.MAT_FIRST_ROW
    assert decide([k] * 32 + [count(1)], [M.U64("c%d" % i) for i in range(33)]) == K.MAT_TOO_WIDE
    assert decide([k] * 31 + [count(1)], [M.U64("c%d" % i) for i in range(32)]) == K.MAT_DEVICE
    # a bare scan
    plan = Plan(S, scan_select=[k, a])
    assert M.decide(plan, cols, base) == K.MAT_BARE_SCAN
    # the sort column: optional, float, boolean, string
    sel = [k, min_(nb), col("fv"), col("fb"), s]
    specs = [M.U64("k"), M.U64("m", dlevel_max=1), M.F64("fv"), M.BOOL("fb"), M.STR("s")]
    assert decide(sel, specs, sort_by="k") == K.MAT_DEVICE
    for name in ("m", "fv", "fb", "s"):
        assert decide(sel, specs, sort_by=name) == K.MAT_SORT_KEY, name
        assert name in E.last_error()
    assert decide([k, count(1)], [M.U64("k", dlevel_max=1), M.U64("n")], sort_by="k") == K.MAT_SORT_KEY
    # EVQL_EARG
    assert decide([k, count(1)], base, mode=K.MODE_PARTIAL) == K.MAT_PARTIAL_MODE
    assert decide([k, count(1)], base + [M.U64("y")]) == K.MAT_COLUMN_COUNT
    assert decide([k, count(1)], base[:1]) == K.MAT_COLUMN_COUNT
    assert decide([k, count(1)], [M.U64("k"), M.U64("x", rlevel_max=1)]) == K.MAT_NESTED_SPEC
    assert decide([k, count(1)], [M.U64("k"), M.U64("x", dlevel_max=2)]) == K.MAT_NESTED_SPEC
    assert decide([k, count(1)], base, sort_by=2) == K.MAT_SORT_COLUMN
    assert decide([k, count(1)], base, sort_by=-2) == K.MAT_SORT_COLUMN
    for wrong in (M.F64("x"), M.STR("x"), M.BOOL("x"), M.TS("x"),
                  M.spec("x", K.COL_SIGNED_INT, K.ENC_UINT64_PLAIN)):
        assert decide([k, count(1)], [M.U64("k"), wrong]) == K.MAT_TYPE_MISMATCH, wrong
    assert decide([k, mean(a)], base) == K.MAT_TYPE_MISMATCH
    assert decide([k, s], [M.U64("k"), M.U64("s")]) == K.MAT_TYPE_MISMATCH
    assert "type" in E.last_error()


def test_nil_typed_column(built):
    k, a = col("k"), col("a")
    plan = Plan(M.ID_SCHEMA, select=[k, Call("to_nil", a), count(1)], group_by=[k])
    assert M.decide(plan, M.ID_COLUMNS, [M.U64("k"), M.U64("x"), M.U64("n")]) == K.MAT_NIL
    assert "NIL" in E.last_error()


def test_model_images_read_back(built):
    """the expectations of the GPU tests: the oracle's inner rows, written by E.Writer and
    scanned by the oracle, are the same rows"""
    import oracle_lib as O
    img, c = M.cell_table()
    exp = O.oracle_run(img, M.cell_plan())
    assert exp.nrows == M.CELL_GROUPS
    rows = sorted(exp.rows(), key=M.row_key)
    back = M.scan_image(M.writer_image(M.CELL_SPECS, rows), M.CELL_SPECS)
    assert back.types == exp.types
    M.assert_rows_equal(back.rows(), rows, exp.types, rel=0.0)
    img, c = M.id_table()
    rows = sorted(O.oracle_run(img, M.id_plan()).rows())
    assert len(rows) == M.ID_GROUPS
    for specs in M.ID_SPECS.values():
        assert M.scan_image(M.writer_image(specs, rows), specs).rows() == rows
    assert M.scan_image(M.writer_image(M.KEY_SPECS, []), M.KEY_SPECS).rows() == []


def test_nested_scans_are_refused_for_first_row_columns(built):
    S = {"id": K.T_UINT64, "items.position": K.T_UINT64}
    cols = [dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
            dict(name="items.position", logical_type=K.COL_UNSIGNED_INT,
                 storage_type=K.ENC_UINT32_PLAIN, rlevel_max=1, dlevel_max=1)]
    sel = [col("id"), col("items.position"), count(1)]
    plan = Plan(S, select=sel, group_by=[col("id"), col("items.position")], scan_mode=K.SCAN_NESTED)
    specs = [M.U64("id"), M.U64("p", dlevel_max=1), M.U64("n")]
    assert M.decide(plan, cols, specs) == K.MAT_FIRST_ROW
    assert "nested" in E.last_error()
    # key and aggregates only are fine over a nested scan
    plan = Plan(S, select=[col("id"), count(1)], group_by=[col("id")], scan_mode=K.SCAN_NESTED)
    assert M.decide(plan, cols, [M.U64("id"), M.U64("n")]) == K.MAT_DEVICE


# ---- the host-only plan function under sanitizers ----------------------------------------------
def test_host_only_plan_under_sanitizers(tmp_path):
    """csrc/materialize_plan.cc as a stand-alone program under AddressSanitizer + UBSan: no
    device, no HIP runtime"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "materialize_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "materialize_plan_check.cc"),
                           os.path.join(CSRC, "materialize_plan.cc"),
                           os.path.join(CSRC, "result_cell.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- the kernels ------------------------------------------------------------------------------
NEW_KERNELS = ("k_mat_first_rows", "k_mat_fixed", "k_mat_str_sizes", "k_mat_str_bytes")


def test_kernels_compile_without_scratch(tmp_path):
    out = str(tmp_path / "aot_kernels.hsaco")
    # the device half of the Makefile's aot_kernels.o rule, with the resource-usage remarks
    p = subprocess.run([ROCM + "/bin/hipcc", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I" + ROCM + "/include", "-I" + os.path.join(ROOT, "include"),
                        "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", "-ffp-contract=off",
                        "--cuda-device-only", "--no-gpu-bundle-output",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "aot_kernels.hip"), "-o", out],
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
    for kernel in NEW_KERNELS:
        hits = [n for n in facts if kernel in n]
        assert len(hits) == 1, (kernel, hits)
        f = facts[hits[0]]
        print("%-24s vgpr %3d sgpr %3d lds %d scratch %d occupancy %d" % (
            kernel, f["VGPRs"], f["TotalSGPRs"], f["LDS Size"], f["ScratchSize"], f["Occupancy"]))
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (kernel, f)
        seen.append(kernel)
    assert len(seen) == len(NEW_KERNELS)
