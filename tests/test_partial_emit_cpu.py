"""EVQL_MODE_PARTIAL rows packed on the device, without a GPU: the python model of the wire
rows is pinned on the oracle for every table of test_gpu_partial_emit.py, plan_partial_emit
decides as DESIGN.md 3.7 says (through evql_plan_partial_emit, and on its own under
AddressSanitizer + UBSan), and the new kernels compile for gfx950 without scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Agg, Call, Plan, col, count, lit, sum_
import oracle_lib as O
import partial_emit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
ROCM = os.environ.get("ROCM", "/opt/rocm")
PARTIAL = K.MODE_PARTIAL


# ---- the model is the oracle's ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_model_equals_the_oracle(built, name):
    img, c, rows = M.wide_table()
    cs = M.CASES[name]
    exp = O.oracle_run(img, Plan(M.SCHEMA, mode=PARTIAL, **M.plan_kwargs(cs)))
    model = M.model_rows(cs, c, rows, M.SCHEMA)
    assert exp.nrows == len(model) >= M.MIN_GROUPS
    assert M.oracle_rows(exp) == model


@pytest.mark.parametrize("groups", [M.MIN_GROUPS - 1, M.MIN_GROUPS, M.MIN_GROUPS + 1, 150_001])
def test_model_equals_the_oracle_on_the_threshold_tables(built, groups):
    img, c, rows = M.key_table(groups)
    exp = O.oracle_run(img, Plan(M.KEY_SCHEMA, mode=PARTIAL, **M.plan_kwargs(M.THRESHOLD_CASE)))
    model = M.model_rows(M.THRESHOLD_CASE, c, rows, M.KEY_SCHEMA)
    assert exp.nrows == len(model) == groups
    assert M.oracle_rows(exp) == model


def test_model_bytes():
    assert M.varuint(0) == b"\x00" and M.varuint(127) == b"\x7f" and M.varuint(128) == b"\x80\x01"
    assert [len(M.varuint(x)) for x in M.SUM_VALUES] == [1, 1, 2, 5, 9, 10, 2, 5]
    assert len(M.varuint(M.M64)) == 10
    # the 16-byte quirk: a string of 11
    for n, last in ((10, 0), (11, 0x80), (12, 0)):
        e = M.encoded_cell(K.T_STRING, b"x" * n)
        assert e[0] == K.T_STRING and e[1] == 4 + n + 1 and e[-1] == last
    e = M.encoded_cell(K.T_STRING, b"y" * 128)
    assert e[1:3] == M.varuint(133) and len(M.varuint(133)) == 2
    assert M.encoded_cell(K.T_STRING, None) == bytes([K.T_STRING, 5, 0, 0, 0, 0, 1])
    assert M.encoded_cell(K.T_BOOL, 1) == bytes([K.T_BOOL, 2, 1, 0])
    # tuple lengths of the string key cross one, two and three SHA-1 blocks
    lens = {4 + len(M.group_string(g)) + 1 for g in range(131)}
    assert {55, 56, 64, 119, 120, 128} <= lens
    img, c, rows = M.wide_table()
    assert len(set(c["s"])) >= 70_000


# ---- which plans take the device path ---------------------------------------------------------
def decide(kw, n=M.MIN_GROUPS, merged=False, mode=PARTIAL, schema=M.SCHEMA, columns=M.COLUMNS):
    return E.plan_partial_emit(Plan(schema, mode=mode, **kw), columns, n, merged)


@pytest.mark.parametrize("name", sorted(M.CASES))
def test_accepted_plan_classes(built, name, monkeypatch):
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    kw = M.plan_kwargs(M.CASES[name])
    assert decide(kw) == K.PEMIT_DEVICE
    assert decide(kw, n=M.MIN_GROUPS - 1) == K.PEMIT_FEW_GROUPS
    assert decide(kw, n=10_000_000) == K.PEMIT_DEVICE
    assert decide(kw, mode=K.MODE_FINAL) == K.PEMIT_NOT_PARTIAL


def test_environment_switch(built, monkeypatch):
    kw = M.plan_kwargs(M.CASES["u64"])
    monkeypatch.setenv("EVQL_PARTIAL_DEVICE_EMIT", "0")
    assert decide(kw) == K.PEMIT_SWITCHED_OFF
    monkeypatch.setenv("EVQL_PARTIAL_DEVICE_EMIT", "1")
    assert decide(kw) == K.PEMIT_DEVICE


def test_refused_plan_classes(built, monkeypatch):
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    k, a, b, s, vs = col("k"), col("a"), col("b"), col("s"), col("vs")
    # count_distinct: the saved state is a set
    assert decide(dict(select=[k, Agg("count_distinct", a)], group_by=[k])) == K.PEMIT_AGGREGATE
    # an exact float sum is rounded from 128 bits on the host
    assert decide(dict(select=[k, sum_(vs)], group_by=[k], float_sum_mode=K.FLOAT_SUM_EXACT,
                       float_sum_bound=1e6)) == K.PEMIT_AGGREGATE
    assert decide(dict(select=[k, sum_(vs)], group_by=[k])) == K.PEMIT_DEVICE
    # keys that need eval_expr
    key = Call("add", b, lit(1))
    assert decide(dict(select=[key, count(1)], group_by=[key])) == K.PEMIT_GROUP_EXPR
    assert decide(dict(select=[k, key, count(1)], group_by=[k, key])) == K.PEMIT_GROUP_EXPR
    key = Call("to_int64", b)
    assert decide(dict(select=[k, key, count(1)], group_by=[k, key])) == K.PEMIT_GROUP_EXPR
    # select expressions that do
    assert decide(dict(select=[k, Call("add", b, lit(1)), count(1)],
                       group_by=[k])) == K.PEMIT_SELECT_EXPR
    # more than 32 columns
    assert decide(dict(select=[k] * 32 + [count(1)], group_by=[k])) == K.PEMIT_TOO_WIDE
    assert decide(dict(select=[k] * 31 + [count(1)], group_by=[k])) == K.PEMIT_DEVICE
    # post-aggregate arithmetic does not matter: the row carries the saved state
    assert decide(dict(select=[k, sum_(a) + 1], group_by=[k])) == K.PEMIT_DEVICE


def test_merged_results(built, monkeypatch):
    """after an exchange / a chain merge the first rows live in the records: only exact keys"""
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    assert decide(M.plan_kwargs(M.CASES["sums"]), merged=True) == K.PEMIT_DEVICE
    assert decide(M.plan_kwargs(M.CASES["min_max_mean"]), merged=True) == K.PEMIT_DEVICE
    assert decide(M.plan_kwargs(M.CASES["columns"]), merged=True) == K.PEMIT_SELECT_EXPR
    assert decide(M.plan_kwargs(M.CASES["u64_string"]), merged=True) == K.PEMIT_GROUP_EXPR
    assert decide(M.plan_kwargs(M.CASES["string"]), merged=True) == K.PEMIT_GROUP_EXPR


def test_nested_scans_keep_the_host_loop(built, monkeypatch):
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    S = {"id": K.T_UINT64, "items.position": K.T_UINT64}
    cols = [dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
            dict(name="items.position", logical_type=K.COL_UNSIGNED_INT,
                 storage_type=K.ENC_UINT32_PLAIN, rlevel_max=1, dlevel_max=1)]
    kw = dict(select=[col("id"), count(1)], group_by=[col("id")], scan_mode=K.SCAN_NESTED)
    assert decide(kw, schema=S, columns=cols) == K.PEMIT_NESTED
    kw["scan_mode"] = K.SCAN_FLAT
    assert decide(dict(select=[col("id"), count(1)], group_by=[col("id")]), schema=S,
                  columns=cols) == K.PEMIT_DEVICE


def test_entry_points_through_every_layer(built):
    import ctypes as C
    L = E.lib()
    for name in ("evql_query_emit_stats", "evql_ctx_sha1_ranges", "evql_plan_partial_emit"):
        assert hasattr(L, name)
    assert [f[0] for f in K.EmitStats._fields_] == [
        "device_packed", "partial", "rows", "key_bytes", "data_bytes", "n_kernel_launches",
        "n_host_waits", "pack_ms"]
    assert C.sizeof(K.EmitStats) == 48
    assert callable(getattr(E.Query, "emit_stats", None))
    assert callable(getattr(E.Context, "sha1_ranges", None))
    hpp = open(os.path.join(ROOT, "include", "evql_host.hpp")).read()
    assert "emitStats()" in hpp
    # null arguments are refused before anything touches a device
    assert L.evql_query_emit_stats(None, None) == K.EVQL_EARG
    assert L.evql_ctx_sha1_ranges(None, None, 0, None, 0, None) == K.EVQL_EARG


# ---- the host-only plan function under sanitizers ----------------------------------------------
def test_host_only_plan_under_sanitizers(tmp_path):
    """csrc/partial_emit_plan.cc as a stand-alone program under AddressSanitizer + UBSan: no
    device, no HIP runtime"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "partial_emit_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "partial_emit_plan_check.cc"),
                           os.path.join(CSRC, "partial_emit_plan.cc"),
                           os.path.join(CSRC, "result_cell.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- the kernels ------------------------------------------------------------------------------
NEW_KERNELS = ("k_partial_sizes", "k_partial_tuple_bytes", "k_partial_data_bytes", "k_sha1_ranges")


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
    assert len(seen) == 4
