"""evql_lsm_chain_compact_sorted on the CPU: the entry point's presence through every layer,
its argument refusals that need no device, the key rule of the host-only plan, and the
yardstick of test_gpu_chain_compact_sorted.py (tests/compact_sorted_model.py) checked
against itself."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
import compact_model as M
import compact_sorted_model as SM
import lsm_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the entry point, layer by layer --------------------------------------------------------
def test_library_exports_the_entry_point():
    assert hasattr(E.lib(), "evql_lsm_chain_compact_sorted")


def test_capi_binds_it():
    names = [f[0] for f in K.CompactSortStats._fields_]
    assert names == ["rows", "key_min", "key_max", "presorted", "passes", "n_kernel_launches",
                     "n_host_waits", "sort_ms", "permute_ms"]
    assert ctypes.sizeof(K.CompactSortStats) == 48
    fn = E.lib().evql_lsm_chain_compact_sorted
    assert fn.argtypes is not None and len(fn.argtypes) == 9
    assert fn.argtypes[3] is ctypes.c_char_p


def test_the_tile_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "eventql_amd", "csrc", "aot_kernels.h")).read()
    assert int(re.search(r"kSortTile = (\d+);", src).group(1)) == K.COMPACT_SORT_TILE


def test_the_header_declares_it():
    src = open(os.path.join(ROOT, "include", "evql_gpu.h")).read()
    assert "evql_lsm_chain_compact_sorted(" in src and "evql_compact_sort_stats_t;" in src


def test_wrapper_has_compact_sorted():
    assert callable(getattr(E.LsmChain, "compact_sorted", None))
    # null arguments are refused before anything touches a device
    fn = E.lib().evql_lsm_chain_compact_sorted
    assert fn(None, None, 0, None, 0, 0, None, None, None) == K.EVQL_EARG
    assert fn(None, None, 0, b"k", 0, 0, None, None, None) == K.EVQL_EARG
    # ... and the plain call still is
    assert E.lib().evql_lsm_chain_compact(None, None, 0, 0, 0, None, None) == K.EVQL_EARG


def test_key_rule_of_the_host_only_plan_under_sanitizers(tmp_path):
    """plan_compact_sort_key / plan_compact_sort_rows (csrc/chain_compact_plan.cc) as a
    stand-alone program under AddressSanitizer + UBSan: no device, no HIP runtime"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(ROOT, "eventql_amd", "csrc")
    exe = str(tmp_path / "chain_compact_sort_key_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(ROOT, "tools", "chain_compact_sort_key_check.cc"),
                           os.path.join(csrc, "chain_compact_plan.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- the model ------------------------------------------------------------------------------
def test_sorted_input_is_a_fixed_point_of_the_model():
    # rid ascends in FILE_ORDER: sorting by it changes nothing
    files = lsm_tables.partition("basic")
    specs = M.flat_out_specs()
    cols, rows, perm = SM.expected_columns(files, specs, "rid", M.FILE_ORDER)
    assert (perm == np.arange(rows)).all()
    assert SM.expected_image(files, specs, "rid", M.FILE_ORDER) == \
        M.expected_image(files, specs, M.FILE_ORDER)
    plain, _ = M.expected_columns(files, specs, M.FILE_ORDER)
    assert SM.expected_passes(SM.key_words(specs, plain, "rid"))[:2] == (1, 0)
    # in SCAN_ORDER the files come newest first: descending blocks, another table
    cols2, rows2, perm2 = SM.expected_columns(files, specs, "rid", M.SCAN_ORDER)
    assert rows2 == rows and (perm2 != np.arange(rows)).any()
    assert SM.expected_image(files, specs, "rid", M.SCAN_ORDER) != \
        M.expected_image(files, specs, M.SCAN_ORDER)
    # ... with the same rows, and sorting it again changes nothing
    rid = specs.index(next(s for s in specs if s["name"] == "rid"))
    assert (np.asarray(cols2[rid]["values"]) == np.asarray(cols[rid]["values"])).all()
    assert (np.argsort(np.asarray(cols2[rid]["values"], np.uint64), kind="stable") ==
            np.arange(rows)).all()


@pytest.mark.parametrize("order", [M.SCAN_ORDER, M.FILE_ORDER])
def test_the_model_orders_ties_as_the_plain_order_does(order):
    # k has 40 distinct values over thousands of rows; rid is unique per row
    files = lsm_tables.partition("basic")
    specs = M.flat_out_specs()
    plain, rows = M.expected_columns(files, specs, order)
    cols, rows2, perm = SM.expected_columns(files, specs, "k", order)
    names = [s["name"] for s in specs]
    k, rid = names.index("k"), names.index("rid")
    assert rows == rows2 > 1000
    ks = np.asarray(cols[k]["values"], np.uint64)
    assert len(np.unique(ks)) == 40 and (ks[1:] >= ks[:-1]).all()
    # position of every row in the plain order, by its rid
    where = {int(r): i for i, r in enumerate(np.asarray(plain[rid]["values"]))}
    pos = np.array([where[int(r)] for r in np.asarray(cols[rid]["values"])])
    same = ks[1:] == ks[:-1]
    assert same.sum() > 1000 and (pos[1:][same] > pos[:-1][same]).all()
    # every column moved with its row
    for c in (names.index("a"), names.index("v")):
        assert (np.asarray(cols[c]["values"]) == np.asarray(plain[c]["values"])[pos]).all()
    n = names.index("n")
    assert (cols[n]["present"] == plain[n]["present"][pos]).all()
    s = names.index("s")
    assert cols[s]["values"] == [plain[s]["values"][i] for i in pos]


def test_unsigned_order_and_pass_counts_of_the_model():
    keys = np.array([2**63 + 5, 3, 2**64 - 1, 2**63 - 2, 2**63], np.uint64)
    assert list(np.argsort(keys, kind="stable")) == [1, 3, 4, 0, 2]
    assert SM.expected_passes(keys) == (0, 8, 3, 2**64 - 1)
    base = np.uint64(2**51)
    narrow = base + np.array([999, 0, 500], np.uint64)
    assert SM.expected_passes(narrow) == (0, 2, 2**51, 2**51 + 999)
    assert SM.expected_passes(np.array([7, 7, 7], np.uint64)) == (1, 0, 7, 7)
    assert SM.expected_passes(np.array([], np.uint64)) == (1, 0, 0, 0)
    assert SM.expected_passes(np.array([9, 8], np.uint64)) == (0, 1, 8, 9)
