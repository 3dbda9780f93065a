"""evql_lsm_chain_compact on the CPU: the yardstick of test_gpu_chain_compact.py pinned, and
the entry point's presence through every layer.

tests/compact_model.expected_image is what the GPU tests compare the compacted table with,
byte for byte.  Here the model itself is checked against the oracle's PartitionCursor
(orc_query_run_chain, pinned on the reference in test_lsm_partition.py): a scan of the
model's table must hand out the rows the cursor lets through, in the cursor's order, and
GROUP BYs over it -- including a first-row select expression, which depends on that order --
must give the chain's results."""
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_, max_
import compact_model as M
import lsm_nested_tables as LN
import lsm_tables
import oracle_lib as O
import tables as T

NESTED = K.SCAN_NESTED


def _partition(kind, pname):
    if kind == "flat":
        return (lsm_tables.partition(pname), lsm_tables.LSM_SCHEMA, M.flat_out_specs(), "rid")
    return (LN.partition(pname), LN.NESTED_LSM_SCHEMA, M.nested_out_specs(), "id")


CASES = [("flat", "basic"), ("flat", "mixed"), ("flat", "quiet"), ("nested", "edges")]


@pytest.mark.parametrize("kind,pname", CASES)
def test_model_table_scans_like_the_partition_cursor(kind, pname):
    files, schema, specs, rid = _partition(kind, pname)
    filters = O.oracle_partition_filters(files)
    model = lsm_tables.model_filters(files)
    for a, b in zip(filters, model):
        assert (a is None) == (b is None) and (a is None or (a == b).all())
    img = M.expected_image(files, specs, M.SCAN_ORDER)
    P = Plan(schema, scan_select=[col(rid)])
    got = O.oracle_run(img, P)
    exp = O.oracle_run_chain([f[1] for f in reversed(files)], filters, P)
    assert got.nrows == exp.nrows
    assert got.rows() == exp.rows()  # in order
    # oldest file first is another table with the same rows
    img2 = M.expected_image(files, specs, M.FILE_ORDER)
    got2 = O.oracle_run(img2, P)
    assert sorted(got2.rows()) == sorted(exp.rows())
    if len(files) > 1:
        assert got2.rows() != exp.rows()


def test_model_table_groups_like_the_chain():
    # a non-aggregate select expression keeps the group's first row in scan order
    files, schema, specs, _ = _partition("flat", "basic")
    filters = O.oracle_partition_filters(files)
    img = M.expected_image(files, specs, M.SCAN_ORDER)
    kw = dict(select=[col("k"), col("rid"), col("s"), count(1), sum_(col("a")), max_(col("n"))],
              group_by=[col("k")])
    got = O.oracle_run(img, Plan(schema, **kw))
    exp = O.oracle_run_chain([f[1] for f in reversed(files)], filters, Plan(schema, **kw))
    assert got.nrows == exp.nrows
    T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1)
    # a nested plan
    files, schema, specs, _ = _partition("nested", "edges")
    filters = O.oracle_partition_filters(files)
    img = M.expected_image(files, specs, M.SCAN_ORDER)
    kw = dict(select=[col("items.position"), count(1), sum_(col("items.price")), max_(col("id"))],
              group_by=[col("items.position")], scan_mode=NESTED)
    got = O.oracle_run(img, Plan(schema, **kw))
    exp = M.oracle_chain(files, filters, schema, kw)  # (nested chains: merged partials)
    assert got.nrows == exp.nrows
    T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1)


def test_model_applies_the_column_rules():
    files = lsm_tables.partition("basic")
    specs = M.flat_out_specs()
    with pytest.raises(ValueError):
        M.expected_columns(files, specs + [dict(name="__lsm_skip", logical_type=K.COL_BOOLEAN,
                                                storage_type=K.ENC_BOOLEAN_BITPACKED)], M.SCAN_ORDER)
    with pytest.raises(ValueError):
        M.expected_columns(files, specs + [dict(name="new_required", logical_type=K.COL_UNSIGNED_INT,
                                                storage_type=K.ENC_UINT64_PLAIN)], M.SCAN_ORDER)
    cols, rows = M.expected_columns(
        files, specs + [dict(name="new_optional", logical_type=K.COL_UNSIGNED_INT,
                             storage_type=K.ENC_UINT64_PLAIN, dlevel_max=1)], M.SCAN_ORDER)
    assert rows == sum(len(f[4]["ids"]) if x is None else int(x.sum())
                       for f, x in zip(reversed(files), lsm_tables.model_filters(files)))
    assert len(cols[-1]["present"]) == rows and not cols[-1]["present"].any()
    upd = cols[[s["name"] for s in specs].index("__lsm_is_update")]
    assert len(upd["values"]) == rows and not upd["values"].any()
    assert any(f[4]["upd"].any() for f in files)


def test_host_only_plan_under_sanitizers(tmp_path):
    """column resolution and output sizes (csrc/chain_compact_plan.cc) as a stand-alone
    program under AddressSanitizer + UBSan: no device, no HIP runtime"""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "eventql_amd", "csrc")
    exe = str(tmp_path / "chain_compact_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc,
                           os.path.join(root, "tools", "chain_compact_plan_check.cc"),
                           os.path.join(csrc, "chain_compact_plan.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


# ---- the entry point, layer by layer --------------------------------------------------------
def test_library_exports_the_entry_point():
    assert hasattr(E.lib(), "evql_lsm_chain_compact")


def test_capi_binds_it():
    assert K.COMPACT_SCAN_ORDER == 0 and K.COMPACT_FILE_ORDER == 1
    names = [f[0] for f in K.CompactStats._fields_]
    assert names == ["rows_in", "rows_written", "string_bytes", "n_tables", "n_kernel_launches",
                     "n_host_waits", "gather_ms", "encode_ms"]
    import ctypes
    assert ctypes.sizeof(K.CompactStats) == 48
    fn = E.lib().evql_lsm_chain_compact
    assert fn.argtypes is not None and len(fn.argtypes) == 7


def test_wrapper_has_compact():
    assert callable(getattr(E.LsmChain, "compact", None))
    # null arguments are refused before anything touches a device
    assert E.lib().evql_lsm_chain_compact(None, None, 0, 0, 0, None, None) == K.EVQL_EARG
