"""The device merge of PARTIAL rows without a GPU: its host-only frame indexer
(csrc/merge_frame_index.cc) under AddressSanitizer + UBSan, its row offsets against a python
walk of real frames, and the entry points through every layer."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, Col as col, count, sum_, min_, max_, mean, count_distinct
import merge_frames as F
import oracle_lib as O
import tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
S = T.SURVEY_SCHEMA
N = 20_000


def test_frame_indexer_under_sanitizers(tmp_path):
    """truncations at every byte, over-long varuints, lengths behind the end, zero rows"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "merge_frame_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "merge_frame_index_check.cc"),
                           os.path.join(CSRC, "merge_frame_index.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


@pytest.mark.parametrize("kw,cells", [
    (dict(select=[col("k"), sum_(col("a")), count(1)], group_by=[col("k")]), "suu"),
    (dict(select=[col("k"), col("s"), count(1), min_(col("a")), max_(col("v")), mean(col("b")),
                  sum_(col("v"))], group_by=[col("k"), col("s")]), "ssucccf"),
    (dict(select=[count(col("n")), sum_(col("n")), min_(col("n")), mean(col("n"))],
          group_by=[col("n") % 7]), "uucc"),
])
def test_offsets_equal_a_python_walk(built, kw, cells):
    img = T.survey_table(N)[0]
    frame = O.oracle_partial_frame(img, Plan(S, mode=K.MODE_PARTIAL, **kw))
    off = E.merge_index_frame(Plan(S, **kw), frame)
    assert off == F.walk_frame(frame, cells)
    assert len(off) > 2 and off[-1] == len(frame)


def test_indexer_answers_like_add_frame(built):
    kw = dict(select=[col("k"), sum_(col("a"))], group_by=[col("k")])
    plan = Plan(S, **kw)
    assert E.merge_index_frame(plan, O.partial_frame([], [])) == [2]
    good = O.partial_frame([F.key(1)], [F.sv_u64(5) + F.st_uint(9)])
    assert E.merge_index_frame(plan, good) == [2, len(good)]
    for bad in (good[:-1], good[:30], b"\x00", O.varuint(0) + O.varuint(3)):
        with pytest.raises(E.EvqlError) as ei:
            E.merge_index_frame(plan, bad)
        assert ei.value.code == K.EVQL_EIO
        assert "invalid partialaggr result encoding" in ei.value.msg
    # a string where the select expression returns a number: another size class
    with pytest.raises(E.EvqlError) as ei:
        E.merge_index_frame(plan, O.partial_frame([F.key(1)], [F.sv_str(b"x") + F.st_uint(9)]))
    assert ei.value.code == K.EVQL_ENOTSUP
    # ... NIL fits every class
    assert len(E.merge_index_frame(plan, O.partial_frame([F.key(1)], [F.sv_nil() + F.st_uint(9)]))) == 2
    with pytest.raises(E.EvqlError) as ei:
        E.merge_index_frame(Plan(S, select=[col("k"), count_distinct(col("b"))], group_by=[col("k")]),
                            good)
    assert ei.value.code == K.EVQL_ENOTSUP


def test_entry_points_through_every_layer(built):
    L = E.lib()
    for name in ("evql_merge_create_device", "evql_merge_stats", "evql_merge_index_frame"):
        assert hasattr(L, name)
    assert [f[0] for f in K.MergeStats._fields_] == [
        "on_device", "packed_on_device", "frames", "rows_added", "rows_pending", "groups",
        "compactions", "sort_passes", "prefix_collisions", "full_key_sorts", "device_bytes",
        "host_index_ms", "upload_ms", "merge_ms", "pack_ms"]
    assert C.sizeof(K.MergeStats) == 112
    assert callable(getattr(E.Merge, "stats", None))
    hpp = open(os.path.join(ROOT, "include", "evql_host.hpp")).read()
    assert "GroupByMerge(evql_ctx_t* ctx, const evql_plan_desc_t& plan)" in hpp
    assert "evql_merge_create_device" in hpp
    # null arguments are refused before anything touches a device
    assert L.evql_merge_create_device(None, None, None) == K.EVQL_EARG
    assert L.evql_merge_stats(None, None) == K.EVQL_EARG
    # a host merge: every statistic is zero
    m = E.Merge(Plan(S, select=[col("k"), count(1)], group_by=[col("k")]))
    m.add_frame(O.partial_frame([F.key(1)], [F.sv_u64(5) + F.st_uint(9)]))
    st = m.stats()
    assert all(getattr(st, f[0]) == 0 for f in K.MergeStats._fields_)
    m.close()
