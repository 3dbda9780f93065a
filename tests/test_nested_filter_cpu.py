"""Row filters on nested scans (CSTableScan::setFilter, sql/CSTableScan.cc:203-204, 426,
545, 642-645), CPU side: the planner lowers a nested plan that carries a row filter, and
the yardstick of tests/test_gpu_nested_filter.py -- the C oracle's restatement of the
filter -- is pinned by the identities that make a row filter on a nested scan a pure
RECORD mask:

  * an all-ones filter changes nothing;
  * grouping by the record id under a filter returns exactly the ids whose bit is set,
    with the per-record aggregates of the unfiltered run;
  * AGGREGATE_WITHIN_RECORD_FLAT emits popcount(filter) rows;
  * the partial aggregates under f and under ~f merge to the unfiltered result, in both
    scan modes (which is what lets oracle_partial_frame + oracle_merge state the result of
    a nested scan over a chain of files)."""
import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_, min_, max_, out
import lsm_nested_tables as LN
import lsm_tables
import nested_tables as N
import oracle_lib as O
import tables as T

ITEM_COLS = [
    dict(name="id", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="items.position", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_PLAIN,
         rlevel_max=1, dlevel_max=2),
    dict(name="items.price", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN,
         rlevel_max=1, dlevel_max=2)]
S = {"id": K.T_UINT64, "items.position": K.T_UINT64, "items.price": K.T_UINT64}
rid, pos, price = col("id"), col("items.position"), col("items.price")
WR = K.SCAN_NESTED_WITHIN_RECORD

NREC = 3000


def nested_kw():
    return dict(select=[pos, count(1), sum_(price), max_(rid)], group_by=[pos],
                where=price > 500, scan_mode=K.SCAN_NESTED)


def within_kw():
    return dict(scan_select=[count(pos), sum_(price), sum_(rid)],
                select=[out(0), count(1), sum_(out(1)), max_(out(2))], group_by=[out(0)],
                scan_mode=WR)


def test_filtered_nested_plans_are_lowered(built, tmp_path):
    """a SCAN_NESTED and a SCAN_NESTED_WITHIN_RECORD plan with a row filter compile to a
    code object (the planner used to answer EVQL_ENOTSUP "row filter on a nested scan");
    the filter only switches on the row-filter line flat plans already use"""
    f = np.arange(NREC) % 3 != 0
    for kw in (nested_kw(), within_kw()):
        assert E.compile_only(Plan(S, row_filter=f, **kw), ITEM_COLS, cache_dir=str(tmp_path)) > 4000


def test_within_record_where_stays_refused_under_a_filter(built):
    f = np.ones(NREC, bool)
    plan = Plan(S, scan_select=[count(1)], select=[sum_(out(0))], where=rid > 3, scan_mode=WR,
                row_filter=f)
    with pytest.raises(E.EvqlError) as ei:
        E.compile_only(plan, ITEM_COLS)
    assert ei.value.code == K.EVQL_ENOTSUP
    assert "WHERE in a WITHIN RECORD scan" in ei.value.msg


def test_row_range_on_a_nested_scan_stays_refused(built):
    for kw in (dict(row_end=10), dict(row_begin=5, row_end=10)):
        with pytest.raises(E.EvqlError) as ei:
            E.compile_only(Plan(S, **dict(nested_kw(), **kw)), ITEM_COLS)
        assert ei.value.code == K.EVQL_ENOTSUP and "row range" in ei.value.msg


@pytest.fixture(scope="module")
def items(built):
    img, st = N.items_table(NREC)
    f = np.random.default_rng(5).random(NREC) < 0.6
    return img, st, f


def rows_of(img, **kw):
    r = O.oracle_run(img, Plan(N.ITEMS_SCHEMA, **kw))
    return r, sorted(r.rows(), key=repr)


def test_oracle_all_ones_filter_is_no_filter(items):
    img, _, _ = items
    ones = np.ones(NREC, bool)
    for kw in (nested_kw(), within_kw(), dict(select=[count(1)], scan_mode=K.SCAN_NESTED)):
        a, ra = rows_of(img, **kw)
        b, rb = rows_of(img, row_filter=ones, **kw)
        assert ra == rb
        assert (a.rows_scanned, a.rows_passed) == (b.rows_scanned, b.rows_passed)


def test_oracle_filter_is_a_record_mask(items):
    img, st, f = items
    ids = np.arange(NREC, dtype=np.uint64) * np.uint64(7)  # synth.items_table_image
    kw = dict(select=[rid, count(1), sum_(price), sum_(pos)], group_by=[rid], scan_mode=K.SCAN_NESTED)
    full, _ = rows_of(img, **kw)
    part, _ = rows_of(img, row_filter=f, **kw)
    by_id = {r[0]: r for r in full.rows()}
    assert sorted(r[0] for r in part.rows()) == [int(x) for x in ids[f]]
    assert all(by_id[r[0]] == r for r in part.rows())
    # the nested loop counts the rows of rejected records as scanned, not as passed
    assert part.rows_scanned == full.rows_scanned == st["total"]
    assert part.rows_passed == int(np.maximum(st["cnt"], 1)[f].sum())
    # one row per kept record
    wr, _ = rows_of(img, row_filter=f, scan_select=[count(1), sum_(rid)],
                    select=[count(1), sum_(out(0)), sum_(out(1))], scan_mode=WR)
    assert wr.rows() == [(int(f.sum()), int(f.sum()), int(ids[f].sum()))]
    assert wr.rows_passed == int(f.sum())
    # the column-less loop: a rejected record is not even counted as scanned
    nc, _ = rows_of(img, row_filter=f, select=[count(1)], scan_mode=K.SCAN_NESTED)
    assert nc.rows() == [(int(f.sum()),)]
    assert (nc.rows_scanned, nc.rows_passed) == (int(f.sum()), int(f.sum()))
    # a filter shorter than the table drops the records behind it
    short, _ = rows_of(img, row_filter=f[:1000], **kw)
    assert sorted(r[0] for r in short.rows()) == [int(x) for x in ids[:1000][f[:1000]]]


def test_oracle_complementary_filters_merge_to_the_unfiltered_result(items):
    img, _, f = items
    for kw in (nested_kw(), within_kw(),
               dict(select=[count(1), sum_(price), min_(rid)], scan_mode=K.SCAN_NESTED)):
        final = Plan(N.ITEMS_SCHEMA, **kw)
        frames = [O.oracle_partial_frame(img, Plan(N.ITEMS_SCHEMA, mode=K.MODE_PARTIAL, row_filter=x, **kw))
                  for x in (f, ~f)]
        merged = O.oracle_merge(final, frames)
        exp = O.oracle_run(img, final)
        T.compare_results(merged.rows(), exp.rows(), exp.types, key_cols=len(kw.get("group_by", [])))


@pytest.mark.parametrize("pname", sorted(LN.PARTITIONS))
def test_nested_partitions(built, pname):
    """the helper's partitions: the C restatement of PartitionCursor's filters agrees with
    the python model on them, and the shapes the GPU tests rely on are there"""
    files = LN.partition(pname)
    got = O.oracle_partition_filters(files)
    exp = lsm_tables.model_filters(files)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert (g is None) == (e is None)
        if g is not None:
            assert (g == e).all()
    if pname == "basic":
        assert all(g is not None and g.sum() < len(g) for g in got[1:])  # records superseded
    if pname == "edges":
        assert [len(f[4]["ids"]) for f in files] == [2600, 1, 1800]
        for _, _, _, _, c in files[::2]:
            assert c["cnt"][1] == 0
            r = int(np.flatnonzero(c["cnt"] == 30)[0])
            assert c["starts"][r] < 2048 < c["starts"][r] + 30
