"""GroupByMergeExpression on the device (evql_merge_create_device): frames of
the oracle's PartialGroupBy restatement over the survey table and hand-built frames, against
the oracle's merge and the host merge of the same frames."""
import math
import struct

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, Col as col, count, sum_, min_, max_, mean, count_distinct
import merge_frames as F
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

N = 200_000
S = T.SURVEY_SCHEMA
SORT_TILE = 2048       # kSortTile
DEVICE_PACK = 1 << 16  # kDeviceEmitMinGroups

# test_merge_cpu.py's plans, without the count_distinct one
PLANS = [
    (dict(select=[col("k"), sum_(col("a")), count(1), sum_(col("b"))], group_by=[col("k")],
          where=(col("a") > 30000) & (col("b") < 30000)), 1),
    (dict(select=[col("k"), col("s"), count(1), min_(col("a")), max_(col("v")), mean(col("b")),
                  sum_(col("v"))], group_by=[col("k"), col("s")]), 2),
    (dict(select=[count(col("n")), sum_(col("n")), min_(col("n")), mean(col("n"))],
          group_by=[col("n") % 7]), 0),
    (dict(select=[col("k"), col("a"), count(1)], group_by=[col("k")]), 1),
    (dict(select=[count(1), sum_(col("a")) + count(1), max_(col("b"))]), 0),
]


@pytest.fixture(scope="module")
def survey(built):
    return T.survey_table(N)[0]


def _ranges(n, parts):
    step = (n + parts - 1) // parts
    return [(i * step, min(n, (i + 1) * step)) for i in range(parts)]


def _part(lo, hi, **kw):
    mask = np.zeros(N, np.uint8)
    mask[lo:hi] = 1
    return Plan(S, mode=K.MODE_PARTIAL, row_filter=mask, **kw)


_frames_cache = {}


def _survey_frames(img, kw_index, kw, parts):
    """the frames of one plan over `parts` row ranges: computed once"""
    key = (kw_index, parts)
    if key not in _frames_cache:
        _frames_cache[key] = [O.oracle_partial_frame(img, _part(lo, hi, **kw))
                              for lo, hi in _ranges(N, parts)]
    return _frames_cache[key]


def _run(plan, frames, ctx=None):
    """(Result, MergeStats) of a merge of `frames`: on the device with a context"""
    m = E.Merge(plan, ctx)
    for f in frames:
        m.add_frame(f)
    res = m.fetch_all()
    st = m.stats()
    m.close()
    return res, st


def _same_rows(got, exp):
    assert got.types == exp.types
    assert sorted(map(repr, got.rows())) == sorted(map(repr, exp.rows()))


@pytest.mark.parametrize("idx", range(len(PLANS)))
def test_plans_of_the_host_merge_suite(survey, ctx, idx):
    kw, nkeys = PLANS[idx]
    frames = _survey_frames(survey, idx, kw, 3)
    plan = Plan(S, **kw)
    got, st = _run(plan, frames, ctx)
    exp = O.oracle_merge(plan, frames)
    host, _ = _run(plan, frames)
    assert st.on_device == 1 and st.frames == 3 and st.rows_pending == 0
    assert st.groups == got.nrows == exp.nrows
    assert got.types == exp.types
    if nkeys:
        T.compare_results(got.rows(), exp.rows(), got.types, key_cols=nkeys, rel=0)
    else:
        assert sorted(map(repr, got.rows())) == sorted(map(repr, exp.rows()))
    # the host merge folds in the same order: the same bits, floats included
    _same_rows(got, host)


def test_count_distinct_is_left_to_the_host_merge(ctx):
    plan = Plan(S, select=[col("k"), count_distinct(col("b"))], group_by=[col("k")])
    with pytest.raises(E.EvqlError) as ei:
        E.Merge(plan, ctx)
    assert ei.value.code == K.EVQL_ENOTSUP
    E.Merge(plan).close()


def test_non_aggregates_take_the_last_frame(ctx):
    """groupby.cc:606-610 on hand-built rows: a numeric, a string and a NIL cell, and a string
    whose tag byte is 0x80 (STAG_INLINE), which comes out as it went in"""
    plan = Plan(S, select=[col("k"), col("s"), count(1)], group_by=[col("k")])
    A, B, C_, D = (F.key(i) for i in range(4))
    f1 = O.partial_frame([A, B, C_, D], [
        F.sv_u64(1) + F.sv_str(b"first") + F.st_uint(1),
        F.sv_u64(2) + F.sv_str(b"bee") + F.st_uint(1),
        F.sv_u64(3) + F.sv_str(b"sea") + F.st_uint(1),
        F.sv_u64(4) + F.sv_str(b"dee") + F.st_uint(1)])
    f2 = O.partial_frame([C_, A, B], [
        F.sv_nil() + F.sv_str(b"sea2") + F.st_uint(1),
        F.sv_u64(10) + F.sv_str(b"hello world", tag=0x80) + F.st_uint(1),
        F.sv_u64(20) + F.sv_nil() + F.st_uint(1)])
    got, _ = _run(plan, [f1, f2], ctx)
    host, _ = _run(plan, [f1, f2])
    assert sorted(map(repr, got.rows())) == sorted(map(repr, [
        (10, b"hello world", 2), (20, None, 2), (None, b"sea2", 2), (4, b"dee", 1)]))
    _same_rows(got, host)
    elem = struct.pack("<I", 11) + b"hello world" + b"\x80"
    assert elem in got.raw[1] and elem in host.raw[1]
    assert len(got.raw[1]) == len(host.raw[1])


def test_adding_after_a_fetch_restarts_the_iteration(ctx):
    """the doubled sums of test_merge_cpu.py test_reference_verified_bytes"""
    key = bytes.fromhex("72d31a72564b88de26a4bd48ce436c184f0d38f4")
    data = bytes.fromhex("01096301000000000000008c89f60eb607")
    plan = Plan(S, select=[col("k"), sum_(col("a")), count(1)], group_by=[col("k")])
    m = E.Merge(plan, ctx)
    m.add_frame(O.partial_frame([key], [data]))
    assert m.fetch_all().rows() == [(355, 31294604, 950)]
    m.add_frame(O.partial_frame([key], [data], flags=1))
    assert m.num_groups == 1
    assert m.fetch_all().rows() == [(355, 2 * 31294604, 1900)]
    assert m.fetch_all().rows() == []  # (drained, as the host merge)
    st = m.stats()
    assert st.frames == 2 and st.rows_added == 2 and st.groups == 1 and st.compactions == 2
    m.close()


@pytest.mark.parametrize("n", [0, 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1])
def test_small_and_border_shapes(ctx, n):
    plan = Plan(S, select=[col("k"), sum_(col("a")), sum_(col("v"))], group_by=[col("k")])
    keys = [F.key(i) for i in range(n)]
    rows = lambda order, scale: [F.sv_u64(i) + F.st_uint(i * scale) + F.st_f64(0.1 * i * scale)
                                 for i in order]
    f1 = O.partial_frame(keys, rows(range(n), 1))
    f2 = O.partial_frame(keys[::-1], rows(range(n - 1, -1, -1), 3))
    md, mh = E.Merge(plan, ctx), E.Merge(plan)
    for frames in ([f1], [f2]):
        for f in frames:
            md.add_frame(f)
            mh.add_frame(f)
        got, host = md.fetch_all(), mh.fetch_all()
        assert got.nrows == n == md.num_groups
        _same_rows(got, host)
    st = md.stats()
    assert st.frames == 2 and st.rows_added == 2 * n and st.prefix_collisions == 0
    md.close()
    mh.close()


def test_one_key_many_times_folds_in_arrival_order(ctx):
    """5,000 float states of one group in one frame: the sum is the host merge's bit for bit"""
    plan = Plan(S, select=[col("k"), sum_(col("v")), mean(col("v"))], group_by=[col("k")])
    vals = np.random.default_rng(5).normal(0, 1e6, 5000)
    frame = O.partial_frame([F.key(9)] * 5000,
                            [F.sv_u64(9) + F.st_f64(x) + F.st_cnt_f64(1, x) for x in vals])
    got, _ = _run(plan, [frame], ctx)
    host, _ = _run(plan, [frame])
    assert got.nrows == 1 and got.raw == host.raw


def test_ieee_edge_values(ctx):
    plan = Plan(S, select=[col("k"), sum_(col("v")), min_(col("v")), max_(col("v"))],
                group_by=[col("k")])
    inf, nan = float("inf"), float("nan")
    groups = [[-0.0], [-0.0, -0.0], [0.0, -0.0], [inf, 1.0], [inf, -inf], [-inf, -1.0], [nan, 1.0],
              [1.0, nan], [1e308, 1e308], [5e-324, 5e-324]]
    depth = max(map(len, groups))
    frames = []
    for j in range(depth):
        sel = [(g, v[j]) for g, v in enumerate(groups) if j < len(v)]
        frames.append(O.partial_frame(
            [F.key(g) for g, _ in sel],
            [F.sv_u64(g) + F.st_f64(x) + F.st_cnt_f64(1, x) + F.st_cnt_f64(1, x) for g, x in sel]))
    got, _ = _run(plan, frames, ctx)
    host, _ = _run(plan, frames)
    exp = O.oracle_merge(plan, frames)
    T.compare_results(got.rows(), exp.rows(), got.types, key_cols=1, rel=0)
    T.compare_results(got.rows(), host.rows(), got.types, key_cols=1, rel=0)
    by_key = {r[0]: r for r in got.rows()}
    # the fold starts from the zero state: 0.0 + -0.0 = 0.0; min / max take the first value as it is
    assert math.copysign(1, by_key[0][1]) == 1 and math.copysign(1, by_key[0][2]) == -1
    assert math.copysign(1, by_key[1][1]) == 1
    assert by_key[3][1:] == (inf, 1.0, inf) and math.isnan(by_key[4][1])
    assert math.isnan(by_key[6][2]) and by_key[7][2:] == (1.0, 1.0)
    assert by_key[8][1] == inf and by_key[9][1] == 1e-323


def test_states_without_a_value_are_null(ctx):
    plan = Plan(S, select=[col("k"), min_(col("a")), max_(col("v")), mean(col("b"))],
                group_by=[col("k")])
    empty = F.st_cnt_u64(0, 0) + F.st_cnt_f64(0, 0.0) + F.st_cnt_f64(0, 0.0)
    full = F.st_cnt_u64(2, 7) + F.st_cnt_f64(2, -1.5) + F.st_cnt_f64(4, 10.0)
    f1 = O.partial_frame([F.key(0), F.key(1)], [F.sv_u64(0) + empty, F.sv_u64(1) + empty])
    f2 = O.partial_frame([F.key(1), F.key(0)], [F.sv_u64(1) + full, F.sv_u64(0) + empty])
    got, _ = _run(plan, [f1, f2], ctx)
    host, _ = _run(plan, [f1, f2])
    assert sorted(map(repr, got.rows())) == sorted(map(repr, [(0, None, None, None), (1, 7, -1.5, 2.5)]))
    _same_rows(got, host)


def test_forced_compactions_keep_device_memory_bounded(survey, ctx, monkeypatch):
    monkeypatch.setenv("EVQL_MERGE_PENDING_ROWS", "1000")
    kw = dict(select=[col("k"), col("s"), count(1), sum_(col("v"))], group_by=[col("k")])
    frames = _survey_frames(survey, "compactions", kw, 7)
    plan = Plan(S, **kw)
    m = E.Merge(plan, ctx)
    monkeypatch.delenv("EVQL_MERGE_PENDING_ROWS")  # (read at create)
    bytes_after = []
    for f in frames:
        m.add_frame(f)
        bytes_after.append(m.stats().device_bytes)
    got = m.fetch_all()
    st = m.stats()
    m.close()
    host, _ = _run(plan, frames)
    assert st.compactions >= 2 and st.rows_pending == 0
    # records are 3 key words, 2 words per non-aggregate, 1 per count / sum
    frame_rows = max(len(E.merge_index_frame(plan, f)) - 1 for f in frames)
    one_frame = max(map(len, frames)) + frame_rows * (3 + 2 + 2 + 1 + 1) * 8
    assert bytes_after[6] <= bytes_after[2] + one_frame, bytes_after
    _same_rows(got, host)


def test_keys_that_share_their_first_eight_bytes(ctx):
    plan = Plan(S, select=[col("k"), sum_(col("a")), sum_(col("v"))], group_by=[col("k")])
    A, B, C_ = b"PREFIX!!" + b"\x01" * 12, b"PREFIX!!" + b"\x01" * 11 + b"\x02", F.key(5)
    row = lambda k, a: F.sv_u64(k) + F.st_uint(a) + F.st_f64(a / 4)
    f1 = O.partial_frame([A, B, C_], [row(1, 10), row(2, 200), row(3, 5)])
    f2 = O.partial_frame([A, B], [row(1, 30), row(2, 400)])
    got, st = _run(plan, [f1, f2], ctx)
    assert st.prefix_collisions > 0 and st.full_key_sorts == 1
    assert sorted(got.rows()) == [(1, 40, 10.0), (2, 600, 150.0), (3, 5, 1.25)]
    _same_rows(got, _run(plan, [f1, f2])[0])


def test_large_results_are_packed_on_the_device(ctx):
    """70,000 groups (>= kDeviceEmitMinGroups) over three frames, some keys in all of them"""
    n = 70_000
    assert n >= DEVICE_PACK
    rng = np.random.default_rng(11)
    keys = [bytes(k) for k in rng.integers(0, 256, (n, 20), dtype=np.uint8)]
    a = rng.integers(0, 1 << 40, n)
    v = rng.normal(0, 1000, n)
    plan = Plan(S, select=[count(1), sum_(col("a")), mean(col("b")), min_(col("v")), col("k"),
                           col("s"), sum_(col("a")) + 1], group_by=[col("k")])

    def frame(ids, j):
        return O.partial_frame(
            [keys[i] for i in ids],
            [F.st_uint(j + 1) + F.st_uint(int(a[i]) + j) + F.st_cnt_f64(i % 3, float(i) * (j + 1))
             + F.st_cnt_f64((i + j) % 2, v[i] - j) + F.sv_u64(i) + F.sv_str(b"s%d_%d" % (i, j) * (i % 3))
             + F.st_uint(int(a[i]) + j) for i in ids])

    frames = [frame(range(0, 40_000), 0),
              frame(list(range(0, 20_000)) + list(range(40_000, 55_000)), 1),
              frame(list(range(0, 20_000)) + list(range(55_000, n)), 2)]
    got, st = _run(plan, frames, ctx)
    host, hst = _run(plan, frames)
    assert st.packed_on_device == 1 and hst.on_device == 0
    assert got.nrows == n == st.groups
    _same_rows(got, host)
    assert [len(r) for r in got.raw] == [len(r) for r in host.raw]


def test_malformed_frames_change_nothing(survey, ctx):
    kw = dict(select=[col("k"), sum_(col("a"))], group_by=[col("k")])
    frame = O.oracle_partial_frame(survey, Plan(S, mode=K.MODE_PARTIAL, row_end=5000, **kw))
    m = E.Merge(Plan(S, **kw), ctx)
    m.add_frame(frame)
    before, rows_added = m.fetch_all(), m.stats().rows_added
    assert before.nrows > 0
    for bad in (frame[:-1], frame[:30], b"\x00", O.varuint(0) + O.varuint(3)):
        with pytest.raises(E.EvqlError) as ei:
            m.add_frame(bad)
        assert ei.value.code == K.EVQL_EIO
        assert "invalid partialaggr result encoding" in ei.value.msg
        assert m.stats().rows_added == rows_added and m.stats().frames == 1
    assert m.fetch_all().nrows == 0  # (still drained: no add succeeded, as on the host)
    m.add_frame(O.partial_frame([], []))  # zero rows: restarts the iteration, adds nothing
    after = m.fetch_all()
    assert after.raw == before.raw and m.stats().rows_added == rows_added
    m.close()


def test_add_rows_takes_next_batch_vectors(survey, ctx):
    kw = dict(select=[col("s"), count(1), sum_(col("a"))], group_by=[col("s")])
    plan = Plan(S, **kw)
    m, h = E.Merge(plan, ctx), E.Merge(plan)
    for lo, hi in _ranges(N, 2):
        r = O.oracle_run(survey, _part(lo, hi, **kw))
        keys_raw = b"".join((20).to_bytes(4, "little") + r.keys[20 * i:20 * i + 20] + b"\0"
                            for i in range(r.nrows))
        m.add_rows(keys_raw, r.raw[0], r.nrows)
        h.add_rows(keys_raw, r.raw[0], r.nrows)
    exp = O.oracle_run(survey, plan)
    got = m.fetch_all()
    T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1)
    _same_rows(got, h.fetch_all())
    with pytest.raises(E.EvqlError) as ei:
        m.add_rows(keys_raw[:-1], r.raw[0], r.nrows)
    assert ei.value.code == K.EVQL_EIO and "invalid partial aggregate rows" in ei.value.msg
    m.close()
    h.close()
