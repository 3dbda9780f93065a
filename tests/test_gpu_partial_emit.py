"""EVQL_MODE_PARTIAL rows of large results packed on the device: the
(SHA-1 key -> saved states) rows must equal the oracle's byte for byte -- on both sides of the
65,536-group threshold, from both record sources, for every key and state class, through the
host loop as well (EVQL_PARTIAL_DEVICE_EMIT=0), in slices of every size -- and the plans
plan_partial_emit refuses must keep the host loop.  tests/partial_emit_model.py holds the
tables and plans; test_partial_emit_cpu.py pins its model of the rows on the same oracle."""
import ctypes as C
import functools
import hashlib
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Agg, Call, Plan, col, count, lit, sum_, unpack_svector
import nested_tables as NT
import oracle_lib as O
import partial_emit_model as M

pytestmark = pytest.mark.gpu
PARTIAL = K.MODE_PARTIAL


@pytest.fixture(scope="module")
def wide(ctx):
    t = ctx.open_image(M.wide_table()[0])
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's rows of a case of the wide table: computed once, shared, never changed"""
    plan = Plan(M.SCHEMA, mode=PARTIAL, **M.plan_kwargs(M.CASES[name]))
    return M.oracle_rows(O.oracle_run(M.wide_table()[0], plan))


def run_partial(t, schema, kw, batch=1024):
    """-> ({key: data}, rows, emit stats, bytes of the two columns)"""
    q = t.query(Plan(schema, mode=PARTIAL, **kw))
    try:
        q.execute()
        res = q.fetch_all(batch)
        return dict(res.rows()), res.nrows, q.emit_stats(), [len(r) for r in res.raw]
    finally:
        q.close()


def check_stats(st, nrows, sizes, packed):
    assert st["device_packed"] == (1 if packed else 0), st
    assert st["partial"] == 1 and st["rows"] == nrows, st
    if packed:
        assert st["key_bytes"] == 25 * nrows == sizes[0] and st["data_bytes"] == sizes[1], (st, sizes)
        assert st["n_kernel_launches"] >= 6 and 1 <= st["n_host_waits"] <= 2 and st["pack_ms"] > 0, st
    else:
        assert st["key_bytes"] == 0 and st["data_bytes"] == 0 and st["n_kernel_launches"] == 0, st


# ---- 1. the threshold --------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [M.MIN_GROUPS - 1, M.MIN_GROUPS, M.MIN_GROUPS + 1, 150_001])
def test_threshold(ctx, groups):
    img = M.key_table(groups)[0]
    kw = M.plan_kwargs(M.THRESHOLD_CASE)
    exp = M.oracle_rows(O.oracle_run(img, Plan(M.KEY_SCHEMA, mode=PARTIAL, **kw)))
    assert len(exp) == groups
    t = ctx.open_image(img)
    try:
        got, nrows, st, sizes = run_partial(t, M.KEY_SCHEMA, kw)
    finally:
        t.close()
    check_stats(st, groups, sizes, packed=groups >= M.MIN_GROUPS)
    assert nrows == len(got) == groups
    assert got == exp


def test_emit_stats_before_a_fetch_and_for_final_results(ctx):
    img = M.key_table(M.MIN_GROUPS)[0]
    t = ctx.open_image(img)
    q = t.query(Plan(M.KEY_SCHEMA, **M.plan_kwargs(M.THRESHOLD_CASE)))
    try:
        with pytest.raises(E.EvqlError) as ei:
            q.emit_stats()
        assert ei.value.code == K.EVQL_EARG
        q.execute()
        with pytest.raises(E.EvqlError) as ei:
            q.emit_stats()
        assert ei.value.code == K.EVQL_EARG
        res = q.fetch_all()
        st = q.emit_stats()
        assert st["device_packed"] == 1 and st["partial"] == 0 and st["rows"] == res.nrows == M.MIN_GROUPS
        assert st["key_bytes"] == 0 and st["data_bytes"] == 0 and st["n_kernel_launches"] >= 1
    finally:
        q.close()
        t.close()


# ---- 2. - 5. record sources, keys, states; the device path and the host path -------------------
RUNS = [(name, 0) for name in sorted(M.CASES)] + [("u64", 200_000), ("u64_string", 200_000),
                                                   ("sums", 200_000), ("u64", 1000),
                                                   ("u64_string", 1000)]


@pytest.mark.parametrize("name,hint", RUNS)
def test_rows_equal_the_oracle_on_both_paths(wide, monkeypatch, name, hint):
    """groups_hint 200000: the dense records of the partitioned path; 1000: an LDS table far too
    small, the groups are compacted from the HBM table; 0: whichever the cardinality probe picks"""
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    kw = dict(M.plan_kwargs(M.CASES[name]), groups_hint=hint)
    exp = expected(name)
    assert len(exp) >= M.MIN_GROUPS
    got, nrows, st, sizes = run_partial(wide, M.SCHEMA, kw)
    check_stats(st, len(exp), sizes, packed=True)
    assert nrows == len(got) == len(exp)
    assert got == exp
    # the switch is read when the query is created
    monkeypatch.setenv("EVQL_PARTIAL_DEVICE_EMIT", "0")
    host, nrows, st, sizes = run_partial(wide, M.SCHEMA, kw)
    check_stats(st, len(exp), sizes, packed=False)
    assert nrows == len(host) == len(exp)
    assert host == exp


def test_the_cases_cover_the_borders():
    exp = expected("u64_null_max")
    null_key = hashlib.sha1(M.element(K.T_UINT64, None)).digest()
    max_key = hashlib.sha1(M.element(K.T_UINT64, M.M64)).digest()
    assert null_key in exp and max_key in exp
    # sums whose varuints are 1, 2, 5, 9 and 10 bytes long; negative int64 sums
    lens = {len(M.varuint(x)) for x in M.SUM_VALUES}
    assert lens == {1, 2, 5, 9, 10}
    c = M.wide_table()[1]
    assert int(c["b"][0::75_000].sum()) - 3000 < 0 < int(c["b"][1499::75_000].sum()) - 3000
    # groups without a non-NULL value
    assert not c["nb_present"][0] and c["nb_present"][1]
    # first-row strings of 10, 11, 12 and >= 128 bytes
    assert {10, 11, 12, 128, 130} <= {len(x) for x in c["s"][:131]}


# ---- 6. slices ---------------------------------------------------------------------------------
def test_slices_of_every_size(wide):
    kw = M.plan_kwargs(M.CASES["u64_string"])
    exp = expected("u64_string")
    q = wide.query(Plan(M.SCHEMA, mode=PARTIAL, **kw))
    try:
        for _ in range(2):  # execute twice on one query
            q.execute()
            keys, datas, total = [], [], 0
            for size in [1, 1, 1, 1000, 1000] + [1 << 20] * 2:
                n, raw = q.next_batch(size)
                assert n == min(size, len(exp) - total)
                assert len(raw[0]) == 25 * n
                keys.append(raw[0])
                datas.append(raw[1])
                total += n
            assert total == len(exp) and q.next_batch(1)[0] == 0
            st = q.emit_stats()
            assert st["device_packed"] == 1
            kraw, draw = b"".join(keys), b"".join(datas)
            assert len(kraw) == st["key_bytes"] and len(draw) == st["data_bytes"]
            got = dict(zip(unpack_svector(K.T_STRING, kraw), unpack_svector(K.T_STRING, draw)))
            assert got == exp
    finally:
        q.close()


def test_two_queries_drained_alternately(wide):
    names = ("u64", "string")
    qs = [wide.query(Plan(M.SCHEMA, mode=PARTIAL, **M.plan_kwargs(M.CASES[n]))) for n in names]
    try:
        for q in qs:
            q.execute()
        raws = [[[], []], [[], []]]
        live = [True, True]
        while any(live):
            for i, q in enumerate(qs):
                if not live[i]:
                    continue
                n, raw = q.next_batch(7001)
                live[i] = n > 0
                raws[i][0].append(raw[0])
                raws[i][1].append(raw[1])
        for i, name in enumerate(names):
            assert qs[i].emit_stats()["device_packed"] == 1
            got = dict(zip(unpack_svector(K.T_STRING, b"".join(raws[i][0])),
                           unpack_svector(K.T_STRING, b"".join(raws[i][1]))))
            assert got == expected(name)
    finally:
        for q in qs:
            q.close()


# ---- 7. fallbacks ------------------------------------------------------------------------------
FALLBACKS = {
    "count_distinct": dict(select=[col("k"), Agg("count_distinct", col("b")), count(1)],
                           group_by=[col("k")]),
    "exact_float_sum": dict(select=[col("k"), sum_(col("v"))], group_by=[col("k")],
                            float_sum_mode=K.FLOAT_SUM_EXACT, float_sum_bound=65536.0),
    "computed_key": dict(select=[Call("add", col("k"), lit(1)), count(1)],
                         group_by=[Call("add", col("k"), lit(1))]),
    "computed_second_key": dict(select=[col("k"), Call("add", col("b"), lit(1)), count(1)],
                                group_by=[col("k"), Call("add", col("b"), lit(1))]),
    # (an INT64 scan column does not exist: an int64 key is always computed)
    "int64_second_key": dict(select=[col("k"), Call("to_int64", col("b")), count(1)],
                             group_by=[col("k"), Call("to_int64", col("b"))]),
    "computed_select": dict(select=[col("k"), Call("add", col("b"), lit(1)), count(1)],
                            group_by=[col("k")]),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_keep_the_host_loop(wide, monkeypatch, name):
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    kw = FALLBACKS[name]
    exp = M.oracle_rows(O.oracle_run(M.wide_table()[0], Plan(M.SCHEMA, mode=PARTIAL, **kw)))
    assert len(exp) >= M.MIN_GROUPS
    got, nrows, st, sizes = run_partial(wide, M.SCHEMA, kw)
    check_stats(st, len(exp), sizes, packed=False)
    assert got == exp


def test_nested_scan_keeps_the_host_loop(ctx, monkeypatch):
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    img = NT.items_table(70_000)[0]
    kw = dict(select=[col("id"), count(1), sum_(col("items.price"))], group_by=[col("id")],
              scan_mode=K.SCAN_NESTED)
    exp = M.oracle_rows(O.oracle_run(img, Plan(NT.ITEMS_SCHEMA, mode=PARTIAL, **kw)))
    assert len(exp) == 70_000
    t = ctx.open_image(img)
    try:
        got, nrows, st, sizes = run_partial(t, NT.ITEMS_SCHEMA, kw)
    finally:
        t.close()
    check_stats(st, 70_000, sizes, packed=False)
    assert got == exp


# ---- 8. merged results -------------------------------------------------------------------------
def test_merged_result_is_packed_on_the_device(monkeypatch):
    """the hub exchange of two ranks: every rank ends with all groups in its merged table"""
    monkeypatch.delenv("EVQL_PARTIAL_DEVICE_EMIT", raising=False)
    parts = [M.key_table(70_001), M.key_table(M.MIN_GROUPS + 1)]
    w = E.Writer(M.KEY_COLUMNS)
    for name in ("k", "a"):
        w.put(name, np.concatenate([p[1][name] for p in parts]))
    w.commit(sum(p[2] for p in parts))
    whole = w.image()
    w.close()
    kw = dict(M.plan_kwargs(M.THRESHOLD_CASE), mode=PARTIAL)
    exp = M.oracle_rows(O.oracle_run(whole, Plan(M.KEY_SCHEMA, **kw)))
    assert len(exp) == 70_001
    hub = E.Hub(2)
    out, errs = [None, None], []

    def work(r):
        try:
            ctx = E.Context(0)
            t = ctx.open_image(parts[r][0])
            q = t.query(Plan(M.KEY_SCHEMA, **kw))
            x = E.Exchange.hub(ctx, hub, r)
            q.execute()
            q.exchange(x, K.EXCHANGE_GATHER_ALL)
            res = q.fetch_all()
            out[r] = (dict(res.rows()), res.nrows, q.emit_stats(), [len(b) for b in res.raw])
            q.close()
            x.close()
            t.close()
            ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            raise

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank hangs"
    assert not errs, errs
    hub.close()
    for got, nrows, st, sizes in out:
        check_stats(st, 70_001, sizes, packed=True)
        assert nrows == len(got) and got == exp


# ---- 9. the SHA-1 kernel on its own -------------------------------------------------------------
def test_sha1_ranges(ctx):
    rng = np.random.default_rng(11)
    chunks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in range(201)]
    chunks.append(rng.integers(0, 256, 100_000, dtype=np.uint8).tobytes())
    got = ctx.sha1_ranges(chunks)
    assert got == [hashlib.sha1(c).digest() for c in chunks]
    assert ctx.sha1_ranges([]) == []
    assert ctx.sha1_ranges([b"", b"abc", b""]) == [hashlib.sha1(x).digest() for x in (b"", b"abc", b"")]


def test_sha1_ranges_refuses_bad_offsets(ctx):
    L = E.lib()
    out = C.create_string_buffer(40)
    offs = (C.c_uint64 * 3)(0, 4, 2)
    assert L.evql_ctx_sha1_ranges(ctx.h, b"abcdef", 6, offs, 2, out) == K.EVQL_EARG
    offs = (C.c_uint64 * 3)(0, 4, 7)
    assert L.evql_ctx_sha1_ranges(ctx.h, b"abcdef", 6, offs, 2, out) == K.EVQL_EARG
    assert L.evql_ctx_sha1_ranges(ctx.h, b"abcdef", 6, None, 2, out) == K.EVQL_EARG
    assert L.evql_ctx_sha1_ranges(ctx.h, b"abcdef", 6, offs, 2, None) == K.EVQL_EARG
    offs = (C.c_uint64 * 3)(0, 4, 6)
    assert L.evql_ctx_sha1_ranges(ctx.h, b"abcdef", 6, offs, 2, out) == 0
    assert out.raw == hashlib.sha1(b"abcd").digest() + hashlib.sha1(b"ef").digest()


# ---- 10. the rows feed the merge ----------------------------------------------------------------
def test_device_packed_rows_merge_to_the_whole_table_group_by(wide):
    kw = M.plan_kwargs(M.CASES["min_max_mean"])
    whole = O.oracle_run(M.wide_table()[0], Plan(M.SCHEMA, **kw))
    m = E.Merge(Plan(M.SCHEMA, **kw))
    rows = M.wide_table()[2]
    for lo, hi in ((0, 150_000), (150_000, rows)):
        q = wide.query(Plan(M.SCHEMA, mode=PARTIAL, row_begin=lo, row_end=hi, **kw))
        try:
            q.execute()
            while True:
                n, raw = q.next_batch(1 << 16)
                if n == 0:
                    break
                m.add_rows(raw[0], raw[1], n)
            assert q.emit_stats()["device_packed"] == (1 if hi - lo >= M.MIN_GROUPS else 0)
        finally:
            q.close()
    got = m.fetch_all()
    m.close()
    assert got.nrows == whole.nrows
    assert sorted(got.rows(), key=lambda r: r[0]) == sorted(whole.rows(), key=lambda r: r[0])
