"""Required UINT64_PLAIN columns kept once more as narrow bit-packed pages:
every plan below runs over a table opened with EVQL_NARROW_PLAIN=1 (every table narrows)
and is compared row for row with the oracle, and with the same table opened with
EVQL_NARROW_PLAIN=0 (the file's own 8-byte pages)."""
import contextlib
import os

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K, synth
from eventql_amd.plan import Plan, col, count, sum_, max_, min_
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

UINT = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
FLOAT = lambda name: dict(name=name, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)


@contextlib.contextmanager
def narrow_env(value):
    """the switch is read when a table becomes resident"""
    old = os.environ.get("EVQL_NARROW_PLAIN")
    os.environ["EVQL_NARROW_PLAIN"] = str(value)
    try:
        yield
    finally:
        if old is None:
            del os.environ["EVQL_NARROW_PLAIN"]
        else:
            os.environ["EVQL_NARROW_PLAIN"] = old


def open_table(ctx, img, narrow=1):
    with narrow_env(narrow):
        return ctx.open_image(img)


def write(specs, cols, n, chunk=None):
    w = E.Writer(specs)
    for lo in range(0, n, chunk or n):
        for s in specs:
            w.put(s["name"], cols[s["name"]][lo:lo + (chunk or n)])
    w.commit(n)
    img = w.image()
    w.close()
    return img


def accessors(q, i):
    """how the fused kernel loads scan column i"""
    src = q.kernel_source()
    for name in ("evql_plain64_x2", "evql_plain32_x2", "evql_bitpacked_x2<8>", "evql_bitpacked_x2<16>",
                 "evql_bitpacked_x2<32>", "evql_soa_x2"):
        if "%s(A.col[%d]." % (name, i) in src:
            return name
    raise AssertionError("no load of column %d" % i)


def check(tn, tp, img, schema, key_cols=1, **kw):
    """tn: the narrowing table, tp: the same image with the switch off"""
    plan = Plan(schema, **kw)
    oplan = plan
    if kw.get("row_begin"):
        # the oracle knows row_end and row filters only: the same rows as a filter that
        # drops everything in front of row_begin
        okw = dict(kw)
        lo = okw.pop("row_begin")
        oplan = Plan(schema, row_filter=np.arange(tn.num_rows) >= lo, **okw)
    exp = O.oracle_run(img, oplan)
    out = []
    for t in (tn, tp):
        q = t.query(plan)
        try:
            got = q.run()
            assert [q.column_type(i) for i in range(q.column_count())] == exp.types
            assert got.nrows == exp.nrows, (got.nrows, exp.nrows)
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=key_cols)
            assert q.stats()["rows_passed"] == exp.rows_passed
            out.append((got, q.kernel_source()))
        finally:
            q.close()
    # integer columns bit-identical either way
    ints = [i for i, ty in enumerate(exp.types) if ty != K.T_FLOAT64]
    rn = sorted(tuple(repr(r[i]) for i in ints) for r in out[0][0].rows())
    rp = sorted(tuple(repr(r[i]) for i in ints) for r in out[1][0].rows())
    assert rn == rp
    return out[0][1], out[1][1]


N = 400_000  # four 131,072-value pages of the copy, seven 65,536-value pages of the file


@pytest.fixture(scope="module")
def kabv(ctx):
    c = synth.table_columns(N)
    img = write([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")], c, N)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    yield tn, tp, img, c
    tn.close()
    tp.close()


def test_benchmark_shapes_and_the_switch(kabv):
    tn, tp, img, _ = kabv
    k, a, b, v = col("k"), col("a"), col("b"), col("v")
    shapes = (dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k],       # config 3
                   where=(a > 30000) & (b < 30000), groups_hint=1000),
              dict(select=[k, sum_(v), count(1)], group_by=[k], groups_hint=1000))  # config 2
    for kw in shapes:
        sn, sp = check(tn, tp, img, B.SCHEMA, **kw)
        # the switch: 0 = the file's pages (no packed accessor), on = 16-bit pages
        assert "evql_bitpacked_x2<" not in sp and "evql_plain64_x2(A.col[0]." in sp
        assert "evql_bitpacked_x2<16>(A.col[0]." in sn
    # k, a, b narrow; the float column v never does
    q = tn.query(B.config3())
    assert [accessors(q, i) for i in range(4)] == ["evql_bitpacked_x2<16>"] * 3 + ["evql_plain64_x2"]
    q.close()


@pytest.mark.parametrize("top,want", [(255, "evql_bitpacked_x2<8>"), (256, "evql_bitpacked_x2<16>"),
                                      (65535, "evql_bitpacked_x2<16>"), (65536, "evql_bitpacked_x2<32>"),
                                      ((1 << 32) - 1, "evql_bitpacked_x2<32>"),
                                      (1 << 32, "evql_plain64_x2")])
def test_maxima_straddling_each_width(ctx, top, want):
    """x holds its maximum `top` exactly once; y stays wide, z stays tiny: a mixed table"""
    n = 150_001
    rng = np.random.default_rng(top % 1000003)
    x = rng.integers(0, top, n, dtype=np.uint64)  # < top
    x[n - 7] = top
    c = dict(g=rng.integers(0, 41, n, dtype=np.uint64), x=x,
             y=rng.integers(0, 1 << 63, n, dtype=np.uint64), z=rng.integers(0, 3, n, dtype=np.uint64))
    S = dict(g=K.T_UINT64, x=K.T_UINT64, y=K.T_UINT64, z=K.T_UINT64)
    img = write([UINT("g"), UINT("x"), UINT("y"), UINT("z")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        g, xx, y, z = col("g"), col("x"), col("y"), col("z")
        check(tn, tp, img, S, select=[g, sum_(xx), max_(xx), min_(xx), count(1), sum_(y), sum_(z)],
              group_by=[g], where=xx > top // 3, groups_hint=64)
        check(tn, tp, img, S, key_cols=0, select=[max_(xx), sum_(xx), count(1)], where=xx >= top)
        q = tn.query(Plan(S, select=[g, sum_(xx), sum_(y), sum_(z)], group_by=[g], groups_hint=64))
        assert [accessors(q, i) for i in range(4)] == [
            "evql_bitpacked_x2<8>", want, "evql_plain64_x2", "evql_bitpacked_x2<8>"]
        q.close()
    finally:
        tn.close()
        tp.close()


def test_row_ranges_at_odd_offsets_and_page_borders(kabv):
    tn, tp, img, _ = kabv
    k, a, b, v = col("k"), col("a"), col("b"), col("v")
    kw = dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=(a > 30000) & (b < 30000),
              groups_hint=1000)
    for lo, hi in ((1, 131071), (131071, 131073), (131072, 262144), (65535, 196609), (3, N - 1),
                   (262143, 0), (393215, 393217), (N - 1, 0)):
        check(tn, tp, img, B.SCHEMA, row_begin=lo, row_end=hi, **kw)


def test_first_row_values_of_narrowed_columns(kabv):
    tn, tp, img, _ = kabv
    k, a, b, v = col("k"), col("a"), col("b"), col("v")
    # non-aggregate select expressions: gathered from the group's first row
    check(tn, tp, img, B.SCHEMA, select=[k, a, b, v, count(1)], group_by=[k], groups_hint=1000)
    check(tn, tp, img, B.SCHEMA, select=[k, a + b, count(1)], group_by=[k], where=a > 60000,
          row_begin=131071, groups_hint=1000)
    check(tn, tp, img, B.SCHEMA, key_cols=0, select=[a, b, count(1)], where=b > 65000)
    # many groups: the results are packed on the device, the gather runs there too
    check(tn, tp, img, B.SCHEMA, select=[a, k, b, count(1)], group_by=[a], groups_hint=70000)


def test_float_and_bool_views_of_a_narrowed_column(kabv):
    tn, tp, img, _ = kabv
    S = dict(k=K.T_UINT64, a=K.T_FLOAT64, b=K.T_BOOL, v=K.T_FLOAT64)
    k, a, b, v = col("k"), col("a"), col("b"), col("v")
    s1, _ = check(tn, tp, img, S, select=[k, sum_(a), count(1), sum_(v)], group_by=[k],
                  where=a > 30000.5, groups_hint=1000)
    assert "evql_bitpacked_x2<16>(A.col[" in s1
    check(tn, tp, img, S, key_cols=2, select=[k, b, count(1), max_(a)], group_by=[k, b],
          groups_hint=2000)


def test_interleaved_pages_and_the_device_writer(ctx):
    """the PLAIN pages of a column need not be contiguous in the file: the host writer fed
    in row chunks interleaves the columns' pages, so does the device writer in row order"""
    n = 300_000
    c = synth.table_columns(n)
    specs = [UINT("k"), UINT("a"), UINT("b"), FLOAT("v")]
    whole = write(specs, c, n)
    img = write(specs, c, n, chunk=50_000)
    assert len(img) == len(whole) and img != whole
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    k, a, b, v = col("k"), col("a"), col("b"), col("v")
    try:
        sn, _ = check(tn, tp, img, B.SCHEMA, select=[k, sum_(v), count(1), sum_(b)], group_by=[k],
                      where=(a > 30000) & (b < 30000), groups_hint=1000)
        assert "evql_bitpacked_x2<16>(A.col[0]." in sn
        check(tn, tp, img, B.SCHEMA, select=[k, sum_(a), max_(b)], group_by=[k], row_begin=65537,
              row_end=262145, groups_hint=1000)
    finally:
        tn.close()
        tp.close()
    import torch
    cols = {x: torch.from_numpy(c[x].view(np.int64)).cuda() for x in "kabv"}
    with narrow_env(1):
        td = ctx.table_from_device_columns(specs, {x: cols[x].data_ptr() for x in "kabv"}, None, n,
                                           page_order=K.PAGE_ORDER_ROWS)
    try:
        dimg = td.download_image()
        plan = B.config3()
        q = td.query(plan)
        assert "evql_bitpacked_x2<16>(A.col[0]." in q.kernel_source()
        exp = O.oracle_run(dimg, plan)
        T.compare_results(q.run().rows(), exp.rows(), exp.types)
        q.close()
    finally:
        td.close()


def test_partitioned_plan_over_narrowed_columns(ctx):
    """high cardinality: the partition kernels read the columns through the same accessors"""
    n = 600_000
    c = synth.table_columns(n)
    c["u"] = c["x"] % np.uint64(200_000)
    specs = [UINT("u"), UINT("a"), FLOAT("v")]
    img = write(specs, c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        u, a, v = col("u"), col("a"), col("v")
        sn, sp = check(tn, tp, img, B.SCHEMA, select=[u, sum_(a), count(1), sum_(v)], group_by=[u],
                       groups_hint=200_000)
        assert "evql_part_scatter" in sn and "evql_part_scatter" in sp
        assert "evql_bitpacked_x2<32>(A.col[0]." in sn and "evql_bitpacked_x2<16>(A.col[1]." in sn
        assert "evql_bitpacked_x2<" not in sp
    finally:
        tn.close()
        tp.close()


def lsm_file(rng, fi, n, has_skiplist, id_space, k_top, a_top, rid_base):
    """one LSM file of a partition (lsm_tables._file_image's columns) whose payload integer
    columns rid, k, a are UINT64_PLAIN with maxima chosen per file"""
    import lsm_tables
    who = rng.integers(0, id_space, n)
    i = np.arange(n, dtype=np.uint64)
    c = dict(rid=np.uint64(rid_base) + i, k=rng.integers(0, 97, n, dtype=np.uint64),
             a=rng.integers(0, a_top, n, dtype=np.uint64),
             v=rng.integers(0, 1 << 20, n).astype(np.float64) / 64.0,
             ids=[lsm_tables.lsm_id(int(w)) for w in who],
             upd=(rng.random(n) < 0.3).astype(np.uint64), skip=(rng.random(n) < 0.1).astype(np.uint64))
    c["k"][1] = k_top  # one row of a group of its own sets the width
    c["a"][2] = a_top - 1
    bits = lambda name: dict(name=name, logical_type=K.COL_BOOLEAN, storage_type=K.ENC_BOOLEAN_BITPACKED)
    leb = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128)
    specs = [UINT("rid"), UINT("k"), UINT("a"), FLOAT("v"), bits("__lsm_is_update")]
    if has_skiplist:
        specs.append(bits("__lsm_skip"))
    specs += [dict(name="__lsm_id", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
              leb("__lsm_version"), leb("__lsm_sequence")]
    w = E.Writer(specs)
    for name in ("rid", "k", "a", "v"):
        w.put(name, c[name])
    w.put("__lsm_is_update", c["upd"])
    if has_skiplist:
        w.put("__lsm_skip", c["skip"])
    w.put("__lsm_id", c["ids"])
    w.put("__lsm_version", i + np.uint64(1))
    w.put("__lsm_sequence", i + np.uint64(fi * 1_000_000 + 1))
    w.commit(n)
    img = w.image()
    w.close()
    return img, c


def test_chain_of_files_that_narrow_to_different_widths(ctx):
    """a partition of three LSM files behind one chain operator (PartitionCursor): k fits 8
    bits in the oldest file, 16 in the middle one, 32 in the newest; a 16 / 32 / not at all;
    rid 32 / 32 / not at all.  Row filters, the merge across the parts and the first-row
    gather (rid, a non-aggregate select column) run over differently packed parts."""
    rng = np.random.default_rng(5)
    S = dict(rid=K.T_UINT64, k=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64)
    # oldest first: (rows, has_skiplist, has_updates, max k, bound of a, first rid)
    shape = [(70_001, 0, 1, 200, 60_000, 0), (140_000, 1, 1, 50_000, 1 << 20, 10_000_000),
             (33_333, 0, 1, 1 << 20, 1 << 40, 1 << 33)]
    total = sum(f[0] for f in shape)
    files = []
    for fi, (n, skl, upd, kt, at, rb) in enumerate(shape):
        img, c = lsm_file(rng, fi, n, bool(skl), total // 2, kt, at, rb)
        files.append(("f%d" % fi, img, bool(skl), bool(upd), c))
    filters = O.oracle_partition_filters(files)          # scan order: newest first
    scan = list(reversed(files))
    imgs = [f[1] for f in scan]
    assert any(f is not None and not f.all() for f in filters)
    rid, k, a, v = col("rid"), col("k"), col("a"), col("v")
    kw = dict(select=[k, rid, count(1), sum_(a), max_(a), sum_(v)], group_by=[k], where=a > 1000,
              groups_hint=1000)
    exp = O.oracle_run_chain(imgs, filters, Plan(S, **kw))
    results = {}
    for narrow in (1, 0):
        tabs = [open_table(ctx, img, narrow) for img in imgs]
        ch = E.LsmChain(ctx)
        for t, f in zip(tabs, scan):
            ch.add(t, has_skiplist=f[2], has_updates=f[3])
        ch.build()
        for i, e in enumerate(filters):
            got_f, _ = ch.filter(i)
            assert (got_f is None) == (e is None) and (e is None or (got_f == e).all())
        q = ch.query(Plan(S, **kw))
        try:
            got = q.run()
            assert got.nrows == exp.nrows
            T.compare_results(got.rows(), exp.rows(), exp.types)
            st = q.stats()
            assert st["rows_scanned"] == total and st["rows_passed"] == exp.rows_passed
            results[narrow] = (got.rows(), st)
        finally:
            q.close()
        # how each part's kernel loads a (WHERE first), k, rid: newest file first
        per_table = [t.query(Plan(S, **kw)) for t in tabs]
        acc = [[accessors(pq, i) for i in range(3)] for pq in per_table]
        for pq in per_table:
            pq.close()
        if narrow:
            assert acc == [["evql_plain64_x2", "evql_bitpacked_x2<32>", "evql_plain64_x2"],
                           ["evql_bitpacked_x2<32>", "evql_bitpacked_x2<16>", "evql_bitpacked_x2<32>"],
                           ["evql_bitpacked_x2<16>", "evql_bitpacked_x2<8>", "evql_bitpacked_x2<32>"]]
        else:
            assert acc == [["evql_plain64_x2"] * 3] * 3
        ch.close()
        for t in tabs:
            t.close()
    # integer columns (first-row rid included) identical with and without the copies
    strip = lambda rows: sorted(r[:5] for r in rows)
    assert strip(results[1][0]) == strip(results[0][0])
    # algorithmic bytes of the chain: per part and column min(file payload, streamed copy)
    copy = lambda n, bits: 4 + 16 * bits * ((n + 127) // 128)
    result = exp.nrows * 8 * (1 + 4)
    n2, n1, n0 = (f[0] for f in reversed(shape))
    want = (8 * n2 + copy(n2, 32) + 8 * n2 + 8 * n2            # newest: a plain, k 32, rid plain
            + copy(n1, 32) + copy(n1, 16) + copy(n1, 32) + 8 * n1
            + copy(n0, 16) + copy(n0, 8) + copy(n0, 32) + 8 * n0 + result)
    assert results[1][1]["algorithmic_bytes"] == want
    assert results[0][1]["algorithmic_bytes"] == 4 * 8 * total + result


def test_algorithmic_bytes_and_device_footprint(ctx):
    n = 262_144 + 77
    c = synth.table_columns(n)
    img = write([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")], c, n)
    tn, tp = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        base_n, base_p = tn.device_bytes(), tp.device_bytes()
        assert base_n == base_p >= len(img)
        qn, qp = tn.query(B.config3()), tp.query(B.config3())
        qn.run()
        qp.run()
        groups = qn.stats()["num_groups"]
        result = groups * 8 * (1 + 3)
        # per column min(file payload, bytes of the copy the kernel streams)
        copy16 = 4 + 16 * 16 * ((n + 127) // 128)
        assert qp.stats()["algorithmic_bytes"] == 4 * 8 * n + result
        assert qn.stats()["algorithmic_bytes"] == 3 * min(8 * n, copy16) + 8 * n + result
        # the footprint grows by the three copies (pages + 1 MiB slack + page table each)
        assert tp.device_bytes() == base_p
        grown = tn.device_bytes() - base_n
        pages = (n + 131071) // 131072
        assert grown >= 3 * (4 + pages * 16 * 16 * 1024 + (1 << 20))
        # (two allocations per copy -- pages and page table -- each rounded up by the
        # allocator to at most its 2 MiB granule)
        assert grown <= 3 * (4 + pages * 16 * 16 * 1024 + (1 << 20) + 2 * (2 << 20))
        # a second operator reuses the copies
        q2 = tn.query(B.config2())
        q2.run()
        assert tn.device_bytes() - base_n == grown
        for q in (qn, qp, q2):
            q.close()
    finally:
        tn.close()
        tp.close()


def test_default_threshold_leaves_small_tables_alone(ctx):
    """without the variable only tables of at least 2^26 rows narrow"""
    old = os.environ.pop("EVQL_NARROW_PLAIN", None)
    try:
        c = synth.table_columns(100_000)
        t = ctx.open_image(write([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")], c, 100_000))
        q = t.query(B.config3())
        assert "evql_bitpacked_x2<" not in q.kernel_source()
        q.close()
        t.close()
    finally:
        if old is not None:
            os.environ["EVQL_NARROW_PLAIN"] = old
