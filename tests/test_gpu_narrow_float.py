"""Required FLOAT_IEEE754 columns whose every value is exactly float32, kept once more as a
flat float32 array: every plan below runs over a table opened with
EVQL_NARROW_FLOAT=1 (every table tries) and is compared with the oracle and with the same
image opened with EVQL_NARROW_FLOAT=0 (the file's own 8-byte pages).  Widening float32 is
exact, so whatever does not depend on the order of a fast float sum is bit-identical."""
import contextlib
import os

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K, synth
from eventql_amd.plan import Plan, col, count, sum_, max_, min_
import oracle_lib as O
import tables as T
import narrow_float_model as M

pytestmark = pytest.mark.gpu

UINT = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
FLOAT = lambda name, **kw: dict(name=name, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754, **kw)
SCHEMA = dict(k=K.T_UINT64, a=K.T_UINT64, b=K.T_UINT64, v=K.T_FLOAT64, g=K.T_FLOAT64)
SPECS = [UINT("k"), UINT("a"), UINT("b"), FLOAT("v"), FLOAT("g")]
k, a, b, v, g = [col(x) for x in "kabvg"]

F32 = "evql_f32_x2"
PLAIN = "evql_plain64_x2"


@contextlib.contextmanager
def env(**kw):
    """the switches are read when a table becomes resident; None = unset"""
    old = {n: os.environ.get(n) for n in kw}
    for n, val in kw.items():
        if val is None:
            os.environ.pop(n, None)
        else:
            os.environ[n] = str(val)
    try:
        yield
    finally:
        for n, val in old.items():
            if val is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = val


def open_table(ctx, img, float_=1, plain=None):
    with env(EVQL_NARROW_FLOAT=float_, EVQL_NARROW_PLAIN=plain):
        return ctx.open_image(img)


def write(specs, cols, n):
    w = E.Writer(specs)
    for s in specs:
        w.put(s["name"], cols[s["name"]])
    w.commit(n)
    img = w.image()
    w.close()
    return img


def columns(n):
    c = synth.table_columns(n)
    c["g"] = (c["k"] % np.uint64(7)).astype(np.float64) * 0.5 - 1.0  # 7 distinct values, -0.0 none
    assert M.column_qualifies(c["v"]) and M.column_qualifies(c["g"])
    return c


def loads_of(src):
    """accessor name per scan column index, from the generated text"""
    out = {}
    for name in (F32, PLAIN, "evql_bitpacked_x2<8>", "evql_bitpacked_x2<16>", "evql_bitpacked_x2<32>",
                 "evql_soa_x2", "evql_plain32_x2"):
        at = 0
        while True:
            at = src.find(name + "(A.col[", at)
            if at < 0:
                break
            at += len(name) + 7
            out[int(src[at:src.index("]", at)])] = name
    return out


def bits_of(x):
    return repr(x) if not isinstance(x, float) else np.float64(x).tobytes().hex()


def run_both(ton, toff, img, schema, key_cols=1, fast=(), bare=False, **kw):
    """the plan on both tables against the oracle; columns not in `fast` (fast float sums,
    whose last bits depend on the order of addition) bit-identical on and off.  Returns the
    two kernel texts."""
    plan = Plan(schema, **kw)
    oplan = plan
    if kw.get("row_begin"):
        # (the oracle knows row_end and row filters only)
        okw = dict(kw)
        lo = okw.pop("row_begin")
        oplan = Plan(schema, row_filter=np.arange(ton.num_rows) >= lo, **okw)
    exp = O.oracle_run(img, oplan)
    out = []
    for t in (ton, toff):
        q = t.query(plan)
        try:
            src = q.kernel_source()
            got = q.run()
            assert [q.column_type(i) for i in range(q.column_count())] == list(exp.types)
            assert got.nrows == exp.nrows, (got.nrows, exp.nrows)
            if bare:
                assert got.raw == exp.raw
            else:
                T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=key_cols)
            assert q.stats()["rows_passed"] == exp.rows_passed
            out.append((got, src))
        finally:
            q.close()
    if bare:
        assert out[0][0].raw == out[1][0].raw
    else:
        cols = [i for i in range(len(exp.types)) if i not in fast]
        key = lambda rows: sorted(tuple(bits_of(r[i]) for i in cols) for r in rows)
        assert key(out[0][0].rows()) == key(out[1][0].rows())
    return out[0][1], out[1][1]


def third_filter(n):
    return np.arange(n) % 3 != 0


WHERE3 = (a > 30000) & (b < 30000)
# name -> (plan keywords, key columns, result columns that are fast float sums, bare scan?)
PLANS = {
    "config3": (dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=WHERE3,
                     groups_hint=1000), 1, (1,), False),
    "config3-exact": (dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=WHERE3,
                           groups_hint=1000, float_sum_mode=K.FLOAT_SUM_EXACT), 1, (), False),
    "config2": (dict(select=[k, sum_(v), count(1)], group_by=[k], groups_hint=1000), 1, (1,), False),
    "ungrouped": (dict(select=[min_(v), max_(v), sum_(v), count(1)]), 0, (2,), False),
    "ungrouped-exact": (dict(select=[min_(v), max_(v), sum_(v), count(1)],
                             float_sum_mode=K.FLOAT_SUM_EXACT), 0, (), False),
    "where-v": (dict(select=[k, count(1), sum_(a), max_(v)], group_by=[k], where=v > 8000.25,
                     groups_hint=1000), 1, (), False),
    "group-by-g": (dict(select=[g, count(1), sum_(a), min_(v)], group_by=[g], groups_hint=16),
                   1, (), False),
    "first-row": (dict(select=[k, v, g, count(1)], group_by=[k], groups_hint=1000), 1, (), False),
    "bare": (dict(scan_select=[v, v * 2.0], where=a > 30000), 0, (), True),
}
ROWS = [1, 127, 129, 8191, 8193, 131072 + 5, 3 * 131072 + 8191]


@pytest.fixture(scope="module")
def border_tables(ctx):
    """per row count: the table with the copies, the table without, the image"""
    made = {}
    for n in ROWS:
        img = write(SPECS, columns(n), n)
        made[n] = (open_table(ctx, img, 1, plain=1), open_table(ctx, img, 0, plain=1), img)
    yield made
    for ton, toff, _ in made.values():
        ton.close()
        toff.close()


def v_loads(src, kw):
    """accessors of the FLOAT columns v / g in the text of plan `kw`"""
    return sorted(set(name for name in loads_of(src).values() if name in (F32, PLAIN)))


@pytest.mark.parametrize("name", sorted(PLANS))
def test_border_row_counts(border_tables, name):
    kw, key_cols, fast, bare = PLANS[name]
    for n in ROWS:
        ton, toff, img = border_tables[n]
        son, soff = run_both(ton, toff, img, SCHEMA, key_cols=key_cols, fast=fast, bare=bare, **kw)
        # k, a, b come from their integer copies on both; the float columns switch accessor
        assert v_loads(son, kw) == [F32], (n, loads_of(son))
        assert v_loads(soff, kw) == [PLAIN], (n, loads_of(soff))
        assert F32 not in soff


@pytest.mark.parametrize("n", ROWS)
def test_row_ranges_and_row_filters(border_tables, n):
    ton, toff, img = border_tables[n]
    kw, key_cols, fast, _ = PLANS["config3"]
    # an odd first row and a short end; then a filter that drops every third row
    run_both(ton, toff, img, SCHEMA, key_cols=key_cols, fast=fast, row_begin=(n // 3) | 1,
             row_end=n - n // 5, **kw)
    run_both(ton, toff, img, SCHEMA, key_cols=key_cols, fast=fast, row_filter=third_filter(n), **kw)
    bkw = PLANS["bare"][0]
    run_both(ton, toff, img, SCHEMA, bare=True, row_begin=(n // 3) | 1, row_end=n - n // 5, **bkw)
    run_both(ton, toff, img, SCHEMA, bare=True, row_filter=third_filter(n), **bkw)


# ---- the value matrix -------------------------------------------------------------------------
NM = 131072 + 5
S1 = dict(k=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64)
SPECS1 = [UINT("k"), UINT("a"), FLOAT("v")]
MINMAX = dict(select=[min_(v), max_(v), count(1)])


@pytest.fixture(scope="module")
def base_columns():
    c = synth.table_columns(NM)
    return dict(k=c["k"], a=c["a"], v=c["v"])


def test_qualifying_edge_values_get_the_copy(ctx, base_columns):
    c = dict(base_columns)
    vals = np.array(list(M.QUALIFYING.values()), dtype=np.float64)
    vv = c["v"].copy()
    # the first rows, rows around the unit border of the copy, the last rows
    at = np.concatenate([np.arange(len(vals)), 131072 - 4 + np.arange(len(vals))])
    vv[at] = np.tile(vals, 2)
    vv[-1] = vals[1]  # -0.0 in the last row
    vv[-2] = vals[4]  # the quiet NaN
    assert M.column_qualifies(vv)
    c["v"] = vv
    img = write(SPECS1, c, NM)
    ton, toff = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        before = ton.device_bytes()
        son, soff = run_both(ton, toff, img, S1, key_cols=0, **MINMAX)
        assert F32 in son and F32 not in soff and PLAIN in soff
        assert ton.narrow_float_passes() == 1 and toff.narrow_float_passes() == 0
        assert ton.device_bytes() > before
        # every bit of every value, in row order
        son, _ = run_both(ton, toff, img, S1, bare=True, scan_select=[v, v * 2.0])
        assert F32 in son
        son, _ = run_both(ton, toff, img, S1, fast=(1,), select=[k, sum_(v), count(1), min_(v), max_(v)],
                          group_by=[k], groups_hint=1000)
        assert F32 in son
        run_both(ton, toff, img, S1, select=[k, count(1)], group_by=[k], where=v >= M.FLT_MAX,
                 groups_hint=1000)
        assert ton.narrow_float_passes() == 1
    finally:
        ton.close()
        toff.close()


@pytest.mark.parametrize("name", sorted(M.DISQUALIFYING))
def test_one_disqualifying_value_in_the_last_row_keeps_the_pages(ctx, base_columns, name):
    c = dict(base_columns)
    vv = c["v"].copy()
    vv[-1] = M.DISQUALIFYING[name]  # row 131072 + 4: behind a unit border of the copy
    mask = M.exact_f32_mask(vv)
    assert mask[:-1].all() and not mask[-1]
    c["v"] = vv
    img = write(SPECS1, c, NM)
    ton, toff = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        before = ton.device_bytes()
        son, soff = run_both(ton, toff, img, S1, key_cols=0, **MINMAX)
        assert F32 not in son and PLAIN in son and son == soff
        assert ton.device_bytes() == before
        assert ton.narrow_float_passes() == 1
        # a second operator: no second pass, nothing held
        son, _ = run_both(ton, toff, img, S1, bare=True, scan_select=[v, a], where=a > 65000)
        assert F32 not in son
        q = ton.query(Plan(S1, select=[k, max_(v), count(1)], group_by=[k], groups_hint=1000))
        assert F32 not in q.kernel_source()
        q.close()
        assert ton.narrow_float_passes() == 1
        assert ton.device_bytes() == before
    finally:
        ton.close()
        toff.close()


# ---- accounting ---------------------------------------------------------------------------------
def test_algorithmic_bytes_and_device_footprint(ctx):
    n = 262_144 + 77
    c = columns(n)
    img = write(SPECS[:4], c, n)
    ton, toff = open_table(ctx, img, 1, plain=1), open_table(ctx, img, 0, plain=1)
    try:
        base_on, base_off = ton.device_bytes(), toff.device_bytes()
        assert base_on == base_off
        qon, qoff = ton.query(B.config3()), toff.query(B.config3())
        qon.run()
        qoff.run()
        result = qon.stats()["num_groups"] * 8 * (1 + 3)
        copy = lambda bits: 4 + 16 * bits * ((n + 127) // 128)
        assert qoff.stats()["algorithmic_bytes"] == 3 * copy(16) + 8 * n + result
        assert qon.stats()["algorithmic_bytes"] == 3 * copy(16) + copy(32) + result
        # the footprint: the three integer copies on both, the float32 copy on one --
        # narrow_copy_bytes(n, 32), rounded up by the allocator to at most its 2 MiB granule
        units = (n + 131071) // 131072
        copy_bytes = units * 131072 * 4 + (1 << 20) + 256
        grown = (ton.device_bytes() - base_on) - (toff.device_bytes() - base_off)
        assert copy_bytes <= grown <= copy_bytes + (2 << 20), (grown, copy_bytes)
        # a second operator reuses the copy
        held = ton.device_bytes()
        q2 = ton.query(B.config2())
        assert F32 in q2.kernel_source()
        q2.run()
        assert ton.device_bytes() == held and ton.narrow_float_passes() == 1
        for q in (qon, qoff, q2):
            q.close()
    finally:
        ton.close()
        toff.close()


# ---- other paths --------------------------------------------------------------------------------
def lsm_file(rng, fi, n, vv, id_space):
    """one LSM file of a partition (lsm_tables._file_image's columns) with payload k, v"""
    import lsm_tables
    who = rng.integers(0, id_space, n)
    i = np.arange(n, dtype=np.uint64)
    c = dict(k=rng.integers(0, 97, n, dtype=np.uint64), v=vv,
             ids=[lsm_tables.lsm_id(int(w)) for w in who],
             upd=(rng.random(n) < 0.3).astype(np.uint64))
    bits = lambda name: dict(name=name, logical_type=K.COL_BOOLEAN, storage_type=K.ENC_BOOLEAN_BITPACKED)
    leb = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128)
    specs = [UINT("k"), FLOAT("v"), bits("__lsm_is_update"),
             dict(name="__lsm_id", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
             leb("__lsm_version"), leb("__lsm_sequence")]
    w = E.Writer(specs)
    w.put("k", c["k"])
    w.put("v", c["v"])
    w.put("__lsm_is_update", c["upd"])
    w.put("__lsm_id", c["ids"])
    w.put("__lsm_version", i + np.uint64(1))
    w.put("__lsm_sequence", i + np.uint64(fi * 1_000_000 + 1))
    w.commit(n)
    img = w.image()
    w.close()
    return img, c


def test_chain_in_which_one_file_does_not_qualify(ctx):
    """three LSM files behind one chain operator: v is float32-exact in the oldest and the
    newest, not in the middle one -- each file decides for itself"""
    rng = np.random.default_rng(11)
    S = dict(k=K.T_UINT64, v=K.T_FLOAT64)
    sizes = [40_001, 70_000, 33_333]
    total = sum(sizes)
    files = []
    for fi, n in enumerate(sizes):
        vv = rng.integers(0, 1 << 20, n).astype(np.float64) / 64.0
        if fi == 1:
            vv[n // 2] = 0.1
        assert M.column_qualifies(vv) == (fi != 1)
        img, c = lsm_file(rng, fi, n, vv, total // 2)
        files.append(("f%d" % fi, img, False, True, c))
    filters = O.oracle_partition_filters(files)  # scan order: newest first
    scan = list(reversed(files))
    imgs = [f[1] for f in scan]
    kw = dict(select=[col("k"), col("v"), count(1), max_(col("v")), sum_(col("v"))],
              group_by=[col("k")], where=col("v") > 100.5, groups_hint=1000,
              float_sum_mode=K.FLOAT_SUM_EXACT, float_sum_bound=16384.0)
    exp = O.oracle_run_chain(imgs, filters, Plan(S, **kw))
    results = {}
    for on in (1, 0):
        tabs = [open_table(ctx, img, on) for img in imgs]
        ch = E.LsmChain(ctx)
        for t, f in zip(tabs, scan):
            ch.add(t, has_skiplist=f[2], has_updates=f[3])
        ch.build()
        q = ch.query(Plan(S, **kw))
        try:
            got = q.run()
            assert got.nrows == exp.nrows
            T.compare_results(got.rows(), exp.rows(), exp.types)
            assert q.stats()["rows_passed"] == exp.rows_passed
            results[on] = got.rows()
        finally:
            q.close()
        per_table = [t.query(Plan(S, **kw)) for t in tabs]
        # how each part's kernel loads v (k stays on its 8-byte pages): newest file first
        acc = [F32 in pq.kernel_source() for pq in per_table]
        for pq in per_table:
            assert PLAIN in pq.kernel_source()
            pq.close()
        assert acc == ([True, False, True] if on else [False] * 3)
        assert [t.narrow_float_passes() for t in tabs] == ([1, 1, 1] if on else [0, 0, 0])
        ch.close()
        for t in tabs:
            t.close()
    key = lambda rows: sorted(tuple(bits_of(x) for x in r) for r in rows)
    assert key(results[1]) == key(results[0])


def test_partitioned_plan_reads_the_copy(ctx):
    """high cardinality: evql_part_count / evql_part_scatter load through the same accessor"""
    n = 300_000
    c = synth.table_columns(n)
    c["u"] = c["x"] % np.uint64(100_000)
    S = dict(u=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64)
    img = write([UINT("u"), UINT("a"), FLOAT("v")], c, n)
    ton, toff = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        u = col("u")
        son, soff = run_both(ton, toff, img, S, select=[u, sum_(a), count(1), sum_(v), max_(v)],
                             group_by=[u], groups_hint=100_000, float_sum_mode=K.FLOAT_SUM_EXACT)
        assert "evql_part_scatter" in son and "evql_part_scatter" in soff
        assert loads_of(son)[2] == F32 and loads_of(soff)[2] == PLAIN
    finally:
        ton.close()
        toff.close()


def test_nullable_float_column_is_never_copied(ctx):
    n = 50_000
    c = synth.table_columns(n)
    nulls = np.arange(n) % 5 == 0
    specs = [UINT("k"), FLOAT("nv", dlevel_max=1)]
    w = E.Writer(specs)
    w.put("k", c["k"])
    w.put("nv", c["v"], present=~nulls)
    w.commit(n)
    img = w.image()
    w.close()
    S = dict(k=K.T_UINT64, nv=K.T_FLOAT64)
    ton, toff = open_table(ctx, img, 1), open_table(ctx, img, 0)
    try:
        son, soff = run_both(ton, toff, img, S, select=[k, count(1), max_(col("nv"))], group_by=[k],
                             groups_hint=1000)
        assert F32 not in son and son == soff
        assert ton.narrow_float_passes() == 0
    finally:
        ton.close()
        toff.close()


def test_switches(ctx):
    n = 100_000
    c = synth.table_columns(n)
    img = write([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")], c, n)
    cases = [
        # unset: only tables of at least 2^26 rows try
        (dict(EVQL_NARROW_FLOAT=None, EVQL_NARROW_PLAIN=None), PLAIN),
        (dict(EVQL_NARROW_FLOAT=0, EVQL_NARROW_PLAIN=None), PLAIN),
        (dict(EVQL_NARROW_FLOAT=n + 1, EVQL_NARROW_PLAIN=None), PLAIN),
        (dict(EVQL_NARROW_FLOAT=n, EVQL_NARROW_PLAIN=None), F32),
        # "the file's own pages" turns the float copies off too ...
        (dict(EVQL_NARROW_FLOAT=1, EVQL_NARROW_PLAIN=0), PLAIN),
        # ... and a low integer threshold does not lower the float one
        (dict(EVQL_NARROW_FLOAT=None, EVQL_NARROW_PLAIN=1), PLAIN),
    ]
    for switches, want in cases:
        with env(**switches):
            t = ctx.open_image(img)
        q = t.query(B.config3())
        assert loads_of(q.kernel_source())[3] == want, (switches, loads_of(q.kernel_source()))
        assert t.narrow_float_passes() == (1 if want == F32 else 0)
        q.close()
        t.close()
