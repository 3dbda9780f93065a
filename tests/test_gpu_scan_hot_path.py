"""The per-row work of the fused scan after its loads: the row-window test in
32 bits, the one-entry accumulator cache of a lane, and the identity slots of a step's two rows
read ahead of their updates.  Config 3's query over 3 tiles + 5 rows against the oracle, over
the narrow float32 shape (EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1: small tables keep the
copies) and over the file's plain pages, with key layouts chosen for the cache's cases and the
probe, and row windows chosen for the tile borders in every tile loop that tests them."""
import contextlib
import os
import re

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K, synth
from eventql_amd.plan import Plan, col, count, max_, sum_
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

TILE = 8192  # config 3's tile
N = 3 * TILE + 5
UINT = lambda name, **kw: dict(name=name, logical_type=K.COL_UNSIGNED_INT,
                               storage_type=K.ENC_UINT64_PLAIN, **kw)
FLOAT = lambda name: dict(name=name, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)
SCHEMA = dict(B.SCHEMA)
k, a, b, v, u = [col(x) for x in "kabvu"]
WHERE3 = (a > 30000) & (b < 30000)
EMPTY = (1 << 64) - 1  # EVQL_EMPTY: a free slot's word, and a legal key


@contextlib.contextmanager
def env(**kw):
    """the switches are read when a table becomes resident"""
    old = {n: os.environ.get(n) for n in kw}
    os.environ.update({n: str(val) for n, val in kw.items()})
    try:
        yield
    finally:
        for n, val in old.items():
            if val is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = val


@pytest.fixture(scope="module")
def base_columns():
    c = synth.table_columns(N)
    row = np.arange(N, dtype=np.uint64)
    return dict(a=c["a"], b=c["b"], v=c["v"], u=(row * np.uint64(2654435761)) % np.uint64(100003))


def image(cols, key, present=None):
    w = E.Writer([UINT("k", dlevel_max=0 if present is None else 1), UINT("a"), UINT("b"), FLOAT("v"),
                  UINT("u")])
    w.put("k", key, present=present)
    for name in "abvu":
        w.put(name, cols[name])
    w.commit(N)
    img = w.image()
    w.close()
    return img


def open_table(ctx, img, narrow):
    with env(EVQL_NARROW_PLAIN=1 if narrow else 0, EVQL_NARROW_FLOAT=1 if narrow else 0):
        return ctx.open_image(img)


def bits(x):
    return np.float64(x).tobytes().hex() if isinstance(x, float) else repr(x)


def check(t, img, exact, bare=False, key_cols=1, window=None, **kw):
    """the plan on `t` against the oracle: exact float sums bit for bit, fast ones within the
    parity tests' 1e-6, everything else equal.  Returns the kernel text."""
    fs = dict(float_sum_mode=K.FLOAT_SUM_EXACT) if exact else {}
    if window is None:
        plan = oplan = Plan(SCHEMA, **fs, **kw)
    else:
        # (the oracle knows row filters, not windows)
        lo, hi = window
        idx = np.arange(N)
        plan = Plan(SCHEMA, row_begin=lo, row_end=hi, **fs, **kw)
        oplan = Plan(SCHEMA, row_filter=(idx >= lo) & (idx < hi), **fs, **kw)
    exp = O.oracle_run(img, oplan)
    q = t.query(plan)
    try:
        src = q.kernel_source()
        got = q.run()
        assert [q.column_type(i) for i in range(q.column_count())] == list(exp.types)
        assert got.nrows == exp.nrows, (got.nrows, exp.nrows)
        if bare:
            assert got.raw == exp.raw
        elif exact:
            key = lambda rows: sorted(tuple(bits(x) for x in r) for r in rows)
            assert key(got.rows()) == key(exp.rows())
        else:
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=key_cols)
        assert q.stats()["rows_passed"] == exp.rows_passed
        return src
    finally:
        q.close()


CONFIG3 = dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=WHERE3, groups_hint=1000)
ROW = np.arange(N, dtype=np.uint64)
# the one-entry cache: always the same slot; never the same slot twice; a lane's row pair on one
# slot; two slots in turn; long runs
KEYS = {
    "one-key": np.full(N, 7, np.uint64),
    "row-mod-1000": ROW % np.uint64(1000),
    "pairs-mod-7": (ROW // np.uint64(2)) % np.uint64(7),
    "row-mod-2": ROW % np.uint64(2),
    "runs-of-4096": (ROW // np.uint64(4096)) % np.uint64(3),
}


def narrow_shape(src):
    return "evql_f32_x2(" in src and "evql_bitpacked_x2<16>(" in src and "evql_plain64_x2(" not in src


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("layout", sorted(KEYS))
def test_key_layouts(ctx, base_columns, layout, exact):
    img = image(base_columns, KEYS[layout])
    t = open_table(ctx, img, True)
    try:
        src = check(t, img, exact, **CONFIG3)
        assert narrow_shape(src) and "#define EVQL_LCACHE 1\n" in src
    finally:
        t.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_plain_pages(ctx, base_columns, exact):
    img = image(base_columns, KEYS["row-mod-1000"])
    t = open_table(ctx, img, False)
    try:
        src = check(t, img, exact, **CONFIG3)
        assert "evql_plain64_x2(" in src and "evql_f32_x2(" not in src
    finally:
        t.close()


def lds_slots(ctx, base_columns, narrow):
    """slots of config 3's LDS table in the compiled shape"""
    img = image(base_columns, KEYS["one-key"])
    t = open_table(ctx, img, narrow)
    q = t.query(Plan(SCHEMA, **CONFIG3))
    try:
        return int(re.search(r"#define EVQL_LDS_SLOTS (\d+)", q.kernel_source()).group(1))
    finally:
        q.close()
        t.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_three_keys_share_an_identity_slot(ctx, base_columns, exact):
    """5, 5 + S and 5 + 2S have the identity slot 5: two of them live on the hashed chain, and
    the word read ahead for a row may belong to either neighbour (S = 4096 keeps the keys
    inside the 16-bit copy)"""
    S = lds_slots(ctx, base_columns, True)
    assert S & (S - 1) == 0 and 5 + 2 * S < 65536
    key = np.uint64(5) + (ROW % np.uint64(3)) * np.uint64(S)
    img = image(base_columns, key)
    t = open_table(ctx, img, True)
    try:
        assert narrow_shape(check(t, img, exact, **CONFIG3))
    finally:
        t.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_the_empty_word_as_a_key(ctx, base_columns, exact):
    """2^64 - 1 next to small keys: a group of its own outside the probed slots (plain pages: the
    value does not fit a copy)"""
    key = np.where(ROW % np.uint64(5) == 0, np.uint64(EMPTY), ROW % np.uint64(11))
    img = image(base_columns, key)
    t = open_table(ctx, img, False)
    try:
        src = check(t, img, exact, **CONFIG3)
        assert "evql_plain64_x2(" in src
    finally:
        t.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_nullable_key(ctx, base_columns, exact):
    present = (ROW % np.uint64(4) != 1).astype(np.uint8)
    img = image(base_columns, ROW % np.uint64(13), present=present)
    t = open_table(ctx, img, True)
    try:
        check(t, img, exact, **CONFIG3)
    finally:
        t.close()


# ---- row windows: every tile loop that tests them ------------------------------------------------
WINDOWS = [(0, 1), (8191, 8193), (8192, 16384), (1, 8191), (8200, 8200), (5, N + 100_000),
           (16383, N)]
LOOPS = {
    "grouped": (CONFIG3, 1, False, "evql_scan_agg"),
    "ungrouped": (dict(select=[count(1), sum_(v), sum_(b), max_(k)], where=WHERE3), 0, False,
                  "evql_scan_agg"),
    "bare": (dict(scan_select=[k, b + 1, v * 2.0], where=a > 30000), 0, True, "evql_scan_emit"),
    "partitioned": (dict(select=[u, sum_(a), count(1), sum_(v)], group_by=[u], groups_hint=200_000),
                    1, False, "evql_part_scatter"),
}


@pytest.fixture(scope="module")
def window_table(ctx, base_columns):
    img = image(base_columns, KEYS["row-mod-1000"])
    t = open_table(ctx, img, True)
    yield t, img
    t.close()


@pytest.mark.parametrize("loop", sorted(LOOPS))
def test_row_windows(window_table, loop):
    t, img = window_table
    kw, key_cols, bare, kernel = LOOPS[loop]
    for window in WINDOWS:
        # (exact sums where the reduction order is the only freedom; config 4's query as it is)
        src = check(t, img, exact=loop in ("grouped", "ungrouped"), bare=bare, key_cols=key_cols,
                    window=window, **kw)
        assert kernel + "(" in src, (loop, window)


def test_row_windows_over_plain_pages(ctx, base_columns):
    img = image(base_columns, KEYS["row-mod-1000"])
    t = open_table(ctx, img, False)
    try:
        for window in WINDOWS:
            check(t, img, exact=True, window=window, **CONFIG3)
    finally:
        t.close()
