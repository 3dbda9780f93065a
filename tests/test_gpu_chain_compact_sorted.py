"""evql_lsm_chain_compact_sorted on the device: the rows of the plain compaction in ascending
order of one key column, ties in the plain order (a stable LSD radix sort between the gather
and the device writer).  Every image is compared byte for byte with
tests/compact_sorted_model.py -- numpy's stable argsort over compact_model's columns, written
by the host writer -- and the sort's own figures (presorted, passes, key_min / key_max, waits)
with what the keys imply."""
import functools

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_
import compact_model as M
import compact_sorted_model as SM
import lsm_nested_tables as LN
import lsm_tables
import oracle_lib as O
import tables as T
from test_gpu_chain_compact import (Chain, WAITS_FIXED, WAITS_WITH_STRINGS, hand_file,
                                    keep_pattern, model_counts, _rows)

pytestmark = pytest.mark.gpu

U, S = K.COL_UNSIGNED_INT, K.COL_STRING
ORDERS = [M.SCAN_ORDER, M.FILE_ORDER]
TILE = K.COMPACT_SORT_TILE
ZONE = 2048


@pytest.fixture(scope="module")
def chains(ctx):
    made = {}

    def get(kind, pname):
        if (kind, pname) not in made:
            files = lsm_tables.partition(pname) if kind == "flat" else LN.partition(pname)
            made[kind, pname] = Chain(ctx, files).build()
        return made[kind, pname]
    yield get
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def plain_columns(pname, order):
    """the plain compaction of a flat lsm_tables partition, computed once per order and shared
    by the keys (never changed: compact_sorted_model copies)"""
    return M.expected_columns(lsm_tables.partition(pname), M.flat_out_specs(), order)


def sorted_image(chain, specs, key, order, page_order=K.PAGE_ORDER_COLUMNS):
    t = chain.ch.compact_sorted(specs, key, row_order=order, page_order=page_order)
    try:
        return (t.download_image(), t.num_rows, dict(chain.ch.compact_stats),
                dict(chain.ch.compact_sort_stats))
    finally:
        t.close()


def plain_image(chain, specs, order):
    t = chain.ch.compact(specs, row_order=order)
    try:
        return t.download_image(), dict(chain.ch.compact_stats)
    finally:
        t.close()


def check_sort_stats(ss, keys, rows):
    presorted, passes, lo, hi = SM.expected_passes(keys)
    assert ss["rows"] == rows
    assert (ss["presorted"], ss["passes"]) == (presorted, passes), ss
    assert (ss["key_min"], ss["key_max"]) == (lo, hi), ss
    if presorted:
        assert ss["permute_ms"] == 0
    else:
        assert ss["sort_ms"] > 0 and ss["n_kernel_launches"] >= 1 + 3 * passes
    return presorted, passes


# ---------------------------------------------------------------------------------------
# every flat partition of the LSM tests
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["k", "a", "rid"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pname", sorted(lsm_tables.PARTITIONS))
def test_flat_partitions_are_byte_identical_to_the_model(chains, pname, order, key):
    c = chains("flat", pname)
    specs = M.flat_out_specs()
    plain, rows = plain_columns(pname, order)
    cols, _ = SM.sorted_columns(specs, plain, key)
    exp = SM.image_of(specs, cols, rows)
    dev, nrows, st, ss = sorted_image(c, specs, key, order)
    assert len(dev) == len(exp)
    assert dev == exp
    rows_in, kept = model_counts(c.files)
    assert (st["rows_in"], st["rows_written"], nrows, rows) == (rows_in, kept, kept, kept)
    assert st["n_host_waits"] == WAITS_WITH_STRINGS and ss["n_host_waits"] == 0
    presorted, passes = check_sort_stats(ss, SM.key_words(specs, plain, key), kept)
    if key == "a":
        assert passes == 2       # 16 bits
    if key == "k":
        assert passes == 1       # 40 values: ties everywhere
    if key == "rid":
        if order == M.FILE_ORDER:
            # already ascending: no pass, no permute, the plain compaction's bytes
            assert (presorted, passes, ss["permute_ms"]) == (1, 0, 0)
            assert dev == plain_image(c, specs, M.FILE_ORDER)[0]
        elif len(c.files) > 1:
            assert presorted == 0 and passes >= 1  # descending blocks: the full path


# ---------------------------------------------------------------------------------------
# hand-built files: one UINT64 key, one optional column, one string column
# ---------------------------------------------------------------------------------------
KEY_SPECS = [
    dict(name="t", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="o", logical_type=U, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
    dict(name="s", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
]
KEY_OUT = KEY_SPECS + M.lsm_columns()


def key_file(fi, keys, keep):
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    i = np.arange(n, dtype=np.uint64)
    pres = (i % np.uint64(3) != 1).astype(np.uint8)
    payload = dict(
        t=M._col(keys, U),
        o=M._col(i * np.uint64(31) + np.uint64(fi), U, present=pres, dlevel_max=1),
        s=M._col([b"" if r % 5 == 2 else b"f%d.%d" % (fi, r) for r in range(n)], S))
    return hand_file(fi, n, keep, KEY_SPECS, payload)


def key_files(keys):
    """`keys` are the keys of the KEPT rows in FILE order: the first third in an older file
    that keeps every row, the rest in a newer one that keeps every other row"""
    keys = np.asarray(keys, np.uint64)
    a = len(keys) // 3
    newer = np.zeros(2 * (len(keys) - a), np.uint64)
    newer[::2] = keys[a:]
    newer[1::2] = np.uint64(12345)  # (dropped rows)
    return [key_file(0, keys[:a], keep_pattern("all", a)),
            key_file(1, newer, keep_pattern("alternate", len(newer)))]


def check_key_chain(ctx, files, specs=KEY_OUT, key="t", orders=ORDERS, expect=None):
    """byte identity with the model in every order; returns the last order's sort stats"""
    c = Chain(ctx, files).build()
    try:
        filters = lsm_tables.model_filters(files)
        for order in orders:
            plain, rows = M.expected_columns(files, specs, order, filters)
            cols, _ = SM.sorted_columns(specs, plain, key)
            exp = SM.image_of(specs, cols, rows)
            dev, nrows, st, ss = sorted_image(c, specs, key, order)
            assert len(dev) == len(exp), order
            assert dev == exp, order
            assert (st["rows_in"], st["rows_written"]) == model_counts(files, filters)
            assert nrows == rows == st["rows_written"]
            presorted, passes = check_sort_stats(ss, SM.key_words(specs, plain, key), rows)
            if presorted:
                assert dev == plain_image(c, specs, order)[0]
            if expect is not None:
                expect(order, ss, dev, plain_image(c, specs, order)[0])
        return ss
    finally:
        c.close()


@pytest.mark.parametrize("kept", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_tile_borders(ctx, kept):
    rng = np.random.default_rng(kept)
    # 20 bits: 3 passes; many ties (kept rows > distinct values of the low digits)
    keys = rng.integers(0, 1 << 20, kept).astype(np.uint64)
    keys[::7] = keys[0]
    ss = check_key_chain(ctx, key_files(keys))
    assert ss["passes"] == 3 and ss["presorted"] == 0


def test_nothing_kept_and_one_row(ctx):
    files = [key_file(0, np.arange(70) * 3, keep_pattern("none", 70)),
             key_file(1, [5], keep_pattern("none", 1))]
    ss = check_key_chain(ctx, files)
    assert (ss["rows"], ss["presorted"], ss["passes"], ss["key_min"], ss["key_max"]) == (0, 1, 0, 0, 0)
    files = [key_file(0, (np.arange(70)[::-1] + 4) * 3, keep_pattern("last", 70)),
             key_file(1, [5], keep_pattern("none", 1))]
    ss = check_key_chain(ctx, files)
    assert (ss["rows"], ss["presorted"], ss["passes"], ss["key_min"], ss["key_max"]) == (1, 1, 0, 12, 12)


def test_all_keys_equal(ctx):
    def expect(order, ss, dev, plain):
        assert ss["passes"] == 0 and ss["presorted"] == 1  # no descent among equal keys
        assert dev == plain
    check_key_chain(ctx, key_files(np.full(TILE + 77, 2**40 + 9, np.uint64)), expect=expect)


def test_strictly_descending_keys(ctx):
    n = 2 * TILE + 300
    keys = (np.uint64(10**9) - np.arange(n, dtype=np.uint64) * np.uint64(7))
    ss = check_key_chain(ctx, key_files(keys), orders=[M.FILE_ORDER])
    assert ss["presorted"] == 0 and ss["passes"] == 2


def test_unsigned_order_over_the_whole_word(ctx):
    rng = np.random.default_rng(63)
    n = 4100
    near = np.uint64(2**63) + rng.integers(-50, 50, n).astype(np.int64).astype(np.uint64)
    keys = np.where(np.arange(n) % 3 == 0, np.uint64(2**64 - 1), near)
    keys[5] = 1
    ss = check_key_chain(ctx, key_files(keys))
    assert ss["passes"] == 8 and (ss["key_min"], ss["key_max"]) == (1, 2**64 - 1)


def test_a_narrow_range_at_a_large_base_takes_two_passes(ctx):
    rng = np.random.default_rng(51)
    n = 4100
    keys = np.uint64(2**51) + rng.integers(0, 1000, n).astype(np.uint64)
    keys[7], keys[8] = 2**51 + 999, 2**51
    ss = check_key_chain(ctx, key_files(keys))
    assert ss["passes"] == 2
    assert (ss["key_min"], ss["key_max"]) == (2**51, 2**51 + 999)


# ---------------------------------------------------------------------------------------
# waits
# ---------------------------------------------------------------------------------------
def test_the_key_statistics_ride_on_the_heap_size_wait(chains):
    c = chains("flat", "basic")
    with_s = M.flat_out_specs()
    without = [s for s in with_s if s["logical_type"] != S]
    for specs, own, plain_waits in ((with_s, 0, WAITS_WITH_STRINGS), (without, 1, WAITS_FIXED)):
        _, pst = plain_image(c, specs, M.SCAN_ORDER)
        dev, _, st, ss = sorted_image(c, specs, "a", M.SCAN_ORDER)
        assert ss["n_host_waits"] == own
        assert st["n_host_waits"] == pst["n_host_waits"] == plain_waits
        assert st["n_kernel_launches"] == pst["n_kernel_launches"]
        assert dev == SM.expected_image(c.files, specs, "a", M.SCAN_ORDER)


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_refusals(chains, ctx):
    c = chains("flat", "basic")
    specs = M.flat_out_specs()

    def refused(ch, specs, key, code, **kw):
        with pytest.raises(E.EvqlError) as ei:
            ch.compact_sorted(specs, key, **kw)
        assert ei.value.code == code, ei.value
        return ei.value.msg

    assert "optional" in refused(c.ch, specs, "n", K.EVQL_ENOTSUP)
    assert "float" in refused(c.ch, specs, "v", K.EVQL_ENOTSUP)
    assert "string" in refused(c.ch, specs, "s", K.EVQL_ENOTSUP)
    assert "boolean" in refused(c.ch, specs, "__lsm_is_update", K.EVQL_ENOTSUP)
    refused(c.ch, specs, None, K.EVQL_EARG)
    refused(c.ch, specs, "nowhere", K.EVQL_EARG)
    refused(c.ch, [s for s in specs if s["name"] != "k"], "k", K.EVQL_EARG)
    refused(c.ch, specs, "k", K.EVQL_EARG, row_order=7)
    refused(c.ch, specs, "k", K.EVQL_EARG, page_order=7)
    n = chains("nested", "basic")
    assert "items." in refused(n.ch, M.nested_out_specs(), "id", K.EVQL_ENOTSUP)
    refused(n.ch, M.nested_out_specs(), "items.price", K.EVQL_EARG)
    unbuilt = Chain(ctx, lsm_tables.partition("quiet"))
    try:
        assert "not built" in refused(unbuilt.ch, specs, "k", K.EVQL_EARG)
    finally:
        unbuilt.close()
    # the chain is unchanged and usable after the refusals
    dev, _, _, _ = sorted_image(c, specs, "k", M.SCAN_ORDER)
    assert dev == SM.expected_image(c.files, specs, "k", M.SCAN_ORDER)


# ---------------------------------------------------------------------------------------
# the plain call is untouched
# ---------------------------------------------------------------------------------------
def test_compact_after_compact_sorted(chains):
    c = chains("flat", "mixed")
    specs = M.flat_out_specs()
    sorted_image(c, specs, "a", M.SCAN_ORDER)
    for order in ORDERS:
        dev, st = plain_image(c, specs, order)
        assert dev == M.expected_image(c.files, specs, order)
        assert st["n_host_waits"] == WAITS_WITH_STRINGS
    nostr = [s for s in specs if s["logical_type"] != S]
    dev, st = plain_image(c, nostr, M.SCAN_ORDER)
    assert dev == M.expected_image(c.files, nostr, M.SCAN_ORDER)
    assert st["n_host_waits"] == WAITS_FIXED and st["string_bytes"] == 0


# ---------------------------------------------------------------------------------------
# the compacted table answers like the chain
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["basic", "mixed"])
def test_the_sorted_table_is_the_chain(chains, pname):
    c = chains("flat", pname)
    schema, specs = lsm_tables.LSM_SCHEMA, M.flat_out_specs()
    k, s, a, n = col("k"), col("s"), col("a"), col("n")
    plans = {
        "where": dict(select=[k, count(1), sum_(a), sum_(n)], group_by=[k], where=a >= 20000),
        "string-key": dict(select=[s, count(1), sum_(a)], group_by=[s]),
    }
    filters = O.oracle_partition_filters(c.files)
    t = c.ch.compact_sorted(specs, "a", row_order=M.SCAN_ORDER)
    try:
        for name, kw in plans.items():
            exp = M.oracle_chain(c.files, filters, schema, kw)
            for q in (c.ch.query(Plan(schema, **kw)), t.query(Plan(schema, **kw))):
                got = _rows(q)
                assert got.nrows == exp.nrows, name
                T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1, rel=1e-6)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------
# the payoff: zone maps prune the sorted table and cannot prune the file-order one
# ---------------------------------------------------------------------------------------
PAYOFF_SPECS = [
    dict(name="t", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="k", logical_type=U, storage_type=K.ENC_UINT64_LEB128),
    dict(name="a", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
]
PAYOFF_SCHEMA = dict(t=K.T_UINT64, k=K.T_UINT64, a=K.T_UINT64)


def test_zone_maps_prune_the_sorted_table(ctx):
    """three files whose t ranges interleave (file f holds t = 3 i + f) with the rows of a
    file in arrival order, not key order: every 2048-row zone of the file-order table spans
    the whole range (the chance that a zone of 2048 arrivals misses the top tenth is
    0.9^2048), the zones of the sorted table are narrow"""
    n = 40_000
    files = []
    for f in range(3):
        i = np.random.default_rng(400 + f).permutation(n).astype(np.uint64)
        payload = dict(t=M._col(np.uint64(3) * i + np.uint64(f), U),
                       k=M._col((i * np.uint64(7) + np.uint64(f)) % np.uint64(23), U),
                       a=M._col((i * np.uint64(2654435761)) % np.uint64(1000), U))
        files.append(hand_file(f, n, keep_pattern("all", n), PAYOFF_SPECS, payload))
    out_specs = PAYOFF_SPECS + M.lsm_columns()
    c = Chain(ctx, files).build()
    tabs = []
    try:
        plain, rows = M.expected_columns(files, out_specs, M.FILE_ORDER)
        tkeys = SM.key_words(out_specs, plain, "t")
        L = int(np.sort(tkeys)[int(0.9 * rows)])
        kw = dict(select=[col("k"), count(1), sum_(col("a"))], group_by=[col("k")],
                  where=col("t") >= L, groups_hint=100)
        exp = M.oracle_chain(files, O.oracle_partition_filters(files), PAYOFF_SCHEMA, kw)
        by_file = c.ch.compact(out_specs, row_order=M.FILE_ORDER)
        tabs.append(by_file)
        by_key = c.ch.compact_sorted(out_specs, "t", row_order=M.FILE_ORDER)
        tabs.append(by_key)
        ss = dict(c.ch.compact_sort_stats)
        assert (ss["presorted"], ss["passes"]) == (0, 3)  # 3 * 40,000 values: 17 bits
        assert by_key.download_image() == SM.expected_image(files, out_specs, "t", M.FILE_ORDER)
        stats = {}
        rows_of = {}
        for name, t in (("file", by_file), ("key", by_key)):
            q = t.query(Plan(PAYOFF_SCHEMA, **kw))
            got = q.run()
            stats[name] = q.zone_stats()
            q.close()
            assert got.nrows == exp.nrows
            T.compare_results(got.rows(), exp.rows(), exp.types, key_cols=1)
            rows_of[name] = sorted(got.rows())
        assert rows_of["file"] == rows_of["key"]
        # numpy's zones over the sorted keys
        srt = np.sort(tkeys)
        nz = -(-rows // ZONE)
        zmax = np.array([srt[z * ZONE:(z + 1) * ZONE].max() for z in range(nz)])
        excluded = int((zmax < np.uint64(L)).sum())
        assert excluded > 0
        assert stats["key"]["zones_excluded"] == excluded
        assert stats["key"]["tiles_skipped"] > 0
        assert stats["file"]["zones_excluded"] == 0 and stats["file"]["tiles_skipped"] == 0
        zmin, _ = by_key.zone_map("t")
        assert len(zmin) == nz and (zmin[1:] >= zmin[:-1]).all()
    finally:
        for t in tabs:
            t.close()
        c.close()
