"""evql_lsm_chain_compact on the device: the rows a partition's filters keep, gathered in
HBM and written as one cstable.  Every image is compared byte for byte with
tests/compact_model.expected_image (the model is pinned on the oracle's PartitionCursor in
test_chain_compact_cpu.py); the row-wise page placement with the reference's own
CSTableWriter; and the compacted table must answer queries as the chain does."""
import struct

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_, max_, count_distinct, out
import compact_model as M
import float_edges as FE
import lsm_nested_tables as LN
import lsm_tables
from lsm_tables import lsm_id
import oracle_lib as O
import tables as T

pytestmark = pytest.mark.gpu

U, B, S, F = K.COL_UNSIGNED_INT, K.COL_BOOLEAN, K.COL_STRING, K.COL_FLOAT
ORDERS = [M.SCAN_ORDER, M.FILE_ORDER]
# one wait for the sizes, one more when a STRING column is written
WAITS_FIXED, WAITS_WITH_STRINGS = 1, 2


class Chain:
    """a partition's files (oldest first) resident and chained, newest first"""

    def __init__(self, ctx, files, arena_skips=None):
        self.files = files
        self.tabs = [ctx.open_image(f[1]) for f in reversed(files)]
        self.ch = E.LsmChain(ctx)
        for i, (t, f) in enumerate(zip(self.tabs, reversed(files))):
            sk = None if arena_skips is None else arena_skips.get(len(files) - 1 - i)
            if sk is not None:
                self.ch.add(t, arena_skiplist=sk)
            else:
                self.ch.add(t, has_skiplist=f[2], has_updates=f[3])

    def build(self):
        self.ch.build()
        return self

    def close(self):
        self.ch.close()
        for t in self.tabs:
            t.close()


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


def compacted_image(chain, specs, order, page_order=K.PAGE_ORDER_COLUMNS):
    t = chain.ch.compact(specs, row_order=order, page_order=page_order)
    try:
        return t.download_image(), t.num_rows, dict(chain.ch.compact_stats)
    finally:
        t.close()


def model_counts(files, filters=None):
    filters = lsm_tables.model_filters(files) if filters is None else filters
    rows_in = sum(len(f[4]["ids"]) for f in files)
    kept = sum(len(f[4]["ids"]) if x is None else int(np.asarray(x).sum())
               for f, x in zip(reversed(files), filters))
    return rows_in, kept


# ---------------------------------------------------------------------------------------
# byte identity over the partitions of the LSM tests
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pname", sorted(lsm_tables.PARTITIONS))
def test_flat_partitions_are_byte_identical_to_the_model(chains, pname, order):
    c = chains("flat", pname)
    specs = M.flat_out_specs()
    dev, nrows, st = compacted_image(c, specs, order)
    exp = M.expected_image(c.files, specs, order)
    assert len(dev) == len(exp)
    assert dev == exp
    rows_in, kept = model_counts(c.files)
    assert (st["rows_in"], st["rows_written"], nrows) == (rows_in, kept, kept)
    assert st["n_tables"] == len(c.files)
    assert st["n_host_waits"] == WAITS_WITH_STRINGS
    assert st["string_bytes"] == 20 * kept + sum(
        len(x) for x in M.expected_columns(c.files, specs, order)[0][5]["values"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pname", sorted(LN.PARTITIONS))
def test_nested_partitions_are_byte_identical_to_the_model(chains, pname, order):
    c = chains("nested", pname)
    specs = M.nested_out_specs()
    dev, nrows, st = compacted_image(c, specs, order)
    exp = M.expected_image(c.files, specs, order)
    assert len(dev) == len(exp)
    assert dev == exp
    rows_in, kept = model_counts(c.files)
    assert (st["rows_in"], st["rows_written"], nrows) == (rows_in, kept, kept)
    assert st["n_host_waits"] == WAITS_WITH_STRINGS


def test_a_table_without_strings_takes_one_host_wait(chains):
    c = chains("flat", "basic")
    specs = [s for s in M.flat_out_specs() if s["logical_type"] != S]
    dev, _, st = compacted_image(c, specs, M.SCAN_ORDER)
    assert dev == M.expected_image(c.files, specs, M.SCAN_ORDER)
    assert st["n_host_waits"] == WAITS_FIXED and st["string_bytes"] == 0


# ---------------------------------------------------------------------------------------
# EVQL_PAGE_ORDER_ROWS against the reference's CSTableWriter
# ---------------------------------------------------------------------------------------
@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's cstable library) not built")
@pytest.mark.parametrize("kind,pname", [("flat", "basic"), ("nested", "edges")])
def test_row_order_is_byte_identical_to_the_reference_writer(chains, kind, pname, tmp_path):
    """the reference writer of the test suite appends integer and float columns record by
    record (oracle_lib.ref_write_table_by_records takes no strings), so the output keeps the
    non-string columns; TableSchema carries no bit-pack maximum, so bit-packed output columns
    use the reference's defaults"""
    from test_gpu_writer import _ref_schema, _in_reference_header_order
    c = chains(kind, pname)
    declared = []
    for s in (M.flat_out_specs() if kind == "flat" else M.nested_out_specs()):
        if s["logical_type"] == S:
            continue
        s = dict(s)
        s.pop("bitpack_max_value", None)
        if s.get("rlevel_max", 0):
            s["optional"] = 1  # REPEATED RECORD items { OPTIONAL leaf }: dlevel_max 2
        declared.append(s)
    specs = _in_reference_header_order(declared, tmp_path)
    dev, nrows, _ = compacted_image(c, specs, M.SCAN_ORDER, K.PAGE_ORDER_ROWS)
    cols, rows = M.expected_columns(c.files, specs, M.SCAN_ORDER)
    assert rows == nrows
    rcols = []
    for s, x in zip(specs, cols):
        kind_ = "float" if s["logical_type"] == F else "uint"
        rcols.append((s["name"], kind_, x["values"], x["rl"], x["dl"], x["present"]))
    path = str(tmp_path / "ref.cst")
    O.ref_write_table_by_records(path, _ref_schema(declared), rcols, rows)
    ref = open(path, "rb").read()
    assert len(dev) == len(ref)
    assert dev == ref


# ---------------------------------------------------------------------------------------
# hand-built chains: tile borders, keep patterns, NULL runs, float edges
# ---------------------------------------------------------------------------------------
FLOAT_EDGES = [0.0, -0.0, FE.TINY, -FE.TINY, FE.SUBMAX, FE.DMAX, -FE.DMAX, FE.INF, -FE.INF,
               FE.NAN, FE.NAN_ONES, FE.from_bits(0x7ff0000000000123),
               FE.from_bits(0xfff8dead0000beef), 1.5]
EDGE_BITS = np.array([FE.bits(x) for x in FLOAT_EDGES], np.uint64)


def keep_pattern(name, n):
    k = np.zeros(n, bool)
    if name == "all":
        k[:] = True
    elif name == "first":
        k[0] = True
    elif name == "last":
        k[-1] = True
    elif name == "alternate":
        k[::2] = True
    else:
        assert name == "none"
    return k


EDGE_SPECS = [
    dict(name="x", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="f", logical_type=F, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="o", logical_type=U, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
    dict(name="s", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
    dict(name="os", logical_type=S, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1),
]


def _lsm_specs(has_skiplist=True):
    specs = [dict(name="__lsm_is_update", logical_type=B, storage_type=K.ENC_BOOLEAN_BITPACKED)]
    if has_skiplist:
        specs.append(dict(name="__lsm_skip", logical_type=B, storage_type=K.ENC_BOOLEAN_BITPACKED))
    return specs + M.lsm_columns(("__lsm_id", "__lsm_version", "__lsm_sequence"))


def hand_file(fi, n, keep, payload_specs=None, payload=None, with_skip_column=True):
    """a file of n rows with unique ids, so that its filter is exactly `keep` (through the
    skiplist); `payload`: name -> M._col(...) replaces the default payload columns"""
    i = np.arange(n, dtype=np.uint64)
    ids = [lsm_id(fi * 10_000_000 + int(r)) for r in i]
    upd = (i % np.uint64(3) == 0).astype(np.uint64)  # set bits that shadow nothing
    skip = (~keep).astype(np.uint64)
    if payload is None:
        payload_specs = EDGE_SPECS
        # NULLs in a run across the border of a 2048-row tile, and every 5th row
        pres = ((i % np.uint64(5) != 0) & ~((i >= 2040) & (i < 2060))).astype(np.uint8)
        payload = dict(
            x=M._col(np.uint64(fi) * np.uint64(1_000_000) + i, U),
            f=M._col(EDGE_BITS[(i + np.uint64(fi)) % np.uint64(len(EDGE_BITS))].view(np.float64), F),
            o=M._col(i * np.uint64(977) + np.uint64(fi), U, present=pres, dlevel_max=1),
            s=M._col([b"" if r % 4 == 1 else b"s%d-%d" % (fi, r) for r in range(n)], S),
            os=M._col([b"" if r % 3 == 0 else b"o%d" % r for r in range(n)], S,
                      present=1 - pres if n else pres, dlevel_max=1))
    specs = list(payload_specs) + _lsm_specs(with_skip_column)
    w = E.Writer(specs)
    for sp in payload_specs:
        c = payload[sp["name"]]
        w.put(sp["name"], c["values"], rlvl=c["rl"], dlvl=c["dl"], present=c["present"])
    w.put("__lsm_is_update", upd)
    if with_skip_column:
        w.put("__lsm_skip", skip)
    w.put("__lsm_id", ids)
    w.put("__lsm_version", i + np.uint64(1))
    w.put("__lsm_sequence", i + np.uint64(fi * 1_000_000 + 1))
    w.commit(n)
    img = w.image()
    w.close()
    columns = dict(payload)
    columns["__lsm_is_update"] = M._col(upd, B)
    columns["__lsm_id"] = M._col(ids, S)
    columns["__lsm_version"] = M._col(i + np.uint64(1), U)
    columns["__lsm_sequence"] = M._col(i + np.uint64(fi * 1_000_000 + 1), U)
    return ("hand_%02d" % fi, img, True, True, dict(ids=ids, upd=upd, skip=skip, columns=columns))


def check_hand_chain(ctx, files, specs, orders=ORDERS, arena_skips=None):
    c = Chain(ctx, files, arena_skips).build()
    try:
        filters = lsm_tables.model_filters(files)
        for k, flt in enumerate(filters):
            got, kept = c.ch.filter(k)
            assert (got is None) == (flt is None)
            assert flt is None or ((got == flt).all() and kept == int(flt.sum()))
        for order in orders:
            dev, nrows, st = compacted_image(c, specs, order)
            exp = M.expected_image(files, specs, order, filters=filters)
            assert len(dev) == len(exp), order
            assert dev == exp, order
            assert (st["rows_in"], st["rows_written"]) == model_counts(files, filters)
            assert nrows == st["rows_written"]
        return dev, nrows
    finally:
        c.close()


EDGE_OUT = EDGE_SPECS + M.lsm_columns()


@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "alternate"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_edge_matrix(ctx, n, pattern):
    """the file under test between a newer and an older one"""
    files = [hand_file(0, 70, keep_pattern("alternate", 70)),
             hand_file(1, n, keep_pattern(pattern, n)),
             hand_file(2, 3, keep_pattern("last", 3))]
    check_hand_chain(ctx, files, EDGE_OUT)


def test_a_file_from_which_nothing_is_kept_between_two_others(ctx):
    files = [hand_file(0, 2049, keep_pattern("all", 2049)),
             hand_file(1, 2100, keep_pattern("none", 2100)),
             hand_file(2, 65, keep_pattern("alternate", 65))]
    check_hand_chain(ctx, files, EDGE_OUT)


def test_a_chain_that_keeps_nothing(ctx):
    files = [hand_file(0, 64, keep_pattern("none", 64)), hand_file(1, 1, keep_pattern("none", 1))]
    _, nrows = check_hand_chain(ctx, files, EDGE_OUT)
    assert nrows == 0


def test_a_one_row_file(ctx):
    _, nrows = check_hand_chain(ctx, [hand_file(0, 1, keep_pattern("all", 1))], EDGE_OUT)
    assert nrows == 1


def test_float_words_are_copied_bit_for_bit(ctx):
    n = 4 * len(FLOAT_EDGES)
    files = [hand_file(0, n, keep_pattern("all", n)), hand_file(1, n, keep_pattern("alternate", n))]
    specs = [EDGE_SPECS[1]]
    dev, nrows = check_hand_chain(ctx, files, specs, orders=[M.SCAN_ORDER])
    cols, _ = M.expected_columns(files, specs, M.SCAN_ORDER)
    want = np.asarray(cols[0]["values"]).view(np.uint64)
    assert set(int(b) for b in EDGE_BITS) == set(int(b) for b in want)
    # the data page of the only column: the words as they were
    t = ctx.open_image(dev)
    page = [c for c in t.columns() if c["name"] == "f"][0]
    t.close()
    assert page["payload_bytes"] == 8 * nrows
    assert struct.pack("<%dQ" % nrows, *[int(b) for b in want]) in dev


def nested_hand_file(fi, cnt, keep):
    """records with cnt[i] items each; items.tag is a repeated STRING"""
    nrec = len(cnt)
    cnt = np.asarray(cnt)
    slots = np.maximum(cnt, 1)
    total = int(slots.sum())
    starts = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.int64)
    rl = np.ones(total, np.uint64)
    rl[starts] = 0
    ros = np.repeat(np.arange(nrec), slots)
    dl = np.where(cnt[ros] > 0, 2, 0).astype(np.uint64)
    j = np.arange(total, dtype=np.uint64)
    payload_specs = [
        dict(name="id", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="items.position", logical_type=U, storage_type=K.ENC_UINT32_BITPACKED,
             rlevel_max=1, dlevel_max=2, bitpack_max_value=63),
        dict(name="items.price", logical_type=U, storage_type=K.ENC_UINT64_LEB128, rlevel_max=1,
             dlevel_max=2),
        dict(name="items.tag", logical_type=S, storage_type=K.ENC_STRING_PLAIN, rlevel_max=1,
             dlevel_max=2),
        dict(name="opt.deep", logical_type=U, storage_type=K.ENC_UINT64_PLAIN, dlevel_max=2)]
    nest = dict(rl=rl, dl=dl, rec_of_slot=ros, rlevel_max=1, dlevel_max=2)
    r = np.arange(nrec, dtype=np.uint64)
    payload = {
        "id": M._col(np.uint64(fi * 1_000_000) + r, U),
        "items.position": M._col((j - starts[ros].astype(np.uint64)) % np.uint64(64), U, **nest),
        "items.price": M._col(j * np.uint64(7919) + np.uint64(fi), U, **nest),
        "items.tag": M._col([b"" if s % 5 == 2 else b"t%d.%d" % (fi, s) for s in range(total)], S,
                            **nest),
        # OPTIONAL RECORD opt { OPTIONAL deep }: levels without repetition, d in 0 .. 2
        "opt.deep": M._col(r * np.uint64(3), U, dl=(r % np.uint64(3)), dlevel_max=2)}
    return hand_file(fi, nrec, keep, payload_specs, payload), payload_specs


def test_nested_edges(ctx):
    """a record without items as the first and as the last kept record of a file, a record
    of 30 items across slot 2048, slots of dropped records between kept ones"""
    cnt = [3, 0] + [2] * 1020          # slots: 3 + 1 + 2040 = 2044 in front of record 1022
    cnt += [30, 1, 0, 4, 0]            # record 1022 holds slots 2044 .. 2073
    keep = np.ones(len(cnt), bool)
    keep[0] = False                    # first kept record: 1, no items
    keep[5:900:3] = False
    keep[-2] = False
    assert keep[1022] and cnt[1] == 0 and cnt[-1] == 0 and keep[-1]
    f0, pspecs = nested_hand_file(0, cnt, keep)
    cnt1 = [0, 5, 0, 0, 7, 1]
    f1, _ = nested_hand_file(1, cnt1, np.array([1, 0, 1, 1, 1, 0], bool))
    f2, _ = nested_hand_file(2, [2, 2], np.zeros(2, bool))
    specs = pspecs + M.lsm_columns()
    check_hand_chain(ctx, [f0, f2, f1], specs)
    # the record of 30 items alone survives
    only = np.zeros(len(cnt), bool)
    only[1022] = True
    f3, _ = nested_hand_file(3, cnt, only)
    check_hand_chain(ctx, [f3], specs, orders=[M.SCAN_ORDER])


# ---------------------------------------------------------------------------------------
# encodings and column rules
# ---------------------------------------------------------------------------------------
def _enc_file(fi, n, enc, keep, extra=None):
    i = np.arange(n, dtype=np.uint64)
    specs = [dict(name="e", logical_type=U, storage_type=enc)]
    payload = {"e": M._col((i * np.uint64(37) + np.uint64(fi)) % np.uint64(1000), U)}
    for sp, c in (extra or []):
        specs.append(sp)
        payload[sp["name"]] = c
    return hand_file(fi, n, keep, specs, payload)


def test_encodings_differ_from_file_to_file_and_from_the_output(ctx):
    n = 300
    files = [_enc_file(0, n, K.ENC_UINT64_LEB128, keep_pattern("alternate", n)),
             _enc_file(1, n, K.ENC_UINT64_PLAIN, keep_pattern("all", n)),
             _enc_file(2, 70, K.ENC_UINT32_PLAIN, keep_pattern("last", 70))]
    out_specs = [dict(name="e", logical_type=U, storage_type=K.ENC_UINT32_BITPACKED,
                      bitpack_max_value=1023)] + M.lsm_columns()
    check_hand_chain(ctx, files, out_specs)


def test_column_rules(ctx):
    n = 130
    i = np.arange(n, dtype=np.uint64)
    opt = (dict(name="late", logical_type=U, storage_type=K.ENC_UINT64_PLAIN, dlevel_max=1),
           M._col(i + np.uint64(5), U, present=(i % np.uint64(2)).astype(np.uint8), dlevel_max=1))
    req = (dict(name="req", logical_type=U, storage_type=K.ENC_UINT64_PLAIN), M._col(i, U))
    lstr = (dict(name="lstr", logical_type=S, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1),
            M._col([b"L%d" % r for r in range(n)], S, present=np.ones(n, np.uint8), dlevel_max=1))
    # the oldest file lacks `late`, `req` and `lstr`
    files = [_enc_file(0, n, K.ENC_UINT64_PLAIN, keep_pattern("alternate", n)),
             _enc_file(1, n, K.ENC_UINT64_PLAIN, keep_pattern("all", n), [opt, req, lstr])]
    e_spec = dict(name="e", logical_type=U, storage_type=K.ENC_UINT64_PLAIN)
    # an optional column absent from one file: NULLs for that file's rows
    specs = [e_spec, opt[0], lstr[0]] + M.lsm_columns()
    dev, nrows = check_hand_chain(ctx, files, specs)
    cols, _ = M.expected_columns(files, specs, M.FILE_ORDER)
    assert not cols[1]["present"][:n // 2].any() and cols[1]["present"][n // 2:].any()
    # __lsm_is_update is all false although the inputs carry set bits: the compared image
    # holds the model's column, which is
    assert all(f[4]["upd"].any() for f in files)
    upd = cols[[s["name"] for s in specs].index("__lsm_is_update")]["values"]
    assert len(upd) == nrows and not upd.any()
    c = Chain(ctx, files)
    try:
        def refused(specs):
            with pytest.raises(E.EvqlError) as ei:
                c.ch.compact(specs)
            assert ei.value.code == K.EVQL_EARG, ei.value
            return ei.value.msg
        assert "not built" in refused([e_spec])                     # an unbuilt chain
        c.build()
        assert "required column" in refused([e_spec, req[0]])       # absent and required
        assert "__lsm_skip" in refused([e_spec, dict(name="__lsm_skip", logical_type=B,
                                                     storage_type=K.ENC_BOOLEAN_BITPACKED)])
        refused([dict(e_spec, logical_type=F, storage_type=K.ENC_FLOAT_IEEE754)])  # type
        refused([dict(e_spec, dlevel_max=1)])                                      # levels
        refused([dict(e_spec, rlevel_max=1, dlevel_max=1)])
        refused([])
        with pytest.raises(E.EvqlError) as ei:
            c.ch.compact([e_spec], row_order=7)
        assert ei.value.code == K.EVQL_EARG
        # the chain is unchanged and usable after the refusals
        t = c.ch.compact([e_spec])
        assert t.num_rows == n + n // 2
        t.close()
    finally:
        c.close()


def test_an_arena_with_a_skiplist_as_the_first_table(ctx):
    n = 2100
    sk = (np.arange(n) % 3 == 1)
    # (the arena's table carries no __lsm_skip column: its skiplist comes with add())
    arena = hand_file(2, n, ~sk, with_skip_column=False)
    files = [hand_file(0, 500, keep_pattern("alternate", 500)), hand_file(1, 64, keep_pattern("all", 64)),
             arena]
    check_hand_chain(ctx, files, EDGE_OUT, arena_skips={2: sk.astype(np.uint8)})


# ---------------------------------------------------------------------------------------
# the compacted table answers as the chain does
# ---------------------------------------------------------------------------------------
def _rows(q):
    try:
        return q.run()
    finally:
        q.close()


def _flat_plans():
    k, rid, s, a, n = col("k"), col("rid"), col("s"), col("a"), col("n")
    return {
        "first-row": dict(select=[k, rid, s, count(1), sum_(a), max_(n)], group_by=[k]),
        "string-key": dict(select=[s, count(1), sum_(a)], group_by=[s]),
        "distinct": dict(select=[k, count_distinct(a % 50), count(1)], group_by=[k]),
    }


def _nested_plans():
    k, s, lid = col("k"), col("s"), col("id")
    lpos, lprice = col("items.position"), col("items.price")
    NESTED, WR = K.SCAN_NESTED, K.SCAN_NESTED_WITHIN_RECORD
    return {
        "first-row": dict(select=[k, lid, s, lpos, lprice, count(1), sum_(lprice)], group_by=[k],
                          scan_mode=NESTED),
        "string-key": dict(select=[s, count(1), sum_(lpos)], group_by=[s], scan_mode=NESTED),
        "distinct": dict(select=[k, count_distinct(lpos), count(1)], group_by=[k], scan_mode=NESTED),
        "nested": dict(select=[lpos, count(1), sum_(lprice), max_(lid)], group_by=[lpos],
                       scan_mode=NESTED),
        "within-record": dict(scan_select=[count(lpos), sum_(lprice), sum_(k)],
                              select=[out(2), count(1), sum_(out(0)), sum_(out(1))],
                              group_by=[out(2)], scan_mode=WR),
    }


@pytest.mark.parametrize("kind,pname", [("flat", "basic"), ("flat", "mixed"), ("nested", "basic")])
def test_the_compacted_table_is_the_chain(chains, kind, pname):
    c = chains(kind, pname)
    if kind == "flat":
        schema, specs, plans, rid = lsm_tables.LSM_SCHEMA, M.flat_out_specs(), _flat_plans(), "rid"
    else:
        schema, specs, plans, rid = LN.NESTED_LSM_SCHEMA, M.nested_out_specs(), _nested_plans(), "id"
    filters = O.oracle_partition_filters(c.files)
    before = {name: _rows(c.ch.query(Plan(schema, **kw))) for name, kw in plans.items()}
    t = c.ch.compact(specs, row_order=M.SCAN_ORDER)
    try:
        for name, kw in plans.items():
            exp = M.oracle_chain(c.files, filters, schema, kw)
            nkeys = len(kw["group_by"])
            got = _rows(t.query(Plan(schema, **kw)))
            again = _rows(c.ch.query(Plan(schema, **kw)))
            for r in (before[name], got, again):
                assert r.nrows == exp.nrows, name
                T.compare_results(r.rows(), exp.rows(), exp.types, key_cols=nkeys, rel=1e-6)
            assert sorted(again.rows(), key=repr) == sorted(before[name].rows(), key=repr), name
        # a bare scan over the compacted table: the cursor's rows in the cursor's order
        sel = [col(rid), col("s")]
        exp = O.oracle_run_chain([f[1] for f in reversed(c.files)], filters,
                                 Plan(schema, scan_select=sel))
        got = _rows(t.query(Plan(schema, scan_select=sel)))
        assert got.rows() == exp.rows()
    finally:
        t.close()
