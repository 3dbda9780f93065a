"""The staging tile loop of evql_scan_agg on the device: the rows that pass
WHERE leave a tuple in a 128-entry ring of their wave and the group table is updated once per
64 of them.  Every case runs with the loop and under EVQL_SCAN_STAGE=0 (the prefetching loop
as it was; the switch is read per query and the kernel cache is keyed by the text, so it is
toggled around table.query()), and both are compared with the oracle and with each other:
groups, counts, integer sums and rows_passed are equal, exact float sums bit for bit, fast float
sums within smoke()'s 1e-6 of the oracle's exactly rounded sums.

One table of (2G+1)*T + 5 rows (G = the CU count, T = 8192 rows per tile: block 1024 x 2 rows x
unroll 4) and its windows, as in test_gpu_scan_prefetch.py.  A wave evaluates 8 rows of 64
lanes per tile: row q = 2u + j of wave w holds the table rows  tile*T + (u*1024 + w*64 + lane)*2
+ j.  The filter columns are written so that the number of lanes that pass in each of them is
exact (`b` always passes):

  ae   by tile, P = (tile + tile // G) % 4: 63 lanes of row 0, and 0 / 1 / 2 / 64 lanes of row 1
       -- 63, 64, 65 tuples in a wave's first tile, and 127 pending reached by 63 + 64.  Values
       are 1 or 40000: `ae > 0` passes every row (a drain behind every row, `tail` wraps the
       ring many times), `ae > 65535` none
  ax   only row 0 and the table's last row pass: the windows [0, n-1) and [1, n) leave one
       (the last row alone: the drain at the end of the kernel, one lane)
  ar   uniform 16-bit values: `ar > 30000` passes 54 %

and the key columns k (1000 keys), k1 (one group: every drained lane hits the lane cache), ks
(k sorted), k5 (5000 keys under hint 1000: rows that find no LDS slot go to the HBM table from
the drain, `bypass` sets in) and km (70,000 keys under hint 1: the HBM table fills, the host
regrows it and runs the scan again, with tuples pending in the rings of the launch that ended).

The column width mixes of scan_width_mixes.PREFETCH that have a WHERE and no first-row column
run over that file's table and the windows of test_gpu_scan_prefetch_widths.py."""
import numpy as np
import pytest

from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_
import oracle_lib as O

import scan_width_mixes as M
import test_gpu_scan_prefetch_widths as W
from test_gpu_narrow_float import env, write

pytestmark = pytest.mark.gpu

T = M.TILE
STAGE = "evql_stage_ring"
NAMES = ["k", "k1", "ks", "k5", "km", "ae", "ax", "ar", "b", "v"]
SCHEMA = {n: (K.T_FLOAT64 if n == "v" else K.T_UINT64) for n in NAMES}
SPECS = [dict(name=n, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754) if n == "v" else
         dict(name=n, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN) for n in NAMES]
EDGE = [[63, 0], [63, 1], [63, 2], [63, 64]]  # lanes that pass in rows 0 and 1 of a wave's tile
PASS, FAIL = 40000, 1


def columns(n, G):
    rng = np.random.default_rng(11)
    row = np.arange(n, dtype=np.uint64)
    c = dict(k=rng.integers(0, 1000, n).astype(np.uint64), k1=np.full(n, 7, np.uint64),
             k5=rng.integers(0, 5000, n).astype(np.uint64), km=(row * np.uint64(2654435761)) % np.uint64(70000),
             ar=rng.integers(0, 65536, n).astype(np.uint64), b=rng.integers(0, 30000, n).astype(np.uint64),
             v=rng.integers(0, 1 << 24, n).astype(np.float64) / 1024.0)
    c["ks"] = np.sort(c["k"])
    tile, off = row // np.uint64(T), row % np.uint64(T)
    u, tid, j = off // np.uint64(2048), (off % np.uint64(2048)) // np.uint64(2), off % np.uint64(2)
    q, lane = (u * np.uint64(2) + j).astype(np.int64), (tid % np.uint64(64)).astype(np.int64)
    p = ((tile + tile // np.uint64(G)) % np.uint64(4)).astype(np.int64)
    lanes = np.zeros((4, 8), np.int64)
    lanes[:, :2] = EDGE
    c["ae"] = np.where(lane < lanes[p, q], PASS, FAIL).astype(np.uint64)
    c["ax"] = np.full(n, FAIL, np.uint64)
    c["ax"][[0, n - 1]] = PASS
    return c


def cases(G, n):
    """name -> (key, filter, literal of `filter > literal`, row_begin, row_end, hint, sums)"""
    return {
        "no row passes": ("k", "ae", 65535, 0, n, 1000, "exact"),
        "every row passes": ("k", "ae", 0, 0, n, 1000, "exact"),
        "every row passes, fast sums": ("k", "ae", 0, 0, n, 1000, "fast"),
        "63, 64, 65 and 63 + 64 in a first tile": ("k", "ae", 30000, 0, G * T, 1000, "exact"),
        "63, 64, 65 and 63 + 64 across a workgroup's turns": ("k", "ae", 30000, 0, n, 1000, "exact"),
        "only the last row passes": ("k", "ax", 30000, 1, n, 1000, "exact"),
        "only the first row passes": ("k", "ax", 30000, 0, n - 1, 1000, "exact"),
        "a window that cuts a pair, a tile and a last turn": ("k", "ar", 30000, G * T + 101, 2 * G * T + 77,
                                                              1000, "exact"),
        "workgroups without a tile": ("k", "ar", 30000, 0, T + 1, 1000, "exact"),
        "one group": ("k1", "ar", 30000, 0, n, 1000, "exact"),
        "input sorted by key": ("ks", "ar", 30000, 0, n, 1000, "exact"),
        "5000 groups under hint 1000": ("k5", "ar", 30000, 0, n, 1000, "exact"),
        "the HBM table fills and the scan runs again": ("km", "ar", 30000, 0, n, 1, "exact"),
        "uniform filter, fast sums": ("k", "ar", 30000, 0, n, 1000, "fast"),
    }


def plan_kw(case, exact):
    key, f, lit, lo, hi, hint, _ = case
    fs = dict(float_sum_mode=K.FLOAT_SUM_EXACT) if exact else {}
    return dict(select=[col(key), sum_(col("v")), count(1), sum_(col("b"))], group_by=[col(key)],
                where=(col(f) > lit) & (col("b") < 30000), groups_hint=hint, **fs)


@pytest.fixture(scope="module")
def world(ctx, tmp_path_factory):
    import torch
    G = torch.cuda.get_device_properties(0).multi_processor_count
    assert G >= 2
    n = (2 * G + 1) * T + 5
    cols = columns(n, G)
    img = write(SPECS, cols, n)
    path = str(tmp_path_factory.mktemp("scan_stage") / "big.cst")
    with open(path, "wb") as f:  # (the oracle maps the file)
        f.write(img)
    with env(EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1):
        table = ctx.open_image(img)
    del img
    yield G, n, table, path, cols
    table.close()


def run(table, schema, kw, stage):
    plan = Plan(schema, **kw)
    with env(EVQL_SCAN_STAGE=None if stage else 0, EVQL_SCAN_PREFETCH=None):
        q = table.query(plan)
    try:
        got = q.run()
        return dict(rows=[tuple(r) for r in got.rows()], nrows=got.nrows, text=q.kernel_source(),
                    types=[q.column_type(i) for i in range(q.column_count())],
                    passed=q.stats()["rows_passed"], plan=plan)
    finally:
        q.close()


_oracle = {}


def oracle(path, n, case):
    """the oracle's rows with EXACT sums, shared by a case's fast form (it knows row filters, not
    windows)"""
    key = case[:6]
    if key not in _oracle:
        kw = plan_kw(case, True)
        lo, hi = case[3], case[4]
        if (lo, hi) != (0, n):
            idx = np.arange(n)
            kw["row_filter"] = (idx >= lo) & (idx < hi)
        _oracle[key] = O.oracle_run(path, Plan(SCHEMA, **kw))
    return _oracle[key]


def passing(case, cols):
    _, f, lit, lo, hi, _, _ = case
    return int(((cols[f][lo:hi] > np.uint64(lit)) & (cols["b"][lo:hi] < np.uint64(30000))).sum())


@pytest.mark.parametrize("name", sorted(cases(2, 100)))
def test_ring_edges(world, name):
    G, n, table, path, cols = world
    case = cases(G, n)[name]
    exact = case[6] == "exact"
    kw = dict(plan_kw(case, exact), row_begin=case[3], row_end=case[4])
    on, off = run(table, SCHEMA, kw, True), run(table, SCHEMA, kw, False)
    assert STAGE in on["text"] and STAGE not in off["text"], name
    assert M.MARKER in on["text"] and M.MARKER in off["text"], name
    exp = oracle(path, n, case)
    print("%s: %d rows pass, %d groups" % (name, exp.rows_passed, exp.nrows))
    assert exp.rows_passed == passing(case, cols), name
    W.compare(name, exp, on, off, exact)


def test_the_filter_columns_are_what_the_cases_say(world):
    G, n, table, path, cols = world
    cs = cases(G, n)
    per_wave = lambda f, tile: (cols[f][tile * T:(tile + 1) * T] > 30000).reshape(4, 16, 64, 2).sum(axis=(0, 2, 3))
    # tiles 0 .. 3: 63, 64, 65 and 127 rows of every wave pass, in its rows 0 and 1
    assert [per_wave("ae", t).tolist() for t in range(4)] == [[x] * 16 for x in (63, 64, 65, 127)]
    assert passing(cs["no row passes"], cols) == 0
    assert passing(cs["every row passes"], cols) == n
    assert passing(cs["only the last row passes"], cols) == 1 == passing(cs["only the first row passes"], cols)
    assert cols["ax"][n - 1] == PASS and cols["ax"][0] == PASS
    # the turns of one workgroup differ: tiles w, w + G, w + 2G
    assert len({int((t + t // G) % 4) for t in (0, G, 2 * G)}) == 3
    assert len(np.unique(cols["km"])) == 70000 and len(np.unique(cols["k5"])) == 5000


def test_a_full_table_is_regrown_with_tuples_pending(world):
    G, n, table, path, cols = world
    case = cases(G, n)["the HBM table fills and the scan runs again"]
    # more groups than the 65,536 slots the table starts with, whatever the hint
    assert oracle(path, n, case).nrows > 65536 + 2


# ---- the column width mixes ------------------------------------------------------------------
def staged_mix(mix):
    """a WHERE, and nothing but the key selected bare (a bare column is a first-row value)"""
    sel = Plan(M.SCHEMA, **mix.plan_kw(True)).select
    return bool(mix.filt) and not any(not p.is_aggregate for p in sel[1:])


STAGED = [m for m in M.PREFETCH if staged_mix(m)]


def test_the_mixes_that_stage():
    assert [m.name for m in STAGED] == ["k8-a8-b8-v", "k32-a32-b32-v", "k16-a8-b32-v", "k8-a32-b8-v",
                                        "k32-a16-b8-w", "k32-a32-b32", "g3-a32-b8-v", "l16-a8-b32-v"]


@pytest.fixture(scope="module")
def mix_world(ctx, tmp_path_factory):
    import torch
    G = torch.cuda.get_device_properties(0).multi_processor_count
    d = tmp_path_factory.mktemp("scan_stage_mixes")
    tables = {}
    for name, n in (("big", (2 * G + 1) * T + 5), ("small", T + 1)):
        cols = M.table_columns(n, G)
        img = write(M.FILE_COLUMNS, cols, n)
        path = str(d / (name + ".cst"))
        with open(path, "wb") as f:
            f.write(img)
        with env(EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1):
            tables[name] = (ctx.open_image(img), path, cols, n)
        del img
    yield G, tables
    for t in tables.values():
        t[0].close()


@pytest.mark.parametrize("mix", STAGED, ids=repr)
def test_mix_at_every_window(mix_world, mix):
    G, tables = mix_world
    for name, win in W.windows(G).items():
        table, path, cols, n = tables[win[0]]
        lo, hi = W.bounds(win, n)
        # 0 and each width's maximum at the rows where a pair, a tile and the table end, and
        # those rows pass WHERE
        edges = [r for r in M.edge_rows(n, G) if lo <= r < hi]
        assert len(edges) >= 4 and mix.passes(cols)[edges].all(), (mix, name)
        exp = W.oracle(path, n, mix, win)
        assert exp.rows_passed == int(mix.passes(cols)[lo:hi].sum()), (mix, name)
        for mode in mix.modes():
            kw = mix.plan_kw(mode == "exact", row_begin=win[1], row_end=win[2])
            on, off = run(table, M.SCHEMA, kw, True), run(table, M.SCHEMA, kw, False)
            assert STAGE in on["text"] and STAGE not in off["text"], (mix, name)
            assert M.MARKER in off["text"], (mix, name)
            W.compare((mix, name, mode), exp, on, off, mode == "exact")
