"""The prefetching tile loop of evql_scan_agg on the device, at every column width mix
(the mixes and their table: scan_width_mixes.py).  The loop holds one raw word
per step for an 8- or 16-bit copy and two for a 32-bit or float32 copy, each width with its own
load and decode; the other device tests of the loop run config 3's three 16-bit copies and one
float32 copy.

Two tables, G = the CU count, T = 8192 rows per tile: (2G+1)*T + 5 rows and T + 1 rows.  A
window [0, n) of the big one sees the tiles a table of n rows has (tile0 = row_begin / T,
ntiles = ceil(row_end / T) - tile0), so one image serves the row counts at which the loop's
bookkeeping changes; its real end covers the zero fill and the clamped load:

  [0, T+1)                   one workgroup evaluates a second, one-row tile
  [0, G*T+1)                 the second tile of exactly one workgroup
  [G*T+101, 2*G*T+77)        an odd begin inside a tile, tile0 != 0; the first and the last
                             tile of the workgroup that gets two
  the whole table            three tiles for one workgroup, two for the rest, the real end
  the small table            its real end one row into the second tile

Every integer column holds 0 or its width's maximum at the rows where a pair, a tile, a
workgroup's turn or the table ends (scan_width_mixes.edge_rows), and those rows pass every
mix's WHERE: asserted below, on the host.

Every (mix, window) runs with the prefetch on and with EVQL_SCAN_PREFETCH=0.  The switch is read
per query (build_kernel_plan) and the kernel cache is keyed by the generated text, so it is
toggled around table.query() in this process.  Both runs are compared with the oracle and with
each other: integers, counts, group sets, first-row values and rows_passed are equal; with
exact float sums every float column is bit-equal; fast sums (the two single-width mixes) lie
within 1e-6 of the oracle's exactly rounded sums.  The text of every query is asserted to load
each column through the accessor of its width, and to carry the loop (or not) as the mix's list
says."""
import concurrent.futures
import os
import re

import numpy as np
import pytest

from eventql_amd import capi as K
from eventql_amd.plan import Plan
import oracle_lib as O

import scan_width_mixes as M
from scan_prefetch_child import bits
from test_gpu_narrow_float import env, write

pytestmark = pytest.mark.gpu

T = M.TILE


def windows(G):
    """name -> (table, row_begin, row_end); 0, 0 = the whole table"""
    return {"T+1": ("big", 0, T + 1),
            "GT+1": ("big", 0, G * T + 1),
            "second-to-last": ("big", G * T + 101, 2 * G * T + 77),
            "whole": ("big", 0, 0),
            "small": ("small", 0, 0)}


@pytest.fixture(scope="module")
def world(ctx, tmp_path_factory):
    """G, and per table: (resident table, path of its image, columns, rows)"""
    import torch
    G = torch.cuda.get_device_properties(0).multi_processor_count
    assert G >= 2
    d = tmp_path_factory.mktemp("scan_prefetch_widths")
    tables = {}
    for name, n in (("big", (2 * G + 1) * T + 5), ("small", T + 1)):
        cols = M.table_columns(n, G)
        img = write(M.FILE_COLUMNS, cols, n)
        path = str(d / (name + ".cst"))
        with open(path, "wb") as f:  # (the oracle maps the file: no copy of the image per run)
            f.write(img)
        with env(EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1):
            tables[name] = (ctx.open_image(img), path, cols, n)
        del img
    yield G, tables
    for t in tables.values():
        t[0].close()


def bounds(win, n):
    _, lo, hi = win
    return lo, (hi or n)


def oracle(path, n, mix, win):
    """the oracle's rows with EXACT sums (the oracle knows row filters, not windows)"""
    lo, hi = bounds(win, n)
    kw = mix.plan_kw(True)
    if (lo, hi) != (0, n):
        idx = np.arange(n)
        kw["row_filter"] = (idx >= lo) & (idx < hi)
    return O.oracle_run(path, Plan(M.SCHEMA, **kw))


def run(table, mix, win, exact, prefetch):
    _, lo, hi = win
    plan = Plan(M.SCHEMA, **mix.plan_kw(exact, row_begin=lo, row_end=hi))
    with env(EVQL_SCAN_PREFETCH=None if prefetch else 0):
        q = table.query(plan)
    try:
        got = q.run()
        return dict(rows=[tuple(r) for r in got.rows()], nrows=got.nrows, text=q.kernel_source(),
                    types=[q.column_type(i) for i in range(q.column_count())],
                    passed=q.stats()["rows_passed"], plan=plan)
    finally:
        q.close()


def check_text(mix, g, prefetch):
    text = g["text"]
    for i, name in enumerate(g["plan"].scan_columns):
        # (a column that stayed on the file's pages fails here, not vacuously passes)
        assert M.accessor(name, i) in text, (mix, name, i)
    assert int(re.search(r"#define EVQL_LCACHE (\d+)", text).group(1)) == mix.lcache, mix
    # the loop: FALLS_BACK mixes were compiled with it, reported scratch and were compiled again
    want = prefetch and mix in M.PREFETCH
    assert (M.MARKER in text) == want, (mix, prefetch)


def by_key(rows):
    out = {r[0]: r for r in rows}
    assert len(out) == len(rows)
    return out


def compare(case, exp, on, off, exact):
    aggregate = [p.is_aggregate for p in on["plan"].select]
    for tag, g in (("on", on), ("off", off)):
        assert g["types"] == list(exp.types), (case, tag)
        assert g["nrows"] == exp.nrows, (case, tag, g["nrows"], exp.nrows)
        assert g["passed"] == exp.rows_passed, (case, tag, g["passed"], exp.rows_passed)
    e, x, y = by_key(exp.rows()), by_key(on["rows"]), by_key(off["rows"])
    assert set(x) == set(e) and set(y) == set(e), case
    for key, er in e.items():
        for i, ty in enumerate(exp.types):
            if ty == K.T_FLOAT64 and aggregate[i] and not exact:
                for got in (x[key][i], y[key][i]):
                    assert abs(got - er[i]) <= 1e-6 * abs(er[i]), (case, key, i, got, er[i])
            else:
                assert bits(x[key][i]) == bits(er[i]) == bits(y[key][i]), (case, key, i, x[key], y[key], er)


@pytest.mark.parametrize("mix", M.ALL, ids=repr)
def test_mix_at_every_window(world, mix):
    G, tables = world
    wins = windows(G)
    with concurrent.futures.ThreadPoolExecutor(len(wins)) as pool:
        # the oracle runs next to the device (ctypes releases the lock), one thread per window
        exp = {name: pool.submit(oracle, tables[win[0]][1], tables[win[0]][3], mix, win)
               for name, win in wins.items()}
        got = {}
        for name, win in wins.items():
            table, _, cols, n = tables[win[0]]
            lo, hi = bounds(win, n)
            # the edge rows of the window pass WHERE: edges that are filtered away pin nothing
            edges = [r for r in M.edge_rows(n, G) if lo <= r < hi]
            assert len(edges) >= 4, (mix, name, edges)
            passes = mix.passes(cols)
            assert passes[edges].all(), (mix, name, [r for r in edges if not passes[r]])
            for mode in mix.modes():
                for prefetch in (True, False):
                    g = run(table, mix, win, mode == "exact", prefetch)
                    check_text(mix, g, prefetch)
                    got[name, mode, prefetch] = g
        for name, win in wins.items():
            e = exp[name].result()
            _, _, cols, n = tables[win[0]]
            lo, hi = bounds(win, n)
            # (the host's reading of WHERE is the plan's)
            assert e.rows_passed == int(mix.passes(cols)[lo:hi].sum()), (mix, name)
            for mode in mix.modes():
                compare((mix, name, mode), e, got[name, mode, True], got[name, mode, False], mode == "exact")


def test_edge_rows_hold_both_ends_of_every_width(world):
    """at the listed rows every integer column holds 0 and its width's maximum, the two rows of
    a listed pair hold both, and the float columns hold -0.0 and the largest and the smallest
    magnitude their exact sum's quantum allows"""
    G, tables = world
    for tname, (_, _, cols, n) in tables.items():
        edges = M.edge_rows(n, G)
        for r in (4098, T, 2 * T - 1, G * T, n - 1, n - 2):
            assert r in edges or r >= n, (tname, r)
        assert 4099 in edges and 4098 % 2 == 0
        for name, width in M.WIDTHS.items():
            at = cols[name][edges]
            if width == "f32":
                for want in M.float_edges(name):
                    assert any(bits(float(x)) == bits(want) for x in at), (tname, name, want)
                assert float(np.abs(cols[name]).max()) == M.float_edges(name)[1]
                assert np.array_equal(cols[name].astype(np.float32).astype(np.float64), cols[name])
                continue
            top = M.TOP[width or 16]
            assert set(at.tolist()) <= {0, top} and top in at, (tname, name)
            pairs = np.concatenate([at, cols[name][[r ^ 1 for r in edges if (r ^ 1) < n]]])
            assert {0, top} <= set(pairs.tolist()), (tname, name)
            if name[0] != "a":
                assert 0 in at, (tname, name)
            assert int(cols[name].max()) == top
