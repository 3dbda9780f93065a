"""The prefetching tile loop of evql_scan_agg on the device: config 3's query
over its generator's columns, narrow copies in force (EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1:
a table keeps them only from 2^26 rows on, the switches lower that to every table), at the row
counts where the loop's bookkeeping changes -- T = 8192 rows per tile, G workgroups (one per
CU: the 1024-thread block and its LDS table fill one):

  1, T-1, T, T+1        one workgroup, one tile; every other workgroup runs zero iterations
  G*T-1, G*T+1          the second tile of exactly one workgroup: evaluate, copy, then
                        evaluate what the clamped prefetch left in place
  (2G+1)*T+5            three tiles for one workgroup, two for the rest

Every case runs twice, in two fresh child processes (scan_prefetch_child.py): prefetch on and
EVQL_SCAN_PREFETCH=0.  Integer aggregates and groups are equal between the two and to the
oracle; with exact float sums every column is bit-equal; fast sums lie within smoke()'s 1e-6
of the oracle's exactly rounded sums.  One oracle run per image and plan, shared."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K, synth
import oracle_lib as O

import scan_prefetch_child as C

pytestmark = pytest.mark.gpu

UINT = lambda name: dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
FLOAT = lambda name: dict(name=name, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)


def write(cols, n):
    w = E.Writer([UINT("k"), UINT("a"), UINT("b"), FLOAT("v")])
    for name in "kabv":
        w.put(name, cols[name][:n])
    w.commit(n)
    img = w.image()
    w.close()
    return img


@pytest.fixture(scope="module")
def runs(ctx, tmp_path_factory):
    """(G, images, results with prefetch on, results with the switch off)"""
    import torch
    G = torch.cuda.get_device_properties(0).multi_processor_count
    d = tmp_path_factory.mktemp("scan_prefetch")
    ns = C.sizes(G)
    cols = synth.table_columns(max(ns))
    images = {n: write(cols, n) for n in ns}
    # a table whose zone maps exclude whole tiles under a > 30000 (tiles 0 and 2)
    nz = 3 * C.TILE + 5
    row = np.arange(nz, dtype=np.uint64)
    zc = dict(cols, a=((row // np.uint64(C.TILE)) % np.uint64(2)) * np.uint64(40000) + row % np.uint64(5000))
    images["zones"] = write(zc, nz)
    # 70,000 keys, and a second tile for one workgroup
    nm = G * C.TILE + 1
    row = np.arange(nm, dtype=np.uint64)
    images["many"] = write(dict(cols, k=(row * np.uint64(2654435761)) % np.uint64(C.MANY_KEYS)), nm)
    for name, img in images.items():
        with open(str(d / ("%s.cst" % name)), "wb") as f:
            f.write(img)
    with open(str(d / "G"), "w") as f:
        f.write(str(G))
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scan_prefetch_child.py")
    procs = {}
    for tag, value in (("on", None), ("off", "0")):
        env = dict(os.environ)
        env.pop("EVQL_SCAN_PREFETCH", None)
        if value is not None:
            env["EVQL_SCAN_PREFETCH"] = value
        procs[tag] = subprocess.Popen([sys.executable, "-s", child, str(d), str(d / (tag + ".pkl"))],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for tag, p in procs.items():
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (tag, err[-3000:])
        with open(str(d / (tag + ".pkl")), "rb") as f:
            out[tag] = pickle.load(f)
    return G, images, out["on"], out["off"]


_oracle = {}


def oracle(images, which, kw, nrows):
    """the oracle's rows of plan `kw` with EXACT sums (shared by the fast and the exact case)"""
    key = (which, repr(sorted((n, repr(x)) for n, x in kw.items())))
    if key not in _oracle:
        okw = dict(kw)
        lo, hi = okw.pop("row_begin", None), okw.pop("row_end", None)
        if lo is not None:  # (the oracle knows row filters, not windows)
            idx = np.arange(nrows)
            okw["row_filter"] = (idx >= lo) & (idx < hi)
        _oracle[key] = O.oracle_run(images[which], C.plan_of(okw, True))
    return _oracle[key]


def by_key(rows):
    return {r[0]: r for r in rows}


def compare(case, G, images, on, off):
    which, kw, exact = C.cases(G)[case]
    nrows = which if isinstance(which, int) else {"zones": 3 * C.TILE + 5, "many": G * C.TILE + 1}[which]
    exp = oracle(images, which, kw, nrows)
    g_on, g_off = on[case], off[case]
    for tag, g in (("on", g_on), ("off", g_off)):
        assert g["types"] == list(exp.types), (case, tag)
        assert g["nrows"] == exp.nrows, (case, tag, g["nrows"], exp.nrows)
        assert g["passed"] == exp.rows_passed, (case, tag)
    e, x, y = by_key(exp.rows()), by_key(g_on["rows"]), by_key(g_off["rows"])
    assert set(x) == set(e) and set(y) == set(e), case
    for key, er in e.items():
        for i, ty in enumerate(exp.types):
            if ty != K.T_FLOAT64 or exact:
                assert C.bits(x[key][i]) == C.bits(er[i]) == C.bits(y[key][i]), (case, key, i, x[key], y[key], er)
            else:
                for got in (x[key][i], y[key][i]):
                    assert abs(got - er[i]) <= 1e-6 * abs(er[i]), (case, key, i, got, er[i])
    return g_on, g_off


def test_the_switch_selects_the_loop(runs):
    G, _, on, off = runs
    assert G >= 2
    for case in C.cases(G):
        assert on[case]["prefetch"] and not off[case]["prefetch"], case
        # (config 3's WHERE prunes: both texts carry the loop with zone test as well)
        assert on[case]["zone_loop"] == off[case]["zone_loop"], case


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("sums", ["fast", "exact"])
def test_row_counts(runs, which, sums):
    G, images, on, off = runs
    n = C.sizes(G)[which]
    compare("rows-%d-%s" % (n, sums), G, images, on, off)


def test_row_window_from_a_second_tile_into_a_last(runs):
    G, images, on, off = runs
    compare("window", G, images, on, off)


def test_hint_far_too_small_regrows_and_reruns(runs):
    G, images, on, off = runs
    g_on, _ = compare("small-hint", G, images, on, off)
    # more groups than the slots the table started with: the first launch filled it
    assert g_on["nrows"] > 65536 + 2


def test_zone_bitmap_takes_the_unchanged_loop(runs):
    G, images, on, off = runs
    g_on, g_off = compare("zones", G, images, on, off)
    assert g_on["zone_loop"] and g_on["tiles_skipped"] > 0 and g_off["tiles_skipped"] == g_on["tiles_skipped"]
