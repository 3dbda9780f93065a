"""Child process of test_gpu_scan_prefetch.py: runs every case over the images the test wrote,
under the EVQL_SCAN_PREFETCH of its environment, and pickles the rows.  Also imported by the
test for the cases themselves.

usage: scan_prefetch_child.py IMAGE_DIR OUT_FILE"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from eventql_amd import bench_plans as B, capi as K  # noqa: E402
from eventql_amd.plan import Plan, col, count, sum_  # noqa: E402

TILE = 8192  # config 3's tile: block 1024 x 2 rows x unroll 4
k, a, b, v = [col(x) for x in "kabv"]
CONFIG3 = dict(select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=(a > 30000) & (b < 30000),
               groups_hint=1000)
# 70,000 groups under a hint of 1: more than the 65,536 slots the HBM table starts with, whatever
# the hint -- it fills, the host regrows it and runs the scan again; the workgroups that see the
# status word leave their loop with a prefetch in flight (the image "many": k = 70,000 keys)
MANY_KEYS = 70_000
SMALL_HINT = dict(CONFIG3, groups_hint=1)


def sizes(G):
    return [1, TILE - 1, TILE, TILE + 1, G * TILE - 1, G * TILE + 1, (2 * G + 1) * TILE + 5]


def cases(G):
    """name -> (rows of the image, plan keywords, exact sums?)"""
    out = {}
    for n in sizes(G):
        out["rows-%d-fast" % n] = (n, CONFIG3, False)
        out["rows-%d-exact" % n] = (n, CONFIG3, True)
    big = (2 * G + 1) * TILE + 5
    # begins inside tile G and ends inside tile 2G: the first and the last tile of the workgroup
    # that gets two of the window's G + 1 tiles
    out["window"] = (big, dict(CONFIG3, row_begin=G * TILE + 100, row_end=2 * G * TILE + 77), True)
    out["small-hint"] = ("many", SMALL_HINT, True)
    out["zones"] = ("zones", CONFIG3, True)
    return out


def plan_of(kw, exact):
    fs = dict(float_sum_mode=K.FLOAT_SUM_EXACT) if exact else {}
    return Plan(B.SCHEMA, **fs, **kw)


def bits(x):
    return np.float64(x).tobytes().hex() if isinstance(x, float) else repr(x)


def main(image_dir, out_file):
    import eventql_amd as E
    os.environ["EVQL_NARROW_PLAIN"] = "1"  # small tables keep the copies
    os.environ["EVQL_NARROW_FLOAT"] = "1"
    ctx = E.Context(0)
    with open(os.path.join(image_dir, "G")) as f:
        G = int(f.read())
    tables, out = {}, {}
    for name, (which, kw, exact) in cases(G).items():
        if which not in tables:
            with open(os.path.join(image_dir, "%s.cst" % which), "rb") as f:
                tables[which] = ctx.open_image(f.read())
        q = tables[which].query(plan_of(kw, exact))
        try:
            src = q.kernel_source()
            got = q.run()
            out[name] = dict(rows=[tuple(r) for r in got.rows()], nrows=got.nrows,
                             types=[q.column_type(i) for i in range(q.column_count())],
                             passed=q.stats()["rows_passed"],
                             prefetch="have || t < A.ntiles" in src, zone_loop="A.tile_skip" in src,
                             tiles_skipped=q.zone_stats()["tiles_skipped"])
        finally:
            q.close()
    for t in tables.values():
        t.close()
    ctx.close()
    with open(out_file, "wb") as f:
        pickle.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
