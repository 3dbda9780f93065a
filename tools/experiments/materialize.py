#!/usr/bin/env python3
"""Result materialisation, measured.

Workload: config 4's inner statement `select u, count(1), sum(a) from t group by u` over
1.25e8 * --scale rows with 1e7 * --scale keys, executed once per operator (not timed: the
scan is the same whatever happens to its groups).  Timed, per repeat, wall clock around the
whole call with the device idle before and after:
  (a) Query.to_table unsorted and sorted by u (evql_table_from_query), with the phases of
      evql_materialize_stats_t
  (b) the way that exists without it: every group to the host (next_batch), the SVector
      bytes decoded with numpy, E.Writer (the host cstable writer), Context.open_image
  (c) `select n, count(1), sum(sum_a) group by n` over the table of (a, sorted) and of (b):
      the answers must be equal; kernel_ms of both
--warmup calls of each are thrown away, --reps are kept: median, minimum and maximum.

usage: materialize.py [--scale F] [--reps N] [--warmup N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import eventql_amd as E  # noqa: E402
from eventql_amd import capi as K  # noqa: E402
from eventql_amd.plan import Plan, col, count, sum_  # noqa: E402

SCHEMA = dict(u=K.T_UINT64, a=K.T_UINT64)
SPECS = [dict(name="u", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
         dict(name="n", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
         dict(name="sum_a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)]
OUT_SCHEMA = dict(u=K.T_UINT64, n=K.T_UINT64, sum_a=K.T_UINT64)


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), runs=xs)


def inner_plan(n_keys):
    return Plan(SCHEMA, select=[col("u"), count(1), sum_(col("a"))], group_by=[col("u")],
                groups_hint=n_keys)


def executed(table, n_keys):
    q = table.query(inner_plan(n_keys))
    q.execute()
    return q


def to_table_once(ctx, q, sort_by):
    ctx.synchronize()
    t0 = time.perf_counter()
    tab = q.to_table(SPECS, sort_by=sort_by)
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return tab, dict(q.materialize_stats, wall_ms=wall)


def host_way_once(ctx, q):
    """fetch, decode, write, open: the phases in ms and the table"""
    ctx.synchronize()
    t0 = time.perf_counter()
    chunks = [[], [], []]
    while True:
        n, raw = q.next_batch(1 << 16)
        if n == 0:
            break
        for c, r in zip(chunks, raw):
            c.append(r)
    t1 = time.perf_counter()
    rec = np.dtype([("v", "<u8"), ("t", "u1")])
    cols = [np.ascontiguousarray(np.frombuffer(b"".join(c), dtype=rec)["v"]) for c in chunks]
    t2 = time.perf_counter()
    w = E.Writer(SPECS)
    for sp, v in zip(SPECS, cols):
        w.put(sp["name"], v)
    w.commit(len(cols[0]))
    img = w.image()
    w.close()
    t3 = time.perf_counter()
    tab = ctx.open_image(img)
    ctx.synchronize()
    t4 = time.perf_counter()
    ms = lambda a, b: (b - a) * 1e3
    return tab, dict(fetch_ms=ms(t0, t1), decode_ms=ms(t1, t2), write_ms=ms(t2, t3),
                     open_ms=ms(t3, t4), wall_ms=ms(t0, t4), rows=int(len(cols[0])))


def outer(tab):
    plan = Plan(OUT_SCHEMA, select=[col("n"), count(1), sum_(col("sum_a"))], group_by=[col("n")],
                groups_hint=1000)
    q = tab.query(plan)
    q.run().rows()  # (compiles)
    q.close()
    q = tab.query(plan)
    rows = sorted(q.run().rows())
    st = q.stats()
    q.close()
    return rows, st["kernel_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = int(125_000_000 * a.scale)
    n_keys = max(1, int(10_000_000 * a.scale))
    ctx = E.Context(0)
    table = ctx.generate(rows, "ua", u_mod=n_keys)
    res = dict(rows=rows, n_keys=n_keys, reps=a.reps, warmup=a.warmup)

    q = executed(table, n_keys)
    res["groups"] = q.stats()["num_groups"]
    kept = {}
    for name, sort_by in (("unsorted", None), ("sorted", "u")):
        runs = []
        for it in range(a.warmup + a.reps):
            tab, st = to_table_once(ctx, q, sort_by)
            if it >= a.warmup:
                runs.append(st)
            if it + 1 < a.warmup + a.reps:
                tab.close()
        kept[name] = tab
        res["to_table_" + name] = dict(
            wall_ms=summary([r["wall_ms"] for r in runs]),
            gather_ms=summary([r["gather_ms"] for r in runs]),
            sort_ms=summary([r["sort_ms"] for r in runs]),
            encode_ms=summary([r["encode_ms"] for r in runs]),
            presorted=runs[0]["presorted"], passes=runs[0]["passes"],
            n_kernel_launches=runs[0]["n_kernel_launches"], n_host_waits=runs[0]["n_host_waits"],
            image_bytes=E.lib().evql_table_image_size(tab.h))
        print(name, json.dumps(res["to_table_" + name]["wall_ms"]), flush=True)
    q.close()

    runs = []
    for it in range(a.warmup + a.reps):
        q = executed(table, n_keys)
        tab, st = host_way_once(ctx, q)
        q.close()
        if it >= a.warmup:
            runs.append(st)
        if it + 1 < a.warmup + a.reps:
            tab.close()
    kept["host"] = tab
    res["host_way"] = {k: summary([r[k] for r in runs])
                       for k in ("wall_ms", "fetch_ms", "decode_ms", "write_ms", "open_ms")}
    print("host way", json.dumps(res["host_way"]["wall_ms"]), flush=True)

    rows_dev, ms_dev = outer(kept["sorted"])
    rows_uns, ms_uns = outer(kept["unsorted"])
    rows_host, ms_host = outer(kept["host"])
    res["outer"] = dict(equal=bool(rows_dev == rows_host == rows_uns), groups=len(rows_dev),
                        kernel_ms_sorted=ms_dev, kernel_ms_unsorted=ms_uns, kernel_ms_host=ms_host)
    for t in kept.values():
        t.close()
    table.close()
    ctx.close()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
