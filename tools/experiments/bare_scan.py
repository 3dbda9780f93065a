#!/usr/bin/env python3
"""Device time of a bare scan (evql_scan_count + evql_scan_emit) against its yardstick.

Workload: the config-3 table (k, a, b, v plain 64-bit columns, generated on the device),
`select k, v from t where W` for config 3's W (24.9 % of the rows pass) and for a W that
passes ~0.1 %.

Yardstick T_c: kernel_ms of `select count(1) from t where W` over the same table -- one
streaming pass of the existing fused kernel over the WHERE columns (16 B / row) -- taken
in a process of its own that may load ANOTHER build of the library (--yardstick-lib: a
libevql_mi355x.so built from the parent commit), alternating with the bare scan, `--reps`
times.  The bare scan streams the WHERE columns twice and the payload columns once:

    count  reads 16 B / row
    emit   reads 32 B / row of every tile that holds a passing row, writes 16 B / passing row
    gate   count + emit <= T_c * (16 + emit bytes / row) / 16 + spread of T_c

Also: rows/s through evql_query_next_batch at 24.9 %, next to the drain of config 4's
1e7 groups, and -- with --rocprof -- `rocprofv3 --kernel-trace --stats` of one
bare scan in a run of its own.

usage: bare_scan.py [--rows N] [--reps R] [--yardstick-lib PATH] [--rocprof [--rocprof-dir DIR]]
       [--out FILE]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WHERES = {"24.9%": (30000, 30000), "0.1%": (65000, 8000)}


def where_of(name):
    from eventql_amd.plan import col
    lo, hi = WHERES[name]
    return (col("a") > lo) & (col("b") < hi)


def leg_yardstick(rows, warm=2, steps=5):
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    from eventql_amd.plan import Plan, count
    ctx = E.Context(0)
    t = ctx.generate(rows, "kabv")
    out = {}
    for name in WHERES:
        q = t.query(Plan(B.SCHEMA, select=[count(1)], where=where_of(name)))
        ms = []
        for i in range(warm + steps):
            q.execute()
            if i >= warm:
                ms.append(q.stats()["kernel_ms"])
        out[name] = dict(kernel_ms=ms, rows_passed=q.stats()["rows_passed"])
        q.close()
    return out


def drain(q, batch=1 << 20):
    n = 0
    t0 = time.perf_counter()
    while True:
        m, _ = q.next_batch(batch)
        if m == 0:
            break
        n += m
    return n, time.perf_counter() - t0


def leg_bare(rows, warm=1, steps=3):
    import re
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    from eventql_amd.plan import Plan, col
    ctx = E.Context(0)
    t = ctx.generate(rows, "kabv")
    out = {}
    for name in WHERES:
        q = t.query(Plan(B.SCHEMA, scan_select=[col("k"), col("v")], where=where_of(name)))
        src = q.kernel_source()
        tile = int(re.search(r"#define EVQL_TILE_ROWS (\d+)", src).group(1))
        runs = []
        for i in range(warm + steps):
            q.execute()
            n, wall = drain(q)
            st = q.stats()
            if i >= warm:
                runs.append(dict(count_ms=st["kernel_ms"], emit_ms=st["total_ms"] - st["kernel_ms"],
                                 rows=n, drain_s=wall))
        out[name] = dict(runs=runs, tile_rows=tile, rows_passed=st["rows_passed"])
        q.close()
    return out


def leg_config4_drain(rows):
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    ctx = E.Context(0)
    t = ctx.generate(rows, "kabvu", u_mod=10_000_000)
    q = t.query(B.config4())
    q.execute()
    n, wall = drain(q)
    q.close()
    return dict(groups=n, drain_s=wall, rows_per_s=n / wall)


def child(leg, rows, lib=None):
    env = dict(os.environ)
    if lib:
        env["EVQL_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--rows", str(rows)],
                       env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("%s leg failed (%d): %s" % (leg, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None)
    args = ap.parse_args()
    if args.leg:
        fn = dict(yardstick=leg_yardstick, bare=leg_bare, config4=leg_config4_drain)[args.leg]
        print(json.dumps(fn(args.rows)))
        return
    res = dict(rows=args.rows, reps=[], yardstick_lib=args.yardstick_lib or "this build")
    for _ in range(args.reps):
        res["reps"].append(dict(yardstick=child("yardstick", args.rows, args.yardstick_lib),
                                bare=child("bare", args.rows)))
    res["config4_drain"] = child("config4", 125_000_000 if args.rows >= 100_000_000 else args.rows)
    summary = {}
    for name in WHERES:
        tc = [x for r in res["reps"] for x in r["yardstick"][name]["kernel_ms"]]
        per_rep = [min(r["yardstick"][name]["kernel_ms"]) for r in res["reps"]]
        cnt = [x["count_ms"] for r in res["reps"] for x in r["bare"][name]["runs"]]
        emit = [x["emit_ms"] for r in res["reps"] for x in r["bare"][name]["runs"]]
        b0 = res["reps"][0]["bare"][name]
        passed, tile = b0["rows_passed"], b0["tile_rows"]
        # tiles without a passing row are not read again by the emit pass
        p_row = passed / args.rows
        live_tiles = 1.0 - (1.0 - p_row) ** tile
        emit_bytes_row = 32.0 * live_tiles + 16.0 * p_row
        t_c = sorted(tc)[len(tc) // 2]
        spread = max(per_rep) - min(per_rep)
        bound = t_c * (16.0 + emit_bytes_row) / 16.0 + spread
        c_ms, e_ms = sorted(cnt)[len(cnt) // 2], sorted(emit)[len(emit) // 2]
        dr = [x["rows"] / x["drain_s"] for r in res["reps"] for x in r["bare"][name]["runs"] if x["rows"]]
        summary[name] = dict(
            rows_passed=passed, T_c_ms=t_c, T_c_spread_ms=spread, T_c_min_max=[min(tc), max(tc)],
            count_ms=c_ms, emit_ms=e_ms, total_ms=c_ms + e_ms, bound_ms=bound,
            gate="met" if c_ms + e_ms <= bound else "MISSED",
            yardstick_TBps=16.0 * args.rows / (t_c * 1e9), count_TBps=16.0 * args.rows / (c_ms * 1e9),
            emit_TBps=emit_bytes_row * args.rows / (e_ms * 1e9) if e_ms else None,
            emit_bytes_per_row=emit_bytes_row,
            drain_rows_per_s=sorted(dr)[len(dr) // 2] if dr else None)
    res["summary"] = summary
    if args.rocprof:
        import tempfile
        d = args.rocprof_dir or tempfile.mkdtemp(prefix="bare_scan_rocprof_")
        os.makedirs(d, exist_ok=True)
        p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "bare_scan",
                            "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                            "--leg", "bare", "--rows", str(args.rows)],
                           capture_output=True, text=True, timeout=900)
        stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
        res["rocprof"] = dict(rc=p.returncode, kernel_stats_csv=open(stats[0]).read() if stats else "",
                              stderr=p.stderr[-500:] if p.returncode else "")
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res["summary"], indent=1))
    print(json.dumps(res["config4_drain"]))


if __name__ == "__main__":
    main()
