#!/usr/bin/env python3
"""Zone maps measured against the parent commit.

Table: `--rows` rows (default 1e8) of config 3's columns -- k, a, b random, v float -- plus
an ascending DATETIME column `t`, built on the device (torch RNG, fixed seed) and encoded by
the device writer; every leg rebuilds the same table in a process of its own.

  nothing may get slower
    config 3's query (WHERE a > 30000 AND b < 30000: the shape prunes, the bitmap is empty
    on random data): kernel_ms here against the parent's; gate: min here <= min of the
    parent + the range of the parent's per-repetition minima.
    `bench.py --steps 20 --warmup 3` of both trees (--bench): ms_per_step, gate +-5 %.
    The one-off cost of the statistics passes: create + first execute of config 3's query
    here minus the parent's (both make the narrow copies of a and b first).

  pruned queries
    `select count(1), sum(a) from t where t >= L` with 100 %, 10 % and 0.1 % of the rows
    behind L.  Yardstick T_p: the parent's kernel_ms for the same query.  Gate:
    kernel_ms <= T_p * tiles_kept / tiles_total + t(k_zone_select) + spread of T_p.
    Achieved bytes/s: the algorithmic bytes of the tiles actually read over kernel_ms.

Repetitions (--reps, default 5) run in processes of their own, alternating parent and
this tree; minima are taken.  --parent-root is a checkout of the parent commit with its
library built (the legs of the parent import ITS python package).  --rocprof adds one
`rocprofv3 --kernel-trace --stats` run of the pruned queries, in a run of its own.

usage: zone_maps.py --parent-root DIR [--rows N] [--reps R] [--bench] [--no-queries]
                    [--rocprof] [--rocprof-dir DIR] [--out FILE]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
T0, T_STEP = 1438055327000000, 1000
FRACTIONS = {"100%": 1.0, "10%": 0.1, "0.1%": 0.001}


def build_table(E, K, ctx, rows):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(20251)
    cols = dict(
        k=torch.randint(0, 1000, (rows,), generator=g, device="cuda", dtype=torch.int64),
        a=torch.randint(0, 65536, (rows,), generator=g, device="cuda", dtype=torch.int64),
        b=torch.randint(0, 65536, (rows,), generator=g, device="cuda", dtype=torch.int64),
        v=torch.rand(rows, generator=g, device="cuda", dtype=torch.float64) * 16384.0,
        t=torch.arange(rows, device="cuda", dtype=torch.int64) * T_STEP + T0)
    specs = [dict(name=n, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)
             for n in "kab"]
    specs.append(dict(name="v", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754))
    specs.append(dict(name="t", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_PLAIN))
    torch.cuda.synchronize()
    t = ctx.table_from_device_columns(specs, {n: c.data_ptr() for n, c in cols.items()}, None, rows)
    torch.cuda.synchronize()
    del cols
    torch.cuda.empty_cache()
    return t


def timed_runs(q, warm, steps):
    ms = []
    for i in range(warm + steps):
        q.execute()
        if i >= warm:
            ms.append(q.stats()["kernel_ms"])
    return ms


def leg_queries(root, rows, warm=3, steps=10):
    sys.path.insert(0, root)
    import eventql_amd as E
    from eventql_amd import bench_plans as B, capi as K
    from eventql_amd.plan import Plan, col, count, lit, sum_
    ctx = E.Context(0)
    t = build_table(E, K, ctx, rows)
    schema = dict(B.SCHEMA, t=K.T_TIMESTAMP64)
    out = dict(tree="here" if root == HERE else "parent")

    def c3(l1, l2):
        return Plan(schema, select=[col("k"), sum_(col("v")), count(1), sum_(col("b"))],
                    group_by=[col("k")], where=(col("a") > l1) & (col("b") < l2), groups_hint=1000)

    # first query on the table: narrow copies of k, a, b (+ here: the statistics of a and b)
    w0 = time.perf_counter()
    q = t.query(c3(30000, 30000))
    q.execute()
    first_ms = (time.perf_counter() - w0) * 1e3
    ms = timed_runs(q, warm, steps)
    st = q.stats()
    out["config3"] = dict(first_create_execute_ms=first_ms, kernel_ms=ms, rows_passed=st["rows_passed"],
                          algorithmic_bytes=st["algorithmic_bytes"],
                          zone_stats=q.zone_stats() if hasattr(q, "zone_stats") else None)
    q.close()
    # the same shape with other literals: what a later query of the shape costs to create
    w0 = time.perf_counter()
    q = t.query(c3(30001, 29999))
    q.execute()
    out["config3"]["later_create_execute_ms"] = (time.perf_counter() - w0) * 1e3
    q.close()
    out["pruned"] = {}
    for name, frac in FRACTIONS.items():
        first_row = rows - int(rows * frac)
        L = lit(T0 + first_row * T_STEP, K.T_TIMESTAMP64)
        plan = Plan(schema, select=[count(1), sum_(col("a"))], where=col("t") >= L)
        w0 = time.perf_counter()
        q = t.query(plan)
        create_ms = (time.perf_counter() - w0) * 1e3
        ms = timed_runs(q, warm, steps)
        st = q.stats()
        got = q.fetch_all().rows()
        out["pruned"][name] = dict(create_ms=create_ms, kernel_ms=ms, rows_passed=st["rows_passed"],
                                   algorithmic_bytes=st["algorithmic_bytes"], result=got,
                                   zone_stats=q.zone_stats() if hasattr(q, "zone_stats") else None)
        q.close()
    out["device_bytes"] = t.device_bytes()
    return out


def child(args, leg, root):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--root", root,
                        "--rows", str(args.rows)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("%s leg of %s failed (%d): %s" % (leg, root, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def bench_once(root):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       cwd=root, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("bench.py of %s failed (%d): %s" % (root, p.returncode, p.stderr[-2000:]))
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            return dict(ms_per_step=r.get("ms_per_step"), kernel_ms=r.get("kernel_ms"))
    raise RuntimeError("bench.py printed no result line")


def summarize(res, rows):
    here = [r["here"] for r in res["reps"]]
    par = [r["parent"] for r in res["reps"]]
    s = {}
    if res.get("bench"):
        pb = [b["parent"]["ms_per_step"] for b in res["bench"]]
        hb = [b["here"]["ms_per_step"] for b in res["bench"]]
        s["bench"] = dict(parent_ms_per_step=pb, here_ms_per_step=hb, parent_min=min(pb), here_min=min(hb),
                          ratio=min(hb) / min(pb), gate="met" if min(hb) <= 1.05 * min(pb) else "MISSED")
    if not here:
        return s
    pm = [min(x["config3"]["kernel_ms"]) for x in par]
    hm = [min(x["config3"]["kernel_ms"]) for x in here]
    spread = max(pm) - min(pm)
    s["config3"] = dict(parent_min_ms=min(pm), parent_spread_ms=spread, here_min_ms=min(hm),
                        here_spread_ms=max(hm) - min(hm),
                        gate="met" if min(hm) <= min(pm) + spread else "MISSED",
                        first_query_ms_parent=min(x["config3"]["first_create_execute_ms"] for x in par),
                        first_query_ms_here=min(x["config3"]["first_create_execute_ms"] for x in here),
                        later_query_ms_parent=min(x["config3"]["later_create_execute_ms"] for x in par),
                        later_query_ms_here=min(x["config3"]["later_create_execute_ms"] for x in here),
                        zone_stats=here[0]["config3"]["zone_stats"])
    s["pruned"] = {}
    for name in FRACTIONS:
        pm = [min(x["pruned"][name]["kernel_ms"]) for x in par]
        hm = [min(x["pruned"][name]["kernel_ms"]) for x in here]
        zs = here[0]["pruned"][name]["zone_stats"]
        kept = (zs["tiles_total"] - zs["tiles_skipped"]) / max(zs["tiles_total"], 1)
        spread = max(pm) - min(pm)
        t_select = res.get("k_zone_select_ms") or 0.0
        bound = min(pm) * kept + t_select + spread
        read_bytes = here[0]["pruned"][name]["algorithmic_bytes"] * kept
        s["pruned"][name] = dict(
            T_p_ms=min(pm), T_p_spread_ms=spread, kernel_ms=min(hm), tiles_kept_fraction=kept,
            zone_stats=zs, k_zone_select_ms=t_select, bound_ms=bound,
            gate="met" if min(hm) <= bound else "MISSED",
            TBps_over_tiles_read=read_bytes / (min(hm) * 1e9) if kept else None,
            parent_TBps=par[0]["pruned"][name]["algorithmic_bytes"] / (min(pm) * 1e9),
            create_ms=min(x["pruned"][name]["create_ms"] for x in here),
            same_result=all(x["pruned"][name]["result"] == par[0]["pruned"][name]["result"]
                            for x in here + par))
    return s


def rocprof(args):
    import tempfile
    d = args.rocprof_dir or tempfile.mkdtemp(prefix="zone_maps_rocprof_")
    os.makedirs(d, exist_ok=True)
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "zone_maps",
                        "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                        "--leg", "queries", "--root", HERE, "--rows", str(args.rows)],
                       capture_output=True, text=True, timeout=900)
    stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
    text = open(stats[0]).read() if stats else ""
    select_ms = None
    import csv
    for f in csv.reader(text.splitlines()):  # Name, Calls, TotalDurationNs, AverageNs, ...
        if f and "k_zone_select" in f[0]:
            select_ms = float(f[3]) / 1e6
    return dict(rc=p.returncode, kernel_stats_csv=text, k_zone_select_ms=select_ms,
                stderr=p.stderr[-500:] if p.returncode else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--no-queries", action="store_true", help="only the bench.py alternation")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-dir", default=None, help="where rocprofv3 writes (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(dict(queries=leg_queries)[args.leg](os.path.abspath(args.root), args.rows)))
        return
    if not args.parent_root:
        ap.error("--parent-root is required")
    parent = os.path.abspath(args.parent_root)
    res = dict(rows=args.rows, reps=[], bench=[])

    def save():
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    for i in range(0 if args.no_queries else args.reps):
        res["reps"].append(dict(parent=child(args, "queries", parent), here=child(args, "queries", HERE)))
        print("rep %d done" % i, flush=True)
        save()
    if args.rocprof:
        res["rocprof"] = rocprof(args)
        res["k_zone_select_ms"] = res["rocprof"]["k_zone_select_ms"]
        print("rocprof done", flush=True)
        save()
    if args.bench:
        for i in range(args.reps):
            res["bench"].append(dict(parent=bench_once(parent), here=bench_once(HERE)))
            print("bench rep %d done" % i, flush=True)
            save()
    res["summary"] = summarize(res, args.rows)
    save()
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    main()
