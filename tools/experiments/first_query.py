#!/usr/bin/env python3
"""first_query.py -- what the FIRST run of a query costs: evql_query_create + the first
evql_query_execute, wall time, for config 3's query over a 1e7-row table resident in HBM:

  cold          a shape the kernel cache has never seen (empty directory, fresh context):
                text generation + hiprtc + module load + scan
  memory        the same shape with literals it has never seen, same context: the module
                is found among the context's modules
  disk          the same with yet other literals in a fresh context: the code object is
                read from the directory and loaded

`compiles`, `disk_hits` and `memory_hits` are the differences of
evql_ctx_kernel_cache_stats over the case (null where the library has no such call).

--suite runs `pytest -m gpu` once into an EMPTY in-tree kernel cache first (it deletes
eventql_amd/_kcache/*.hsaco) and reports the code objects the run leaves and its wall time.
--root DIR measures the library of another checkout of this repository (for instance the
parent commit), --label names the entry; entries are merged into --out by label.

usage: tools/experiments/first_query.py [--root DIR] [--label NAME] [--suite] [--rows N]
                                        [--out profiles/first_query.json]"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def suite(root):
    cache = os.path.join(root, "eventql_amd", "_kcache")
    for f in glob.glob(cache + "/*.hsaco"):
        os.unlink(f)
    t0 = time.perf_counter()
    rc = subprocess.call([sys.executable, "-m", "pytest", "tests", "-q", "-m", "gpu", "-p",
                          "no:cacheprovider"], cwd=root)
    return dict(exit_code=rc, wall_s=round(time.perf_counter() - t0, 1),
                code_objects=len(glob.glob(cache + "/*.hsaco")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--label", default="this")
    ap.add_argument("--suite", action="store_true")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    out_path = args.out or os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles",
                                        "first_query.json")
    entry = dict(rows=args.rows, query="k, sum(v), count(1), sum(b) WHERE a > L1 AND b < L2 GROUP BY k")
    if args.suite:
        entry["suite"] = suite(root)  # (before this process opens the GPU)

    sys.path.insert(0, root)
    import eventql_amd as E
    from eventql_amd.plan import Plan, col, count, sum_
    from eventql_amd import bench_plans as B

    def plan(l1, l2):
        return Plan(B.SCHEMA, select=[col("k"), sum_(col("v")), count(1), sum_(col("b"))],
                    group_by=[col("k")], where=(col("a") > l1) & (col("b") < l2), groups_hint=1000)

    def counters(ctx):
        if not hasattr(ctx, "kernel_cache_stats"):
            return None
        s = ctx.kernel_cache_stats()
        return dict(compiles=s.compiles, disk_hits=s.disk_hits, memory_hits=s.memory_hits,
                    compile_ms=s.compile_ms)

    def first_run(ctx, t, l1, l2):
        p = plan(l1, l2)
        c0 = counters(ctx)
        ctx.synchronize()
        t0 = time.perf_counter()
        q = t.query(p)
        t1 = time.perf_counter()
        q.execute()
        t2 = time.perf_counter()
        st = q.stats()
        q.close()
        c1 = counters(ctx)
        r = dict(create_ms=(t1 - t0) * 1e3, execute_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3,
                 kernel_ms=st["kernel_ms"], rows_passed=st["rows_passed"])
        for key in ("compiles", "disk_hits", "memory_hits", "compile_ms"):
            r[key] = None if c0 is None else c1[key] - c0[key]
        return r

    E.lib().evql_set_kernel_cache_dir(tempfile.mkdtemp(prefix="first_query_kcache_").encode())
    ctx = E.Context(0)
    t = ctx.generate(args.rows, "kabv")
    ctx.synchronize()
    entry["cold"] = first_run(ctx, t, 30000, 30000)
    mem = [first_run(ctx, t, 30001 + 997 * i, 29999 - 991 * i) for i in range(7)]
    entry["memory"] = dict(runs=mem, min_total_ms=min(r["total_ms"] for r in mem),
                           median_total_ms=statistics.median(r["total_ms"] for r in mem),
                           median_create_ms=statistics.median(r["create_ms"] for r in mem),
                           compiles=None if mem[0]["compiles"] is None else sum(r["compiles"] for r in mem))
    t.close()
    ctx.close()
    ctx = E.Context(0)
    t = ctx.generate(args.rows, "kabv")
    ctx.synchronize()
    entry["disk"] = first_run(ctx, t, 12345, 54321)
    t.close()
    ctx.close()

    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc[args.label] = entry
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.label: entry}))


if __name__ == "__main__":
    main()
