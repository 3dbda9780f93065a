#!/usr/bin/env python3
"""ORDER BY over a large GROUP BY result measured against the parent commit.
Scratch: a measurement protocol, not a product tool.

Workload: config 4's table and grouping (--rows rows, --groups distinct u64 keys; select
u, sum(a), count(1), sum(v) group by u).  Cases, each timed from the first next_batch to the
last row (the first call fetches, orders and packs):

  count_desc_key   ORDER BY count(1) DESC, u           no LIMIT
  fsum_key         ORDER BY sum(v), u                  no LIMIT
  deep_limit       ORDER BY count(1) DESC, u LIMIT 100 OFFSET 0.9 * groups
  unordered        no ORDER BY: the fetch + drain that 6k measured (fetch_results is shared)

Every tree runs in fresh child processes with the python package and library of its own tree,
parent and this tree alternating, --procs processes per tree.  A child generates the table,
and per case executes and drains once to warm up, then --reps times.  A child stops adding
repetitions to a case once it has spent --budget-s seconds on it (never fewer than two; the
figure then says how many ran).  Figures per tree and case: every run of every process,
median, minimum, maximum.  Done means: median(parent) - median(here) > the parent's range for
the ordered cases; the unordered median of this tree inside the parent's range.

--parent-root is a checkout of the parent commit with its library built.  Results go to --out
(profiles/order_sort_measure.json).

usage: order_sort.py --parent-root DIR [--rows N] [--groups N] [--reps 3] [--procs 2]
                     [--budget-s 150] [--host-variant] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_TIMEOUT = 900
CASES = ("count_desc_key", "fsum_key", "deep_limit", "unordered")


def child(root, rows, groups, reps, budget_s, cases):
    sys.path.insert(0, root)
    import torch  # noqa: F401  (loads the HIP runtime first)
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    from eventql_amd.plan import Order
    ctx = E.Context(0)
    t = ctx.generate(rows, "uav", u_mod=groups)
    plan = B.config4(groups_hint=groups)
    orders = dict(count_desc_key=dict(specs=[(2, True), (0, False)]),
                  fsum_key=dict(specs=[(3, False), (0, False)]),
                  deep_limit=dict(specs=[(2, True), (0, False)], limit=100, offset=groups * 9 // 10),
                  unordered=None)
    pc = time.perf_counter
    out = {}
    for case in cases:
        q = t.query(plan)
        if orders[case] is not None:
            q.set_order(Order(plan, **orders[case]))
        drains, executes, nrows, nbytes = [], [], 0, 0
        started = pc()
        for rep in range(reps + 1):
            if rep > 2 and pc() - started > budget_s:
                break
            t0 = pc()
            q.execute()
            t1 = pc()
            nrows = nbytes = 0
            while True:
                n, raw = q.next_batch(1024)
                if n == 0:
                    break
                nrows += n
                nbytes += sum(len(r) for r in raw)
            t2 = pc()
            if rep:  # (the first repetition warms up: kernel cache, pinned buffers)
                executes.append((t1 - t0) * 1e3)
                drains.append((t2 - t1) * 1e3)
        r = dict(drain_ms=drains, execute_ms=executes, rows=nrows, bytes=nbytes,
                 num_groups=q.stats()["num_groups"])
        if hasattr(q, "order_stats"):
            r["order_stats"] = q.order_stats()
        if hasattr(q, "emit_stats"):
            r["emit_stats"] = q.emit_stats()
        out[case] = r
        print("# %s %s" % (case, json.dumps(r)), file=sys.stderr, flush=True)
        q.close()
    print(json.dumps(out))


def run_child(root, args, env_extra=None):
    env = dict(os.environ)
    env.pop("EVQL_ORDER_DEVICE_SORT", None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--rows", str(args.rows),
           "--groups", str(args.groups), "--reps", str(args.reps), "--budget-s", str(args.budget_s),
           "--cases", args.cases]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("child of %s failed (%d): %s" % (root, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--groups", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--budget-s", type=float, default=150.0)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--parent-root")
    ap.add_argument("--host-variant", action="store_true",
                    help="also this tree under EVQL_ORDER_DEVICE_SORT=0")
    ap.add_argument("--box", default="", help="which machine the numbers come from")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "order_sort_measure.json"))
    args = ap.parse_args()
    cases = args.cases.split(",")
    if args.child:
        return child(args.child, args.rows, args.groups, args.reps, args.budget_s, cases)
    if not args.parent_root:
        ap.error("--parent-root is required")
    parent = os.path.abspath(args.parent_root)
    res = dict(box=args.box, rows=args.rows, groups=args.groups, reps=args.reps, procs=args.procs,
               timed="first next_batch(1024) to the last row, ms", runs={}, summary={})
    variants = [("parent", parent, None), ("here", HERE, None)]
    if args.host_variant:
        variants.append(("here_host_sort", HERE, {"EVQL_ORDER_DEVICE_SORT": "0"}))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for i in range(args.procs):
        for tag, root, env in variants:
            r = run_child(root, args, env)
            res["runs"].setdefault(tag, []).append(r)
            for case in cases:
                print("proc %d %-15s %-15s drain ms %s rows %d" % (
                    i, tag, case, ["%.1f" % v for v in r[case]["drain_ms"]], r[case]["rows"]), flush=True)
            save()
    for case in cases:
        s = {}
        for tag, runs in res["runs"].items():
            v = [x for r in runs for x in r[case]["drain_ms"]]
            s[tag] = dict(n=len(v), median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                          range_ms=max(v) - min(v), rows=runs[-1][case]["rows"])
            for k in ("order_stats", "emit_stats"):
                if k in runs[-1][case]:
                    s[tag][k] = runs[-1][case][k]
        gain = s["parent"]["median_ms"] - s["here"]["median_ms"]
        s["gain_ms"] = gain
        s["speedup"] = s["parent"]["median_ms"] / s["here"]["median_ms"]
        if case == "unordered":
            inside = s["parent"]["min_ms"] <= s["here"]["median_ms"] <= s["parent"]["max_ms"]
            s["gate"] = "met" if inside or gain > 0 else "MISSED"
        else:
            s["gate"] = "met" if gain > s["parent"]["range_ms"] else "MISSED"
        res["summary"][case] = s
    save()
    print(json.dumps(res["summary"], indent=1), flush=True)


if __name__ == "__main__":
    main()
