#!/usr/bin/env python3
"""The tail of a group-by step measured against the parent commit.

  --phases    config 3 at 1e9 rows: host time of launch, finish, the first and the second
              next_batch of a step and kernel_ms, averaged over 30 steps, --reps (default 3)
              fresh child processes per tree, parent and this tree alternating; this tree
              also with EVQL_EAGER_TAIL=records (the eager block, result columns packed by
              the row interpreter) and EVQL_EAGER_TAIL=0 (the lazy tail)
  --trace     one `rocprofv3 --hip-trace --kernel-trace` run of `bench.py --steps 10
              --warmup 2` per tree (runtime tracing only, no counters): HIP API calls and
              kernels per steady-state step, host duration of the blocking calls.  A step is
              what lies between two launches of the fused scan kernel, the only kernel
              launched with hipModuleLaunchKernel.
  --metric    `bench.py --steps 20 --warmup 3`, --metric-reps (default 5) alternating pairs of
              fresh processes.  Gate: the ms_per_step ranges of the two trees do not overlap
              AND the medians differ by at least the parent's spread (max - min);
              roofline.kernel_ms stays within the parent's spread.
  --others    config2, config2 --k-bits 10, config3l, config4, config4s, config5, config5w:
              --other-reps (default 3) alternating pairs.  Gate: min here <= parent min +
              parent spread.
  --outputs   bench.py --dump-outputs at the timed size on both trees: k, count, sum_b and
              num_rows equal; sum_v no further from the parent than two runs of the parent
              from each other; with --float-sums exact every column bit-equal.

--parent-root is a checkout of the parent commit with its library built; its bench.py runs
with ITS python package.  Results are added to --out (profiles/step_tail_measure.json).

usage: step_tail.py --parent-root DIR [--phases] [--trace] [--metric] [--others] [--outputs]
                    [--only W[,W..]] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OTHERS = {
    "config2": ["--workload", "config2"],
    "config2-k10": ["--workload", "config2", "--k-bits", "10"],
    "config3l": ["--workload", "config3l"],
    "config4": ["--workload", "config4"],
    "config4s": ["--workload", "config4s"],
    "config5": ["--workload", "config5"],
    "config5w": ["--workload", "config5w"],
}
CHILD_TIMEOUT = 420  # seconds: table generation + narrow copies + the steps, with room


# ---- --phases: runs in a child process, with the package of the tree in `root` ----------
def child_phases(root, rows, steps):
    sys.path.insert(0, root)
    import torch  # noqa: F401  (loads the HIP runtime first)
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    ctx = E.Context(0)
    t = ctx.generate(rows, "kabv")
    q = t.query(B.config3())
    for _ in range(3):
        q.launch()
        q.finish()
        while q.next_batch(1024)[0]:
            pass
    acc = dict(launch=0.0, finish=0.0, next_batch_1=0.0, next_batch_2=0.0, step=0.0, kernel_ms=0.0)
    pc = time.perf_counter
    for _ in range(steps):
        t0 = pc()
        q.launch()
        t1 = pc()
        q.finish()
        t2 = pc()
        n1 = q.next_batch(1024)[0]
        t3 = pc()
        n2 = q.next_batch(1024)[0]
        t4 = pc()
        assert n1 == 1000 and n2 == 0, (n1, n2)
        acc["launch"] += t1 - t0
        acc["finish"] += t2 - t1
        acc["next_batch_1"] += t3 - t2
        acc["next_batch_2"] += t4 - t3
        acc["step"] += t4 - t0
        acc["kernel_ms"] += q.stats()["kernel_ms"] * 1e-3
    out = {k: v / steps * 1e3 for k, v in acc.items()}  # ms
    out["n_kernel_launches"] = q.stats()["n_kernel_launches"]
    print(json.dumps(out))


def phases_once(root, mode, rows, steps):
    env = dict(os.environ)
    env.pop("EVQL_EAGER_TAIL", None)
    if mode:
        env["EVQL_EAGER_TAIL"] = mode
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-phases", root, "--rows",
                        str(rows), "--steps", str(steps)], cwd=root, env=env, capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("phases child of %s failed (%d): %s" % (root, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


# ---- bench.py in a fresh process ---------------------------------------------------------
def bench_once(root, extra=(), steps=20, warmup=3):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)] + list(extra), cwd=root, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("bench.py %s of %s failed (%d): %s" % (" ".join(extra), root, p.returncode,
                                                                 p.stderr[-2000:]))
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            return dict(ms_per_step=r.get("ms_per_step"),
                        kernel_ms=(r.get("roofline") or {}).get("kernel_ms"), value=r.get("value"))
    raise RuntimeError("bench.py printed no result line")


def figures(pairs, key):
    par = [p["parent"][key] for p in pairs if p["parent"].get(key) is not None]
    here = [p["here"][key] for p in pairs if p["here"].get(key) is not None]
    if not par or not here:
        return None
    return dict(parent=par, here=here, parent_min=min(par), here_min=min(here),
                parent_max=max(par), here_max=max(here),
                parent_median=statistics.median(par), here_median=statistics.median(here),
                parent_spread=max(par) - min(par), here_spread=max(here) - min(here))


def summarize(res):
    s = {}
    if res.get("metric"):
        ms = figures(res["metric"], "ms_per_step")
        ms["gain_of_medians"] = ms["parent_median"] - ms["here_median"]
        apart = ms["here_max"] < ms["parent_min"]
        ms["ranges_overlap"] = not apart
        ms["gate"] = "met" if apart and ms["gain_of_medians"] >= ms["parent_spread"] else "MISSED"
        km = figures(res["metric"], "kernel_ms")
        km["median_shift"] = km["here_median"] - km["parent_median"]
        km["gate"] = "met" if abs(km["median_shift"]) <= km["parent_spread"] else "MISSED"
        s["config3"] = dict(ms_per_step=ms, kernel_ms=km)
    if res.get("phases"):
        ph = {}
        for tag, runs in res["phases"].items():
            ph[tag] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        s["phases_median_ms"] = ph
    s["others"] = {}
    for name, pairs in (res.get("others") or {}).items():
        f = figures(pairs, "ms_per_step")
        f["gate"] = "met" if f["here_min"] <= f["parent_min"] + f["parent_spread"] else "MISSED"
        s["others"][name] = f
    return s


# ---- --trace -------------------------------------------------------------------------------
def read_rows(d, pattern):
    rows = []
    for f in glob.glob(d + "/**/*" + pattern, recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    return rows


def trace(root, tag, profiles_dir):
    d = tempfile.mkdtemp(prefix="step_tail_trace_")
    try:
        p = subprocess.run(["rocprofv3", "--hip-trace", "--kernel-trace", "-d", d, "-o", "step_tail",
                            "--output-format", "csv", "--", sys.executable, "bench.py", "--gpus", "1",
                            "--steps", "10", "--warmup", "2"], cwd=root, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT + 180)
        out = dict(rc=p.returncode, stderr=p.stderr[-500:] if p.returncode else "")
        api = read_rows(d, "hip_api_trace.csv")
        ker = read_rows(d, "kernel_trace.csv")
        ts = lambda r, k: int(r[k])  # noqa: E731
        launches = sorted(ts(r, "Start_Timestamp") for r in api if r["Function"] == "hipModuleLaunchKernel")
        if len(launches) < 11:
            out["error"] = "%d scan launches in the trace" % len(launches)
            return out
        # 9 whole steps: from the 10th-last launch of the scan kernel to the last
        lo, hi, nsteps = launches[-10], launches[-1], 9
        calls = {}
        for r in api:
            if lo <= ts(r, "Start_Timestamp") < hi:
                c = calls.setdefault(r["Function"], [0, 0])
                c[0] += 1
                c[1] += ts(r, "End_Timestamp") - ts(r, "Start_Timestamp")
        out["api_per_step"] = {f: dict(calls=c[0] / nsteps, host_us_per_step=c[1] / nsteps / 1e3,
                                       host_us_per_call=c[1] / c[0] / 1e3)
                               for f, c in sorted(calls.items())}
        scans = sorted(ts(r, "Start_Timestamp") for r in ker if "evql_scan_agg" in r["Kernel_Name"])
        klo, khi = scans[-10], scans[-1]
        kernels = {}
        for r in ker:
            if klo <= ts(r, "Start_Timestamp") < khi:
                # evql::(anonymous namespace)::k_table_tail(evql::TableTailArgs) -> k_table_tail
                m = re.search(r"(\w+)\(", r["Kernel_Name"])
                name = m.group(1) if m else r["Kernel_Name"]
                c = kernels.setdefault(name, [0, 0])
                c[0] += 1
                c[1] += ts(r, "End_Timestamp") - ts(r, "Start_Timestamp")
        out["kernels_per_step"] = {k: dict(dispatches=c[0] / nsteps, gpu_us_per_step=c[1] / nsteps / 1e3)
                                   for k, c in sorted(kernels.items())}
        if profiles_dir:
            for what, table, cols in (("api", out["api_per_step"], ("calls", "host_us_per_step", "host_us_per_call")),
                                      ("kernels", out["kernels_per_step"], ("dispatches", "gpu_us_per_step"))):
                dst = os.path.join(profiles_dir, "step_tail_%s_per_step_%s.csv" % (what, tag))
                with open(dst, "w") as fh:
                    fh.write("name," + ",".join(cols) + "\n")
                    for name, row in table.items():
                        fh.write(name + "," + ",".join("%.3f" % row[c] for c in cols) + "\n")
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ---- --outputs -----------------------------------------------------------------------------
def dump(root, dirname, exact):
    extra = ["--dump-outputs", dirname] + (["--float-sums", "exact"] if exact else [])
    bench_once(root, extra, steps=3, warmup=1)


def outputs(parent):
    import numpy as np
    base = tempfile.mkdtemp(prefix="step_tail_out_")
    try:
        load = lambda d: {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(d + "/*.npy")}  # noqa: E731
        runs = {}
        for tag, root, exact in (("parent_a", parent, False), ("parent_b", parent, False),
                                 ("here", HERE, False), ("parent_exact", parent, True),
                                 ("here_exact", HERE, True)):
            d = os.path.join(base, tag)
            dump(root, d, exact)
            runs[tag] = load(d)
            print("outputs %s done" % tag, flush=True)
        out = {}
        for c in ("k", "count", "sum_b", "num_rows"):
            out[c + "_equal"] = bool(np.array_equal(runs["parent_a"][c], runs["here"][c]))
        pp = float(np.max(np.abs(runs["parent_a"]["sum_v"] - runs["parent_b"]["sum_v"])))
        ph = float(np.max(np.abs(runs["parent_a"]["sum_v"] - runs["here"]["sum_v"])))
        out["sum_v_max_abs_diff_parent_vs_parent"] = pp
        out["sum_v_max_abs_diff_parent_vs_here"] = ph
        out["sum_v_rel_parent_vs_here"] = float(np.max(
            np.abs(runs["parent_a"]["sum_v"] - runs["here"]["sum_v"]) / np.abs(runs["parent_a"]["sum_v"])))
        out["sum_v_gate"] = "met" if ph <= pp else "MISSED"
        out["exact_bit_equal"] = {c: bool(np.array_equal(runs["parent_exact"][c].view(np.uint64),
                                                         runs["here_exact"][c].view(np.uint64)))
                                  for c in sorted(runs["parent_exact"])}
        return out
    finally:
        shutil.rmtree(base, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child-phases", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--parent-root")
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--metric", action="store_true")
    ap.add_argument("--others", action="store_true")
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--metric-reps", type=int, default=5)
    ap.add_argument("--other-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of the other workloads")
    ap.add_argument("--profiles-dir", default=os.path.join(HERE, "profiles"))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "step_tail_measure.json"))
    args = ap.parse_args()
    if args.child_phases:
        return child_phases(args.child_phases, args.rows, args.steps)
    if not args.parent_root:
        ap.error("--parent-root is required")
    parent = os.path.abspath(args.parent_root)
    res = dict(phases={}, metric=[], others={}, traces={})
    if os.path.exists(args.out):  # a later call adds to what an earlier one measured
        with open(args.out) as f:
            res = json.load(f)
        res.pop("summary", None)

    def save():
        res["summary"] = summarize(res)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    if args.phases:
        for i in range(args.reps):
            for tag, root, mode in (("parent", parent, None), ("here", HERE, None),
                                    ("here_records", HERE, "records"), ("here_lazy", HERE, "0")):
                res["phases"].setdefault(tag, []).append(phases_once(root, mode, args.rows, args.steps))
                print("phases rep %d %s: %s" % (i, tag, json.dumps(res["phases"][tag][-1])), flush=True)
                save()
    if args.trace:
        for tag, root in (("parent", parent), ("here", HERE)):
            res["traces"][tag] = trace(root, tag, args.profiles_dir)
            print("trace %s done (rc %s)" % (tag, res["traces"][tag].get("rc")), flush=True)
            save()
    for i in range(args.metric_reps if args.metric else 0):
        res["metric"].append(dict(parent=bench_once(parent), here=bench_once(HERE)))
        print("config3 rep %d: %s" % (i, json.dumps(res["metric"][-1])), flush=True)
        save()
    names = [n for n in OTHERS if not args.only or n in args.only.split(",")]
    for name in names if args.others else []:
        for i in range(args.other_reps):
            res["others"].setdefault(name, []).append(
                dict(parent=bench_once(parent, OTHERS[name]), here=bench_once(HERE, OTHERS[name])))
            print("%s rep %d: %s" % (name, i, json.dumps(res["others"][name][-1])), flush=True)
            save()
    if args.outputs:
        res["outputs"] = outputs(parent)
        save()
    save()
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    main()
