#!/usr/bin/env python3
"""The float32 copy of float32-exact FLOAT64 columns measured against the
parent commit.  The protocol of flat_narrow.py:

  the metric workload
    `bench.py --steps 20 --warmup 3` (config 3, 1e9 rows): --reps (default 5) pairs, the
    parent and this tree alternating, each run in a fresh child process under its own
    timeout.  Recorded: ms_per_step and roofline.kernel_ms.  Gate, for both figures: the
    median here lies below the parent's median by MORE than twice the parent's spread (the
    range of its repetitions), and the two ranges do not overlap.

  nothing may get slower
    config2, config2 --k-bits 10, config3l, config4, config4s, config5, config5w:
    --other-reps (default 3) alternating pairs each.  Gate: minimum here <= the parent's
    minimum + the parent's spread.

--parent-root is a checkout of the parent commit with its library built; its bench.py runs
with ITS python package.  --rocprof adds one `rocprofv3 --kernel-trace --stats` run of
`bench.py --steps 10 --warmup 2` per tree and stores the kernel summaries as
<--profiles-dir>/narrow_float_kernel_stats_{parent,here}.csv; --pmc adds one
`rocprofv3 --pmc FETCH_SIZE` run per tree, with no tracing flag, and records the sum of the
counter over the dispatches of evql_scan_agg.  Every run is a process of its own; the first
one that fails ends the script.

usage: narrow_float.py --parent-root DIR [--reps R] [--other-reps R] [--only W[,W..]]
                       [--skip-metric] [--rocprof] [--pmc] [--profiles-dir DIR] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

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
CHILD_TIMEOUT = 420  # seconds: table generation + the copies + 23 steps, with room


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
            roof = r.get("roofline") or {}
            return dict(ms_per_step=r.get("ms_per_step"), kernel_ms=roof.get("kernel_ms"),
                        achieved_GBps=roof.get("achieved_GBps"), value=r.get("value"),
                        algorithmic_bytes=roof.get("algorithmic_bytes"), line=r)
    raise RuntimeError("bench.py printed no result line")


def figures(pairs, key):
    par = [p["parent"][key] for p in pairs if p["parent"].get(key) is not None]
    here = [p["here"][key] for p in pairs if p["here"].get(key) is not None]
    if not par or not here:
        return None
    return dict(parent=par, here=here, parent_min=min(par), here_min=min(here),
                parent_median=statistics.median(par), here_median=statistics.median(here),
                parent_spread=max(par) - min(par), here_spread=max(here) - min(here))


def summarize(res):
    s = {}
    if res["metric"]:
        s["config3"] = {}
        for key in ("ms_per_step", "kernel_ms"):
            f = figures(res["metric"], key)
            if f is None:
                s["config3"][key] = None
                continue
            f["gain"] = f["parent_median"] - f["here_median"]
            apart = max(f["here"]) < min(f["parent"])
            f["gate"] = "met" if f["gain"] > 2 * f["parent_spread"] and apart else "MISSED"
            s["config3"][key] = f
    s["others"] = {}
    for name, pairs in res["others"].items():
        f = figures(pairs, "ms_per_step")
        f["gate"] = "met" if f["here_min"] <= f["parent_min"] + f["parent_spread"] else "MISSED"
        s["others"][name] = f
    return s


def rocprof(root, tag, profiles_dir, pmc):
    d = tempfile.mkdtemp(prefix="narrow_float_rocprof_")
    try:
        flags = ["--pmc", "FETCH_SIZE"] if pmc else ["--kernel-trace", "--stats"]
        p = subprocess.run(["rocprofv3"] + flags + ["-d", d, "-o", "narrow_float", "--output-format",
                            "csv", "--", sys.executable, "bench.py", "--gpus", "1", "--steps", "10",
                            "--warmup", "2"], cwd=root, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT + 180)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run of %s failed (%d): %s" % (root, p.returncode, p.stderr[-2000:]))
        out = {}
        if pmc:
            total, calls = 0.0, 0
            for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                for row in csv.DictReader(open(f)):
                    if "evql_scan_agg" in row.get("Kernel_Name", "") and row.get("Counter_Name") == "FETCH_SIZE":
                        total += float(row["Counter_Value"])
                        calls += 1
            out.update(fetch_size_sum=total, dispatches=calls)
        else:
            stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
            if stats and profiles_dir:
                dst = os.path.join(profiles_dir, "narrow_float_kernel_stats_%s.csv" % tag)
                shutil.copyfile(stats[0], dst)
                out["kernel_stats_csv"] = os.path.basename(dst)
            out["kernel_stats"] = open(stats[0]).read() if stats else ""
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--other-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of the other workloads")
    ap.add_argument("--skip-metric", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--profiles-dir", default=os.path.join(HERE, "profiles"))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "narrow_float_measure.json"))
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_root)
    res = dict(metric=[], others={}, profiles={})
    if os.path.exists(args.out):  # a later call adds to what an earlier one measured
        with open(args.out) as f:
            res = json.load(f)
        res.pop("summary", None)

    def save():
        res["summary"] = summarize(res)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    if args.rocprof:
        for tag, root in (("parent", parent), ("here", HERE)):
            res["profiles"]["kernel_stats_" + tag] = rocprof(root, tag, args.profiles_dir, False)
            print("rocprof %s done" % tag, flush=True)
            save()
    if args.pmc:
        for tag, root in (("parent", parent), ("here", HERE)):
            res["profiles"]["pmc_" + tag] = rocprof(root, tag, None, True)
            print("pmc %s done" % tag, flush=True)
            save()
    for i in range(0 if args.skip_metric else args.reps):
        res["metric"].append(dict(parent=bench_once(parent), here=bench_once(HERE)))
        print("config3 rep %d: %s" % (i, json.dumps({k: {x: y for x, y in v.items() if x != "line"}
                                                     for k, v in res["metric"][-1].items()})), flush=True)
        save()
    names = [n for n in OTHERS if not args.only or n in args.only.split(",")]
    for name in names if args.other_reps else []:
        for i in range(args.other_reps):
            res["others"].setdefault(name, []).append(
                dict(parent=bench_once(parent, OTHERS[name]), here=bench_once(HERE, OTHERS[name])))
            last = res["others"][name][-1]
            print("%s rep %d: parent %s here %s" % (name, i, last["parent"]["ms_per_step"],
                                                    last["here"]["ms_per_step"]), flush=True)
            save()
    save()
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    main()
