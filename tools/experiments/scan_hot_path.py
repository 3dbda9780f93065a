#!/usr/bin/env python3
"""The per-row instruction work of the fused scan measured against the
parent commit.  The protocol of narrow_float.py:

  the metric workload
    `bench.py --steps 20 --warmup 3` (config 3, 1e9 rows): --reps (default 5) pairs, the
    parent and this tree alternating, each run in a fresh child process under its own
    timeout.  Gate, for ms_per_step and roofline.kernel_ms: the median here lies below the
    parent's median by MORE than twice the parent's spread, and the two ranges do not overlap.

  nothing may get slower
    config2, config2 --k-bits 10, config3l, config4, config4s, config5, config5w:
    --other-reps (default 3) alternating pairs each.  Gate: minimum here <= the parent's
    minimum + the parent's spread.  --skew: the same gate on the kernel time of config 2's
    query under hint 1000 over 2e8 rows with one group, one dominant key (90 %) and input
    sorted by key -- what the lane-private accumulator cache exists for.

  where the time goes
    --rocprof   one `rocprofv3 --kernel-trace --stats` run of `bench.py --steps 10 --warmup 2`
                per tree -> <--profiles-dir>/scan_hot_path_kernel_stats_{parent,here}.csv
    --pmc       one SQ-counter pass per tree (the counters of scripts/pmc_sq.sh, no tracing
                flag, a run of its own).  From the raw values of evql_scan_agg:
                  per-SIMD VALU utilisation = SQ_ACTIVE_INST_VALU x W / SQ_WAVE_CYCLES
                with W = resident waves per SIMD (EVQL_BLOCK / 64 / 4: one workgroup per CU)
    --floor     kernel time of config 3 and of the ungrouped plan over the same table that
                reads the same four columns under the same WHERE (count(1), sum(v), sum(b),
                max(k)): loads + decode + filter + register accumulation, no group table

--parent-root is a checkout of the parent commit with its library built; its bench.py runs
with ITS python package.  --trees parent / here restricts the profile runs to one tree (the
parent's figures are taken before anything changes).  Every run is a process of its own;
the first one that fails ends the script.

usage: scan_hot_path.py --parent-root DIR [--reps R] [--other-reps R] [--only W[,W..]]
                        [--skip-metric] [--rocprof] [--pmc] [--floor] [--skew]
                        [--trees parent,here] [--profiles-dir DIR] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from narrow_float import CHILD_TIMEOUT, OTHERS, bench_once, figures, summarize  # noqa: E402

SQ = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY",
      "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"]
SKEW_ROWS = 200_000_000


def rocprof(root, tag, profiles_dir, pmc):
    d = tempfile.mkdtemp(prefix="scan_hot_path_rocprof_")
    try:
        flags = ["--pmc"] + SQ if pmc else ["--kernel-trace", "--stats"]
        steps = ["--steps", "2", "--warmup", "1"] if pmc else ["--steps", "10", "--warmup", "2"]
        p = subprocess.run(["rocprofv3"] + flags + ["-d", d, "-o", "scan_hot_path", "--output-format",
                            "csv", "--", sys.executable, "bench.py", "--gpus", "1"] + steps,
                           cwd=root, capture_output=True, text=True, timeout=CHILD_TIMEOUT + 180)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 run of %s failed (%d): %s" % (root, p.returncode, p.stderr[-2000:]))
        out = {}
        if pmc:
            vals = {}
            for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Kernel_Name", "").split("(")[0] == "evql_scan_agg":
                        vals.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
                        out["workgroup_size"] = int(float(row.get("Workgroup_Size") or 0))
            raw = {n: sum(v) / len(v) for n, v in vals.items()}
            out.update(raw_mean_per_dispatch=raw, dispatches=len(vals.get("SQ_WAVE_CYCLES", [])))
            wc = raw.get("SQ_WAVE_CYCLES")
            if wc:
                out["share_of_wave_cycles"] = {n: v / wc for n, v in raw.items()}
                waves = (out.get("workgroup_size") or 1024) // 64 // 4
                out["resident_waves_per_simd"] = waves
                out["valu_utilisation_per_simd"] = raw.get("SQ_ACTIVE_INST_VALU", 0.0) * waves / wc
                out["issue_utilisation_per_simd"] = raw.get("SQ_ACTIVE_INST_ANY", 0.0) * waves / wc
        else:
            stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
            if stats and profiles_dir:
                dst = os.path.join(profiles_dir, "scan_hot_path_kernel_stats_%s.csv" % tag)
                shutil.copyfile(stats[0], dst)
                out["kernel_stats_csv"] = os.path.basename(dst)
            out["kernel_stats"] = open(stats[0]).read() if stats else ""
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def child(root, what):
    """one measurement with the package of `root`, in a process of its own"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--parent-root", root],
                       cwd=root, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("%s of %s failed (%d): %s" % (what, root, p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def kernel_times(q, warm=3, reps=10):
    for _ in range(warm):
        q.launch()
        q.finish()
    ms = []
    for _ in range(reps):
        q.launch()
        q.finish()
        ms.append(q.stats()["kernel_ms"])
    return ms


def child_main(root, what):
    sys.path.insert(0, root)
    import eventql_amd as E
    from eventql_amd import bench_plans as B, capi as K
    from eventql_amd.plan import Plan, col, count, max_, sum_
    ctx = E.Context(0)
    out = {}
    if what == "floor":
        t = ctx.generate(1_000_000_000, "kabv")
        floor = Plan(B.SCHEMA, select=[count(1), sum_(col("v")), sum_(col("b")), max_(col("k"))],
                     where=(col("a") > 30000) & (col("b") < 30000))
        for name, plan in (("config3", B.config3()), ("ungrouped", floor), ("config3_again", B.config3())):
            q = t.query(plan)
            out[name] = kernel_times(q)
            q.close()
        t.close()
    else:
        import torch
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        n = SKEW_ROWS
        keys = {
            "one_group": lambda: torch.full((n,), 7, device="cuda", dtype=torch.int64),
            "dominant_90": lambda: torch.where(
                torch.rand(n, generator=g, device="cuda") < 0.9, 7,
                torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int64)),
            "sorted_by_key": lambda: torch.sort(
                torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int64))[0],
        }
        v = (torch.randint(0, 1 << 24, (n,), generator=g, device="cuda", dtype=torch.int64)
             .to(torch.float64) / 1024.0)
        cols = [c for c in B.PLAIN_COLUMNS if c["name"] in "kv"]
        for name, make in keys.items():
            k = make()
            torch.cuda.synchronize()
            t = ctx.table_from_device_columns(cols, {"k": k.data_ptr(), "v": v.data_ptr()}, None, n)
            torch.cuda.synchronize()
            q = t.query(B.config2(groups_hint=1000))
            out[name] = kernel_times(q, reps=5)
            q.close()
            t.close()
            del k
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--other-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of the other workloads")
    ap.add_argument("--skip-metric", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--floor", action="store_true")
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--trees", default="parent,here")
    ap.add_argument("--profiles-dir", default=os.path.join(HERE, "profiles"))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "scan_hot_path_measure.json"))
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_root)
    if args.child:
        return child_main(parent, args.child)
    res = dict(metric=[], others={}, profiles={})
    if os.path.exists(args.out):  # a later call adds to what an earlier one measured
        with open(args.out) as f:
            res = json.load(f)
        res.pop("summary", None)
    trees = [(tag, root) for tag, root in (("parent", parent), ("here", HERE))
             if tag in args.trees.split(",")]

    def save():
        res["summary"] = summarize(res)
        sk = res["profiles"].get("skew", [])
        if sk and all("parent" in p and "here" in p for p in sk):
            res["summary"]["skew"] = {}
            for name in sk[0]["parent"]:
                par = [min(p["parent"][name]) for p in sk]
                here = [min(p["here"][name]) for p in sk]
                spread = max(max(p["parent"][name]) for p in sk) - min(par)
                res["summary"]["skew"][name] = dict(
                    parent_min=min(par), here_min=min(here), parent_spread=spread,
                    gate="met" if min(here) <= min(par) + spread else "MISSED")
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for flag, key, run in (
            (args.rocprof, "kernel_stats_", lambda tag, root: rocprof(root, tag, args.profiles_dir, False)),
            (args.pmc, "sq_", lambda tag, root: rocprof(root, tag, None, True)),
            (args.floor, "floor_", lambda tag, root: child(root, "floor"))):
        for tag, root in trees if flag else []:
            res["profiles"][key + tag] = run(tag, root)
            print("%s%s done" % (key, tag), flush=True)
            save()
    if args.skew:
        res["profiles"].setdefault("skew", []).append({tag: child(root, "skew") for tag, root in trees})
        print("skew: %s" % json.dumps(res["profiles"]["skew"][-1]), flush=True)
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
