#!/usr/bin/env python3
"""The staging tile loop of the fused scan measured against the parent
commit.  The protocol of scan_prefetch.py:

  the metric workload
    `bench.py --steps 20 --warmup 3` (config 3, 1e9 rows): --reps (default 5) pairs, the
    parent and this tree alternating, each run in a fresh child process under its own
    timeout.  Gate, for ms_per_step and roofline.kernel_ms: the median here lies below the
    parent's median by MORE than twice the parent's spread, and the two ranges do not overlap.
    --switch adds a third arm to every pair: this tree under EVQL_SCAN_STAGE=0 (the
    prefetching loop as the parent has it), recorded as `here_off`.

  nothing may get slower
    config2, config2 --k-bits 10, config3l, config4, config4s, config5, config5w:
    --other-reps (default 3) alternating pairs each.  Gate: minimum here <= the parent's
    minimum + the parent's spread.  --skew: the same gate on the kernel time of config 3's
    query over 2e8 rows (narrow copies, float32 `v`): with the literals of WHERE moved so that
    about 100 %, 50 %, 25 % and 1 % of the rows pass, and at 25 % with one group, one dominant
    key (90 %) and input sorted by key.

  where the time goes
    --rocprof   one `rocprofv3 --kernel-trace --stats` run of `bench.py --steps 10 --warmup 2`
                per tree -> <--profiles-dir>/scan_stage_kernel_stats_{parent,here}.csv
    --pmc       one SQ-counter pass per tree (no tracing flag, a run of its own): of
                evql_scan_agg, SQ_WAIT_ANY / SQ_WAVE_CYCLES and the per-SIMD VALU utilisation
                SQ_ACTIVE_INST_VALU x W / SQ_WAVE_CYCLES, W = resident waves per SIMD
                -> <--profiles-dir>/scan_stage_sq_counters.txt

  results
    --outputs   `bench.py --dump-outputs` at the timed size on both trees, fast and exact
                float sums: every array compared bit for bit (fast sums also within 1e-6)

--parent-root is a checkout of the parent commit with its library built; its bench.py runs
with ITS python package.  Every run is a process of its own under its own timeout; the first
one that fails ends the script.

usage: scan_stage.py --parent-root DIR [--reps R] [--other-reps R] [--only W[,W..]]
                     [--skip-metric] [--switch] [--rocprof] [--pmc] [--skew] [--outputs]
                     [--profiles-dir DIR] [--out FILE]"""
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
from narrow_float import CHILD_TIMEOUT, OTHERS, figures, summarize  # noqa: E402

SQ = ["SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU"]
SKEW_ROWS = 200_000_000
OFF = {"EVQL_SCAN_STAGE": "0"}


def bench_once(root, extra=(), steps=20, warmup=3, env=None):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)] + list(extra), cwd=root, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT, env=dict(os.environ, **(env or {})))
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


def rocprof(root, tag, profiles_dir, pmc):
    d = tempfile.mkdtemp(prefix="scan_stage_rocprof_")
    try:
        flags = ["--pmc"] + SQ if pmc else ["--kernel-trace", "--stats"]
        steps = ["--steps", "2", "--warmup", "1"] if pmc else ["--steps", "10", "--warmup", "2"]
        p = subprocess.run(["rocprofv3"] + flags + ["-d", d, "-o", "scan_stage", "--output-format",
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
                dst = os.path.join(profiles_dir, "scan_stage_kernel_stats_%s.csv" % tag)
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


def child_main(root):
    """selectivity and skew: config 3's query over 2e8 rows, a, b < 65536 and a float32-exact v,
    so that the table keeps all four copies.  The literals of `a > A AND b < B` are data of the
    launch: every case runs the one kernel."""
    sys.path.insert(0, root)
    import torch
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    from eventql_amd.plan import Plan, col, count, sum_
    ctx = E.Context(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    n = SKEW_ROWS
    rnd = lambda top: torch.randint(0, top, (n,), generator=g, device="cuda", dtype=torch.int64)
    keys = {
        "spread_1000": lambda: rnd(1000),
        "one_group": lambda: torch.full((n,), 7, device="cuda", dtype=torch.int64),
        "dominant_90": lambda: torch.where(torch.rand(n, generator=g, device="cuda") < 0.9, 7, rnd(1000)),
        "sorted_by_key": lambda: torch.sort(rnd(1000))[0],
    }
    # a in [1, 65536): `a > 0` passes every row
    a, b = rnd(65535) + 1, rnd(65536)
    v = rnd(1 << 24).to(torch.float64) / 1024.0
    cols = [c for c in B.PLAIN_COLUMNS if c["name"] in "kabv"]

    def plan(lo, hi):
        k_, a_, b_, v_ = [col(x) for x in "kabv"]
        return Plan(B.SCHEMA, select=[k_, sum_(v_), count(1), sum_(b_)], group_by=[k_],
                    where=(a_ > lo) & (b_ < hi), groups_hint=1000)

    # name -> (a > lo, b < hi): the share of the rows that pass
    select = {"pass_100": (0, 65536), "pass_50": (0, 32768), "pass_25": (30000, 30000), "pass_1": (58982, 6554)}
    out = {}
    for name, make in keys.items():
        k = make()
        torch.cuda.synchronize()
        t = ctx.table_from_device_columns(
            cols, {"k": k.data_ptr(), "a": a.data_ptr(), "b": b.data_ptr(), "v": v.data_ptr()}, None, n)
        torch.cuda.synchronize()
        for sname, (lo, hi) in select.items() if name == "spread_1000" else [(name, select["pass_25"])]:
            q = t.query(plan(lo, hi))
            for _ in range(3):
                q.launch()
                q.finish()
            ms = []
            for _ in range(5):
                q.launch()
                q.finish()
                ms.append(q.stats()["kernel_ms"])
            out[sname] = ms
            out.setdefault("stage_in_text", "evql_stage_ring" in q.kernel_source())
            q.close()
        t.close()
        del k
    print(json.dumps(out), flush=True)


def outputs(parent):
    """--dump-outputs on both trees, fast and exact sums"""
    import numpy as np
    res = {}
    for mode in ("fast", "exact"):
        dirs = {}
        for tag, root in (("parent", parent), ("here", HERE)):
            dirs[tag] = tempfile.mkdtemp(prefix="scan_stage_out_")
            bench_once(root, ["--dump-outputs", dirs[tag], "--float-sums", mode], steps=2, warmup=1)
        names = sorted(os.path.basename(f) for f in glob.glob(dirs["parent"] + "/*.npy"))
        assert names and names == sorted(os.path.basename(f) for f in glob.glob(dirs["here"] + "/*.npy"))
        cmp = {}
        for nme in names:
            x, y = np.load(os.path.join(dirs["parent"], nme)), np.load(os.path.join(dirs["here"], nme))
            equal = x.shape == y.shape and x.tobytes() == y.tobytes()
            rel = 0.0
            if not equal and x.shape == y.shape and x.dtype.kind == "f":
                rel = float(np.max(np.abs(x - y) / np.maximum(np.abs(x), 1e-300)))
            cmp[nme] = dict(bit_equal=bool(equal), max_rel=rel)
        res[mode] = cmp
        for d in dirs.values():
            shutil.rmtree(d, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--other-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of the other workloads")
    ap.add_argument("--skip-metric", action="store_true")
    ap.add_argument("--switch", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--profiles-dir", default=os.path.join(HERE, "profiles"))
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "scan_stage_measure.json"))
    args = ap.parse_args()
    parent = os.path.abspath(args.parent_root)
    if args.child:
        return child_main(parent)
    res = dict(metric=[], others={}, profiles={})
    if os.path.exists(args.out):  # a later call adds to what an earlier one measured
        with open(args.out) as f:
            res = json.load(f)
        res.pop("summary", None)
    trees = (("parent", parent), ("here", HERE))

    def save():
        res["summary"] = summarize(res)
        off = figures([dict(parent=p["parent"], here=p["here_off"]) for p in res["metric"] if "here_off" in p],
                      "ms_per_step") if res["metric"] else None
        if off:
            res["summary"]["config3_switch_off_ms_per_step"] = off["here"]
        sk = res["profiles"].get("skew", [])
        if sk:
            res["summary"]["skew"] = {}
            for name in [n for n in sk[0]["parent"] if n != "stage_in_text"]:
                par = [min(p["parent"][name]) for p in sk]
                here = [min(p["here"][name]) for p in sk]
                spread = max(max(p["parent"][name]) for p in sk) - min(par)
                res["summary"]["skew"][name] = dict(
                    parent_min=min(par), here_min=min(here), parent_spread=spread,
                    gate="met" if min(here) <= min(par) + spread else "MISSED")
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    for i in range(0 if args.skip_metric else args.reps):
        pair = dict(parent=bench_once(parent), here=bench_once(HERE))
        if args.switch:
            pair["here_off"] = bench_once(HERE, env=OFF)
        res["metric"].append(pair)
        print("config3 rep %d: %s" % (i, json.dumps({k: {x: y for x, y in v.items() if x != "line"}
                                                     for k, v in pair.items()})), flush=True)
        save()
    for flag, key, run in (
            (args.rocprof, "kernel_stats_", lambda tag, root: rocprof(root, tag, args.profiles_dir, False)),
            (args.pmc, "sq_", lambda tag, root: rocprof(root, tag, None, True))):
        for tag, root in trees if flag else []:
            res["profiles"][key + tag] = run(tag, root)
            print("%s%s done" % (key, tag), flush=True)
            save()
    if args.pmc:
        with open(os.path.join(args.profiles_dir, "scan_stage_sq_counters.txt"), "w") as f:
            f.write("evql_scan_agg, config 3 (1e9 rows), one SQ-counter pass per tree, mean per dispatch\n")
            for tag, _ in trees:
                r = res["profiles"]["sq_" + tag]
                f.write("\n[%s] dispatches %d, workgroup %d\n" % (tag, r.get("dispatches", 0),
                                                                 r.get("workgroup_size", 0)))
                for n in SQ:
                    f.write("  %-22s %.6g  (%.1f %% of wave cycles)\n" % (
                        n, r["raw_mean_per_dispatch"].get(n, 0.0),
                        100.0 * r.get("share_of_wave_cycles", {}).get(n, 0.0)))
                f.write("  per-SIMD VALU utilisation  %.1f %%\n" % (100.0 * r.get("valu_utilisation_per_simd", 0.0)))
                f.write("  per-SIMD issue (ANY)       %.2f\n" % r.get("issue_utilisation_per_simd", 0.0))
    if args.outputs:
        res["profiles"]["outputs"] = outputs(parent)
        print("outputs: %s" % json.dumps(res["profiles"]["outputs"]), flush=True)
        save()
    if args.skew:
        res["profiles"].setdefault("skew", []).append({tag: child(root, "skew") for tag, root in trees})
        print("skew: %s" % json.dumps(res["profiles"]["skew"][-1]), flush=True)
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
