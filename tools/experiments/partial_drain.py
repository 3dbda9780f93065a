#!/usr/bin/env python3
"""Fetch + drain of a large EVQL_MODE_PARTIAL result measured against the
parent commit.

Workloads: config 4's table and grouping (--rows rows, --groups distinct u64 keys; select
u, sum(a), count(1), sum(v)) and config 4s' string key.  Variants, each in fresh child
processes with the python package and library of its own tree:

  parent_partial   the parent commit, PARTIAL mode (the host row loop)
  here_partial     this tree, PARTIAL mode (rows packed on the device)
  here_final       this tree, FINAL mode: the device-packed drain of the same groups, the
                   yardstick for what device packing costs
  here_partial_host  (--host-variant) this tree with EVQL_PARTIAL_DEVICE_EMIT=0

A child executes once to warm up and drains, then --reps times: execute, then the timed part:
next_batch(1024) until it returns no row (the first call fetches and packs).  Figure of a
process: the minimum of its repetitions; --procs processes per variant; spread = range of
those minima.  Gate: parent minimum - here minimum > the larger spread of the two.

--trace adds one `rocprofv3 --kernel-trace --stats` run (no counters) of here_partial and
reports the device time per kernel of one drain.

--parent-root is a checkout of the parent commit with its library built.  Results go to
--out (profiles/partial_emit_measure.json).

usage: partial_drain.py --parent-root DIR [--rows N] [--groups N] [--reps 5] [--procs 2]
                        [--workloads config4,config4s] [--trace] [--host-variant] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_TIMEOUT = 540


def child(root, workload, mode, rows, groups, reps):
    sys.path.insert(0, root)
    import torch  # noqa: F401  (loads the HIP runtime first)
    import eventql_amd as E
    from eventql_amd import bench_plans as B, capi as K, synth
    ctx = E.Context(0)
    if workload == "config4s":
        t = B.string_key_table(ctx, rows, groups, synth.SEED)
        plan = B.config4s(groups_hint=groups, mode=K.MODE_PARTIAL if mode == "partial" else K.MODE_FINAL)
    else:
        t = ctx.generate(rows, "uav", u_mod=groups)
        plan = B.config4(groups_hint=groups, mode=K.MODE_PARTIAL if mode == "partial" else K.MODE_FINAL)
    q = t.query(plan)
    pc = time.perf_counter
    drains, executes, nrows, nbytes = [], [], 0, 0
    for rep in range(reps + 1):
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
        if rep:  # (the first repetition warms up: kernel cache, dictionaries, pinned buffers)
            executes.append((t1 - t0) * 1e3)
            drains.append((t2 - t1) * 1e3)
    out = dict(drain_ms=drains, execute_ms=executes, rows=nrows, bytes=nbytes,
               kernel_ms=q.stats()["kernel_ms"])
    if hasattr(q, "emit_stats"):
        out["emit_stats"] = q.emit_stats()
    print(json.dumps(out))


def run_child(root, workload, mode, args, env_extra=None, wrap=()):
    env = dict(os.environ)
    env.pop("EVQL_PARTIAL_DEVICE_EMIT", None)
    env.update(env_extra or {})
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", root, "--workload", workload,
                        "--mode", mode, "--rows", str(args.rows), "--groups", str(args.groups),
                        "--reps", str(1 if wrap else args.reps)]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("child %s %s of %s failed (%d): %s" % (workload, mode, root, p.returncode,
                                                                 p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def trace(workload, args):
    """device time per kernel of the packing: one warm-up drain and one timed drain are in
    the trace, so every packing kernel ran twice"""
    d = tempfile.mkdtemp(prefix="partial_drain_trace_")
    try:
        run_child(HERE, workload, "partial", args,
                  wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "partial_drain",
                        "--output-format", "csv", "--"])
        out = {}
        for f in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    name = r.get("Name", "")
                    if not any(k in name for k in ("k_partial", "k_sha1", "k_exclusive_scan",
                                                   "k_extract_word", "k_gather_rows",
                                                   "k_table_compact")):
                        continue
                    calls = int(r["Calls"])
                    # evql::(anonymous namespace)::k_sha1_ranges(...) -> k_sha1_ranges
                    out[re.search(r"\b(k_\w+)", name).group(1)] = dict(
                        calls=calls, ms_per_call=float(r["TotalDurationNs"]) / calls / 1e6)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="config4", help=argparse.SUPPRESS)
    ap.add_argument("--mode", default="partial", help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--groups", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--workloads", default="config4,config4s")
    ap.add_argument("--parent-root")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--host-variant", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--box", default="", help="which machine the numbers come from")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "partial_emit_measure.json"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.workload, args.mode, args.rows, args.groups, args.reps)
    if not args.parent_root:
        ap.error("--parent-root is required")
    parent = os.path.abspath(args.parent_root)
    res = dict(box=args.box, rows=args.rows, groups=args.groups, reps=args.reps, procs=args.procs,
               workloads={})
    variants = [("parent_partial", parent, "partial", None), ("here_partial", HERE, "partial", None),
                ("here_final", HERE, "final", None)]
    if args.host_variant:
        variants.append(("here_partial_host", HERE, "partial", {"EVQL_PARTIAL_DEVICE_EMIT": "0"}))

    def save():
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")

    if args.trace_only:  # adds the kernel split to what an earlier call measured
        with open(args.out) as f:
            res = json.load(f)
        for wl in args.workloads.split(","):
            res["workloads"][wl]["pack_kernels"] = trace(wl, args)
            print(json.dumps({wl: res["workloads"][wl]["pack_kernels"]}, indent=1), flush=True)
            save()
        return
    for wl in args.workloads.split(","):
        w = res["workloads"].setdefault(wl, dict(runs={}))
        for i in range(args.procs):
            for tag, root, mode, env in variants:
                r = run_child(root, wl, mode, args, env)
                w["runs"].setdefault(tag, []).append(r)
                print("%s proc %d %-18s drain min %.1f ms  execute min %.1f ms  rows %d" % (
                    wl, i, tag, min(r["drain_ms"]), min(r["execute_ms"]), r["rows"]), flush=True)
                save()
        s = {}
        for tag, runs in w["runs"].items():
            mins = [min(r["drain_ms"]) for r in runs]
            s[tag] = dict(minima_ms=mins, min_ms=min(mins), spread_ms=max(mins) - min(mins))
        spread = max(s["parent_partial"]["spread_ms"], s["here_partial"]["spread_ms"])
        gain = s["parent_partial"]["min_ms"] - s["here_partial"]["min_ms"]
        s["gain_ms"] = gain
        s["speedup"] = s["parent_partial"]["min_ms"] / s["here_partial"]["min_ms"]
        s["gate"] = "met" if gain > spread else "MISSED"
        es = w["runs"]["here_partial"][-1].get("emit_stats")
        if es:
            s["here_partial_emit_stats"] = es
        w["summary"] = s
        if args.trace:
            w["pack_kernels"] = trace(wl, args)
        save()
        print(json.dumps({wl: w["summary"], "pack_kernels": w.get("pack_kernels")}, indent=1), flush=True)


if __name__ == "__main__":
    main()
