#!/usr/bin/env python3
"""String functions per row measured against the parent commit.

Table: bench_plans.string_key_table, --rows (default 1.25e8) rows of s = "g" + u with
--keys (default 1000) distinct values, a in [0, 65536).  The table has no integer column of
few values, so the second key of the key measurement is the expression `a % 2`.

  WHERE   select count(1) .. where lcase(s) = 'g17'
          yardstick T_w: kernel_ms of `where s = 'g17'` with the PARENT's library
          gate: within T_w + spread
  key     select lcase(s), a % 2, count(1), sum(a) .. group by lcase(s), a % 2
          yardstick T_k: `group by s, a % 2` with the parent's library (the hashed path:
          composite keys have no dictionary)
          allowance T_h: the parent's k_string_hash time over that column, from one
          `rocprofv3 --kernel-trace --stats` run in a process of its own
          gate: at most T_k + T_h + spread

--reps (default 5) repetitions per library, parent and branch alternating, each in a child
process of its own under its own time limit; a figure is the minimum kernel_ms of --execs
executions, the spread the range of the repetitions' minima of the yardstick.  --bench-reps
adds alternating runs of `bench.py --gpus 1 --steps 20 --warmup 3` (config 3) with either
library: its kernels' digests are unchanged, so kernel_ms must be the parent's.

--parent-lib is libevql_mi355x.so built from the parent commit; the python package is the
same for both (the change does not touch it).

usage: strfn.py --parent-lib FILE [--reps R] [--execs E] [--bench-reps R] [--no-rocprof] [--out FILE]"""
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
CHILD_TIMEOUT = 300


def child(args):
    sys.path.insert(0, HERE)
    import eventql_amd as E
    from eventql_amd import bench_plans as B
    from eventql_amd.plan import Plan, Call, col, count, sum_
    ctx = E.Context(0)
    t = B.string_key_table(ctx, args.rows, args.keys, 7)
    S = B.STRING_KEY_SCHEMA
    s, a = col("s"), col("a")
    lc = Call("lcase", s)
    plans = {
        "where_s": Plan(S, select=[count(1)], where=s.eq("g17")),
        "key_s": Plan(S, select=[s, a % 2, count(1), sum_(a)], group_by=[s, a % 2],
                      groups_hint=2 * args.keys),
    }
    if args.child == "here":
        plans["where_lcase"] = Plan(S, select=[count(1)], where=lc.eq("g17"))
        plans["key_lcase"] = Plan(S, select=[lc, a % 2, count(1), sum_(a)], group_by=[lc, a % 2],
                                  groups_hint=2 * args.keys)
    out = {}
    for name, plan in plans.items():
        q = t.query(plan)
        ms = []
        for _ in range(args.execs):
            q.execute()
            ms.append(q.stats()["kernel_ms"])
        res = q.fetch_all()
        out[name] = dict(kernel_ms=min(ms), groups=res.nrows,
                         checksum=int(sum(r[-1] for r in res.rows()) & ((1 << 63) - 1)))
        q.close()
    t.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(which, lib, args, prefix=()):
    env = dict(os.environ)
    if lib:
        env["EVQL_LIB"] = lib
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", which, "--rows",
                          str(args.rows), "--keys", str(args.keys), "--execs", str(args.execs)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise RuntimeError("child %s failed (%d): %s" % (which, p.returncode, p.stderr[-2000:]))
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("child %s printed no result" % which)


def string_hash_ms(args):
    """the parent's k_string_hash over the column: total of its dispatches in one traced run"""
    d = tempfile.mkdtemp(prefix="strfn_rocprof_")
    try:
        a2 = argparse.Namespace(**dict(vars(args), execs=1))
        run_child("parent", args.parent_lib, a2,
                  prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "strfn",
                          "--output-format", "csv", "--"])
        rows = []
        for fn in glob.glob(d + "/**/*kernel_stats.csv", recursive=True):
            rows += [r for r in csv.DictReader(open(fn)) if "k_string_hash" in r.get("Name", "")]
        if not rows:
            return None
        return dict(calls=sum(int(r["Calls"]) for r in rows),
                    total_ms=sum(float(r["TotalDurationNs"]) for r in rows) / 1e6)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def bench_once(lib):
    env = dict(os.environ)
    if lib:
        env["EVQL_LIB"] = lib
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"],
                       cwd=HERE, env=env, capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        raise RuntimeError("bench.py failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    for line in reversed(p.stdout.strip().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            return dict(ms_per_step=r.get("ms_per_step"), kernel_ms=(r.get("roofline") or {}).get("kernel_ms"))
    raise RuntimeError("bench.py printed no result line")


def summarize(res):
    def col_(side, name):
        return [r[side][name]["kernel_ms"] for r in res["reps"] if name in r.get(side, {})]
    s = {}
    if not res["reps"]:
        return s
    tw, tk = col_("parent", "where_s"), col_("parent", "key_s")
    th = (res.get("string_hash") or {}).get("total_ms")
    w, k = col_("here", "where_lcase"), col_("here", "key_lcase")
    s["where"] = dict(T_w=min(tw), spread=max(tw) - min(tw), here=min(w), here_all=w, parent_all=tw,
                      here_where_s=min(col_("here", "where_s")),
                      gate="met" if min(w) <= min(tw) + (max(tw) - min(tw)) else "MISSED")
    s["key"] = dict(T_k=min(tk), spread=max(tk) - min(tk), T_h=th, here=min(k), here_all=k, parent_all=tk,
                    here_key_s=min(col_("here", "key_s")))
    if th is not None:
        s["key"]["gate"] = "met" if min(k) <= min(tk) + th + (max(tk) - min(tk)) else "MISSED"
    if res.get("bench"):
        p = [b["parent"]["kernel_ms"] for b in res["bench"]]
        h = [b["here"]["kernel_ms"] for b in res["bench"]]
        s["config3_kernel_ms"] = dict(parent=p, here=h, parent_min=min(p), here_min=min(h))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=["parent", "here"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=125_000_000)
    ap.add_argument("--keys", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--execs", type=int, default=7)
    ap.add_argument("--bench-reps", type=int, default=2)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "strfn_measure.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    args.parent_lib = os.path.abspath(args.parent_lib)
    res = dict(rows=args.rows, keys=args.keys, execs=args.execs, reps=[], bench=[], string_hash=None)

    def save():
        res["summary"] = summarize(res)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")

    for i in range(args.reps):
        res["reps"].append(dict(parent=run_child("parent", args.parent_lib, args),
                                here=run_child("here", None, args)))
        print("rep %d: %s" % (i, json.dumps(res["reps"][-1])), flush=True)
        save()
    if not args.no_rocprof:
        res["string_hash"] = string_hash_ms(args)
        print("k_string_hash: %s" % json.dumps(res["string_hash"]), flush=True)
        save()
    for i in range(args.bench_reps):
        res["bench"].append(dict(parent=bench_once(args.parent_lib), here=bench_once(None)))
        print("config3 rep %d: %s" % (i, json.dumps(res["bench"][-1])), flush=True)
        save()
    print(json.dumps(res["summary"], indent=1))


if __name__ == "__main__":
    main()
