#!/usr/bin/env python3
"""The export of a chain head into evql_query_exchange measured against its
yardstick.

One hub rank, a chain of two synthetic files (columns u, a; u uniform in [0, G)) with no
row filter anywhere, `select u, count(1), sum(a) group by u`, for every G of --groups
(default 1e6 and 1e7 groups).  A repetition is

    execute()               both files scanned, their groups merged into d_mtab (chain_merge)
    exchange(GATHER_ALL)    k_mtab_compact over d_mtab, then the rest of the exchange
    execute()               the same merge again: the same table (capacity, words per slot,
                            contents), freshly written
    next_batch(1)           under ORDER BY count desc LIMIT 1: the fetch compacts d_mtab with
                            k_table_compact -- THE YARDSTICK: the kernel as the parent commit
                            has it

Either kernel runs right behind a chain_merge of the same data, so neither finds the table
in a cache the other has warmed.  --reps (default 5) repetitions run in ONE child process
under `rocprofv3 --kernel-trace`; the durations come from its per-dispatch trace: of every
repetition the k_mtab_compact dispatch and the fetch's k_table_compact dispatch (told from
those chain_merge may launch over the files' own tables by their position in the sequence).
Recorded per G: both kernels'
times (minimum and range), the bytes either reads -- (mcap + 8) * m_words * 8, mcap = the
capacity chain_merge gives the merged table: the power of two >= 65536 that holds twice the
sum of the files' group counts --, the bytes per second at the minimum, and export_ms, transfer_ms
and merge_ms of evql_exchange_last_stats (host clock: from the call's entry to the end of its
export steps, then the collectives and copies, then the merge up to the call's return).
One device only: transfer and merge are exercised, not measured as a multi-GPU figure.

usage: chain_exchange.py [--groups G[,G..]] [--reps R] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_TIMEOUT = 420  # seconds: two tables of 2 G rows each, R x (two scans, a fetch, an exchange)


def child(groups, reps):
    sys.path.insert(0, HERE)
    import eventql_amd as E
    from eventql_amd import capi as K
    from eventql_amd.plan import Order, Plan, col, count, sum_
    schema = dict(u=K.T_UINT64, a=K.T_UINT64)
    kw = dict(select=[col("u"), count(1), sum_(col("a"))], group_by=[col("u")], groups_hint=groups)
    ctx = E.Context(0)
    hub = E.Hub(1)
    x = E.Exchange.hub(ctx, hub, 0)
    tabs = [ctx.generate(2 * groups, columns="ua", seed=11 + i, u_mod=groups) for i in range(2)]
    per_file = []
    for t in tabs:
        q = t.query(Plan(schema, **kw))
        q.execute()
        per_file.append(q.stats()["num_groups"])
        q.close()
    ch = E.LsmChain(ctx)
    for t in tabs:
        ch.add(t, has_skiplist=False, has_updates=False)
    ch.build()
    plan = Plan(schema, **kw)
    q = ch.query(plan)
    q.set_order(Order(plan, [(1, True)], limit=1))
    m_words = q.record_words() - 1
    out = dict(groups_asked=groups, rows_per_file=2 * groups, groups_per_file=per_file,
               m_words=m_words, export_ms=[], transfer_ms=[], merge_ms=[], merged_groups=None,
               exchanged_groups=None)
    for _ in range(reps):
        q.execute()
        out["merged_groups"] = q.stats()["num_groups"]
        q.exchange(x, K.EXCHANGE_GATHER_ALL)
        st = x.stats()
        for phase in ("export_ms", "transfer_ms", "merge_ms"):
            out[phase].append(st[phase])
        out["exchanged_groups"] = st["groups_received"]
        out["merge_buckets"] = st["merge_buckets"]
        q.execute()
        n, _raw = q.next_batch(1)
        assert n == 1
    mcap = 1 << 16
    while mcap < 2 * sum(per_file):
        mcap <<= 1
    out["mcap"] = mcap
    out["bytes_read"] = (mcap + 8) * m_words * 8
    q.close()
    ch.close()
    for t in tabs:
        t.close()
    x.close()
    hub.close()
    ctx.close()
    print(json.dumps(out))


def spread(v):
    return dict(values=v, min=min(v), range=max(v) - min(v)) if v else None


def measure(groups, reps):
    d = tempfile.mkdtemp(prefix="chain_exchange_rocprof_")
    try:
        # a session of its own: at the time limit the profiler AND the python process under it
        # (which holds the GPU) are ended
        p = subprocess.Popen(["rocprofv3", "--kernel-trace", "-d", d, "-o", "chain_exchange",
                              "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                              "--child", str(groups), "--reps", str(reps)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             start_new_session=True)
        try:
            stdout, stderr = p.communicate(timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.communicate()
            raise
        if p.returncode != 0:
            raise RuntimeError("child for %d groups failed (%d): %s" % (groups, p.returncode, stderr[-2000:]))
        res = None
        for line in reversed(stdout.strip().splitlines()):
            if line.startswith("{"):
                res = json.loads(line)
                break
        if res is None:
            raise RuntimeError("the child printed no result line")
        disp = []  # (start, name, duration ms) of the two compaction kernels
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for row in csv.DictReader(open(f)):
                name = row.get("Kernel_Name", "")
                if "k_mtab_compact" in name or "k_table_compact" in name:
                    t0, t1 = int(row["Start_Timestamp"]), int(row["End_Timestamp"])
                    disp.append((t0, "mtab" if "k_mtab_compact" in name else "table", (t1 - t0) / 1e6))
        disp.sort()
        # Behind the first export every execute() launches the same number c of
        # k_table_compact dispatches (chain_merge over the files' own tables, possibly none) and
        # every fetch one more: [mtab, c, fetch] per repetition, c more before the next one.
        new = [ms for _, kind, ms in disp if kind == "mtab"]
        first = next((i for i, x in enumerate(disp) if x[1] == "mtab"), len(disp))
        tables = [ms for _, kind, ms in disp[first:] if kind == "table"]
        c, rest = divmod(len(tables) - reps, 2 * reps - 1) if len(tables) >= reps else (0, 1)
        if len(new) != reps or rest:
            raise RuntimeError("unexpected dispatch pattern: %d exports, %d compactions behind the first"
                               % (len(new), len(tables)))
        yard = [tables[r * (2 * c + 1) + c] for r in range(reps)]
        res["k_mtab_compact_ms"] = spread(new)
        res["k_table_compact_ms"] = spread(yard)
        for phase in ("export_ms", "transfer_ms", "merge_ms"):
            res[phase] = spread(res[phase])
        b = res["bytes_read"]
        res["k_mtab_compact_GBps"] = b / (min(new) * 1e6)
        res["k_table_compact_GBps"] = b / (min(yard) * 1e6)
        # the same reads and one OR more per record: the same bytes per second to within the
        # range of the repetitions
        tol = max(res["k_table_compact_ms"]["range"], res["k_mtab_compact_ms"]["range"])
        res["within_range_of_yardstick"] = min(new) <= min(yard) + tol
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "chain_exchange_measure.json"))
    ap.add_argument("--child", type=int, default=None)
    args = ap.parse_args()
    if args.child is not None:
        child(args.child, args.reps)
        return
    res = dict(workload="one hub rank, two-file chain, select u, count(1), sum(a) group by u",
               yardstick="k_table_compact (unchanged from the parent commit) over the same merged "
                         "table, timed in the same process", reps=args.reps, cases=[],
               note="one device: transfer and merge were exercised, not measured across GPUs")
    for g in [int(v) for v in args.groups.split(",")]:
        res["cases"].append(measure(g, args.reps))
        print("%d groups done" % g, flush=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
