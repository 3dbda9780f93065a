#!/usr/bin/env python3
"""Sorted compaction of a partition file chain, measured.

Workload: the partition of chain_compact.py (four files, 6e7 rows in times
--scale, ten columns) plus a microsecond timestamp column `t`, ascending inside every file:
  --layout ordered    file f covers its own hour, so `t` ascends in FILE_ORDER (a healthy
                      partition: the sorted call must find nothing to do)
  --layout overlap    every file covers the same hour: the files overlap completely
  --layout late       overlap, and one row in ten is a late event: its t is uniform over the
                      hour, so every 2048-row zone of a file spans the hour (not asked for by
                      the gate; run once for the payoff)

  child new        builds the partition and its chain, runs evql_lsm_chain_compact_sorted
                   (key t, FILE_ORDER) --inner times and reports the stats of the fastest
                   (gather_ms + sort_ms + permute_ms + encode_ms); with --payoff also runs
                   `select k, count(1), sum(a) where t >= L group by k` (L = 90th percentile)
                   over the chain, over the file-order table and over the sorted table
  child yardstick  the same partition and chain with the package and library of --root (a
                   checkout of the parent commit): plain evql_lsm_chain_compact(FILE_ORDER),
                   gather_ms + encode_ms of the fastest of --inner calls
  (default)        --reps (default 5) alternating pairs of fresh child processes per layout;
                   spread = range of the yardstick processes' minima.  Gate (ordered layout):
                     gather + sort + permute + encode
                        <= yardstick * (1 + 8 B * rows / (B_gather + B_encode)) + spread
                   the one extra pass being the read of the key words; B_gather and B_encode
                   from the shapes as in chain_compact.traffic (+ the column t).
                   The overlapping layout is reported only.
  --trace DIR      one `rocprofv3 --kernel-trace --stats` run of `child new --layout overlap`
                   (its own run: no timing is taken from it); the kernel stats CSV is copied
                   to profiles/chain_compact_sorted_kernel_stats.csv

usage: chain_compact_sorted.py [--parent-root DIR] [--scale F] [--reps N] [--out FILE] [--trace DIR]"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_compact as CC  # noqa: E402  (the partition of 6h)

CHILD_TIMEOUT = 420
HOUR_US = 3_600_000_000
T0_US = 1_700_000_000_000_000  # ~2^50.6


def out_specs(K):
    specs = CC.out_specs(K)
    t = dict(name="t", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_PLAIN)
    return specs[:6] + [t] + specs[6:]


def make_file(torch, E, K, ctx, fi, nrows, has_skiplist, id_space, seed, layout):
    """chain_compact.make_file's table with the column t: nrows timestamps spread evenly
    over an hour, ascending"""
    real = ctx.table_from_device_columns
    i = torch.arange(nrows, dtype=torch.int64, device="cuda")
    step = max(1, HOUR_US // max(nrows, 1))
    t = T0_US + (fi * HOUR_US if layout == "ordered" else fi) + i * step
    if layout == "late":
        g = torch.Generator(device="cuda")
        g.manual_seed(seed * 77 + fi)
        late = torch.rand(nrows, generator=g, device="cuda") < 0.1
        anywhere = T0_US + torch.randint(0, HOUR_US, (nrows,), generator=g, device="cuda",
                                         dtype=torch.int64)
        t = torch.where(late, anywhere, t)
    tspec = dict(name="t", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_PLAIN)

    def with_t(specs, vals, nulls, n, heaps=None, **kw):
        specs = specs[:6] + [tspec] + specs[6:]
        vals = dict(vals, t=t.data_ptr())
        return real(specs, vals, nulls, n, heaps=heaps, **kw)
    ctx.table_from_device_columns = with_t
    try:
        tab, c = CC.make_file(torch, E, K, ctx, fi, nrows, has_skiplist, id_space, seed)
    finally:
        del ctx.table_from_device_columns
    c["t"] = t
    return tab, c


def build_partition(scale, seed, layout):
    import torch
    import eventql_amd as E
    from eventql_amd import capi as K
    ctx = E.Context(0)
    files = [(max(1, int(n * scale)), skl) for n, skl in CC.FILES]
    id_space = max(4, sum(n for n, _ in files) // 2)
    tabs, cols = [], []
    for fi, (n, skl) in enumerate(files):
        tab, c = make_file(torch, E, K, ctx, fi, n, bool(skl), id_space, seed, layout)
        tabs.append(tab)
        cols.append(c)
    ch = E.LsmChain(ctx)
    for fi in reversed(range(len(files))):  # newest first
        ch.add(tabs[fi], has_skiplist=bool(files[fi][1]), has_updates=True)
    ch.build()
    return torch, E, K, ctx, files, tabs, cols, ch


def run_query(q):
    try:
        t0 = time.perf_counter()
        res = q.run()
        wall = (time.perf_counter() - t0) * 1e3
        st = q.stats()
        zs = q.zone_stats()
        return sorted(res.rows(), key=repr), dict(
            wall_ms=wall, kernel_ms=st.get("kernel_ms"), rows_passed=st.get("rows_passed"),
            tiles_skipped=zs["tiles_skipped"], tiles_total=zs["tiles_total"],
            zones_excluded=zs["zones_excluded"], zones_total=zs["zones_total"])
    finally:
        q.close()


def child_new(a):
    torch, E, K, ctx, files, tabs, cols, ch = build_partition(a.scale, a.seed, a.layout)
    specs = out_specs(K)
    best = None
    for it in range(a.inner):
        t0 = time.perf_counter()
        t = ch.compact_sorted(specs, "t", row_order=K.COMPACT_FILE_ORDER)
        wall = (time.perf_counter() - t0) * 1e3
        st = dict(ch.compact_stats, wall_ms=wall, sort=dict(ch.compact_sort_stats))
        st["total_ms"] = st["gather_ms"] + st["encode_ms"] + st["sort"]["sort_ms"] + st["sort"]["permute_ms"]
        if best is None or st["total_ms"] < best["total_ms"]:
            best = st
        if it + 1 < a.inner:
            t.close()
    kept, has_filter = [], []
    for k in range(len(files)):  # scan order
        f, n = ch.filter(k)
        kept.append(n)
        has_filter.append(f is not None)
    best.update(kept_scan_order=kept, has_filter=has_filter, files=files, layout=a.layout)
    best["image_bytes"] = E.lib().evql_table_image_size(t.h)
    if a.payoff:
        from eventql_amd.plan import Plan, col, count, sum_
        schema = dict(k=K.T_UINT64, a=K.T_UINT64, t=K.T_TIMESTAMP64)
        zmin, zmax = t.zone_map("t")
        lo, hi = int(zmin.min()), int(zmax.max())
        L = lo + (hi - lo) * 9 // 10  # t is spread evenly: the 90th percentile
        from eventql_amd.plan import lit
        kw = dict(select=[col("k"), count(1), sum_(col("a"))], group_by=[col("k")],
                  where=col("t") >= lit(L, K.T_TIMESTAMP64), groups_hint=100)
        plain = ch.compact(specs, row_order=K.COMPACT_FILE_ORDER)
        out = {}
        rows = {}
        for name, src in (("chain", ch), ("file_order_table", plain), ("sorted_table", t)):
            run_query(src.query(Plan(schema, **kw)))  # (compiles, builds the zone map)
            rows[name], out[name] = run_query(src.query(Plan(schema, **kw)))
        out["equal"] = bool(rows["chain"] == rows["file_order_table"] == rows["sorted_table"])
        out["groups"] = len(rows["chain"])
        out["L"] = L
        best["payoff"] = out
        plain.close()
    t.close()
    print("RESULT " + json.dumps(best))


def child_yardstick(a):
    torch, E, K, ctx, files, tabs, cols, ch = build_partition(a.scale, a.seed, a.layout)
    specs = out_specs(K)
    best = None
    for _ in range(a.inner):
        t = ch.compact(specs, row_order=K.COMPACT_FILE_ORDER)
        st = dict(ch.compact_stats)
        if best is None or st["gather_ms"] + st["encode_ms"] < best["gather_ms"] + best["encode_ms"]:
            best = st
        image_bytes = E.lib().evql_table_image_size(t.h)
        t.close()
    best.update(image_bytes=image_bytes, lib=E.LIB_PATH, layout=a.layout,
                has_sorted_call=hasattr(E.LsmChain, "compact_sorted"))
    print("RESULT " + json.dumps(best))


def run_child(mode, a, layout, root=HERE, prefix=None, payoff=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root,
           "--layout", layout, "--scale", str(a.scale), "--seed", str(a.seed),
           "--inner", str(a.inner)]
    cmd += ["--payoff"] if payoff else []
    p = subprocess.run((prefix or []) + cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (mode, p.returncode, p.stderr[-3000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def traffic(K, n0, image_bytes):
    files = [tuple(f) for f in n0["files"]]
    b_gather, b_encode = CC.traffic(K, files, n0["kept_scan_order"], n0["has_filter"],
                                    n0["string_bytes"], image_bytes)
    rows_in, rows_out = n0["rows_in"], n0["rows_written"]
    # the column t: PLAIN64 pages read, SoA words written, then read by the writer
    return b_gather + 8 * rows_in + 8 * rows_out, b_encode + 8 * rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["new", "yardstick"])
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--root", default=HERE, help="(children) the tree whose package is imported")
    ap.add_argument("--layout", choices=["ordered", "overlap", "late"], default="overlap")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--payoff", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "chain_compact_sorted_measure.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.child == "new":
        return child_new(a)
    if a.child == "yardstick":
        return child_yardstick(a)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        run_child("new", a, "overlap", prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace,
                                               "--output-format", "csv", "--"])
        stats = glob.glob(os.path.join(a.trace, "**", "*kernel_stats.csv"), recursive=True)
        if stats:
            shutil.copy(stats[0], os.path.join(HERE, "profiles", "chain_compact_sorted_kernel_stats.csv"))
        print("kernel stats:", stats)
        return
    if not a.parent_root:
        raise SystemExit("--parent-root is needed for the yardstick")
    from eventql_amd import capi as K
    res = dict(scale=a.scale, seed=a.seed)
    for layout in ("ordered", "overlap"):
        news, yards = [], []
        for r in range(a.reps):
            yards.append(run_child("yardstick", a, layout, root=a.parent_root))
            assert not yards[-1]["has_sorted_call"], "the yardstick must be the parent's library"
            news.append(run_child("new", a, layout, payoff=(r == 0 and layout == "overlap")))
            print("%s pair %d: yardstick %.3f ms, new %.3f ms (sort %.3f, permute %.3f)" %
                  (layout, r, yards[-1]["gather_ms"] + yards[-1]["encode_ms"], news[-1]["total_ms"],
                   news[-1]["sort"]["sort_ms"], news[-1]["sort"]["permute_ms"]), flush=True)
        n0 = news[0]
        ymins = [y["gather_ms"] + y["encode_ms"] for y in yards]
        yard, spread = min(ymins), max(ymins) - min(ymins)
        new = min(n["total_ms"] for n in news)
        b_gather, b_encode = traffic(K, n0, yards[0]["image_bytes"])
        out = dict(files_oldest_first=n0["files"], rows_in=n0["rows_in"],
                   rows_written=n0["rows_written"], B_gather=b_gather, B_encode=b_encode,
                   yardstick_ms=yard, yardstick_spread_ms=spread, yardstick_runs=ymins,
                   new_runs=[dict(gather_ms=n["gather_ms"], encode_ms=n["encode_ms"],
                                  wall_ms=n["wall_ms"], **n["sort"]) for n in news],
                   new_min_ms=new, payoff=n0.get("payoff"))
        if layout == "ordered":
            bound = yard * (1 + 8.0 * n0["rows_written"] / (b_gather + b_encode)) + spread
            out.update(bound_ms=bound, gate_met=bool(new <= bound))
        res[layout] = out
    late = run_child("new", a, "late", payoff=True)
    res["late"] = dict(rows_written=late["rows_written"], gather_ms=late["gather_ms"],
                       encode_ms=late["encode_ms"], payoff=late["payoff"], **late["sort"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
