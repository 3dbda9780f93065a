#!/usr/bin/env python3
"""Compaction of a partition file chain on the device, measured.

Workload: a flat partition of tests/lsm_tables.LSM_SCHEMA's shape, four files of
3.2e7 / 1.6e7 / 8e6 / 4e6 rows times --scale (oldest first), generated on the device from
--seed (torch columns, then evql_table_from_device_columns): 20-byte ids from a pool of half
the rows, so that the newer files shadow the older ones, about 30 % updates, the second
file with a skiplist (10 % skipped).

  child new        builds the partition and its chain, runs evql_lsm_chain_compact --inner
                   times, reports the stats of the fastest; with --check also compares a
                   config-3-shaped and a string-key GROUP BY over the chain and over the
                   compacted table
  child yardstick  the same partition and chain with the package and library of --root (a
                   checkout of the parent commit), the kept rows gathered with torch into SoA columns, then the
                   time of evql_table_from_device_columns_ordered over them: the encode a
                   compaction cannot avoid.  Host clock around the call, which returns
                   synchronised
  (default)        --reps (default 5) alternating pairs of fresh child processes; spread =
                   range of the yardstick processes' minima.  Gate:
                     gather_ms + encode_ms <= yardstick * (1 + B_gather / B_encode) + spread
                   with B_gather = bytes the gather must read (filter words, the form of every
                   needed column the kernels read) plus bytes it writes (SoA words, NULL
                   bytes, heaps) and B_encode = SoA bytes read plus image bytes written,
                   both computed here from the shapes.
  --trace DIR      one `rocprofv3 --kernel-trace --stats` run of `child new` (its own run: no
                   timing is taken from it); the kernel stats CSV is copied to
                   profiles/chain_compact_kernel_stats.csv

usage: chain_compact.py [--parent-root DIR] [--scale F] [--reps N] [--out FILE] [--trace DIR]"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FILES = [(32_000_000, 0), (16_000_000, 1), (8_000_000, 0), (4_000_000, 0)]  # (rows, skiplist)
CHILD_TIMEOUT = 420
S_WORDS = [b"g%d" % i for i in range(13)]


def out_specs(K):
    U, F, S, B = K.COL_UNSIGNED_INT, K.COL_FLOAT, K.COL_STRING, K.COL_BOOLEAN
    return [
        dict(name="rid", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="k", logical_type=U, storage_type=K.ENC_UINT64_LEB128),
        dict(name="a", logical_type=U, storage_type=K.ENC_UINT64_PLAIN),
        dict(name="n", logical_type=U, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
        dict(name="v", logical_type=F, storage_type=K.ENC_FLOAT_IEEE754),
        dict(name="s", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
        dict(name="__lsm_is_update", logical_type=B, storage_type=K.ENC_BOOLEAN_BITPACKED),
        dict(name="__lsm_id", logical_type=S, storage_type=K.ENC_STRING_PLAIN),
        dict(name="__lsm_version", logical_type=U, storage_type=K.ENC_UINT64_LEB128),
        dict(name="__lsm_sequence", logical_type=U, storage_type=K.ENC_UINT64_LEB128)]


def mix64(torch, x):
    """splitmix64 finaliser on int64 tensors (wrapping arithmetic)"""
    x = (x ^ (x >> 30).bitwise_and(0x3ffffffff)) * -0x40a7b892e31b1a47
    x = (x ^ (x >> 27).bitwise_and(0x1fffffffff)) * -0x6b2fb644ecceee15
    return x ^ (x >> 31).bitwise_and(0x1ffffffff)


def make_file(torch, E, K, ctx, fi, nrows, has_skiplist, id_space, seed):
    """(table, device columns dict) of file fi"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 1000 + fi)
    dev = "cuda"
    i = torch.arange(nrows, dtype=torch.int64, device=dev)
    who = torch.randint(0, id_space, (nrows,), generator=g, device=dev, dtype=torch.int64)
    c = {}
    c["rid"] = fi * 1_000_000_000 + i
    c["k"] = who % 40
    c["a"] = torch.randint(0, 65536, (nrows,), generator=g, device=dev, dtype=torch.int64)
    c["n"] = torch.randint(0, 1 << 34, (nrows,), generator=g, device=dev, dtype=torch.int64)
    c["n_null"] = (torch.rand(nrows, generator=g, device=dev) < 0.2).to(torch.uint8)
    c["v"] = (torch.randint(0, 1 << 20, (nrows,), generator=g, device=dev, dtype=torch.int64)
              .to(torch.float64) / 64.0).view(torch.int64)
    # s: one of 13 short words (a shared heap), the empty string for every 7th id
    lens = torch.tensor([len(w) for w in S_WORDS], dtype=torch.int64, device=dev)
    offs = torch.cumsum(lens, 0) - lens
    w13 = who % 13
    c["s"] = torch.where(who % 7 == 0, torch.zeros_like(who), (lens[w13] << 40) | offs[w13])
    c["s_heap"] = torch.frombuffer(bytearray(b"".join(S_WORDS)), dtype=torch.uint8).to(dev)
    c["upd"] = (torch.rand(nrows, generator=g, device=dev) < 0.3).to(torch.int64)
    c["skip"] = (torch.rand(nrows, generator=g, device=dev) < 0.1).to(torch.int64)
    ids = torch.stack([mix64(torch, who * 3 + 1), mix64(torch, who * 3 + 2),
                       mix64(torch, who * 3 + 3)], 1).contiguous()
    c["id_bytes"] = ids.view(torch.uint8).view(nrows, 24)[:, :20].contiguous()
    c["id"] = (20 << 40) | (i * 20)
    c["version"] = i + 1
    c["sequence"] = i + fi * 1_000_000 + 1
    U, B = K.COL_UNSIGNED_INT, K.COL_BOOLEAN
    specs = out_specs(K)[:7]
    if has_skiplist:
        specs.append(dict(name="__lsm_skip", logical_type=B, storage_type=K.ENC_BOOLEAN_BITPACKED))
    specs += out_specs(K)[7:]
    vals = {"rid": c["rid"], "k": c["k"], "a": c["a"], "n": c["n"], "v": c["v"], "s": c["s"],
            "__lsm_is_update": c["upd"], "__lsm_skip": c["skip"], "__lsm_id": c["id"],
            "__lsm_version": c["version"], "__lsm_sequence": c["sequence"]}
    torch.cuda.synchronize()
    t = ctx.table_from_device_columns(
        specs, {s["name"]: vals[s["name"]].data_ptr() for s in specs},
        {"n": c["n_null"].data_ptr()}, nrows,
        heaps={"s": c["s_heap"].data_ptr(), "__lsm_id": c["id_bytes"].data_ptr()})
    return t, c


def build_partition(scale, seed):
    import torch
    import eventql_amd as E
    from eventql_amd import capi as K
    ctx = E.Context(0)
    files = [(max(1, int(n * scale)), skl) for n, skl in FILES]
    id_space = max(4, sum(n for n, _ in files) // 2)
    tabs, cols = [], []
    for fi, (n, skl) in enumerate(files):
        t, c = make_file(torch, E, K, ctx, fi, n, bool(skl), id_space, seed)
        tabs.append(t)
        cols.append(c)
    ch = E.LsmChain(ctx)
    for fi in reversed(range(len(files))):  # newest first
        ch.add(tabs[fi], has_skiplist=bool(files[fi][1]), has_updates=True)
    ch.build()
    return torch, E, K, ctx, files, tabs, cols, ch


def traffic(K, files, kept_scan_order, has_filter, heap_bytes, image_bytes):
    """B_gather, B_encode in bytes, from the shapes.  Forms the gather reads, per input row:
    PLAIN64 / FLOAT pages 8; a required LEB128 column its narrow copy (k: 1, version and
    sequence: 4); the optional LEB128 column its SoA words and tag bytes, 8 + 1; a string
    column its position words and tag bytes, 8 + 1, plus the kept strings' bytes;
    __lsm_is_update is not read."""
    rows_in = sum(n for n, _ in files)
    rows_out = sum(kept_scan_order)
    per_row_in = 8 + 1 + 8 + 9 + 8 + 9 + 9 + 4 + 4
    filters = sum((n + 7) // 8 for (n, _), f in zip(reversed(files), has_filter) if f)
    soa = rows_out * (8 * 10 + 1)
    b_gather = filters + rows_in * per_row_in + soa + 2 * heap_bytes + 2 * 16 * rows_out
    b_encode = soa + heap_bytes + image_bytes
    return b_gather, b_encode


def child_new(a):
    torch, E, K, ctx, files, tabs, cols, ch = build_partition(a.scale, a.seed)
    specs = out_specs(K)
    best = None
    for _ in range(a.inner):
        t0 = time.perf_counter()
        t = ch.compact(specs, row_order=K.COMPACT_SCAN_ORDER)
        wall = (time.perf_counter() - t0) * 1e3
        st = dict(ch.compact_stats, wall_ms=wall)
        if best is None or st["gather_ms"] + st["encode_ms"] < best["gather_ms"] + best["encode_ms"]:
            best = st
        last = t
        if _ + 1 < a.inner:
            t.close()
    kept, has_filter = [], []
    for k in range(len(files)):  # scan order
        f, n = ch.filter(k)
        kept.append(n)
        has_filter.append(f is not None)
    best["kept_scan_order"] = kept
    best["has_filter"] = has_filter
    best["files"] = files
    if a.check:
        from eventql_amd.plan import Plan, col, count, sum_
        schema = dict(rid=K.T_UINT64, k=K.T_UINT64, a=K.T_UINT64, n=K.T_UINT64, v=K.T_FLOAT64,
                      s=K.T_STRING)
        plans = {
            "config3-shaped": dict(select=[col("k"), sum_(col("a")), count(1), sum_(col("v"))],
                                   group_by=[col("k")], where=(col("a") > 30000) & (col("rid") % 3 < 2)),
            "string-key": dict(select=[col("s"), count(1), sum_(col("a"))], group_by=[col("s")])}
        best["equal_outputs"] = {}
        for name, kw in plans.items():
            q = ch.query(Plan(schema, **kw))
            x = sorted(q.run().rows(), key=repr)
            q.close()
            q = last.query(Plan(schema, **kw))
            y = sorted(q.run().rows(), key=repr)
            q.close()
            same = len(x) == len(y) and all(
                all((u == w) if not isinstance(u, float) else abs(u - w) <= 1e-9 * abs(u)
                    for u, w in zip(r, s)) for r, s in zip(x, y))
            best["equal_outputs"][name] = dict(groups=len(x), equal=bool(same))
    last.close()
    print("RESULT " + json.dumps(best))


def child_yardstick(a):
    torch, E, K, ctx, files, tabs, cols, ch = build_partition(a.scale, a.seed)
    specs = out_specs(K)
    parts = {name: [] for name in ("rid", "k", "a", "n", "n_null", "v", "s", "id_bytes",
                                   "version", "sequence")}
    for k in range(len(files)):  # scan order
        fi = len(files) - 1 - k
        f, _ = ch.filter(k)
        c = cols[fi]
        if f is None:
            idx = torch.arange(files[fi][0], device="cuda")
        else:
            idx = torch.from_numpy(f).cuda().nonzero().flatten()
        for name in parts:
            parts[name].append(c[name].index_select(0, idx))
    g = {name: torch.cat(v).contiguous() for name, v in parts.items()}
    n = g["rid"].numel()
    g["upd"] = torch.zeros(n, dtype=torch.int64, device="cuda")
    g["id"] = (20 << 40) | (torch.arange(n, dtype=torch.int64, device="cuda") * 20)
    vals = {"rid": g["rid"], "k": g["k"], "a": g["a"], "n": g["n"], "v": g["v"], "s": g["s"],
            "__lsm_is_update": g["upd"], "__lsm_id": g["id"], "__lsm_version": g["version"],
            "__lsm_sequence": g["sequence"]}
    torch.cuda.synchronize()
    times = []
    for _ in range(a.inner):
        t0 = time.perf_counter()
        t = ctx.table_from_device_columns(
            specs, {s["name"]: vals[s["name"]].data_ptr() for s in specs},
            {"n": g["n_null"].data_ptr()}, n,
            heaps={"s": cols[0]["s_heap"].data_ptr(), "__lsm_id": g["id_bytes"].data_ptr()},
            page_order=K.PAGE_ORDER_COLUMNS)
        times.append((time.perf_counter() - t0) * 1e3)
        image_bytes = E.lib().evql_table_image_size(t.h)
        t.close()
    print("RESULT " + json.dumps(dict(encode_ms=min(times), all_ms=times, rows=n,
                                      image_bytes=image_bytes, lib=E.LIB_PATH)))


def run_child(mode, a, root=HERE, prefix=None, check=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root,
           "--scale", str(a.scale), "--seed", str(a.seed), "--inner", str(a.inner)]
    cmd += ["--check"] if check else []
    p = subprocess.run((prefix or []) + cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if p.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s" % (mode, p.returncode, p.stderr[-3000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["new", "yardstick"])
    ap.add_argument("--parent-root", help="checkout of the parent commit, library built")
    ap.add_argument("--root", default=HERE, help="(children) the tree whose package is imported")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "chain_compact_measure.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.child == "new":
        return child_new(a)
    if a.child == "yardstick":
        return child_yardstick(a)
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        run_child("new", a, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace,
                                    "--output-format", "csv", "--"])
        stats = glob.glob(os.path.join(a.trace, "**", "*kernel_stats.csv"), recursive=True)
        if stats:
            shutil.copy(stats[0], os.path.join(HERE, "profiles", "chain_compact_kernel_stats.csv"))
        print("kernel stats:", stats)
        return
    if not a.parent_root:
        raise SystemExit("--parent-root is needed for the yardstick")
    from eventql_amd import capi as K
    news, yards = [], []
    for r in range(a.reps):
        yards.append(run_child("yardstick", a, root=a.parent_root))
        news.append(run_child("new", a, check=(r == 0)))
        print("pair %d: yardstick %.3f ms, new gather %.3f + encode %.3f ms" %
              (r, yards[-1]["encode_ms"], news[-1]["gather_ms"], news[-1]["encode_ms"]), flush=True)
    n0 = news[0]
    files = [tuple(f) for f in n0["files"]]
    b_gather, b_encode = traffic(K, files, n0["kept_scan_order"], n0["has_filter"],
                                 n0["string_bytes"], yards[0]["image_bytes"])
    yard = min(y["encode_ms"] for y in yards)
    spread = max(y["encode_ms"] for y in yards) - yard
    new = min(n["gather_ms"] + n["encode_ms"] for n in news)
    bound = yard * (1 + b_gather / b_encode) + spread
    res = dict(scale=a.scale, seed=a.seed, files_oldest_first=files, rows_in=n0["rows_in"],
               rows_written=n0["rows_written"], string_bytes=n0["string_bytes"],
               image_bytes=yards[0]["image_bytes"], B_gather=b_gather, B_encode=b_encode,
               yardstick_ms=yard, yardstick_spread_ms=spread,
               yardstick_runs=[y["encode_ms"] for y in yards],
               new_runs=[dict(gather_ms=n["gather_ms"], encode_ms=n["encode_ms"],
                              wall_ms=n["wall_ms"]) for n in news],
               new_min_ms=new, bound_ms=bound, gate_met=bool(new <= bound),
               n_kernel_launches=n0["n_kernel_launches"], n_host_waits=n0["n_host_waits"],
               equal_outputs=n0.get("equal_outputs"))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
