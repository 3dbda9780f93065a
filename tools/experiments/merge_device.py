"""Device merge of PARTIAL frames against the host merge.

F frames of the same G random 20-byte keys, four state columns (count, integer sum, float sum,
min over floats) and one string cell per row; timed: add_frame x F plus a full fetch.

    python tools/experiments/merge_device.py --groups 10000,100000,1000000 --host-lib PARENT.so

The yardstick is the host merge of `--host-lib` (the parent commit's build of the library; it
is loaded with ctypes directly, without this package's bindings).  Each side of a repetition
runs in a process of its own, alternating; a process reports the minimum of its inner
iterations; the spread of a side is the range of those minima over the repetitions."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from eventql_amd import capi as K  # noqa: E402
from eventql_amd.plan import Plan, Col as col, count, sum_, min_  # noqa: E402

SCHEMA = dict(k=K.T_UINT64, a=K.T_UINT64, v=K.T_FLOAT64, s=K.T_STRING)
FRAMES = 4


def plan():
    return Plan(SCHEMA, select=[count(1), sum_(col("a")), sum_(col("v")), min_(col("v")), col("s")],
                group_by=[col("k")])


def varuint(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def frames(g):
    """FRAMES payloads of g rows each, fixed-width rows built with numpy"""
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 256, (g, 20), dtype=np.uint8)
    row = np.dtype([("key", "u1", 20), ("count", "u1"), ("sum", "u1", 4), ("fsum", "<f8"),
                    ("mcnt", "u1"), ("min", "<f8"), ("stype", "u1"), ("slen", "u1"), ("len", "<u4"),
                    ("str", "u1", 8), ("tag", "u1")])
    out = []
    for j in range(FRAMES):
        r = np.zeros(g, row)
        r["key"] = keys
        r["count"] = 1
        a = rng.integers(1 << 21, 1 << 28, g, dtype=np.uint32)  # four LEB128 bytes each
        for b in range(4):
            r["sum"][:, b] = ((a >> (7 * b)) & 0x7f) | (0x80 if b < 3 else 0)
        r["fsum"] = rng.normal(0, 1000, g)
        r["mcnt"] = 1
        r["min"] = rng.normal(0, 1000, g)
        r["stype"] = K.T_STRING
        r["slen"] = 13
        r["len"] = 8
        r["str"] = rng.integers(97, 123, (g, 8), dtype=np.uint8)
        out.append(varuint(0) + varuint(g) + r.tobytes())
    return out


def bind_host(path):
    L = C.CDLL(path)
    L.evql_merge_create.argtypes = [C.POINTER(K.PlanDesc), C.POINTER(C.c_void_p)]
    L.evql_merge_destroy.argtypes = [C.c_void_p]
    L.evql_merge_add_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.evql_merge_next_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(K.ColumnBuf),
                                        C.POINTER(C.c_size_t)]
    return L


def drain(L, h, ncols):
    bufs = (K.ColumnBuf * ncols)()
    n = C.c_size_t()
    rows = nbytes = 0
    while True:
        assert L.evql_merge_next_batch(h, 1024, bufs, C.byref(n)) == 0
        if n.value == 0:
            return rows, nbytes
        rows += n.value
        nbytes += sum(bufs[i].size for i in range(ncols))


def child(args):
    g = int(args.groups)
    fr = frames(g)
    p = plan()
    best, stats = None, {}
    if args.side == "host":
        L = bind_host(args.host_lib)
    else:
        import eventql_amd as E
        L = E.lib()
        ctx = E.Context(0)
    for _ in range(args.inner):
        h = C.c_void_p()
        t0 = time.perf_counter()
        if args.side == "host":
            assert L.evql_merge_create(C.byref(p.desc), C.byref(h)) == 0
        else:
            assert L.evql_merge_create_device(ctx.h, C.byref(p.desc), C.byref(h)) == 0
        for f in fr:
            assert L.evql_merge_add_frame(h, f, len(f)) == 0
        rows, nbytes = drain(L, h, 5)
        ms = (time.perf_counter() - t0) * 1e3
        assert rows == g, (rows, g)
        if args.side == "device":
            st = K.MergeStats()
            L.evql_merge_stats(h, C.byref(st))
            stats = {f[0]: getattr(st, f[0]) for f in K.MergeStats._fields_}
        L.evql_merge_destroy(h)
        if best is None or ms < best:
            best, best_stats = ms, dict(stats, result_bytes=nbytes)
    print(json.dumps(dict(side=args.side, groups=g, ms=best, stats=best_stats)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="10000,100000,1000000,10000000")
    ap.add_argument("--host-lib", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--side")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.side:
        return child(args)
    table = []
    for g in [int(x) for x in args.groups.split(",")]:
        minima = dict(host=[], device=[])
        last = {}
        for _ in range(args.reps):
            for side in ("host", "device"):
                out = subprocess.run(
                    [sys.executable, os.path.abspath(__file__), "--side", side, "--groups", str(g),
                     "--host-lib", args.host_lib, "--inner", str(args.inner)],
                    check=True, capture_output=True, text=True, timeout=900).stdout
                r = json.loads(out.strip().splitlines()[-1])
                minima[side].append(r["ms"])
                last[side] = r
        row = dict(groups=g, frames=FRAMES, rows=g * FRAMES,
                   host_ms=min(minima["host"]), device_ms=min(minima["device"]),
                   host_spread_ms=max(minima["host"]) - min(minima["host"]),
                   device_spread_ms=max(minima["device"]) - min(minima["device"]),
                   host_minima=minima["host"], device_minima=minima["device"],
                   device_stats=last["device"]["stats"])
        row["device_wins"] = (row["host_ms"] - row["device_ms"]
                              > max(row["host_spread_ms"], row["device_spread_ms"]))
        table.append(row)
        print(json.dumps(row), flush=True)
    wins = [r["groups"] for r in table if r["device_wins"]]
    res = dict(experiment="merge_device", reps=args.reps, inner=args.inner, table=table,
               crossover_groups=min(wins) if wins else None)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
