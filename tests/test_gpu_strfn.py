"""String functions evaluated per row on the MI355X: group keys, WHERE operands and
operands inside aggregate arguments (evql_strfn.h in the generated kernel).

  * every case of tests/golden/ref_csql_strfn.json / ref_csql_strfnlsm.json -- the
    reference's own engine -- through the C ABI, and the reference engine with the GPU
    operator plugged in;
  * hand-built tables against the oracle: embedded NULs, spaces only, values that fold
    onto each other, NULLs, 11-byte values, page and chunk borders, tiny tables, the
    partitioned path, the exchange between ranks.

Every plan here must lower: nothing returns early or skips on EVQL_ENOTSUP.
"""
import json
import os
import subprocess
import tempfile
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Plan, DumpedPlan, Call, If, Lit, col, count, sum_
import lsm_tables
import oracle_lib as O
import refcases
import sqlgen
import strfn_cases  # noqa: F401  (registers the suites "strfn" and "strfnlsm")
from test_ref_csql_cpu import load, fixture_case, case_plan, check_result, check_partial

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                     "oracle", "_ref", "csql_probe")


def f(name, *args):
    return Call(name, *args)


def run(t, plan):
    """(types, rows) of a plan that must lower; a runtime error as its message"""
    q = t.query(plan)
    try:
        try:
            r = q.run()
        except E.EvqlError as e:
            assert e.code != K.EVQL_ENOTSUP, e
            return e.msg
        return (r.types, r.rows())
    finally:
        q.close()


# ---------------------------------------------------------------------------------------
# the reference fixtures
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ctx):
    img, schema, _ = refcases.table_image("mixed")
    t = ctx.open_image(img)
    yield t, schema
    t.close()


@pytest.mark.parametrize("cid", [c["id"] for c in load("strfn")["cases"]])
def test_hip_path_reproduces_the_reference(mixed, cid):
    fx = fixture_case("strfn", cid)
    c = case_plan("strfn", cid)
    t, schema = mixed
    check_result(fx["result"], run(t, Plan(schema, **c["kw"])))
    check_result(fx["result"], run(t, DumpedPlan(fx["programs"])))
    rp = run(t, Plan(schema, mode=K.MODE_PARTIAL, **c["kw"]))
    assert not isinstance(rp, str), rp
    check_partial(fx["partial"], [k for k, _ in rp[1]], [d for _, d in rp[1]])


@pytest.fixture(scope="module")
def chains(ctx):
    made = {}

    def get(pname):
        if pname not in made:
            files = lsm_tables.partition(pname)
            tabs = [ctx.open_image(x[1]) for x in reversed(files)]
            ch = E.LsmChain(ctx)
            for t, x in zip(tabs, reversed(files)):
                ch.add(t, has_skiplist=x[2], has_updates=x[3])
            ch.build()
            made[pname] = (ch, tabs)
        return made[pname][0]
    yield get
    for ch, tabs in made.values():
        ch.close()
        for t in tabs:
            t.close()


@pytest.mark.parametrize("cid", [c["id"] for c in load("strfnlsm")["cases"]])
def test_hip_chain_operator_reproduces_the_reference(chains, cid):
    fx = fixture_case("strfnlsm", cid)
    c = case_plan("strfnlsm", cid)
    ch = chains(c["table"][4:])
    S = lsm_tables.LSM_SCHEMA
    check_result(fx["result"], run(ch, Plan(S, **c["kw"])))
    check_result(fx["result"], run(ch, DumpedPlan(fx["programs"])))
    rp = run(ch, Plan(S, mode=K.MODE_PARTIAL, **c["kw"]))
    assert not isinstance(rp, str), rp
    check_partial(fx["partial"], [k for k, _ in rp[1]], [d for _, d in rp[1]])


@pytest.mark.skipif(not os.path.exists(PROBE), reason="oracle/_ref/csql_probe not built "
                    "(needs the reference tree at build time)")
def test_reference_engine_with_gpu_operator():
    """the reference's own engine, `MODE gpu`: GpuSchedulerT lowers every GROUP BY of the
    suite and the rows are the CPU operators'"""
    cases = load("strfn")["cases"]
    img, _, kind = refcases.table_image("mixed")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "mixed.cst")
        with open(path, "wb") as fh:
            fh.write(img)
        cmds = ["TABLE t %s %s" % (path, kind), "ROWS on", "MODE gpu"] + ["SQL " + c["sql"] for c in cases]
        p = subprocess.run([PROBE], input="\n".join(cmds) + "\n", capture_output=True, text=True,
                           timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    res = [json.loads(x) for x in p.stdout.splitlines() if x.strip()]
    assert len(res) == len(cases)
    for c, r in zip(cases, res):
        want = c["result"]
        assert r["sql"] == c["sql"] and r["ok"], (c["id"], r.get("error"))
        d = [x for x in r.get("decisions", []) if x["node"] == "groupby"]
        assert d and d[0]["lowered"], (c["id"], r.get("decisions"))
        rows = [list(x) for x in r["rows"]]
        rows.sort(key=lambda row: [(0, "") if v is None else (1, repr(v)) for v in row])
        assert r["types"] == want["types"] and len(rows) == want["nrows"], c["id"]
        assert rows[:len(want["rows"])] == want["rows"], c["id"]
        assert sqlgen.rows_digest(rows) == want["digest"], c["id"]


# ---------------------------------------------------------------------------------------
# hand-built tables against the oracle
# ---------------------------------------------------------------------------------------
S = dict(s=K.T_STRING, ns=K.T_STRING, x=K.T_UINT64)
s, ns, x = col("s"), col("ns"), col("x")

# embedded NUL, spaces only, values that fold onto each other, 11 bytes (a boxed SValue of
# exactly 16 bytes: the PARTIAL rows carry STAG_INLINE in its tag)
POOL = [b"", b" ", b"  Ab ", b"aB", b"AB", b"ab", b"Key-7  ", b"key-7", b"x" * 11, b"X" * 11,
        b"  pad", b"pad  ", b"Z\0z", b"z\0Z"]


def build(svals, nsvals, present):
    n = len(svals)
    w = E.Writer([dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
                  dict(name="ns", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1),
                  dict(name="x", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)])
    w.put("s", svals)
    w.put("ns", nsvals, present=present)
    w.put("x", np.arange(n, dtype=np.uint64))
    w.commit(n)
    img = w.image()
    w.close()
    return img


def pool_table(n=5000):
    rng = np.random.default_rng(2024)
    return build([POOL[i] for i in rng.integers(0, len(POOL), n)],
                 [POOL[i] for i in rng.integers(0, len(POOL), n)],
                 (rng.random(n) < 0.8).astype(np.uint8))


def canon(types, rows):
    return sorted(sqlgen.canon_rows(types, rows), key=repr)


def check_against_oracle(t, img, kw, oracle_extra=None, **extra):
    """FINAL rows and PARTIAL (SHA1 key, states) pairs equal the oracle's; -> group count.
    oracle_extra: what the oracle gets in place of `extra` (it takes no row range)"""
    oracle_extra = extra if oracle_extra is None else oracle_extra
    exp = O.oracle_run(img, Plan(S, **dict(kw, **oracle_extra)))
    got = run(t, Plan(S, **dict(kw, **extra)))
    assert not isinstance(got, str), got
    assert canon(*got) == canon(exp.types, exp.rows())
    ep = O.oracle_run(img, Plan(S, mode=K.MODE_PARTIAL, **dict(kw, **oracle_extra)))
    gp = run(t, Plan(S, mode=K.MODE_PARTIAL, **dict(kw, **extra)))
    assert not isinstance(gp, str), gp
    assert sorted(gp[1]) == sorted((ep.keys[20 * i:20 * i + 20], ep.columns[0][i]) for i in range(ep.nrows))
    return exp.nrows


def keyed(key):
    return dict(select=[key, count(1), sum_(x)], group_by=[key])


# plan -> groups of the unfiltered run.  Every (pool value, x % 3) pair occurs among 5000
# rows, so the counts follow from the pool:
#   lcase(s)                     aB / AB / ab, the two runs of 11 and Z\0z / z\0Z fold: 14 - 4
#   rtrim(ltrim(ns))             "", " " and NULL give ""; "  Ab " alone gives "Ab"; "  pad" and
#                                "pad  " give "pad"; "Key-7  " gives "Key-7": 12
#   concat(ucase(s), x % 3)      the 10 upper-cased values times 3
#   substring(s, x % 3 - 2)      "", the last byte and the last two bytes of every value: 21
POOL_PLANS = [
    ("lcase-key", keyed(f("lcase", s)), 10),
    ("trim-nullable-key", keyed(f("rtrim", f("ltrim", ns))), 12),
    ("concat-to-string-key", keyed(f("concat", f("ucase", s), f("to_string", x % 3))), 30),
    ("substring-row-position-key", keyed(f("substring", s, x % 3 - 2)), 21),
    ("concat-in-where", dict(select=[count(1), sum_(x)], where=f("concat", ns, Lit("!")).eq("!")), 1),
    ("affix-in-sum-if", dict(select=[s, sum_(If(f("startswith", f("lcase", ns), Lit("key")), x, 0))],
                             group_by=[s]), 14),
]


@pytest.fixture(scope="module")
def pool(ctx):
    img = pool_table()
    t = ctx.open_image(img)
    yield t, img
    t.close()


@pytest.mark.parametrize("name", [p[0] for p in POOL_PLANS])
def test_pool_table_against_the_oracle(pool, name):
    t, img = pool
    kw, groups = [(p[1], p[2]) for p in POOL_PLANS if p[0] == name][0]
    assert check_against_oracle(t, img, kw) == groups
    keep = np.random.default_rng(5).random(5000) < 0.6
    check_against_oracle(t, img, kw, row_filter=keep)
    # (a tile is at least 2048 rows: both ends cut inside one; the oracle sees the range as
    # a row filter)
    inside = (np.arange(5000) >= 37) & (np.arange(5000) < 4321)
    check_against_oracle(t, img, kw, oracle_extra=dict(row_filter=inside), row_begin=37, row_end=4321)


def test_timestamps_bools_and_nulls_as_text(ctx):
    """to_string of a timestamp, a bool, a negative int64 and a NULL ("NULL")"""
    n = 3000
    rng = np.random.default_rng(9)
    SS = dict(t=K.T_TIMESTAMP64, nu=K.T_UINT64, x=K.T_UINT64)
    w = E.Writer([dict(name="t", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_LEB128),
                  dict(name="nu", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128,
                       dlevel_max=1),
                  dict(name="x", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)])
    w.put("t", np.uint64(1438055327000000) + rng.integers(0, 40, n).astype(np.uint64) * np.uint64(1000003))
    # (values of 1, 10, 19 and 20 digits)
    w.put("nu", rng.choice(np.array([0, 7, 1234567890, 10 ** 18, 2 ** 64 - 1], dtype=np.uint64), n),
          present=(rng.random(n) < 0.7).astype(np.uint8))
    w.put("x", np.arange(n, dtype=np.uint64))
    w.commit(n)
    img = w.image()
    w.close()
    t = ctx.open_image(img)
    try:
        tt, nu, xx = col("t"), col("nu"), col("x")
        keys = [f("to_string", tt), f("to_string", nu), f("to_string", xx % 2 > 0),
                f("concat", f("to_string", f("to_int64", xx % 5) - 2), f("to_string", nu))]
        for key in keys:
            plan = Plan(SS, select=[key, count(1), sum_(xx)], group_by=[key])
            exp = O.oracle_run(img, plan)
            got = run(t, plan)
            assert not isinstance(got, str), got
            assert canon(*got) == canon(exp.types, exp.rows())
    finally:
        t.close()


def test_values_across_page_and_chunk_borders(ctx):
    """the table of test_gpu_strings.py::test_every_header_width_and_chunk_border (values of
    up to 600,000 bytes that straddle 4096-byte chunk and 512 KiB page borders): the case map
    walks every byte of every value, the compare stops at the first"""
    rng = np.random.default_rng(12)
    lens = [0, 1, 2, 126, 127, 128, 129, 255, 256, 1000, 1022, 1023, 1024, 1025, 4090, 4095,
            4096, 4097, 8191, 8192, 16383, 16384, 16385, 40000, 61000, 65535, 65536, 70000,
            200000, 600000]
    vals = []
    for rep in range(6):
        for L in lens:
            vals.append(bytes(rng.integers(0, 256, L, dtype=np.uint8)))
            for _ in range(int(rng.integers(0, 40))):
                vals.append(b"q%d" % rng.integers(0, 1000))
    for target in range(6):
        vals.append(b"z" * 50)
    img = build(vals, vals, np.ones(len(vals), dtype=np.uint8))
    t = ctx.open_image(img)
    try:
        key = f("lcase", s)
        kw = dict(select=[key, count(1), sum_(x)], group_by=[key], where=f("gte", f("ucase", s), Lit("M")))
        plan = Plan(S, **kw)
        exp = O.oracle_run(img, plan)
        got = run(t, plan)
        assert not isinstance(got, str), got
        assert canon(*got) == canon(exp.types, exp.rows())
    finally:
        t.close()


@pytest.mark.parametrize("name", ["one-row", "three-empty", "all-null"])
def test_tiny_tables(ctx, name):
    svals, nsvals, present = {
        "one-row": ([b"Only"], [b"Only"], [1]),
        "three-empty": ([b"", b"", b""], [b"", b"", b""], [1, 1, 1]),
        "all-null": ([b"a", b"B", b"c"], [b"", b"", b""], [0, 0, 0]),
    }[name]
    img = build(svals, nsvals, np.array(present, dtype=np.uint8))
    t = ctx.open_image(img)
    try:
        for kw in (keyed(f("lcase", s)), keyed(f("concat", f("ucase", ns), f("to_string", x))),
                   dict(select=[count(1)], where=f("rtrim", ns).eq(""))):
            check_against_oracle(t, img, kw)
    finally:
        t.close()


def test_partitioned_path(ctx):
    """groups_hint beyond the LDS slots: one group per row, and the same key with a handful
    of distinct values (the shape that once overflowed a partition cursor)"""
    n = 400_000
    rng = np.random.default_rng(31)
    u = rng.integers(0, 1000, n)
    vals = [b"G%d/" % v for v in u]  # (the separator keeps "G1" + "23" apart from "G12" + "3")
    img = build(vals, vals, np.ones(n, dtype=np.uint8))
    few = [b"v%d" % (v % 13) for v in u]
    img_few = build(few, few, np.ones(n, dtype=np.uint8))
    for image, key, groups in ((img, f("concat", s, f("to_string", x)), n),
                               (img_few, f("concat", s, f("to_string", x % 1)), 13)):
        t = ctx.open_image(image)
        try:
            plan = Plan(S, select=[key, count(1), sum_(x)], group_by=[key], groups_hint=400000)
            q = t.query(plan)
            assert "evql_part_scatter" in q.kernel_source()
            got = q.run()
            q.close()
            exp = O.oracle_run(image, plan)
            assert exp.nrows == groups == got.nrows
            assert sorted(got.rows()) == sorted(exp.rows())
        finally:
            t.close()


def test_exchange_between_two_ranks():
    """two hub ranks on one GPU, GROUP BY lcase(s): the merged groups are the oracle's over
    the concatenated tables"""
    def part(seed, n):
        rng = np.random.default_rng(seed)
        v = [(b"Key-%d" if i % 2 else b"KEY-%d") % (i % 700) for i in rng.integers(0, 1 << 20, n)]
        return v
    parts = [part(1, 30_000), part(2, 35_000)]
    key = f("lcase", s)
    kw = dict(select=[key, count(1), sum_(x)], group_by=[key])

    def image(vals):
        return build(vals, vals, np.ones(len(vals), dtype=np.uint8))
    hub = E.Hub(2)
    out, errs = [None, None], []

    def work(r):
        try:
            ctx = E.Context(0)
            t = ctx.open_image(image(parts[r]))
            q = t.query(Plan(S, **kw))
            xch = E.Exchange.hub(ctx, hub, r)
            q.execute()
            q.exchange(xch, K.EXCHANGE_GATHER_ALL)
            res = q.fetch_all()
            out[r] = (res.types, res.rows())
            q.close()
            xch.close()
            t.close()
            ctx.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
            raise
    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for tt in th:
        tt.start()
    for tt in th:
        tt.join(timeout=300)
    assert not any(tt.is_alive() for tt in th), "a rank hangs"
    assert not errs, errs
    hub.close()
    exp = O.oracle_run(image(parts[0] + parts[1]), Plan(S, **kw))
    assert exp.nrows == 700
    # (x is the row number inside a rank's own table: its sums are added up here)
    sums = {}
    for vals in parts:
        for i, v in enumerate(vals):
            sums[v.lower()] = sums.get(v.lower(), 0) + i
    want = {r[0]: (r[1], sums[r[0]]) for r in exp.rows()}
    for types, rows in out:
        assert {r[0]: (r[1], r[2]) for r in rows} == want
