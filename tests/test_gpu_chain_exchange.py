"""evql_query_create_chain followed by evql_query_exchange: a GROUP BY over partitions that
sit on several ranks, where a partition is a chain of LSM files (one operator over the
chain, chain_merge) and the chain heads then exchange their merged groups.

Ranks are threads of this process on the one GPU, joined by the in-process hub, every rank
with its own context and its own LsmChain over a partition of tests/lsm_tables.py.  The
expected rows are the oracle's PartitionCursor restatement (oracle_run_chain) over the
concatenation of all ranks' files in scan order, rank after rank, each file under its own
partition's filter: one GroupByExpression over everything, so a non-aggregate select
expression keeps the first row of the lowest rank, inside a rank of the first file in scan
order, inside a file of the first row."""
import functools
import threading

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Agg, Plan, col, count, sum_, min_, max_, mean
import lsm_nested_tables as LN
import lsm_tables as LT
import oracle_lib as O
import sqlgen
import tables as T
from test_ref_csql_cpu import check_partial

pytestmark = pytest.mark.gpu

S = LT.LSM_SCHEMA
GATHER, OWNER = K.EXCHANGE_GATHER_ALL, K.EXCHANGE_BY_OWNER
JOIN_TIMEOUT = 120


# ---------------------------------------------------------------------------------------
# ranks: ("chain", tables module, partition) -- an LsmChain over the partition's files --
# or ("plain", tables module, partition): the partition's oldest file opened as a table
# of its own, queried without a chain (and without a filter)
# ---------------------------------------------------------------------------------------
_filters = {}


def spec_files(spec):
    """(images, filters) of a rank in scan order"""
    kind, mod, pname = spec
    if kind == "plain":
        return [mod.partition(pname)[0][1]], [None]
    if (mod.__name__, pname) not in _filters:
        _filters[(mod.__name__, pname)] = O.oracle_partition_filters(mod.partition(pname))
    return [f[1] for f in reversed(mod.partition(pname))], list(_filters[(mod.__name__, pname)])


class ExtraPartitions:
    """partitions beside those of lsm_tables, built the same way from seeds of their own:
    the same rids as there, other values in every other column"""
    __name__ = "extra"
    PARTITIONS = {"wide": (311, [(30_000, 0, 1)])}

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def partition(name):
        seed, files = ExtraPartitions.PARTITIONS[name]
        rng = np.random.default_rng(seed)
        id_space = max(4, sum(f[0] for f in files) // 2)
        out = []
        for fi, (nrows, skl, upd) in enumerate(files):
            img, cols = LT._file_image(rng, fi, nrows, bool(skl), id_space)
            out.append(("%s_%02d" % (name, fi), img, bool(skl), bool(upd), cols))
        return out


EXTRA = ExtraPartitions()

_expected = {}


def expected(specs, plan_name, plan):
    """oracle_run_chain over the files of all ranks, in rank order (computed once per case)"""
    key = (tuple((k, m.__name__, p) for k, m, p in specs), plan_name)
    if key not in _expected:
        imgs, flts = [], []
        for sp in specs:
            i, f = spec_files(sp)
            imgs += i
            flts += f
        _expected[key] = O.oracle_run_chain(imgs, flts, plan)
    return _expected[key]


class RankEnv:
    def __init__(self, rank, spec, hub):
        kind, mod, pname = spec
        self.ctx = E.Context(0)
        self.chain = None
        if kind == "chain":
            files = list(reversed(mod.partition(pname)))
            self.tabs = [self.ctx.open_image(f[1]) for f in files]
            self.chain = E.LsmChain(self.ctx)
            for t, f in zip(self.tabs, files):
                self.chain.add(t, has_skiplist=f[2], has_updates=f[3])
            self.chain.build()
        else:
            self.tabs = [self.ctx.open_image(mod.partition(pname)[0][1])]
        self.x = E.Exchange.hub(self.ctx, hub, rank)

    def query(self, plan):
        return (self.chain or self.tabs[0]).query(plan)

    def close(self):
        self.x.close()
        if self.chain:
            self.chain.close()
        for t in self.tabs:
            t.close()
        self.ctx.close()


def run_ranks(specs, body):
    """body(rank, env) on one daemon thread per rank -> list of its return values"""
    n = len(specs)
    hub = E.Hub(n)
    out, errs = [None] * n, []

    def work(r):
        try:
            env = RankEnv(r, specs[r], hub)
            out[r] = body(r, env)
            env.close()
        except Exception as e:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            errs.append((r, e))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_TIMEOUT)
    assert not any(t.is_alive() for t in th), "a rank hangs (errors so far: %r)" % (errs,)
    assert not errs, errs
    hub.close()
    return out


def exchange_body(schema, kw, modes):
    """execute + exchange + fetch once per mode on ONE operator (a Plan per rank)"""
    def body(r, env):
        q = env.query(Plan(schema, **kw))
        res = {}
        for mode in modes:
            q.execute()
            q.exchange(env.x, mode)
            got = q.fetch_all()
            res[mode] = (got.rows(), got.types, env.x.stats())
        q.close()
        return res
    return body


def check_modes(res, exp, key_cols):
    """GATHER_ALL: the whole result, bit-identical on every rank; BY_OWNER: disjoint shares"""
    for out in res:
        rows = out[GATHER][0]
        assert len(rows) == exp.nrows
        T.compare_results(rows, exp.rows(), exp.types, key_cols=key_cols, rel=1e-9)
    canon = [sorted(map(repr, out[GATHER][0])) for out in res]
    assert all(c == canon[0] for c in canon[1:])
    union = [row for out in res for row in out[OWNER][0]]
    assert len(union) == exp.nrows
    T.compare_results(union, exp.rows(), exp.types, key_cols=key_cols, rel=1e-9)
    if exp.nrows > 50:
        assert all(len(out[OWNER][0]) > 0 for out in res), "a rank owns nothing"


# ---------------------------------------------------------------------------------------
# 1. plans x {2, 3} ranks x both modes
# ---------------------------------------------------------------------------------------
RANKS = [("chain", LT, "basic"), ("chain", LT, "quiet"), ("chain", LT, "mixed")]

PLANS = {
    "u64-key": dict(select=[col("k"), count(1), sum_(col("a")), sum_(col("v")), min_(col("v")),
                            max_(col("a")), mean(col("v"))], group_by=[col("k")]),
    # thousands of groups; every rank holds the same rids
    "rid-key": dict(select=[col("rid"), count(1), sum_(col("a"))], group_by=[col("rid")]),
    # the NULL key's group sits in a slot of its own
    "nullable-key": dict(select=[col("n"), count(1), sum_(col("a"))], group_by=[col("n")]),
    # first rows and string heaps; "" is one of the keys
    "string-key": dict(select=[col("s"), count(1), sum_(col("a")), max_(col("v"))],
                       group_by=[col("s")]),
    "two-keys": dict(select=[col("k"), col("s"), count(1), sum_(col("n"))],
                     group_by=[col("k"), col("s")], key_cols=2),
    "where": dict(select=[col("k"), count(1), sum_(col("v"))], group_by=[col("k")],
                  where=(col("a") > 30000) & (col("s") >= "g2")),
    "global": dict(select=[count(1), sum_(col("a")), max_(col("v"))], group_by=[], key_cols=0),
    "distinct-by-k": dict(select=[col("k"), Agg("count_distinct", col("a") % 97), count(1)],
                          group_by=[col("k")]),
    "distinct-global": dict(select=[Agg("count_distinct", col("k")), count(1)], group_by=[],
                            key_cols=0),
}


@pytest.mark.parametrize("name", sorted(PLANS))
@pytest.mark.parametrize("nranks", [2, 3])
def test_chain_heads_exchange_against_the_oracle(name, nranks):
    kw = dict(PLANS[name])
    kc = kw.pop("key_cols", 1)
    specs = RANKS[:nranks]
    exp = expected(specs, name, Plan(S, **kw))
    res = run_ranks(specs, exchange_body(S, kw, [GATHER, OWNER]))
    check_modes(res, exp, kc)


@pytest.mark.parametrize("nranks", [2, 3])
def test_partial_rows_with_count_distinct_of_exchanged_chains(nranks):
    """EVQL_MODE_PARTIAL + count_distinct: the chains' merged pair sets are the source of the
    exchange, and the PartialGroupByExpression rows emitted afterwards carry the values of
    the sets merged across the ranks -- byte for byte the oracle's partial rows over all
    files, and, read as one more partial frame, they merge to the final rows"""
    kw = dict(PLANS["distinct-by-k"])
    pkw = dict(kw, mode=K.MODE_PARTIAL)
    specs = RANKS[:nranks]
    ep = expected(specs, "distinct-by-k/partial", Plan(S, **pkw))
    final = expected(specs, "distinct-by-k", Plan(S, **kw))
    want = sorted((ep.keys[20 * i:20 * i + 20], ep.columns[0][i]) for i in range(ep.nrows))
    pairs = [[k.hex(), d.hex()] for k, d in want]
    fx = dict(nrows=len(pairs), sample=[(k, d[:256], len(d) // 2) for k, d in pairs[:8]],
              digest=sqlgen.rows_digest(pairs))
    res = run_ranks(specs, exchange_body(S, pkw, [GATHER, OWNER]))
    for out in res:
        rows = out[GATHER][0]
        assert sorted(rows) == want
        check_partial(fx, [r[0] for r in rows], [r[1] for r in rows])
        merged = O.oracle_merge(Plan(S, **kw), [O.partial_frame([r[0] for r in rows],
                                                                [r[1] for r in rows])])
        assert sorted(merged.rows()) == sorted(final.rows())
    union = [r for out in res for r in out[OWNER][0]]
    assert sorted(union) == want
    check_partial(fx, [r[0] for r in union], [r[1] for r in union])


# ---------------------------------------------------------------------------------------
# 2. first rows: one position word ordered by (rank, table, row)
# ---------------------------------------------------------------------------------------
FIRST = dict(select=[col("k"), col("s"), col("a"), count(1)], group_by=[col("k")])


@pytest.mark.parametrize("specs", [
    # (keyed by k every group of a chain has its first row in the chain's newest file, table
    # 0: these two cases pin the order of the RANKS; the table field is pinned below)
    [("chain", LT, "basic"), ("plain", LT, "single_plain")],
    [("plain", LT, "single_plain"), ("chain", LT, "mixed")],
], ids=["chain-then-plain", "plain-then-chain"])
def test_first_rows_of_mixed_ranks(specs):
    plan = Plan(S, **FIRST)
    imgs0, flt0 = spec_files(specs[0])
    first0 = {r[0]: (r[1], r[2]) for r in O.oracle_run_chain(imgs0, flt0, plan).rows()}
    assert len(first0) == 40
    both = expected(specs, "first", plan)
    counts = {r[0]: r[3] for r in both.rows()}
    res = run_ranks(specs, exchange_body(S, FIRST, [GATHER, OWNER]))
    for rows in [out[GATHER][0] for out in res] + [[r for out in res for r in out[OWNER][0]]]:
        assert len(rows) == both.nrows
        for k, s, a, c in rows:
            assert c == counts[k]
            if k in first0:
                assert (s, a) == first0[k], k
    # (the other rank's values where rank 0 has no such group: the oracle over everything)
    T.compare_results(res[1][GATHER][0], both.rows(), both.types)


@pytest.mark.parametrize("specs,bucketed", [
    ([("chain", LT, "basic"), ("plain", LT, "single_plain")], False),
    ([("chain", LT, "big"), ("plain", EXTRA, "wide")], True),
], ids=["table-merge", "bucketed-merge"])
def test_a_later_file_of_rank_0_beats_rank_1(specs, bucketed):
    """The rank and table fields of the position word must not overlap.  Keyed by rid, the
    groups of a three-file chain on rank 0 sit in the file that wrote them: rids below 10^7
    in the oldest file, table 2 of the chain in scan order (position 2 << 44 | row), rids from
    10^7 in table 1.  Rank 1 is ONE plain file that holds the rids from 0 too, with other
    values: at (1 << 44 | row), were the rank tagged at bit 44 -- smaller than rank 0's
    (2 << 44 | row).  With rank << (44 + tb) rank 0 wins every group it holds.

    The bucketed merge (2^18 records and more: 235,064 groups of `big` + 30,000) takes a
    group's first-row values from the record with the smallest position, so it is the case
    that fails when the fields overlap (checked once with tb forced to 0: rank 1's values
    come out).  The rank-ordered table merge of the small case takes them from the first
    batch that brings the group, whatever the positions: it pins that order."""
    kw = dict(select=[col("rid"), col("s"), col("a"), count(1)], group_by=[col("rid")])
    if bucketed:
        kw["groups_hint"] = 400_000
    plan = Plan(S, **kw)
    imgs0, flt0 = spec_files(specs[0])
    own0 = {r[0]: (r[1], r[2]) for r in O.oracle_run_chain(imgs0, flt0, plan).rows()}
    own1 = {r[0]: (r[1], r[2]) for r in O.oracle_run(spec_files(specs[1])[0][0], plan).rows()}
    # the case is what it claims: groups of rank 0 whose first row lies in table 2 / table 1,
    # and rank 1 holds table-2 ones with other values
    table2 = [rid for rid in own0 if rid < 10_000_000]
    table1 = [rid for rid in own0 if 10_000_000 <= rid < 20_000_000]
    assert len(table2) > 1000 and len(table1) > 500
    assert sum(rid in own1 and own0[rid] != own1[rid] for rid in table2) > 1000
    both = expected(specs, "first-rid", plan)
    counts = {r[0]: r[3] for r in both.rows()}
    res = run_ranks(specs, exchange_body(S, kw, [GATHER, OWNER]))
    assert all((out[GATHER][2]["merge_buckets"] != 0) == bucketed for out in res)
    for rows in [out[GATHER][0] for out in res] + [[r for out in res for r in out[OWNER][0]]]:
        assert len(rows) == both.nrows == len(set(own0) | set(own1))
        for rid, s, a, c in rows:
            assert c == counts[rid]
            assert (s, a) == (own0[rid] if rid in own0 else own1[rid]), rid


# ---------------------------------------------------------------------------------------
# 3. operator life cycle (one rank: what it sends is merged where it lies)
# ---------------------------------------------------------------------------------------
def test_life_cycle_of_an_exchanged_chain_head():
    specs = [("chain", LT, "basic")]
    kw = dict(select=[col("k"), col("s"), count(1), sum_(col("a")), sum_(col("v"))],
              group_by=[col("k")])
    exp = expected(specs, "life", Plan(S, **kw))

    def body(r, env):
        q = env.query(Plan(S, **kw))
        q.execute()
        # before any exchange: the chain's own result
        T.compare_results(q.fetch_all().rows(), exp.rows(), exp.types, rel=1e-9)
        for mode in (GATHER, OWNER):
            q.exchange(env.x, mode)
            T.compare_results(q.fetch_all().rows(), exp.rows(), exp.types, rel=1e-9)
            with pytest.raises(E.EvqlError) as ei:
                q.exchange(env.x, mode)
            assert ei.value.code == K.EVQL_EARG and "exchanged already" in ei.value.msg
            q.execute()
        T.compare_results(q.fetch_all().rows(), exp.rows(), exp.types, rel=1e-9)
        q.close()
        return True

    assert run_ranks(specs, body) == [True]


# ---------------------------------------------------------------------------------------
# 4. go / no-go: a refusal that only one rank can see reaches every rank
# ---------------------------------------------------------------------------------------
def test_a_rank_that_did_not_execute_refuses_for_everybody():
    specs = [("chain", LT, "basic"), ("chain", LT, "quiet")]
    kw = dict(PLANS["u64-key"])
    exp = expected(specs, "u64-key", Plan(S, **kw))

    def body(r, env):
        q = env.query(Plan(S, **kw))
        if r == 0:
            q.execute()
        with pytest.raises(E.EvqlError) as ei:
            q.exchange(env.x, GATHER)
        refusal = (ei.value.code, ei.value.msg)
        # no transport error: the same hub and exchange objects go on
        q.execute()
        q.exchange(env.x, GATHER)
        rows = q.fetch_all().rows()
        q.close()
        return refusal, rows

    res = run_ranks(specs, body)
    (code0, msg0), (code1, msg1) = res[0][0], res[1][0]
    assert code1 == K.EVQL_EARG and "execute() was not called" in msg1
    assert code0 == K.EVQL_ERUNTIME and "rank 1" in msg0, msg0
    for _, rows in res:
        T.compare_results(rows, exp.rows(), exp.types, rel=1e-9)


# ---------------------------------------------------------------------------------------
# 5. bucketed merge
# ---------------------------------------------------------------------------------------
def test_chain_heads_through_the_bucketed_merge():
    """Record sets of 2^18 records and more are merged bucket by bucket in the LDS.  The
    `big` chain (320,001 rows keyed by rid) keeps 235,064 groups under its filters and `basic`
    5,577: together 240,641, short of 2^18 = 262,144.  A third rank -- one plain file of 30,000
    rows from another seed: rids 0..29,999, which rank 0 holds too, with other values -- brings
    every rank to 270,641 received records; ranks 0 and 1 are the two the case names."""
    specs = [("chain", LT, "big"), ("chain", LT, "basic"), ("plain", EXTRA, "wide")]
    kw = dict(select=[col("rid"), col("s"), count(1), sum_(col("a"))], group_by=[col("rid")],
              groups_hint=400_000)
    plan = Plan(S, **kw)
    imgs0, flt0 = spec_files(specs[0])
    own0 = {r[0]: r[1] for r in O.oracle_run_chain(imgs0, flt0, plan).rows()}
    own2 = {r[0]: r[1] for r in O.oracle_run(spec_files(specs[2])[0][0], plan).rows()}
    assert sum(own0[rid] != s2 for rid, s2 in own2.items() if rid in own0) > 10_000
    exp = expected(specs, "big", plan)
    res = run_ranks(specs, exchange_body(S, kw, [GATHER]))
    assert all(out[GATHER][2]["merge_buckets"] != 0 for out in res), [out[GATHER][2] for out in res]
    want = {r[0]: (r[2], r[3]) for r in exp.rows()}
    for out in res[:2]:
        rows = out[GATHER][0]
        assert len(rows) == exp.nrows
        for rid, s, c, a in rows:
            assert (c, a) == want[rid], rid
            if rid in own0:
                assert s == own0[rid], rid
    assert sorted(map(repr, res[0][GATHER][0])) == sorted(map(repr, res[2][GATHER][0]))


# ---------------------------------------------------------------------------------------
# 6. nested chains
# ---------------------------------------------------------------------------------------
def nested_expected(specs, kw):
    """The oracle does not restate chains of nested scans (oracle_run_chain refuses them):
    as for the nested chains of one rank (test_gpu_nested_filter.oracle_chain), the expected
    rows are the oracle's partial aggregates of every file under its filter, merged by the
    oracle's GroupByMergeExpression.  (No non-aggregate select expression here: the order
    of the frames does not matter.)"""
    NS = LN.NESTED_LSM_SCHEMA
    frames = []
    for sp in specs:
        imgs, flts = spec_files(sp)
        for img, flt in zip(imgs, flts):
            r = O.oracle_run(img, Plan(NS, mode=K.MODE_PARTIAL, row_filter=flt, **kw))
            frames.append(O.partial_frame([r.keys[20 * i:20 * i + 20] for i in range(r.nrows)],
                                          r.columns[0]))
    return O.oracle_merge(Plan(NS, **kw), frames)


@pytest.mark.parametrize("name", ["leaf-key", "string-key"])
def test_nested_chain_heads_exchange(name):
    lpos, lprice = col("items.position"), col("items.price")
    kw = {"leaf-key": dict(select=[lpos, count(1), sum_(lprice)], group_by=[lpos]),
          "string-key": dict(select=[col("s"), count(1), sum_(lpos)], group_by=[col("s")])}[name]
    kw = dict(kw, scan_mode=K.SCAN_NESTED)
    specs = [("chain", LN, "basic"), ("chain", LN, "edges")]
    exp = nested_expected(specs, kw)
    res = run_ranks(specs, exchange_body(LN.NESTED_LSM_SCHEMA, kw, [GATHER, OWNER]))
    check_modes(res, exp, 1)


class MappedKey:
    """an expected result whose key column went through `fn` (NULL stays NULL)"""
    def __init__(self, exp, fn):
        self.types, self.nrows = exp.types, exp.nrows
        self._rows = [((None if r[0] is None else fn(r[0])),) + tuple(r[1:]) for r in exp.rows()]

    def rows(self):
        return self._rows


@pytest.mark.parametrize("name", ["leaf-key", "string-key", "leaf-expr"])
def test_nested_operators_without_a_chain_exchange(name):
    """Nested operators that are no chain heads (one file each, no filter): their first-row
    values -- flattened rows, one column of them with a narrow copy -- are resolved by the
    exchange itself.  `leaf-expr` evaluates its select expression on the group's first row;
    the value depends on the key alone, so which row is first does not matter: the expected
    rows are the oracle's for the bare key with the key mapped k -> 2k + 1."""
    lpos, lprice = col("items.position"), col("items.price")
    kw = {"leaf-key": dict(select=[lpos, count(1), sum_(lprice)], group_by=[lpos]),
          "string-key": dict(select=[col("s"), count(1), sum_(lpos)], group_by=[col("s")]),
          "leaf-expr": dict(select=[lpos * 2 + 1, count(1)], group_by=[lpos])}[name]
    kw = dict(kw, scan_mode=K.SCAN_NESTED)
    specs = [("plain", LN, "single_plain"), ("plain", LN, "single")]
    if name == "leaf-expr":
        exp = MappedKey(nested_expected(specs, dict(kw, select=[lpos, count(1)])),
                        lambda k: 2 * k + 1)
    else:
        exp = nested_expected(specs, kw)
    res = run_ranks(specs, exchange_body(LN.NESTED_LSM_SCHEMA, kw, [GATHER, OWNER]))
    check_modes(res, exp, 1)


# ---------------------------------------------------------------------------------------
# 7. a chain of one file (no chain_merge) beside a chain of several
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u64-key", "string-key"])
def test_one_file_chain_beside_a_multi_file_chain(name):
    kw = dict(PLANS[name])
    specs = [("chain", LT, "single_skip"), ("chain", LT, "basic")]
    exp = expected(specs, name, Plan(S, **kw))
    res = run_ranks(specs, exchange_body(S, kw, [GATHER, OWNER]))
    check_modes(res, exp, 1)
