"""ORDER BY .. LIMIT .. OFFSET pushed into the operator (evql_query_set_order) against the
plain Python model of order_edges.py, bit for bit: k_order_keys on signed sums / min / max /
keys, negative doubles, -0.0 / +0.0, all-NULL min / mean (they read 0, in the middle of the
order), the key 2^64 - 1 (kind 1) and the NULL key (kind 2); the radix select at every cut
of ~160 groups (byte clusters for each of its eight passes, the d < 255 stop of the digit
walk); k_order_collect taking as many boundary ties as needed (one sort key) or all of them
(several); the dense records of the partitioned path; and the refusals of query_set_order.
test_order_edges_cpu.py holds the same model against the oracle on the same cases.

One query per plan: set_order, execute, fetch for every cut (the kernel is compiled once).
set_order belongs before execute (include/evql_gpu.h); a second fetch without a new execute
is not part of the contract, and on the partitioned path it would not see the dense records
again (the fetch leaves the number of fetched groups in the field their view is cut to).

Two changes of the selection show in no result, so no case here can tell them: dropping the
kind-2 test of from_ident in k_order_keys (every writer of the NULL slot stores the identity
0 already), and `hist[d] <= remaining` in the digit walk (where a bucket ends exactly at the
cut it selects the next larger key and wants none of its ties: the same records)."""
import pytest

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Order, Plan, col, count, out, sum_
import order_edges as X

pytestmark = pytest.mark.gpu


def run_cases(q, plan, model, cases, where):
    for case in cases:
        specs, limit, offset = case
        q.set_order(X.order_of(plan, case))
        got = q.run()
        assert q.stats()["num_groups"] == len(model.rows), where   # the groups before LIMIT
        model.check(got.rows(), specs, limit, offset, where)


@pytest.fixture(scope="module")
def edge(ctx):
    img, _ = X.edge_table()
    t = ctx.open_image(img)
    yield t
    t.close()


@pytest.fixture(scope="module")
def main(edge):
    plan = X.main_plan()
    q = edge.query(plan)
    src = q.kernel_source()
    assert "evql_part_scatter" not in src     # the LDS path: records come from k_table_compact
    yield q, plan
    q.close()


@pytest.mark.parametrize("single", [False, True], ids=["then_g", "alone"])
@pytest.mark.parametrize("c", X.SORT_COLUMNS, ids=["%s_%s" % a for a in X.MAIN_AGGS])
def test_main_plan_sweeps(main, c, single):
    """every cut 1 .. G-1 ascending, every seventh and every cut inside a tie run or a byte
    cluster descending, offset 0 and want - 1.  Sort column c then g: a total order, row by
    row.  c alone: the order of ties is free -- the key sequence, every row against the
    model's row of its group, no group twice"""
    q, plan = main
    m = X.main_model()
    run_cases(q, plan, m, X.sweep(m, c, single, X.main_cluster_keys()), "device")


def test_second_keys_pick_among_the_ties(main):
    """two sort keys, the cut inside a tie set of the first (zeros, NULLs that read 0,
    counts): every boundary tie has to leave the device (max_eq = n)"""
    q, plan = main
    run_cases(q, plan, X.main_model(), X.second_key_cases(), "device")


def test_order_without_limit_and_limit_zero(main):
    q, plan = main
    m = X.main_model()
    G = len(m.rows)
    run_cases(q, plan, m, [(((1, False), (0, False)), None, 0), (((8, True), (0, False)), 0, 3),
                           (((2, False), (0, False)), 50, G - 7), (((9, True),), G + 5, 0)], "device")


@pytest.mark.parametrize("name", list(X.VARIANTS))
def test_key_variants(edge, name):
    """the group key itself as sort key 0 (from_ident): signed, float, nullable"""
    aggs, m = X.variant(name)
    plan = X.make_plan(X.SCHEMA, aggs)
    q = edge.query(plan)
    try:
        run_cases(q, plan, m, X.variant_cases(name), "device " + name)
    finally:
        q.close()


@pytest.fixture(scope="module")
def dense(ctx):
    img, _ = X.dense_table()
    t = ctx.open_image(img)
    yield t
    t.close()


@pytest.mark.parametrize("hint", X.DENSE_HINTS)
def test_dense_records(dense, hint):
    """70,001 groups through the partitioned path (scatter only; scatter and refine): the
    selection runs over its dense records"""
    plan = X.dense_plan(groups_hint=hint)
    q = dense.query(plan)
    try:
        src = q.kernel_source()
        assert "evql_part_scatter" in src
        assert ("evql_part_refine" in src) == (hint > 100_000)
        run_cases(q, plan, X.dense_model(), X.dense_cases(), "device hint %d" % hint)
    finally:
        q.close()


def test_refusals(edge, dense):
    """what query_set_order does not fuse, by code and message"""
    def refused(t, plan, order_args, code, fragment):
        q = t.query(plan)
        try:
            with pytest.raises(E.EvqlError) as ei:
                q.set_order(Order(plan, *order_args[0], **order_args[1]))
            assert ei.value.code == code and fragment in ei.value.msg, (ei.value.code, ei.value.msg)
        finally:
            q.close()

    g = [col("g")]
    exact = Plan(X.DENSE_SCHEMA, select=[col("g"), sum_(col("x"))], group_by=g,
                 float_sum_mode=K.FLOAT_SUM_EXACT)
    refused(dense, exact, (([(1, True)],), dict(limit=10)), K.EVQL_ENOTSUP, "exact float sum")
    plain = Plan(X.SCHEMA, select=[col("g"), count(1)], group_by=g)
    refused(edge, plain, (([(out(1) > 1, False)],), dict(limit=10)), K.EVQL_EARG, "no comparator")
    refused(edge, plain, (([(0, False), (out(1) > 1, False)],), dict(limit=10)), K.EVQL_EARG,
            "no comparator")
    partial = Plan(X.SCHEMA, select=[col("g"), count(1)], group_by=g, mode=K.MODE_PARTIAL)
    refused(edge, partial, (([(0, False)],), dict(limit=10)), K.EVQL_EARG, "partial aggregate")
    refused(edge, plain, (([],), dict()), K.EVQL_EARG, "no sort specs")
