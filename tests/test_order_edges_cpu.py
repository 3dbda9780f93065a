"""The ORDER BY / LIMIT model of order_edges.py against the C oracle (OrderByExpression +
LimitExpression restated in oracle/csql_order.inc) on every case of both tables, no GPU: the
model and the inputs are sound before any device run, and the oracle's qsort restatement
sees signed, negative-float, +-0 and NULL-reads-0 sort keys.  A disagreement of the device
with the same model is then a device finding."""
import pytest

from eventql_amd import capi as K
import oracle_lib as O
import order_edges as X


def run_cases(img, plan, model, cases, where):
    for case in cases:
        specs, limit, offset = case
        got = O.oracle_run(img, plan, order=X.order_of(plan, case)).rows()
        model.check(got, specs, limit, offset, where)


def test_the_tables_hold_their_edges():
    """what the cases rely on, read back from the tables"""
    groups = X.edge_groups()
    single = [rs[0] for _, _, rs in groups if len(rs) == 1]
    us = {X.signed(r[0]) for r in single}
    assert set(X.U_EDGES) <= us and -1 in us and -2 ** 63 in us and 2 ** 63 - 1 in us
    for j in range(8):   # per byte a cluster that differs first there; 0x00, 0x80, 0xff occur
        c = X.CLUSTERS[j]
        assert len(c) >= 3 and len({v >> (8 * (j + 1)) for v in c}) == 1
        assert {0x00, 0x80, 0xFF} <= {(v >> (8 * j)) & 0xFF for v in c}
        assert {v & X.M64 for v in c} <= {r[0] for r in single}
    xb = [X.bits(r[1]) for r in single]
    assert {X.bits(v) for v in X.X_EDGES} <= set(xb)
    assert xb.count(X.bits(-0.0)) >= 2 and xb.count(X.bits(0.0)) >= 2
    all_null = [rs for _, _, rs in groups if all(r[2] is None and r[3] is None for r in rs)]
    assert len(all_null) >= 3
    for k in (2, 3):     # nullable columns: negative and positive values next to the NULLs
        vals = [X.signed(r[k]) if k == 3 else r[k] for _, _, rs in groups for r in rs if r[k] is not None]
        assert min(vals) < 0 < max(vals)
    assert sum(1 for _, _, rs in groups if 2 <= len(rs) <= 4) >= 3
    m = X.main_model()
    assert 150 <= len(m.rows) <= 200
    # an all-NULL min / mean reads 0 in the middle of the order: rows on both sides of it
    # (column 11, min(to_int64(nu)): to_int64(NULL) is the value 0, never a NULL)
    assert all(r[11] is not None for r in m.rows) and any(r[11] < 0 for r in m.rows)
    assert {g for g, _, rs in groups if all(r[3] is None for r in rs)} <= {r[0] for r in m.rows if r[11] == 0}
    for c in (9, 10):
        rows = m.ordered(((c, False), (0, False)))
        first = next(i for i, r in enumerate(rows) if r[c] is None)
        last = max(i for i, r in enumerate(rows) if r[c] is None)
        assert 0 < first and last < len(rows) - 1
        assert X.cmp_cell(rows[0][c], None) < 0 < X.cmp_cell(rows[-1][c], None)
    # single-key cuts with the zero ties and the all-NULL ties on both sides (max_eq = remaining)
    for c, tied in ((6, lambda v: v == 0), (9, lambda v: v is None)):
        rows = m.ordered(((c, False),))
        idx = [i for i, r in enumerate(rows) if tied(r[c])]
        assert len(idx) >= 3 and any(idx[0] < want <= idx[-1] for _, want, off in
                                     X.sweep(m, c, True) if off == 0)
    d = X.dense_model()
    assert len(d.rows) == X.DENSE_G
    rows = d.ordered(((4, False), (0, False)))
    assert rows[4400][4] == rows[4399][4] == -7 and rows[4374][4] == -8   # the cut is inside a tie set


def test_the_model_itself():
    """hand-checked orders"""
    rows = [(1, -1, None), (2, 0, -0.0), (3, None, 0.0), (4, 2 ** 63 - 1, -5e-324), (5, -2 ** 63, 1.0)]
    assert [r[0] for r in X.ordered(rows, ((1, False), (0, False)))] == [5, 1, 2, 3, 4]
    assert [r[0] for r in X.ordered(rows, ((1, True), (0, False)))] == [4, 2, 3, 1, 5]
    assert [r[0] for r in X.ordered(rows, ((2, False), (0, True)))] == [4, 3, 2, 1, 5]
    urows = [(1, X.M64), (2, 0), (3, 1 << 63), (4, None)]   # unsigned: 2^64 - 1 is the largest
    assert [r[0] for r in X.ordered(urows, ((1, False), (0, False)))] == [2, 4, 3, 1]
    assert X.limited(rows, 0, 1) == [] and X.limited(rows, 2, 4) == rows[4:] and X.limited(rows, None, 3) == rows
    assert X.tie_cuts([(0, 1), (1, 1), (2, 1), (3, 2)], 1) == {1, 2}
    assert X.sig((0.0, -0.0)) != X.sig((0.0, 0.0)) and X.sig((0.0, -0.0), {1}) == X.sig((0.0, 0.0), {1})
    assert X.sig((1,)) != X.sig((1.0,))
    assert X.agg_cell("isum", [X.M64, X.M64 - 1], False) == -3
    assert X.agg_cell("sum", [X.M64, 2], False) == 1
    assert X.agg_cell("imin", [1, X.M64, None], False) == -1 and X.agg_cell("min", [1, X.M64], False) == 1
    assert X.agg_cell("mean", [None, None], True) is None and X.agg_cell("mean", [1.0, None, 0.5], True) == 0.75
    assert X.agg_cell("mean", [0.25, 0.5, 0.25], True) == 1.0 / 3.0
    with pytest.raises(AssertionError):
        X.check_rows([(1, -0.0)], [(1, 0.0)], frozenset(), "")
    X.check_rows([(1, -0.0)], [(1, 0.0)], frozenset({1}), "")
    by = {X.sig((1,)): X.sig((1, 5)), X.sig((2,)): X.sig((2, 5))}
    X.check_ties_free([(2, 5)], ([(1, 5)], by), 1, frozenset(), "")
    with pytest.raises(AssertionError):       # a group twice
        X.check_ties_free([(2, 5), (2, 5)], ([(1, 5), (2, 5)], by), 1, frozenset(), "")
    with pytest.raises(AssertionError):       # the right key on a wrong row
        X.check_ties_free([(1, 5)], ([(1, 5)], {X.sig((1,)): X.sig((1, 6))}), 1, frozenset(), "")


@pytest.mark.parametrize("single", [False, True], ids=["then_g", "alone"])
@pytest.mark.parametrize("c", X.SORT_COLUMNS, ids=["%s_%s" % a for a in X.MAIN_AGGS])
def test_oracle_main_plan_sweeps(built, c, single):
    """every cut ascending, the thinned sweep descending; sort column c then g (a total
    order: row by row), and c alone (ties free)"""
    img, _ = X.edge_table()
    m = X.main_model()
    plan = X.main_plan()
    if c != 0 and not single:
        assert m.total(((c, False), (0, False)))
    run_cases(img, plan, m, X.sweep(m, c, single, X.main_cluster_keys()), "oracle")


def test_oracle_second_keys_pick_among_the_ties(built):
    img, _ = X.edge_table()
    run_cases(img, X.main_plan(), X.main_model(), X.second_key_cases(), "oracle")


@pytest.mark.parametrize("name", list(X.VARIANTS))
def test_oracle_key_variants(built, name):
    img, _ = X.edge_table()
    aggs, m = X.variant(name)
    run_cases(img, X.make_plan(X.SCHEMA, aggs), m, X.variant_cases(name), "oracle " + name)


def test_oracle_dense_table(built):
    img, _ = X.dense_table()
    run_cases(img, X.dense_plan(), X.dense_model(), X.dense_cases(), "oracle dense")


def test_oracle_order_without_limit_and_limit_zero(built):
    """ORDER BY alone returns every group; LIMIT 0 nothing; a LIMIT past the end the rest"""
    img, _ = X.edge_table()
    m, plan = X.main_model(), X.main_plan()
    G = len(m.rows)
    run_cases(img, plan, m, [(((1, False), (0, False)), None, 0), (((8, True), (0, False)), 0, 3),
                             (((2, False), (0, False)), 50, G - 7), (((9, True),), G + 5, 0)], "oracle")
    assert K.T_INT64 == m.types[1] and K.T_FLOAT64 == m.types[8]
