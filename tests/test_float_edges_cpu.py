"""The exact reference of float_edges.py against the oracle on the IEEE edge tables, no GPU:
the oracle's float sums and means lie within the reference's bounds, its min / max / NULL /
integer columns equal it bit for bit -- over the whole table, under a WHERE, and as
PARTIAL frames of row ranges merged by the oracle's merge.  A disagreement of the device
with the same reference is then a device finding, not a reference bug."""
import math

import numpy as np
import pytest

from eventql_amd import capi as K
from eventql_amd.plan import Plan, col, count, sum_
import oracle_lib as O
import float_edges as F

S = F.SCHEMA
_REF = {}


def ref(aggs, where):
    k = (aggs, where)
    if k not in _REF:
        c = F.main_columns()
        _REF[k] = F.reference(c, aggs, F.where_mask(c) if where else None)
    return _REF[k]


@pytest.mark.parametrize("where", [False, True], ids=["all", "where"])
@pytest.mark.parametrize("aggs", [F.FLOAT_AGGS, F.INT_AGGS], ids=["float", "int"])
@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_oracle_within_the_reference(built, layout, aggs, where):
    img, _ = F.main_table(layout)
    plan = Plan(S, select=F.select(aggs), group_by=[col("g")], where=F.WHERE if where else None)
    F.check_strict(O.oracle_run(img, plan).rows(), ref(aggs, where), where=layout)


@pytest.mark.parametrize("aggs", [F.FLOAT_AGGS, F.INT_AGGS], ids=["float", "int"])
def test_oracle_partial_frames_merged(built, aggs):
    """PARTIAL frames of three row ranges of the strided table, merged by the oracle"""
    img, c = F.main_table("strided")
    n = len(c["g"])
    kw = dict(select=F.select(aggs), group_by=[col("g")], where=F.WHERE)
    frames = []
    for lo, hi in ((0, 333_334), (333_334, 700_001), (700_001, n)):
        mask = np.zeros(n, np.uint8)
        mask[lo:hi] = 1
        frames.append(O.oracle_partial_frame(img, Plan(S, mode=K.MODE_PARTIAL, row_filter=mask, **kw)))
    got = O.oracle_merge(Plan(S, **kw), frames)
    F.check_strict(got.rows(), ref(aggs, True), where="merged")


def test_oracle_global_and_wide(built):
    """no GROUP BY, one class at a time; and the 75,600-group table"""
    c = F.main_columns()
    for name in ("subnormals", "cancel", "zeros_neg_first", "magnitudes", "all_null"):
        d = F.by_class(c, [name])
        plan = Plan(S, select=F.select(F.FLOAT_AGGS, key=None))
        F.check_strict(O.oracle_run(F.image_of(d), plan).rows(),
                       F.reference(d, F.FLOAT_AGGS, key=None), key_cols=0, where=name)
    img, c = F.wide_table()
    assert len(np.unique(c["g"])) >= 70_000
    plan = Plan(S, select=F.select(F.FLOAT_AGGS), group_by=[col("g")])
    F.check_strict(O.oracle_run(img, plan).rows(), F.reference(c, F.FLOAT_AGGS), where="wide")


def test_float_keys_group_by_their_bits(built):
    """-0.0 / +0.0, three NaN bit patterns (one of them all ones) and +-inf are distinct keys"""
    img, c = F.float_key_table()
    plan = Plan(F.FKEY_SCHEMA, select=[col("fk"), count(1), sum_(col("v"))], group_by=[col("fk")])
    got = O.oracle_run(img, plan).rows()
    assert len(got) == len(F.FKEY_VALUES)
    F.check_strict(got, F.float_key_reference(c))


def test_the_reference_itself():
    """hand-checked cases of the reference and the comparator"""
    assert F.exact_quantum_exp(1000.0) == 10 - 61
    assert F.exact_quantum_exp(1024.0) == 11 - 61
    assert F.exact_quantum_exp(math.nextafter(1024.0, 0.0)) == 10 - 61
    assert F.exact_quantum_exp(2.0 ** -962) == -1022 and F.exact_quantum_exp(1e-300) == -1023
    assert F.exact_quantum_exp(F.SUBMAX) == -1023
    # under the clamped quantum 2^-1023: 2^-1074 rounds to 0, 2^-1023 stays, a tie goes even
    assert F.exact_mode_sum([F.TINY] * 5, -1023) == 0.0
    assert F.exact_mode_sum([2.0 ** -1023] * 3, -1023) == 3 * 2.0 ** -1023
    assert F.exact_mode_sum([1.5 * 2.0 ** -1023, 2.5 * 2.0 ** -1023], -1023) == 4 * 2.0 ** -1023
    assert F.exact_mode_sum([1.0, -1.0], -60) == 0.0
    # sums: specials by class, overflow of one sign, exact cancellation
    sc = F._sum_cell
    assert sc([1.0, F.NAN], 1)[1] != sc([1.0, F.NAN], 1)[1]
    assert sc([F.INF, -F.INF], 1)[1] != sc([F.INF, -F.INF], 1)[1]
    assert sc([0.6 * F.DMAX] * 3, 1)[1] == F.INF
    assert sc([1e16, 1.0, -1e16], 1)[1] == 1
    F.check_cell(1.0, sc([1e16, 1.0, -1e16], 1))
    with pytest.raises(AssertionError):
        F.check_cell(2.0 + 1e-9, sc([1.0, 1.0], 1))
    with pytest.raises(AssertionError):
        F.check_cell(-0.0, sc([-0.0, -0.0], 1))                   # a zero sum is +0.0
    with pytest.raises(AssertionError):
        F.check_cell(0.0, sc([F.TINY] * 4, 1))                    # a flushed subnormal sum
    mm = F._minmax_cell([0.0, F.NAN, 1.0], True)
    F.check_cell(0.0, mm)
    with pytest.raises(AssertionError):
        F.check_cell(-0.0, mm)                                    # -0.0 is not in the group
    with pytest.raises(AssertionError):
        F.check_cell(1e-310, F._minmax_cell([F.SUBMAX], True))    # min / max are exact
