"""ORDER BY .. LIMIT .. OFFSET above the GROUP BY (evql_query_set_order) on the sort keys where
the selection can go wrong without the result looking wrong: signed integers, negative
doubles, -0.0 / +0.0, all-NULL min / max / mean (they read 0, in the middle of a signed
order), the key 2^64 - 1 and the NULL key, and keys that differ in one byte only (one
cluster per pass of the radix select).

This module holds the tables, the case lists and a plain Python model:
  * aggregates per group from the column values with Python ints and fractions
  * the order with functools.cmp_to_key and the reference's comparators (boolean.cc:81-180,
    restated in oracle/csql_order.inc): payloads only, so a NULL (None) reads 0; INT64
    signed, UINT64 unsigned, FLOAT64 with < and > (so -0.0 == +0.0); DESC inverts
  * then rows[offset : offset + limit], limit 0 -> nothing
It uses neither the product nor the oracle.  test_order_edges_cpu.py holds the oracle
against it, test_gpu_order_edges.py the device.

NaN sort keys are out of scope: cmp_float64 with a NaN is no strict weak order (a NaN is
"equal" to everything, and equality is then not transitive), the reference's std::sort is
undefined on such input, so there is no answer to pin.  No group of these tables has a NaN
in a sortable column (asserted below).

Every comparison is of bits.  The one exception is the sign of a zero float sum (and of the
mean that is this sum divided by the count): the oracle starts a sum at +0.0, the device
may start it at the first value, and {-0.0} sums to a zero of either sign; both tie."""
import functools
from fractions import Fraction

import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Call, Order, Plan, col, count, max_, mean, min_, sum_
from float_edges import DMAX, INF, SUBMAX, TINY, bits, from_bits

M64 = (1 << 64) - 1


def signed(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---- the edge table --------------------------------------------------------------------------
SCHEMA = dict(g=K.T_UINT64, u=K.T_UINT64, x=K.T_FLOAT64, nx=K.T_FLOAT64, nu=K.T_UINT64)
COLUMNS = [
    dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="u", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="x", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="nx", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754, dlevel_max=1),
    dict(name="nu", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN, dlevel_max=1)]

# bit patterns of u, as signed values
U_EDGES = [-2 ** 63, -2 ** 63 + 1, -2 ** 56 - 1, -2 ** 56, -2 ** 56 + 1, -2 ** 48, -2 ** 32 - 1,
           -2 ** 32, -2 ** 32 + 1, -2 ** 31, -65537, -65536, -257, -256, -255, -2, -1,
           0, 1, 2, 255, 256, 257, 65535, 65536,
           2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 48, 2 ** 56 - 1, 2 ** 56, 2 ** 56 + 1,
           2 ** 63 - 2, 2 ** 63 - 1]
CLUSTER_DIGITS = (0x00, 0x7F, 0x80, 0xFF)


def byte_cluster(j):
    """four patterns that share every byte above j and differ first in byte j (digits 0x00,
    0x7f, 0x80, 0xff); the top byte alternates between a positive and a negative one.  Read
    as doubles they are finite (no exponent of all ones)"""
    hi = 0
    for k in range(7, j, -1):
        hi |= ((0xA0 + j if j % 2 else 0x30 + j) if k == 7 else 0x55) << (8 * k)
    out = []
    for m, d in enumerate(CLUSTER_DIGITS):
        v = hi | d << (8 * j)
        for k in range(j):
            v |= ((0x11 * (m + 1) + k) & 0xFF) << (8 * k)
        out.append(v)
    return out


CLUSTERS = [byte_cluster(j) for j in range(8)]

X_EDGES = [-INF, -DMAX, -1.5, -1.0, -(1.0 - 2.0 ** -53), -2.0 ** -1022, -SUBMAX, -TINY, -0.0,
           0.0, TINY, SUBMAX, 2.0 ** -1022, 1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.5, DMAX, INF]
X_ZEROS = [-0.0, 0.0, -0.0, 0.0]       # with X_EDGES: three groups of each zero

NX_VALUES = [-2.5, 0.0, 3.25, -0.0, -TINY, TINY, 1e300, -1e300, -1.0, 1.0, 0.5]
NU_VALUES = [M64, 0, 1, 1 << 63, (1 << 63) - 1, M64 - 255, 12345]

N_SINGLE = 150
# groups of 2 - 4 rows: (u, x, nx, nu) per row; small binary fractions, the sums are exact
MULTI = [
    [(3, 1.5, 0.25, 7), (M64 - 14, -0.25, None, None)],
    [(M64 - 9, -2.75, None, None), (2, 0.5, None, None), (1, -1.125, None, None)],
    [(10, 0.125, -4.5, M64 - 1), (20, 0.375, 1.25, 3), (M64 - 99, 1.0, -0.75, None)],
    [(5, -8.0, None, 9), (6, 2.5, 6.5, None), (7, 3.25, -6.75, M64 - 2), (8, 1.0, 0.5, 4)],
    [((1 << 40) + 77, 1024.5, 2.0, 1 << 40), (M64 - (1 << 40), -1024.25, 3.0, M64 - (1 << 40))],
    [(0, 7.0, -1.0, None), (0, -3.0, -2.0, None), (M64 - 20, 0.0625, None, None)],
    [(100, -0.5, None, 5), (M64 - 100, -0.5, None, 6), (50, -0.5, 0.75, 7), (25, -0.25, 0.25, 8)],
    [(M64 - 1, 3.0, 1.0, M64), (31, 4.0, 2.0, M64 - 1)],
]


@functools.lru_cache(maxsize=None)
def edge_groups():
    """[(g, cluster byte or None, [(u, x, nx, nu) per row])]: N_SINGLE groups of one row, then
    MULTI.  nx / nu None = NULL"""
    us = [v & M64 for v in U_EDGES] + [v for c in CLUSTERS for v in c]
    is_cluster = [None] * len(U_EDGES) + [j for j, c in enumerate(CLUSTERS) for _ in c]
    for i in range(len(us), N_SINGLE):
        us.append(i * 0x9E3779B97F4A7C15 & M64)
        is_cluster.append(None)
    assert len(set(us)) == N_SINGLE
    # x: the clusters read as doubles, so that the float keys cluster too; the edge values
    # and fillers spread over the other groups
    rest = [i for i in range(N_SINGLE) if is_cluster[i] is None]
    pool = X_EDGES + X_ZEROS
    pool += [((k * 37) % 101 - 50) / 8.0 + 2.0 ** -20 for k in range(len(rest) - len(pool))]
    xs = {}
    for k, i in enumerate(rest):
        xs[i] = pool[(k * 5 + 3) % len(rest)]   # (5 is coprime to len(rest) = 118)
    assert len(rest) == 118
    groups = []
    for i in range(N_SINGLE):
        x = xs[i] if is_cluster[i] is None else from_bits(us[i])
        assert x == x and (is_cluster[i] is None or abs(x) < INF)
        nx = None if i % 4 == 0 else NX_VALUES[i % len(NX_VALUES)]
        nu = None if i % 5 == 0 else NU_VALUES[i % len(NU_VALUES)]
        groups.append(((i * 37 + 11) % 1009, is_cluster[i], [(us[i], x, nx, nu)]))
    for k, rows in enumerate(MULTI):
        groups.append((((N_SINGLE + k) * 37 + 11) % 1009, None, rows))
    assert len({g for g, _, _ in groups}) == len(groups)
    return groups


def _image(columns, cols):
    w = E.Writer(columns)
    for c in columns:
        name = c["name"]
        if c.get("dlevel_max"):
            w.put(name, cols[name], present=cols[name + "_present"])
        else:
            w.put(name, cols[name])
    w.commit(len(cols["g"]))
    img = w.image()
    w.close()
    return img


@functools.lru_cache(maxsize=None)
def edge_table():
    """-> image, rows [(g, u, x, nx, nu)] in table order (the groups' rows interleaved)"""
    rows = [(g,) + r for g, _, rs in edge_groups() for r in rs]
    rows = [rows[i] for i in sorted(range(len(rows)), key=lambda i: (i * 2654435761) % (1 << 32))]
    cols = dict(
        g=np.array([r[0] for r in rows], np.uint64), u=np.array([r[1] for r in rows], np.uint64),
        x=np.array([r[2] for r in rows], np.float64),
        nx=np.array([0.0 if r[3] is None else r[3] for r in rows], np.float64),
        nx_present=np.array([r[3] is not None for r in rows], np.uint8),
        nu=np.array([0 if r[4] is None else r[4] for r in rows], np.uint64),
        nu_present=np.array([r[4] is not None for r in rows], np.uint8))
    assert [bits(v) for v in cols["x"].tolist()] == [bits(r[2]) for r in rows]
    return _image(COLUMNS, cols), rows


# ---- aggregates: expressions and their model -------------------------------------------------
# (fn, column): key / ikey = the group key (ikey: through to_int64), i* = over to_int64(column)
MAIN_AGGS = (("key", "g"), ("isum", "u"), ("imin", "u"), ("imax", "u"), ("sum", "u"), ("sum", "x"),
             ("min", "x"), ("max", "x"), ("mean", "x"), ("min", "nx"), ("mean", "nx"),
             ("imin", "nu"), ("count", None))
FLOAT_COLS = ("x", "nx")


def agg_expr(fn, name):
    c = col(name) if name else None
    if fn == "key":
        return c
    if fn == "ikey":
        return Call("to_int64", c)
    if fn == "count":
        return count(1)
    if fn[0] == "i":
        return {"isum": sum_, "imin": min_, "imax": max_}[fn](Call("to_int64", c))
    return {"sum": sum_, "min": min_, "max": max_, "mean": mean}[fn](c)


def agg_type(fn, name):
    if fn in ("key", "sum", "min", "max"):
        return K.T_FLOAT64 if name in FLOAT_COLS else K.T_UINT64
    if fn == "mean":
        return K.T_FLOAT64
    return K.T_UINT64 if fn == "count" else K.T_INT64


def make_plan(schema, aggs, **kw):
    return Plan(schema, select=[agg_expr(*a) for a in aggs], group_by=[agg_expr(*aggs[0])], **kw)


def _exact_float_sum(vals):
    """the sum of doubles where every order of adding them gives the same double: one value,
    or finite values whose exact sum is a double"""
    if len(vals) == 1:
        return vals[0]
    s = sum(Fraction(v) for v in vals)
    assert float(s) == s, "the sum of a group is not exact: change the inputs"
    return float(s)


def agg_cell(fn, vals, is_float):
    """vals: the column's values over the group's rows, None = NULL.  to_int64 pops the
    payload and pushes it without the tag (conversion.cc:96-99): to_int64(NULL) is the
    value 0, so min(to_int64(nu)) of an all-NULL group is 0, not NULL"""
    if fn == "count":
        return len(vals)
    if fn[0] == "i":
        vals = [signed(v or 0) for v in vals]
    pv = [v for v in vals if v is not None]
    if fn == "sum":          # a NULL adds its 0 payload
        return _exact_float_sum([0.0 if v is None else v for v in vals]) if is_float else sum(pv) & M64
    if fn == "isum":
        return signed(sum(vals))
    if not pv:               # min / max / mean of no value: NULL
        return None
    if fn == "mean":         # the exact sum, one correctly rounded division
        s = _exact_float_sum(pv)
        return s if len(pv) == 1 else float(Fraction(s) / len(pv))
    if is_float:
        assert len(pv) == 1 or all(v != 0 for v in pv)   # (min of -0.0 and +0.0 has no one answer)
    return min(pv) if fn.endswith("min") else max(pv)


def _group_key(fn, v):
    return signed(v or 0) if fn == "ikey" else v


def model_rows(rows, names, aggs):
    """rows: tuples in the order of `names`; aggs[0] is the key.  -> one tuple per group, in
    first-row order.  A float key is grouped by its bits, a NULL key is a group of its own"""
    idx = {n: i for i, n in enumerate(names)}
    kfn, kname = aggs[0]
    groups = {}
    for r in rows:
        v = _group_key(kfn, r[idx[kname]])
        groups.setdefault(("f", bits(v)) if isinstance(v, float) else v, []).append(r)
    out = []
    for rs in groups.values():
        cells = [_group_key(kfn, rs[0][idx[kname]])]
        for fn, name in aggs[1:]:
            vals = [r[idx[name]] for r in rs] if name else rs
            cells.append(agg_cell(fn, vals, name in FLOAT_COLS))
        out.append(tuple(cells))
    return out


# ---- the order -------------------------------------------------------------------------------
def cmp_cell(a, b):
    """cmp#int64/X;X; on payloads: a NULL reads 0.  Python ints compare as the signed or
    unsigned values they are, floats with < and >"""
    a = 0 if a is None else a
    b = 0 if b is None else b
    return -1 if a < b else (1 if a > b else 0)


def row_cmp(specs):
    def cmp(ra, rb):
        for c, desc in specs:
            r = cmp_cell(ra[c], rb[c])
            if r:
                return -r if desc else r
        return 0
    return cmp


def ordered(rows, specs):
    return sorted(rows, key=functools.cmp_to_key(row_cmp(specs)))


def limited(rows, limit, offset):
    if limit is None:
        return rows
    return rows[offset:offset + limit] if limit else []


def is_total(rows, specs):
    """no two rows tie under `specs` (rows: ordered by them)"""
    cmp = row_cmp(specs)
    return all(cmp(a, b) < 0 for a, b in zip(rows, rows[1:]))


# ---- comparing a result with the model ---------------------------------------------------------
def zero_sum_cols(aggs):
    return frozenset(i for i, (fn, name) in enumerate(aggs) if name in FLOAT_COLS and fn in ("sum", "mean"))


def sig(row, zero_ok=frozenset()):
    """a row as something == compares bit for bit (and by type); a zero in a `zero_ok` column
    without its sign"""
    out = []
    for i, v in enumerate(row):
        if isinstance(v, float):
            v = ("f", 0 if v == 0 and i in zero_ok else bits(v))
        out.append(v)
    return tuple(out)


def check_rows(got, want, zero_ok, where):
    """row by row, bit for bit"""
    assert len(got) == len(want), (where, len(got), len(want))
    gs, ws = [sig(r, zero_ok) for r in got], [sig(r, zero_ok) for r in want]
    if gs != ws:
        i = next(i for i, (a, b) in enumerate(zip(gs, ws)) if a != b)
        raise AssertionError((where, "row %d of %d" % (i, len(got)), got[i], want[i]))


def check_ties_free(got, want, sort_col, zero_ok, where):
    """one sort key, ties in unspecified order: the sort key values are the model's slice
    (as the comparator sees them), every row is the model's row of its group, no group
    comes twice.  want: (the model's slice, {group key: signature of the model's row})"""
    slice_, by_key = want
    assert len(got) == len(slice_), (where, len(got), len(slice_))
    seen = set()
    for i, (r, w) in enumerate(zip(got, slice_)):
        # (a NULL ties with a zero: types and bits are checked against the group's own row)
        assert cmp_cell(r[sort_col], w[sort_col]) == 0, (where, "key of row %d" % i, r, w)
        k = sig(r[:1])
        assert k not in seen, (where, "group twice", r)
        seen.add(k)
        assert by_key.get(k) == sig(r, zero_ok), (where, "row %d" % i, r)


class Model:
    """the groups of one plan, ordered on demand"""

    def __init__(self, rows, names, aggs):
        self.aggs = aggs
        self.rows = model_rows(rows, names, aggs)
        self.types = [agg_type(*a) for a in aggs]
        self.zero_ok = zero_sum_cols(aggs)
        self.by_key = {sig(r[:1]): sig(r, self.zero_ok) for r in self.rows}
        assert len(self.by_key) == len(self.rows)
        for i, t in enumerate(self.types):   # no NaN in a sortable column
            assert t != K.T_FLOAT64 or all(r[i] is None or r[i] == r[i] for r in self.rows)
        self._ordered = {}

    def ordered(self, specs):
        specs = tuple(specs)
        if specs not in self._ordered:
            self._ordered[specs] = ordered(self.rows, specs)
        return self._ordered[specs]

    def check(self, got, specs, limit, offset, where=""):
        """a result of ORDER BY specs LIMIT limit OFFSET offset.  One sort key and the order
        is not total: check_ties_free; else row by row"""
        specs = tuple(tuple(s) for s in specs)
        rows = self.ordered(specs)
        want = limited(rows, limit, offset)
        where = "%s order by %s limit %s offset %s" % (where, list(specs), limit, offset)
        if len(specs) == 1 and not self.total(specs):
            check_ties_free(got, (want, self.by_key), specs[0][0], self.zero_ok, where)
        else:
            assert self.total(specs), (where, "the model's order is not total")
            check_rows(got, want, self.zero_ok, where)

    @functools.lru_cache(maxsize=None)
    def total(self, specs):
        return is_total(self.ordered(specs), specs)


# ---- cuts ------------------------------------------------------------------------------------
def tie_cuts(rows, c):
    """the cuts want = offset + limit that fall inside a run of rows that tie in column c:
    all of them for a run of up to 8 rows, else the first, the middle and the last"""
    cuts, s = set(), 0
    for e in range(1, len(rows) + 1):
        if e == len(rows) or cmp_cell(rows[e][c], rows[s][c]) != 0:
            if e - s >= 2:
                inside = range(s + 1, e)
                cuts.update(inside if e - s <= 8 else (s + 1, (s + e) // 2, e - 1))
            s = e
    return cuts


def cluster_cuts(rows, cluster_keys):
    """the cuts between two neighbours that both belong to a byte cluster"""
    return {p for p in range(1, len(rows))
            if rows[p - 1][0] in cluster_keys and rows[p][0] in cluster_keys}


def sweep(model, c, single, cluster_keys=frozenset()):
    """[(specs, limit, offset)] of sort column c: ascending every cut 1 .. G-1; descending
    every seventh and every cut inside a tie run or a byte cluster; each with offset 0 and
    offset want - 1.  single: c is the only sort key, else the (unique) key column follows"""
    G = len(model.rows)
    cases = []
    for desc in (False, True):
        specs = ((c, desc),) if single or c == 0 else ((c, desc), (0, False))
        rows = model.ordered(specs)
        cuts = set(range(1, G)) if not desc else \
            set(range(1, G, 7)) | tie_cuts(rows, c) | cluster_cuts(rows, cluster_keys)
        for want in sorted(cuts):
            for offset in sorted({0, want - 1}):
                cases.append((specs, want - offset, offset))
    return cases


@functools.lru_cache(maxsize=None)
def main_model():
    _, rows = edge_table()
    return Model(rows, ("g", "u", "x", "nx", "nu"), MAIN_AGGS)


@functools.lru_cache(maxsize=None)
def main_cluster_keys():
    return frozenset(g for g, j, _ in edge_groups() if j is not None)


SORT_COLUMNS = list(range(len(MAIN_AGGS)))   # every output column of the main plan sorts


def main_plan(**kw):
    return make_plan(SCHEMA, MAIN_AGGS, **kw)


def second_key_cases():
    """two sort keys, the second not ascending g: per tie class of the first (the zeros of
    the float columns, the NULLs that read 0, the counts) cuts inside the tie set -- the
    device has to send every boundary tie, the second key picks among them"""
    m = main_model()
    cases = []
    for c in (5, 6, 8, 9, 10, 11, 12):
        for desc in (False, True):
            for second in ((0, True), (1, False)):     # g descending; isum(u), unique
                specs = ((c, desc), second)
                for want in sorted(tie_cuts(m.ordered(specs), c)):
                    cases.append((specs, want, 0))
                    cases.append((specs, 1, want - 1))
    return cases


# the from_ident variants: the group key itself is sort key 0.  (key, what it pins)
VARIANTS = {
    "int_key": (("ikey", "u"), "a signed key; the record of bit pattern 2^64 - 1 is kind 1"),
    "float_key": (("key", "x"), "-0.0 and +0.0 are two groups that tie"),
    "nullable_key": (("key", "nu"), "the NULL group is kind 2 and reads 0, next to the key 0"),
    "nullable_float_key": (("key", "nx"), "kind 2 reads 0 between the negative and the positive "
                                          "keys and ties with the keys -0.0 and +0.0"),
}
# (No plan reaches a kind 2 record under the signed view: to_int64(NULL) is the value 0, so
# `group by to_int64(nu)` has no NULL group.  The float view above is the one where the NULL
# key's 0 lies inside the order.)


@functools.lru_cache(maxsize=None)
def variant(name):
    """-> aggs, model: select <key>, count(1), sum(u) group by <key>"""
    aggs = (VARIANTS[name][0], ("count", None), ("sum", "u"))
    _, rows = edge_table()
    m = Model(rows, ("g", "u", "x", "nx", "nu"), aggs)
    assert m.total(((0, False), (2, False)))   # sum(u) separates the keys that tie
    return aggs, m


def variant_cases(name):
    _, m = variant(name)
    G = len(m.rows)
    cases = []
    for desc in (False, True):
        for specs in (((0, desc),), ((0, desc), (2, False)), ((0, desc), (2, True))):
            rows = m.ordered(specs)
            cuts = set(range(1, G)) if not desc else set(range(1, G, 7)) | tie_cuts(rows, 0)
            for want in sorted(cuts):
                for offset in sorted({0, want - 1}):
                    cases.append((specs, want - offset, offset))
    return cases


# ---- the dense-record path --------------------------------------------------------------------
DENSE_G = 70_001
DENSE_SCHEMA = dict(g=K.T_UINT64, u=K.T_UINT64, x=K.T_FLOAT64, t=K.T_UINT64)
DENSE_COLUMNS = [
    dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="u", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="x", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="t", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)]
DENSE_AGGS = (("key", "g"), ("isum", "u"), ("sum", "x"), ("imin", "u"), ("isum", "t"))
DENSE_HINTS = (100_000, 3_000_000)      # scatter only; scatter and refine


@functools.lru_cache(maxsize=None)
def dense_table():
    """70,001 groups of one row: u = i * 0x9E3779B97F4A7C15 mod 2^64, x = to_int64(u) / 2^12
    (one rounding, when the table is made: a group's sum is its one value), t the bit
    pattern of -8 .. 7 in turn"""
    i = np.arange(DENSE_G, dtype=np.uint64)
    u = i * np.uint64(0x9E3779B97F4A7C15)
    x = u.view(np.int64).astype(np.float64) / 4096.0
    t = ((i % np.uint64(16)).astype(np.int64) - 8).view(np.uint64)
    cols = dict(g=i, u=u, x=x, t=t)
    rows = list(zip(i.tolist(), u.tolist(), x.tolist(), t.tolist()))
    return _image(DENSE_COLUMNS, cols), rows


@functools.lru_cache(maxsize=None)
def dense_model():
    _, rows = dense_table()
    return Model(rows, ("g", "u", "x", "t"), DENSE_AGGS)


def dense_plan(**kw):
    return make_plan(DENSE_SCHEMA, DENSE_AGGS, **kw)


def dense_cases():
    cases = []
    for desc in (False, True):
        for c in (1, 2, 3):
            for offset in (0, 1, 35_000, DENSE_G - 101):
                cases.append((((c, desc), (0, False)), 100, offset))
        # isum(t): 16 values, ~4,375 groups each; the cut 4,400 lies inside the second tie set
        cases.append((((4, desc), (0, False)), 100, 4300))
        cases.append((((4, desc),), 100, 4300))
    return cases


def order_of(plan, case):
    specs, limit, offset = case
    return Order(plan, list(specs), limit=limit, offset=offset)
