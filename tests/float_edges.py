"""IEEE edge tables and an exact reference for the build-supplied float aggregates
(sum(float64), min, max, mean) and for the 64-bit integer aggregates at their extremes.

The semantics are the oracle header's (oracle/csql_oracle.c): min / max / mean skip NULL
inputs (sum adds their 0 payload), min / max also skip NaN inputs, a group with no input
left is NULL, a float sum adds every row in row order.  The reference below is plain
Python over the column arrays and the WHERE mask -- neither the oracle nor doubles added
in row order:
  * sum / mean: the exact sum S (math.fsum, or integer arithmetic where fsum overflows)
    and A = sum |x|; NaN and infinities by class
  * min / max: bit-exact over the non-NULL, non-NaN inputs; a zero by value, its sign one
    that occurs in the group (the oracle keeps the first zero it meets, the device order
    is unspecified)
  * integers: Python ints, exact
`check_strict` compares a result with it.  tables.compare_results stays the loose
comparator of the other tests: it lets a subnormal flushed to 0 pass, and it fails a
cancelling sum that is right."""
import functools
import math
import struct
import sys
from fractions import Fraction

import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Call, col, count, count_distinct, max_, mean, min_, sum_

DMAX = sys.float_info.max
TINY = 5e-324                      # 2^-1074, the smallest subnormal
SUBMAX = 2.0 ** -1022 - TINY       # the largest subnormal
NAN = float("nan")
INF = float("inf")
NAN_ONES = struct.unpack("<d", b"\xff" * 8)[0]  # every bit set: the tables' EMPTY marker
U = Fraction(1, 1 << 53)           # unit roundoff of round-to-nearest doubles

SCHEMA = dict(g=K.T_UINT64, x=K.T_FLOAT64, nx=K.T_FLOAT64, u=K.T_UINT64, w=K.T_UINT64)
COLUMNS = [
    dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="x", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="nx", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754, dlevel_max=1),
    dict(name="u", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="w", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_BITPACKED,
         bitpack_max_value=7)]

# WHERE w > 0 removes about a fifth of the rows of every class
WHERE = col("w") > 0


def where_mask(c):
    return c["w"] > 0


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# ---- the edge classes --------------------------------------------------------------------
# the value of row j of a group of s rows in replica r of a class
def _cycle(vals, rotate=True):
    return lambda j, s, r: vals[(j + (r if rotate else 0)) % len(vals)]


def _near_max(j, s, r):
    # finite in every order: the positive partial sums stay below 0.95 DBL_MAX + s
    return (0.75 * DMAX, 0.2 * DMAX, -0.5 * DMAX)[j] if j < 3 else (1.0 if j % 2 else -1.0)


def _magnitudes(j, s, r):
    # +-2^k, k spread evenly over -1074 .. 1023 (every exponent at s = 2098); the
    # alternating signs keep every partial sum below 2/3 of 2^1024, in any order
    k = -1074 + (j * 2097 // (s - 1) if s > 1 else 0)
    return math.ldexp(1.0 if j % 2 else -1.0, k)


def _filler(j, s, r):
    return ((j * 7919 + r * 131) % 4096) / 8.0 - 256.0


# name, value of a row, rows per group in the ~1000-group table
CLASSES = [
    ("nan_only", _cycle([NAN]), 600),
    ("nan_mixed", _cycle([1.5, NAN, -2.25, 3.0, -0.0]), 900),
    ("pinf", _cycle([INF]), 500),
    ("ninf", _cycle([-INF]), 500),
    ("pinf_ninf", _cycle([INF, 2.0, -INF]), 700),
    ("zeros_neg_first", _cycle([-0.0, 0.0], rotate=False), 800),
    ("zeros_pos_first", _cycle([0.0, -0.0], rotate=False), 800),
    ("neg_zeros", _cycle([-0.0]), 800),
    ("subnormals", _cycle([TINY, SUBMAX, 3 * TINY, -TINY, 2.0 ** -1050]), 1200),
    ("subnormals_pos", _cycle([SUBMAX, 7 * TINY, TINY, 2.0 ** -1040]), 1000),
    ("sub_and_normal", _cycle([1e-310, 1.0, -2.5e-320, 2.0 ** -1022, -3.0, SUBMAX]), 1000),
    ("cancel", _cycle([1e16, 1.0, -1e16, -1.0, 2.0 ** -30]), 1000),
    ("overflow", _cycle([0.6 * DMAX]), 3),
    ("near_max", _near_max, 9),
    ("magnitudes", _magnitudes, 2098),
    ("all_null", _cycle([4.0, -8.5]), 700),
    ("single", _cycle([-6.25]), 1),
    ("filler", _filler, 0),          # takes the rows that are left
]
NCLASS = len(CLASSES)
CLASS_INDEX = {c[0]: i for i, c in enumerate(CLASSES)}
NAMES = [c[0] for c in CLASSES]

# uint64 edges; which of them a group holds depends on its replica
U_EDGES = [0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1, 12345]
U_SETS = [U_EDGES, [(1 << 64) - 1, (1 << 64) - 2],
          [(1 << 63) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1]]


def _group_rows(name, s, r):
    fn = CLASSES[CLASS_INDEX[name]][1]
    x = [fn(j, s, r) for j in range(s)]
    if name == "all_null":
        present = [0] * s
    else:  # (j * 3 mod 4 differs for j = 0, 1, 2: at most one of the first three is NULL)
        present = [int((j * 3 + r) % 4 != 1) for j in range(s)]
    us = U_SETS[r % 3]
    u = [us[(j * 5 + r) % len(us)] for j in range(s)]
    w = [(j * 7 + r) % 5 for j in range(s)]
    return x, present, u, w


def build_columns(replicas, total_rows=None, cap=None):
    """one group per (replica, class), key = replica * NCLASS + class, its rows contiguous.
    cap: the most rows of a group (magnitudes keep 6, overflow its 3); the filler groups
    take the rows up to total_rows.  -> dict of column arrays and nx_present"""
    sizes = []
    for r in range(replicas):
        for ci, (name, fn, s) in enumerate(CLASSES):
            if cap is not None and s > 1:
                s = {"magnitudes": 6, "overflow": 3}.get(name, min(s, cap))
            sizes.append([r * NCLASS + ci, name, s])
    fill = [e for e in sizes if e[1] == "filler"]
    if total_rows is not None:
        left = total_rows - sum(e[2] for e in sizes)
        assert left >= len(fill), "table too small for its classes"
        for i, e in enumerate(fill):
            e[2] = left // len(fill) + (1 if i < left % len(fill) else 0)
    else:
        for e in fill:
            e[2] = cap
    g, x, pres, u, w = [], [], [], [], []
    for key, name, s in sizes:
        xs, ps, us, ws = _group_rows(name, s, key // NCLASS)
        g += [key] * s
        x += xs
        pres += ps
        u += us
        w += ws
    c = dict(g=np.array(g, np.uint64), x=np.array(x, np.float64), u=np.array(u, np.uint64),
             w=np.array(w, np.uint64), nx_present=np.array(pres, np.uint8))
    c["nx"] = np.where(c["nx_present"] != 0, c["x"], 0.0)
    return c


def strided(c):
    """the same rows, every group spread evenly over the whole table: row j of a group of s
    rows goes to the relative position (j + 1/2) / s -- for groups of equal size that is
    row i -> group i mod G"""
    o = np.argsort(c["g"], kind="stable")
    c = {k: v[o] for k, v in c.items()}
    g = c["g"]
    _, start, size = np.unique(g, return_index=True, return_counts=True)
    j = np.arange(len(g)) - np.repeat(start, size)
    order = np.lexsort((g, (j + 0.5) / np.repeat(size, size)))
    return {k: v[order] for k, v in c.items()}


def by_class(c, names):
    """the rows of the named classes, every class one group (key = its class index).  Of
    near_max and magnitudes only replica 0: the sum of all replicas would overflow in
    some orders and not in others"""
    cls = c["g"] % np.uint64(NCLASS)
    keep = np.isin(cls, np.array([CLASS_INDEX[n] for n in names], np.uint64))
    one = np.isin(cls, np.array([CLASS_INDEX["near_max"], CLASS_INDEX["magnitudes"]], np.uint64))
    keep &= ~one | (c["g"] < np.uint64(NCLASS))
    d = {k: v[keep] for k, v in c.items()}
    d["g"] = d["g"] % np.uint64(NCLASS)
    return d


def image_of(c):
    w = E.Writer(COLUMNS)
    for name in ("g", "x", "u", "w"):
        w.put(name, c[name])
    w.put("nx", c["nx"], present=c["nx_present"])
    w.commit(len(c["g"]))
    img = w.image()
    w.close()
    return img


@functools.lru_cache(maxsize=None)
def main_columns():
    """~1000 groups (60 replicas of every class) in 1,000,007 rows, a multiple of no tile"""
    return build_columns(60, total_rows=1_000_007)


@functools.lru_cache(maxsize=None)
def main_table(layout="contiguous"):
    c = main_columns()
    if layout == "strided":
        c = strided(c)
    return image_of(c), c


@functools.lru_cache(maxsize=None)
def wide_table():
    """the same classes over 75,600 groups of 1 .. 6 rows (strided): device-packed emission
    (>= 2^16 groups) and the partitioned path"""
    c = strided(build_columns(4200, cap=5))
    return image_of(c), c


# ---- GROUP BY a float key -------------------------------------------------------------------
FKEY_SCHEMA = dict(fk=K.T_FLOAT64, v=K.T_UINT64)
FKEY_VALUES = [-0.0, 0.0, NAN, INF, -INF, NAN_ONES, from_bits(0x7FF0000000000001), TINY, 1.0, -1.0]


@functools.lru_cache(maxsize=None)
def float_key_table(n=100_003):
    i = np.arange(n, dtype=np.uint64)
    kb = np.array([bits(v) for v in FKEY_VALUES], np.uint64)[(i * np.uint64(7)) % np.uint64(len(FKEY_VALUES))]
    fk = kb.view(np.float64)
    v = (i * np.uint64(2654435761)) % np.uint64(1000)
    w = E.Writer([dict(name="fk", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
                  dict(name="v", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)])
    w.put("fk", fk)
    w.put("v", v)
    w.commit(n)
    img = w.image()
    w.close()
    return img, dict(fk=fk, v=v)


def float_key_reference(c):
    """select fk, count(1), sum(v) group by fk: one group per bit pattern of fk (the
    reference keys groups by the SHA1 of the value bytes, groupby.cc:112-135)"""
    b = c["fk"].view(np.uint64)
    out = {}
    for kb in np.unique(b).tolist():
        m = b == np.uint64(kb)
        # (keyed by bits: -0.0 and +0.0 would be one key of a dict of floats)
        out[_key((from_bits(kb),))] = [("exact", int(m.sum())), ("exact", int(c["v"][m].sum()))]
    return out


# ---- select lists -------------------------------------------------------------------------
FLOAT_AGGS = (("sum", "x"), ("min", "x"), ("max", "x"), ("mean", "x"), ("count", None),
              ("sum", "nx"), ("min", "nx"), ("max", "nx"), ("mean", "nx"))
INT_AGGS = (("sum", "u"), ("isum", "u"), ("min", "u"), ("max", "u"), ("imin", "u"),
            ("imax", "u"), ("mean", "u"), ("count_distinct", "u"), ("count", None))


def agg_expr(fn, name):
    c = col(name) if name else None
    if fn in ("isum", "imin", "imax"):
        return {"isum": sum_, "imin": min_, "imax": max_}[fn](Call("to_int64", c))
    if fn == "count":
        return count(1)
    return {"sum": sum_, "min": min_, "max": max_, "mean": mean,
            "count_distinct": count_distinct}[fn](c)


def select(aggs, key="g"):
    return ([col(key)] if key else []) + [agg_expr(fn, name) for fn, name in aggs]


# ---- the reference -------------------------------------------------------------------------
def _signed(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _exact(vals):
    """the exact sum of finite doubles (integers in units of 2^-1074)"""
    t = 0
    for v in vals:
        n, d = v.as_integer_ratio()
        t += n * ((1 << 1074) // d)
    return Fraction(t, 1 << 1074)


def to_double(f):
    """a Fraction rounded to the nearest double (ties to even), +-inf beyond"""
    try:
        return float(f)
    except OverflowError:
        return INF if f > 0 else -INF


def _sum_cell(vals, div):
    """('fsum', S, A, terms, divisor): S exact (a Fraction) or the special result (a float:
    NaN, +-inf)"""
    pinf, ninf = INF in vals, -INF in vals
    if any(v != v for v in vals) or (pinf and ninf):
        return ("fsum", NAN, None, len(vals), div)
    if pinf or ninf:
        return ("fsum", INF if pinf else -INF, None, len(vals), div)
    try:
        S = Fraction(math.fsum(vals))
        A = Fraction(math.fsum(abs(v) for v in vals)) * (1 + U)
    except OverflowError:
        S, A = _exact(vals), _exact([abs(v) for v in vals])
    if math.isinf(to_double(S)):
        # only terms of one sign here: every order of adding them overflows
        assert all(v >= 0 for v in vals) or all(v <= 0 for v in vals)
        return ("fsum", to_double(S), None, len(vals), div)
    return ("fsum", S, A, len(vals), div)


def _minmax_cell(vals, is_min):
    vals = [v for v in vals if v == v]
    if not vals:
        return ("exact", None)
    return ("minmax", min(vals) if is_min else max(vals),
            {math.copysign(1.0, v) for v in vals if v == 0})


def ref_cell(fn, name, c, idx):
    if fn == "count":
        return ("exact", len(idx))
    v = c[name][idx]
    pres = c[name + "_present"][idx] != 0 if name + "_present" in c else np.ones(len(idx), bool)
    if c[name].dtype == np.float64:
        pv = v[pres].tolist()
        if fn == "sum":
            return _sum_cell(np.where(pres, v, 0.0).tolist(), 1)  # a NULL adds its 0 payload
        if fn == "mean":
            return _sum_cell(pv, len(pv)) if pv else ("exact", None)
        return _minmax_cell(pv, fn == "min")
    ints = v[pres].tolist()
    if fn == "sum":
        return ("exact", sum(ints) % (1 << 64))
    if fn == "isum":
        return ("exact", _signed(sum(ints)))
    if fn in ("min", "max", "imin", "imax"):
        if not ints:
            return ("exact", None)
        vals = [_signed(t) for t in ints] if fn[0] == "i" else ints
        return ("exact", min(vals) if fn.endswith("min") else max(vals))
    if fn == "mean":
        return _sum_cell([float(t) for t in ints], len(ints)) if ints else ("exact", None)
    if fn == "count_distinct":
        return ("exact", len(set(ints)))
    raise ValueError(fn)


def reference(c, aggs, mask=None, key="g"):
    """{group key tuple (() without GROUP BY): [expected cell per aggregate]} over the rows
    that pass `mask`"""
    idx = np.arange(len(c["g"])) if mask is None else np.nonzero(mask)[0]
    if key is None:
        return {(): [ref_cell(fn, name, c, idx) for fn, name in aggs]} if len(idx) else {}
    order = idx[np.argsort(c[key][idx], kind="stable")]
    keys, starts = np.unique(c[key][order], return_index=True)
    return {(k,): [ref_cell(fn, name, c, part) for fn, name in aggs]
            for k, part in zip(keys.tolist(), np.split(order, starts[1:]))}


# ---- the strict comparator ------------------------------------------------------------------
def _gamma(n):
    k = Fraction(max(n - 1, 0)) * U
    return k / (1 - k)


def check_cell(got, cell, where=""):
    kind = cell[0]
    if kind == "exact":
        want = cell[1]
        assert got == want and type(got) is type(want), (where, got, want)
        return
    if kind == "minmax":
        want, zeros = cell[1], cell[2]
        assert got is not None, (where, got, want)
        if want == 0:  # by value; the sign one that occurs in the group
            assert got == 0 and math.copysign(1.0, got) in zeros, (where, got, want, zeros)
        else:
            assert bits(got) == bits(want), (where, got, want)
        return
    S, A, n, div = cell[1:]
    assert got is not None, (where, got)
    if isinstance(S, float):  # NaN / +-inf: by class
        assert (got != got) if S != S else (got == S), (where, got, S)
        return
    assert math.isfinite(got), (where, got, float(S))
    if got == 0:  # the oracle's sums start at +0, and round to nearest never reaches -0
        assert math.copysign(1.0, got) > 0, (where, got)
    # any order of adding n terms: |error| <= gamma(n-1) * sum |x|; plus the rounding of S
    bound = _gamma(n) * A + U * abs(S)
    want = S / div
    if div != 1:  # mean: the bound divided by the count, plus the division's rounding
        # (relative, or half the subnormal spacing where the quotient is subnormal)
        bound = bound / div + U * abs(want) + Fraction(1, 1 << 1075)
    err = abs(Fraction(got) - want)
    assert err <= bound, (where, got, float(want), float(err), float(bound))


def _key(t):
    return tuple(("f", bits(v)) if isinstance(v, float) else v for v in t)


def check_strict(got_rows, expected, key_cols=1, where=""):
    """got_rows: result rows, key columns first; expected: reference()"""
    g = {}
    for r in got_rows:
        k = _key(r[:key_cols])
        assert k not in g, (where, "duplicate group", r[:key_cols])
        g[k] = r[key_cols:]
    e = {_key(k): v for k, v in expected.items()}
    assert set(g) == set(e), (where, "group sets differ", len(g), len(e),
                              sorted(set(g) ^ set(e), key=repr)[:10])
    for k, cells in e.items():
        assert len(g[k]) == len(cells), (where, k, g[k])
        for i, (got, cell) in enumerate(zip(g[k], cells)):
            check_cell(got, cell, where="%s group %s column %d" % (where, k, i + key_cols))


def same_cell(x, y):
    """bit for bit (a NaN by class)"""
    if isinstance(x, float) and isinstance(y, float):
        return (y != y) if x != x else bits(x) == bits(y)
    return x == y and type(x) is type(y)


def check_same_bits(a_rows, b_rows, key_cols=1, columns=None, where=""):
    """two results of one plan, rows matched by key; `columns`: the ones to compare"""
    a = {_key(r[:key_cols]): r for r in a_rows}
    b = {_key(r[:key_cols]): r for r in b_rows}
    assert len(a) == len(a_rows) and set(a) == set(b), (where, len(a), len(b))
    for k, ra in a.items():
        for i in (columns if columns is not None else range(len(ra))):
            assert same_cell(ra[i], b[k][i]), (where, k, i, ra[i], b[k][i])


# ---- EVQL_FLOAT_SUM_EXACT --------------------------------------------------------------------
def exact_quantum_exp(bound):
    """e of the quantum 2^e as include/evql_gpu.h states it: 2^(ex-1) <= bound < 2^ex,
    e = max(ex - 61, -1023)"""
    return max(math.frexp(bound if bound > 0 else 1.0)[1] - 61, -1023)


def exact_mode_sum(vals, e):
    """every term rounded half to even to a multiple of 2^e, the multiples added exactly,
    the total rounded once.  (x * 2^-e is exact unless it falls below 2^-1022, where any
    rounding of it still rounds to the integer 0)"""
    total = sum(round(math.ldexp(v, -e)) for v in vals)
    return to_double(Fraction(total) * Fraction(2) ** e)


EXACT_SCHEMA = dict(g=K.T_UINT64, xs=K.T_FLOAT64, xt=K.T_FLOAT64, xp=K.T_FLOAT64,
                    xc=K.T_FLOAT64)


@functools.lru_cache(maxsize=None)
def exact_table(n=200_003):
    """3 groups (row i -> group i mod 3); xs: subnormals only; xt: |x| < 1e-300, normals and
    subnormals; xp: full 53-bit mantissas in (-1000, 1000); xc: group 0 pairs every x with
    -x (exactly 0), group 1 is all negative, group 2 pairs plus 2^-40"""
    rng = np.random.default_rng(1074)
    g = np.arange(n, dtype=np.uint64) % np.uint64(3)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    xs = sign * rng.integers(1, 1 << 52, n).astype(np.float64) * TINY
    xt = sign * 10.0 ** rng.uniform(-323, -300.5, n)
    xp = rng.uniform(-1000.0, 1000.0, n)
    xc = np.zeros(n)
    for k in range(3):
        rows = np.nonzero(g == np.uint64(k))[0]
        half = rng.uniform(-1000.0, 1000.0, len(rows) // 2)
        if k == 1:
            xc[rows] = -rng.uniform(0.0, 1000.0, len(rows))
        else:
            xc[rows[:len(half)]] = half
            xc[rows[len(half):2 * len(half)]] = -half[::-1]
            if len(rows) % 2:
                xc[rows[-1]] = 2.0 ** -40 if k == 2 else 0.0
    cols = dict(g=g, xs=xs, xt=xt, xp=xp, xc=xc)
    w = E.Writer([dict(name="g", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)] +
                 [dict(name=nm, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)
                  for nm in ("xs", "xt", "xp", "xc")])
    for nm, v in cols.items():
        w.put(nm, v)
    w.commit(n)
    img = w.image()
    w.close()
    return img, cols


def exact_reference(c, names, bound=0.0):
    """{(g,): [exact-mode sum per column]}; bound 0: derived from the column's max |x|"""
    out = {}
    for k in range(3):
        m = c["g"] == np.uint64(k)
        out[(k,)] = [exact_mode_sum(c[nm][m].tolist(), exact_quantum_exp(
            bound or float(np.max(np.abs(c[nm]))))) for nm in names]
    return out
