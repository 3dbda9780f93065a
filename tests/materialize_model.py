"""Tables, plans and helpers shared by the tests of result materialisation
(Query.to_table / evql_table_from_query): test_materialize_cpu.py decides plans without a
device, test_gpu_materialize.py compares materialised tables with the oracle.

The expected content of a materialised table is always the oracle's rows of the inner plan;
its expected bytes are the image E.Writer makes of those rows."""
import functools

import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Agg, Plan, col, count, max_, mean, min_, stype_of_column, sum_
import oracle_lib as O
import partial_emit_model as PM

M64 = (1 << 64) - 1
STRING_PAGE = 512 * 1024  # kPlainPageSize, csrc/cstable_format.h: a STRING_PLAIN data page
SORT_TILE = K.COMPACT_SORT_TILE


def spec(name, logical, storage, **kw):
    return dict(name=name, logical_type=logical, storage_type=storage, **kw)


U64 = lambda name, **kw: spec(name, K.COL_UNSIGNED_INT, K.ENC_UINT64_PLAIN, **kw)
LEB = lambda name, **kw: spec(name, K.COL_UNSIGNED_INT, K.ENC_UINT64_LEB128, **kw)
U32 = lambda name, **kw: spec(name, K.COL_UNSIGNED_INT, K.ENC_UINT32_PLAIN, **kw)
BP = lambda name, **kw: spec(name, K.COL_UNSIGNED_INT, K.ENC_UINT32_BITPACKED, **kw)
F64 = lambda name, **kw: spec(name, K.COL_FLOAT, K.ENC_FLOAT_IEEE754, **kw)
BOOL = lambda name, **kw: spec(name, K.COL_BOOLEAN, K.ENC_BOOLEAN_BITPACKED, **kw)
STR = lambda name, **kw: spec(name, K.COL_STRING, K.ENC_STRING_PLAIN, **kw)
TS = lambda name, **kw: spec(name, K.COL_DATETIME, K.ENC_UINT64_LEB128, **kw)


# ---- the table of every cell class --------------------------------------------------------------
CELL_GROUPS, CELL_ROWS = 300, 3000
NULL_KEY_GROUP, MAX_KEY_GROUP, NO_VALUE_GROUP = 5, 6, 7
CELL_SCHEMA = dict(nk=K.T_UINT64, a=K.T_UINT64, vs=K.T_FLOAT64, d=K.T_UINT64, nb=K.T_UINT64,
                   u=K.T_UINT64, fv=K.T_FLOAT64, fb=K.T_BOOL, s=K.T_STRING, ns=K.T_STRING,
                   nu=K.T_UINT64, t=K.T_TIMESTAMP64)
CELL_COLUMNS = [LEB("nk", dlevel_max=1), LEB("a"), F64("vs"), U64("d"), LEB("nb", dlevel_max=1),
                U64("u"), F64("fv"), BOOL("fb"), STR("s"), STR("ns", dlevel_max=1),
                U32("nu", dlevel_max=1), TS("t")]
CELL_NULLABLE = ("nk", "nb", "ns", "nu")


def cell_string(g):
    """lengths 0, 1 and 128, then about 2 KiB each: 300 of them fill more than one 512 KiB page"""
    if g < 3:
        return (b"%d" % g * 128)[:(0, 1, 128)[g]]
    return (b"g%05d." % g) * ((2000 + g) // 7)


@functools.lru_cache(maxsize=1)
def cell_table():
    """every first-row column is a function of the row's group g = i % CELL_GROUPS"""
    i = np.arange(CELL_ROWS, dtype=np.uint64)
    g = i % np.uint64(CELL_GROUPS)
    c = {}
    c["nk"] = g * np.uint64(3) + np.uint64(1)
    c["nk"][g == MAX_KEY_GROUP] = np.uint64(M64)
    c["nk_present"] = (g != NULL_KEY_GROUP).astype(np.uint8)
    c["a"] = i % np.uint64(977) + (g << np.uint64(33))
    c["vs"] = (i % np.uint64(89)).astype(np.float64) * 0.37 + 0.001
    c["d"] = (i // np.uint64(CELL_GROUPS)) % (g % np.uint64(4) + np.uint64(1))
    c["nb"] = (g * np.uint64(7)) % np.uint64(1000) + i // np.uint64(CELL_GROUPS)
    c["nb_present"] = ((i % np.uint64(3) != 0) & (g != NO_VALUE_GROUP)).astype(np.uint8)
    c["u"] = g * np.uint64(11)
    c["fv"] = g.astype(np.float64) * -0.75
    c["fb"] = (g % np.uint64(3) == 0).astype(np.uint64)
    strings = [cell_string(x) for x in range(CELL_GROUPS)]
    c["s"] = [strings[x] for x in g.tolist()]
    c["ns"] = [b"n%d" % (x % 17) for x in g.tolist()]
    c["ns_present"] = (g % np.uint64(10) != 3).astype(np.uint8)
    c["nu"] = g + np.uint64(1 << 20)
    c["nu_present"] = (g % np.uint64(4) != 1).astype(np.uint8)
    c["t"] = np.uint64(1438055327000000) + g * np.uint64(1000003)
    w = E.Writer(CELL_COLUMNS)
    for sp in CELL_COLUMNS:
        name = sp["name"]
        if name in CELL_NULLABLE:
            w.put(name, c[name], present=c[name + "_present"])
        else:
            w.put(name, c[name])
    w.commit(CELL_ROWS)
    img = w.image()
    w.close()
    return img, c


def cell_plan(**kw):
    sel = [col("nk"), count(1), sum_(col("a")), sum_(col("vs")), Agg("count_distinct", col("d")),
           min_(col("nb")), max_(col("nb")), mean(col("nb")), col("u"), col("fv"), col("fb"),
           col("s"), col("ns"), col("nu"), col("t")]
    return Plan(CELL_SCHEMA, select=sel, group_by=[col("nk")], **kw)


CELL_SPECS = [U64("nk", dlevel_max=1), BP("n"), LEB("sum_a"), F64("sum_vs"), U32("cd"),
              LEB("min_nb", dlevel_max=1), U64("max_nb", dlevel_max=1), F64("mean_nb", dlevel_max=1),
              BP("u"), F64("fv"), BOOL("fb"), STR("s"), STR("ns", dlevel_max=1),
              U32("nu", dlevel_max=1), TS("t")]


# ---- byte identity: integer, exact float and string columns over a unique required key -----------
ID_GROUPS, ID_ROWS = 2500, 6000
ID_SCHEMA = dict(k=K.T_UINT64, a=K.T_UINT64, nb=K.T_UINT64, fv=K.T_FLOAT64, s=K.T_STRING,
                 ns=K.T_STRING, fb=K.T_BOOL)
ID_COLUMNS = [U64("k"), LEB("a"), LEB("nb", dlevel_max=1), F64("fv"), STR("s"),
              STR("ns", dlevel_max=1), BOOL("fb")]


@functools.lru_cache(maxsize=1)
def id_table():
    i = np.arange(ID_ROWS, dtype=np.uint64)
    g = (i * np.uint64(7919)) % np.uint64(ID_GROUPS)
    c = dict(k=g * np.uint64(5) + np.uint64(9), a=i % np.uint64(1013),
             nb=i % np.uint64(300), fv=g.astype(np.float64) * 0.125,
             fb=(g & np.uint64(1)))
    c["nb_present"] = ((i + g) % np.uint64(4) != 0).astype(np.uint8)
    strings = [PM.group_string(x) for x in range(ID_GROUPS)]
    c["s"] = [strings[x] for x in g.tolist()]
    c["ns"] = c["s"]
    c["ns_present"] = (g % np.uint64(6) != 2).astype(np.uint8)
    w = E.Writer(ID_COLUMNS)
    for sp in ID_COLUMNS:
        name = sp["name"]
        if name + "_present" in c:
            w.put(name, c[name], present=c[name + "_present"])
        else:
            w.put(name, c[name])
    w.commit(ID_ROWS)
    img = w.image()
    w.close()
    return img, c


def id_plan(**kw):
    sel = [col("k"), count(1), sum_(col("a")), min_(col("nb")), max_(col("a")), col("fv"), col("s"),
           col("ns"), col("fb")]
    return Plan(ID_SCHEMA, select=sel, group_by=[col("k")], **kw)


# the same columns under every storage encoding the device writer takes for their types
ID_SPECS = {
    "plain": [U64("k"), U32("n"), U64("sum_a"), U64("min_nb", dlevel_max=1), U32("max_a"),
              F64("fv"), STR("s"), STR("ns", dlevel_max=1), BOOL("fb")],
    "packed": [BP("k", bitpack_max_value=(1 << 14) - 1), BP("n", bitpack_max_value=7), LEB("sum_a"),
               BP("min_nb", dlevel_max=1, bitpack_max_value=511), BP("max_a"),
               F64("fv"), STR("s"), STR("ns", dlevel_max=1), BOOL("fb")],
    "leb128": [LEB("k"), LEB("n"), LEB("sum_a"), LEB("min_nb", dlevel_max=1), LEB("max_a"),
               F64("fv"), STR("s"), STR("ns", dlevel_max=1), BOOL("fb")],
}


# ---- keys and aggregates only: sizes, sorts, chains, exchanges -----------------------------------
KEY_SPECS = [U64("k"), LEB("n"), LEB("sum_a")]


def key_plan(**kw):
    return Plan(PM.KEY_SCHEMA, select=[col("k"), count(1), sum_(col("a"))], group_by=[col("k")], **kw)


SORT_SCHEMA = dict(k=K.T_UINT64, r=K.T_UINT64, b=K.T_UINT64)
SORT_COLUMNS = [U64("k"), U64("r"), U64("b")]
SORT_SPECS = [U64("k"), U64("r"), LEB("b"), LEB("n")]


@functools.lru_cache(maxsize=8)
def sort_table(groups, stride=2):
    """two rows per group of k = 3 + stride * g; r = 2^40 - k mirrors the key order (a group
    order that ascends in k descends in r), b = g % 200 needs one digit pass, every count is 2"""
    rows = 2 * groups
    i = np.arange(rows, dtype=np.uint64)
    g = i % np.uint64(groups)
    k = g * np.uint64(stride) + np.uint64(3)
    c = dict(k=k, r=np.uint64(1 << 40) - k, b=g % np.uint64(200))
    w = E.Writer(SORT_COLUMNS)
    for name in "krb":
        w.put(name, c[name])
    w.commit(rows)
    img = w.image()
    w.close()
    return img, c


def sort_plan(**kw):
    return Plan(SORT_SCHEMA, select=[col("k"), max_(col("r")), max_(col("b")), count(1)],
                group_by=[col("k")], **kw)


# ---- images and rows ----------------------------------------------------------------------------
def writer_image(specs, rows):
    """the image E.Writer(specs) makes of the row tuples `rows` (None = NULL)"""
    w = E.Writer(specs)
    for ci, sp in enumerate(specs):
        vals = [r[ci] for r in rows]
        present = None
        if sp.get("dlevel_max", 0):
            present = np.array([v is not None for v in vals], dtype=np.uint8)
        lt = sp["logical_type"]
        if lt == K.COL_STRING:
            vals = [b"" if v is None else v for v in vals]
        elif lt == K.COL_FLOAT:
            vals = np.array([0.0 if v is None else v for v in vals], dtype=np.float64)
        else:
            vals = np.array([0 if v is None else int(v) for v in vals], dtype=np.uint64)
        w.put(sp["name"], vals, present=present)
    w.commit(len(rows))
    img = w.image()
    w.close()
    return img


def schema_of(specs):
    return {sp["name"]: stype_of_column(sp["logical_type"]) for sp in specs}


def scan_image(img, specs):
    """every row of a cstable image, in row order: a bare scan of all columns on the oracle"""
    names = [sp["name"] for sp in specs]
    return O.oracle_run(img, Plan(schema_of(specs), scan_select=[col(n) for n in names]))


def row_key(r):
    """sort key of a row whose first cell may be None"""
    return (r[0] is not None, r[0] if r[0] is not None else 0)


def assert_rows_equal(got, exp, types, rel=1e-6):
    """multiset comparison keyed by the (unique) first cell: integers, strings, bools and NULLs
    exact, floats within `rel` relative"""
    assert len(got) == len(exp), (len(got), len(exp))
    g = {r[0]: r for r in got}
    e = {r[0]: r for r in exp}
    assert len(g) == len(got) and len(e) == len(exp), "duplicate keys"
    assert set(g) == set(e)
    for k, er in e.items():
        gr = g[k]
        for ci, (a, b) in enumerate(zip(gr, er)):
            if types[ci] == K.T_FLOAT64 and a is not None and b is not None:
                assert abs(a - b) <= rel * abs(b), (k, ci, a, b)
            else:
                assert a == b and type(a) is type(b), (k, ci, a, b)


# ---- plan decisions (no device) -------------------------------------------------------------------
def decide(plan, columns, specs, sort_by=None, merged=False):
    return E.plan_materialize(plan, columns, specs, sort_by=sort_by, merged=merged)
