"""A model of the EVQL_MODE_PARTIAL wire rows (PartialGroupByExpression, groupby.cc:438-472)
and the tables and plans the partial-emit tests share.

A row is (SHA-1 of the group tuple, concatenated saved states).  The tuple is the packed
SVector element of every group expression, the LAST one first; an aggregate's saved state is a
LEB128 varuint (count, integer sums), 8 raw bytes (float sums) or varuint(count) + 8 raw bytes
(min / max / mean, zeros without a non-NULL value); every other select expression leaves as
SValue::encode: type byte, varuint(size), the element -- where an element of exactly 16 bytes
(a string of 11) keeps bit 7 set in its last byte.

The model works on the python columns a table was written from and is pinned on the oracle by
test_partial_emit_cpu.py; test_gpu_partial_emit.py compares the device with the oracle."""
import functools
import hashlib
import struct

import numpy as np

import eventql_amd as E
from eventql_amd import capi as K
from eventql_amd.plan import Call, col, count, lit, max_, mean, min_, sum_

MIN_GROUPS = 1 << 16  # kDeviceEmitMinGroups
M64 = (1 << 64) - 1


# ---- bytes ------------------------------------------------------------------------------------
def varuint(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def element(stype, value):
    """packed SVector element (svalue.cc:410-517); value None = NULL, numbers as 64-bit words"""
    tag = 1 if value is None else 0
    if stype == K.T_BOOL:
        return bytes([1 if value else 0, tag])
    if stype == K.T_STRING:
        s = b"" if value is None else value
        return struct.pack("<I", len(s)) + s + bytes([tag])
    return struct.pack("<Q", 0 if value is None else value) + bytes([tag])


def encoded_cell(stype, value):
    """SValue::encode of a non-aggregate select expression"""
    e = bytearray(element(stype, value))
    if len(e) == 16:
        e[-1] |= 0x80  # the inline buffer's tag byte keeps STAG_INLINE
    return bytes([stype]) + varuint(len(e)) + bytes(e)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- tables -----------------------------------------------------------------------------------
SCHEMA = dict(k=K.T_UINT64, nk=K.T_UINT64, t=K.T_TIMESTAMP64, f=K.T_BOOL, v=K.T_FLOAT64,
              vs=K.T_FLOAT64, a=K.T_UINT64, b=K.T_UINT64, nb=K.T_UINT64, s=K.T_STRING,
              ns=K.T_STRING)
COLUMNS = [
    dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="nk", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
    dict(name="t", logical_type=K.COL_DATETIME, storage_type=K.ENC_UINT64_LEB128),
    dict(name="f", logical_type=K.COL_BOOLEAN, storage_type=K.ENC_BOOLEAN_BITPACKED),
    dict(name="v", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="vs", logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754),
    dict(name="a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128),
    dict(name="b", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
    dict(name="nb", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_LEB128, dlevel_max=1),
    dict(name="s", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN),
    dict(name="ns", logical_type=K.COL_STRING, storage_type=K.ENC_STRING_PLAIN, dlevel_max=1),
]
NULLABLE = ("nk", "nb", "ns")
# sums whose varuints are 1, 1, 2, 5, 9, 10, 2 and 5 bytes long
SUM_VALUES = [0, 127, 128, 1 << 32, (1 << 56) + 5, (1 << 63) + 9, 16383, 1 << 28]
NAN_PAYLOAD = 0x7ff8000000001234
NULL_KEY_GROUP, MAX_KEY_GROUP, NEG_ZERO_GROUP, NAN_GROUP, NEG_ZERO_SUM_GROUP = 5, 6, 7, 8, 9


def group_string(g):
    """lengths cycle through 0 .. 130; distinct from 3 bytes on"""
    return (struct.pack("<I", g) * 33)[:g % 131]


@functools.lru_cache(maxsize=8)
def wide_table(groups=75_000, rows=160_000):
    """every column is a function of the row's group g = i % groups (nb and vs also of the
    row), so that a group's first row is the same whichever row that is"""
    i = np.arange(rows, dtype=np.uint64)
    g = i % np.uint64(groups)
    c = {}
    c["k"] = g * np.uint64(3) + np.uint64(1)
    c["nk"] = c["k"].copy()
    c["nk"][g == MAX_KEY_GROUP] = np.uint64(M64)
    c["nk_present"] = (g != NULL_KEY_GROUP).astype(np.uint8)
    c["t"] = np.uint64(1438055327000000) + g * np.uint64(1000003)
    c["f"] = g & np.uint64(1)
    v = g.astype(np.float64) * 0.5
    v[g == NEG_ZERO_GROUP] = -0.0
    c["v"] = v
    vs = (g % np.uint64(100)).astype(np.float64) * 0.25  # (sums of three are exact in any order)
    vs[g == NAN_GROUP] = 1.0
    vs[g == NEG_ZERO_SUM_GROUP] = -0.0
    c["vs"] = vs
    c["vs"].view(np.uint64)[NAN_GROUP] = np.uint64(NAN_PAYLOAD)  # one NaN row in its group
    a = np.zeros(rows, dtype=np.uint64)
    first = i < np.uint64(groups)
    a[first] = np.array(SUM_VALUES, dtype=np.uint64)[(g[first] % np.uint64(8)).astype(np.int64)]
    c["a"] = a
    c["b"] = i % np.uint64(1500)
    c["nb"] = (g * np.uint64(7)) % np.uint64(1000) + i // np.uint64(groups)
    c["nb_present"] = (g % np.uint64(3) != 0).astype(np.uint8)
    strings = [group_string(x) for x in range(groups)]
    gl = g.tolist()
    c["s"] = [strings[x] for x in gl]
    c["ns"] = c["s"]
    c["ns_present"] = (g % np.uint64(10) != 3).astype(np.uint8)
    w = E.Writer(COLUMNS)
    for spec in COLUMNS:
        name = spec["name"]
        if name in NULLABLE:
            w.put(name, c[name], present=c[name + "_present"])
        else:
            w.put(name, c[name])
    w.commit(rows)
    img = w.image()
    w.close()
    return img, c, rows


KEY_SCHEMA = dict(k=K.T_UINT64, a=K.T_UINT64)
KEY_COLUMNS = [dict(name="k", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN),
               dict(name="a", logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT64_PLAIN)]


@functools.lru_cache(maxsize=8)
def key_table(groups):
    """exactly `groups` groups of k (the threshold cases)"""
    rows = groups + 500
    i = np.arange(rows, dtype=np.uint64)
    c = dict(k=(i % np.uint64(groups)) * np.uint64(2) + np.uint64(3), a=i % np.uint64(977))
    w = E.Writer(KEY_COLUMNS)
    w.put("k", c["k"])
    w.put("a", c["a"])
    w.commit(rows)
    img = w.image()
    w.close()
    return img, c, rows


# ---- plans ------------------------------------------------------------------------------------
# a case: group columns, then select items ("col", name) | ("count",) | ("sum", name) |
# ("sumi", name, negative literal) | ("sumf", name) | ("min" | "max" | "mean", name)
def case(keys, *items):
    return dict(keys=list(keys), items=[("col", k) for k in keys] + list(items))


THRESHOLD_CASE = case(["k"], ("count",), ("sum", "a"))
CASES = {
    # keys
    "u64": case(["k"], ("count",), ("sum", "a")),
    "u64_null_max": case(["nk"], ("count",), ("sum", "a")),
    "u64_timestamp": case(["k", "t"], ("count",)),
    "u64_bool": case(["k", "f"], ("count",)),
    "u64_float": case(["k", "v"], ("count",)),
    "string": case(["s"], ("count",)),
    "u64_string": case(["k", "s"], ("count",), ("sum", "a")),
    "nullable_string": case(["ns"], ("count",)),
    # states
    "sums": case(["k"], ("count",), ("sum", "a"), ("sumi", "b", -1000), ("sum", "b")),
    "float_sum": case(["k"], ("sumf", "vs"), ("sumf", "v")),
    "min_max_mean": case(["k"], ("min", "nb"), ("max", "nb"), ("mean", "nb"), ("count",)),
    "columns": case(["k"], ("col", "t"), ("col", "f"), ("col", "v"), ("col", "s"), ("col", "ns"),
                    ("count",)),
}


def plan_kwargs(cs):
    """Plan keyword arguments of a case"""
    sel = []
    for it in cs["items"]:
        kind = it[0]
        if kind == "col":
            sel.append(col(it[1]))
        elif kind == "count":
            sel.append(count(1))
        elif kind in ("sum", "sumf"):
            sel.append(sum_(col(it[1])))
        elif kind == "sumi":
            sel.append(sum_(Call("add", col(it[1]), lit(it[2]))))
        else:
            sel.append(dict(min=min_, max=max_, mean=mean)[kind](col(it[1])))
    return dict(select=sel, group_by=[col(k) for k in cs["keys"]])


def _words(c, name, schema):
    """the column as 64-bit words / bytes, None where NULL"""
    vals = c[name]
    if schema[name] == K.T_FLOAT64:
        vals = np.asarray(vals).view(np.uint64)
    vals = vals.tolist() if hasattr(vals, "tolist") else list(vals)
    if name + "_present" in c:
        pres = c[name + "_present"].tolist()
        vals = [x if p else None for x, p in zip(vals, pres)]
    if schema[name] == K.T_BOOL:
        vals = [None if x is None else int(x != 0) for x in vals]
    return vals


def model_rows(cs, c, rows, schema):
    """{key: data} of the PARTIAL rows of a case over the columns `c`"""
    used = set(cs["keys"]) | {it[1] for it in cs["items"] if len(it) > 1}
    w = {name: _words(c, name, schema) for name in used}
    groups = {}
    for r in range(rows):
        groups.setdefault(tuple(w[k][r] for k in cs["keys"]), []).append(r)
    out = {}
    for key, members in groups.items():
        tup = b"".join(element(schema[k], x) for k, x in reversed(list(zip(cs["keys"], key))))
        r0 = members[0]
        data = bytearray()
        for it in cs["items"]:
            kind = it[0]
            if kind == "col":
                data += encoded_cell(schema[it[1]], w[it[1]][r0])
            elif kind == "count":
                data += varuint(len(members))
            elif kind == "sum":
                data += varuint(sum(w[it[1]][r] for r in members) & M64)
            elif kind == "sumi":
                data += varuint(sum(w[it[1]][r] + it[2] for r in members) & M64)
            elif kind == "sumf":
                acc = 0.0
                for r in members:
                    acc += struct.unpack("<d", struct.pack("<Q", w[it[1]][r]))[0]
                data += struct.pack("<d", acc)
            else:
                vals = [w[it[1]][r] for r in members if w[it[1]][r] is not None]
                data += varuint(len(vals))
                if not vals:
                    data += bytes(8)
                elif kind == "mean":
                    data += struct.pack("<d", float(sum(vals)))
                else:
                    data += struct.pack("<Q", min(vals) if kind == "min" else max(vals))
        out[hashlib.sha1(tup).digest()] = bytes(data)
    return out


def oracle_rows(exp):
    """{key: data} of an oracle result in EVQL_MODE_PARTIAL"""
    return {exp.keys[20 * i:20 * i + 20]: exp.columns[0][i] for i in range(exp.nrows)}
