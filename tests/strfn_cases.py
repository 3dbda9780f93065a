"""The cases of tests/golden/ref_csql_strfn.json and ref_csql_strfnlsm.json: string
functions evaluated PER ROW -- as group keys, as operands of WHERE compares and inside
the arguments of numeric aggregates -- run through the reference's own engine.

Importing this module registers the two suites with tests/refcases.py.  The fixtures are
regenerated, where the reference tree and its probe exist, by

    python tests/strfn_cases.py [--refused-by PARENT_LIBRARY]

which hands the suites to tests/golden/gen_ref_csql.py.  With --refused-by, every case is
first planned by that build of the library (one from before string functions were
evaluated per row) and must be answered EVQL_ENOTSUP there: no case is one the library
lowered anyway.
"""
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eventql_amd import capi as K
from eventql_amd.plan import Col, Lit, Call, If, Agg
import refcases
import tables as T

STR_LITS = refcases.RefStrGen.str_lits + ("g17", "s4", "G1", "S")


def holds(e, pred):
    return pred(e) or any(holds(c, pred) for c in e.children())


def per_row_tree(g):
    """a tree of RefStrGen.strx whose root is a function call (a bare column would test
    nothing new), without IF and without to_string of a float column (both stay refused).
    Nor the DATETIME column t: a scan of the reference types it UINT64 where
    tables.MIXED_SCHEMA says TIMESTAMP64, so the dumped programs would not be plan.py's."""
    def refused(e):
        return isinstance(e, If) or (isinstance(e, Col) and e.name == "t") or (
            isinstance(e, Call) and e.name == "to_string" and
            isinstance(e.args[0], Col) and e.args[0].name in g.float_cols)
    while True:
        e = g.strx()
        if isinstance(e, Call) and not holds(e, refused):
            return e


def strfn_kwargs(seed, g):
    r = g.r
    k, k10, a = Col("k"), Col("k10"), Col("a")
    shape = seed % 3
    if shape == 0:
        key = per_row_tree(g)
        return dict(select=[key, Agg("count", Lit(1)), Agg("sum", a)], group_by=[key],
                    where=Call("lt", k, Lit(r.choice([30, 120]))))
    if shape == 1:
        op = r.choice(["eq", "neq", "lt", "gte", "startswith", "endswith"])
        return dict(select=[k10, Agg("count", Lit(1)), Agg("sum", a)], group_by=[k10],
                    where=Call(op, per_row_tree(g), Lit(r.choice(STR_LITS))))
    op = r.choice(["eq", "lt", "startswith"])
    cond = Call(op, per_row_tree(g), per_row_tree(g))
    return dict(select=[k10, Agg("sum", If(cond, a, Lit(0)))], group_by=[k10],
                where=Call("lt", k, Lit(200)))


@refcases.suite("strfn")
def strfn_cases():
    out = []
    for seed in range(60):
        g = refcases.RefStrGen(110_000 + seed, **refcases.MIXED)
        c = None
        while c is None:  # (redrawn when the plan has no SQL text: an unfoldable constant)
            c = refcases._case("strfn-%03d" % seed, "mixed", strfn_kwargs(seed, g), T.MIXED_SCHEMA)
        out.append(c)
    return out


@refcases.suite("strfnlsm")
def strfnlsm_cases():
    import lsm_tables
    k, a, s = Col("k"), Col("a"), Col("s")
    one = Agg("count", Lit(1))
    ucase = Call("ucase", s)
    cat = Call("concat", s, Call("to_string", Call("mod", k, Lit(3))))
    named = [
        ("ucase-key", dict(select=[ucase, one, Agg("sum", a)], group_by=[ucase])),
        ("concat-key", dict(select=[cat, one, Agg("sum", a)], group_by=[cat])),
        ("substring-where", dict(select=[k, one, Agg("sum", a)], group_by=[k],
                                 where=Call("eq", Call("substring", s, Lit(2)), Lit("1")))),
        ("affix-in-sum", dict(select=[k, Agg("sum", If(Call("startswith", Call("concat", Lit("x"), s),
                                                            Lit("xg1")), a, Lit(0)))],
                              group_by=[k])),
    ]
    out = []
    for pname in ("basic", "mixed", "quiet"):
        for cid, kw in named:
            c = refcases._case("strfnlsm-%s-%s" % (pname, cid), "lsm:" + pname, kw,
                               lsm_tables.LSM_SCHEMA)
            assert c is not None, cid
            out.append(c)
    return out


def schema_columns(schema):
    """column descriptions for compile_only that agree with `schema` (the planner's
    decision does not depend on the encodings)"""
    kinds = {K.T_STRING: (K.COL_STRING, K.ENC_STRING_PLAIN),
             K.T_FLOAT64: (K.COL_FLOAT, K.ENC_FLOAT_IEEE754),
             K.T_BOOL: (K.COL_BOOLEAN, K.ENC_UINT64_PLAIN),
             K.T_TIMESTAMP64: (K.COL_DATETIME, K.ENC_UINT64_PLAIN)}
    return [dict(name=n, logical_type=kinds.get(t, (K.COL_UNSIGNED_INT, 0))[0],
                 storage_type=kinds.get(t, (0, K.ENC_UINT64_PLAIN))[1]) for n, t in schema.items()]


def assert_refused_by_the_loaded_library():
    import eventql_amd as E
    from eventql_amd.plan import Plan
    n = 0
    for name in ("strfn", "strfnlsm"):
        for c in refcases.SUITES[name]():
            schema = refcases.table_schema(c["table"])
            try:
                E.compile_only(Plan(schema, **c["kw"]), schema_columns(schema))
            except E.EvqlError as e:
                assert e.code == K.EVQL_ENOTSUP, (c["id"], e)
                n += 1
                continue
            raise AssertionError("%s is lowered by %s" % (c["id"], E.LIB_PATH))
    print("%d cases refused by %s" % (n, E.LIB_PATH))


if __name__ == "__main__":
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    if sys.argv[1:2] == ["--check-refused"]:
        assert_refused_by_the_loaded_library()
        sys.exit(0)
    if sys.argv[1:2] == ["--refused-by"]:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--check-refused"],
                              env=dict(os.environ, EVQL_LIB=os.path.abspath(sys.argv[2])))
    sys.path.insert(0, os.path.join(here, "golden"))
    import gen_ref_csql
    gen_ref_csql.main(["strfn", "strfnlsm"])
