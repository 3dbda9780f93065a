"""The column width mixes that pin the prefetching tile loop of evql_scan_agg:
one table of columns of every copy width, the plans over it, and for each plan which loop it
is to take.  Imported by test_scan_prefetch_widths_cpu.py (the compiled gfx950 code objects)
and test_gpu_scan_prefetch_widths.py (the same plans on the device).

The loop holds one raw word per step for an 8- or 16-bit copy and two for a 32-bit or float32
copy (codegen_kernels.inc raw_words), each width with its own load and decode.  The lists:

  PREFETCH     admitted by choose_launch_shape and compiled without scratch: the prefetching loop
  FALLS_BACK   admitted, but the compiled kernel reports scratch: compile_plan_kernels drops the
               prefetch at run time (empty: see the note at WIDE below)
  PLAIN_LOOP   not admitted -- the planner's unroll budget takes unroll below 4, or a column is
               not read through a flat copy: the plain loop, whatever EVQL_SCAN_PREFETCH says

Every column is a required column; the file's own widths play no part, the plans read the narrow
copies (EVQL_NARROW_PLAIN=1, EVQL_NARROW_FLOAT=1; a required LEB128 column narrows anyway)."""
import numpy as np

from eventql_amd import capi as K
from eventql_amd.plan import col, count, max_, min_, sum_

TILE = 8192  # rows per tile of every plan below: block 1024 x 2 rows x unroll 4
MARKER = "have || t < A.ntiles"  # the head of the prefetching loop in the generated text

# column -> width of the copy a resident table keeps ("f32": the float32 copy; 0: none, the
# bit-packed pages of the file are read as they are)
WIDTHS = dict(k8=8, k16=16, k32=32, g3=8, a8=8, a16=16, a32=32, b8=8, b32=32, v="f32", w="f32",
              l16=16, p16=0)
TOP = {8: 255, 16: 65535, 32: (1 << 32) - 1}
SCHEMA = {n: (K.T_FLOAT64 if w == "f32" else K.T_UINT64) for n, w in WIDTHS.items()}


def _spec(name):
    if WIDTHS[name] == "f32":
        return dict(name=name, logical_type=K.COL_FLOAT, storage_type=K.ENC_FLOAT_IEEE754)
    if name == "p16":  # (the width of a bit-packed column's pages follows its declared maximum)
        return dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=K.ENC_UINT32_BITPACKED,
                    bitpack_max_value=TOP[16])
    enc = K.ENC_UINT64_LEB128 if name == "l16" else K.ENC_UINT64_PLAIN
    return dict(name=name, logical_type=K.COL_UNSIGNED_INT, storage_type=enc)


# what the writer takes, and what compile_only takes for the same table once it is resident
FILE_COLUMNS = [_spec(n) for n in WIDTHS]
COPY_COLUMNS = [dict(_spec(n), bits=16) if n == "p16" else
                dict(_spec(n), narrow_bits=32 if w == "f32" else w) for n, w in WIDTHS.items()]


def accessor(name, i):
    """how the generated text loads scan column i = `name` (test_gpu_flat_narrow.flat)"""
    w = WIDTHS[name]
    if w == "f32":
        return "evql_f32_x2(A.col[%d].base, r, " % i
    if w == 0:
        return "evql_bitpacked_x2<16>(A.col[%d].base, A.col[%d].pages, r, " % (i, i)
    return "evql_bitpacked_x2<%d>(A.col[%d].base, r, " % (w, i)


# ---- the plans -------------------------------------------------------------------------------
def _c1(a):
    """a > c1: about half of the rows, the width's maximum among them"""
    return TOP[WIDTHS[a]] // 2


def _c2(b):
    """b < c2 with c2 = the width's maximum + 1: 0 and the maximum both pass (the compare stays
    in the text -- a copy's values are opaque to the compiler -- and a > c1 does the filtering)"""
    return TOP[WIDTHS[b]] + 1


class Mix:
    """kw: the plan's keywords; kw["where"] = (a, b) stands for WHERE a > c1 AND b < c2"""

    def __init__(self, name, kw, fast=False, lcache=1):
        self.name, self.fast, self.lcache = name, fast, lcache
        self.filt = kw.get("where")
        self.kw = dict(kw)
        if self.filt:
            a, b = self.filt
            self.kw["where"] = (col(a) > _c1(a)) & (col(b) < _c2(b))

    def passes(self, c):
        """the rows of the columns `c` that pass WHERE, on the host"""
        if not self.filt:
            return np.ones(len(c["k8"]), bool)
        a, b = self.filt
        return (c[a] > np.uint64(_c1(a))) & (c[b] < np.uint64(_c2(b)))

    def modes(self):
        return ("exact", "fast") if self.fast else ("exact",)

    def plan_kw(self, exact=True, **window):
        fs = dict(float_sum_mode=K.FLOAT_SUM_EXACT) if exact else {}
        return dict(self.kw, **fs, **window)

    def __repr__(self):
        return self.name


def config3_form(key, a, b, f=None, hint=1000):
    """SELECT key, sum(f), count(1), sum(b) .. WHERE a > c1 AND b < c2 GROUP BY key"""
    sel = [col(key)] + ([sum_(col(f))] if f else [sum_(col(a))]) + [count(1), sum_(col(b))]
    return dict(select=sel, group_by=[col(key)], where=(a, b), groups_hint=hint)


PREFETCH = [
    # every column one raw word, or the float32 copy
    Mix("k8-a8-b8-v", config3_form("k8", "a8", "b8", "v", hint=200), fast=True),
    # every column two raw words
    Mix("k32-a32-b32-v", config3_form("k32", "a32", "b32", "v"), fast=True),
    # mixed widths: different register layouts of c<i>[u][w]
    Mix("k16-a8-b32-v", config3_form("k16", "a8", "b32", "v")),
    Mix("k8-a32-b8-v", config3_form("k8", "a32", "b8", "v", hint=200)),
    Mix("k32-a16-b8-w", config3_form("k32", "a16", "b8", "w")),
    # three columns, integer sums only: the smallest shape the rule admits
    Mix("k32-a32-b32", config3_form("k32", "a32", "b32")),
    # five columns within the unroll budget (3 update words): 32-bit values in max / min and in
    # arithmetic, the other two columns as first-row values
    Mix("five-max", dict(select=[col("k16"), max_(col("a32")), sum_(col("a8") * 3 + 1), col("b32"), col("v")],
                         group_by=[col("k16")], where=("a8", "b32"), groups_hint=1000)),
    Mix("five-min", dict(select=[col("k16"), min_(col("b32")), sum_(col("a8") * 3 + 1), col("a32"), col("v")],
                         group_by=[col("k16")], where=("a8", "b32"), groups_hint=1000)),
    # first-row values come from the raw tile
    Mix("first-row", dict(select=[col("k32"), col("a32"), col("b8"), col("v"), count(1)],
                          group_by=[col("k32")], groups_hint=1000)),
    # three groups under a hint of 3: four lane-private accumulators next to the rotating loop
    Mix("g3-a32-b8-v", config3_form("g3", "a32", "b8", "v", hint=3), lcache=4),
    # a LEB128 column's copy comes from the decode path (table.cc pack_narrow)
    Mix("l16-a8-b32-v", config3_form("l16", "a8", "b32", "v")),
    # WIDE: towards five 32-bit columns.  Five two-word columns within the budget compile without
    # scratch, and a sixth column cannot be admitted: 50 + 4 * 6 * 4 > 144 already takes unroll
    # below 4 (choose_launch_shape).  The budget bites before the registers do, so FALLS_BACK
    # stays empty.
    Mix("five-32", dict(select=[col("k32"), sum_(col("b32")), sum_(col("v")), col("w")],
                        group_by=[col("k32")], where=("a32", "b32"), groups_hint=1000)),
]

FALLS_BACK = []

PLAIN_LOOP = [
    # five columns with max(a32), min(b32), a sum over a8 * 3 + 1 and sum(v): 7 update words,
    # 50 + 4 * 5 * 4 + 4 * 7 > 144 -- unroll 2, outside the rule
    Mix("five-max-min", dict(select=[col("k16"), max_(col("a32")), min_(col("b32")), sum_(col("a8") * 3 + 1),
                                     sum_(col("v")), count(1)],
                             group_by=[col("k16")], where=("a8", "b32"), groups_hint=1000)),
    # six columns: unroll 2 whatever the aggregates
    Mix("six", dict(select=[col("k32"), sum_(col("b32")), count(1), col("v"), col("w"), col("a16")],
                    group_by=[col("k32")], where=("a32", "b32"), groups_hint=1000)),
    # a bit-packed column of the file keeps no flat copy: its pages are read through the page
    # table (ColAccess::BITPACKED), which the rule does not admit
    Mix("p16-a8-b32-v", config3_form("p16", "a8", "b32", "v")),
]

ALL = PREFETCH + FALLS_BACK + PLAIN_LOOP
BY_NAME = {m.name: m for m in ALL}


# ---- the table -------------------------------------------------------------------------------
def spread(count_, top):
    """`count_` distinct values over [0, top], both ends among them"""
    return (np.arange(count_, dtype=np.uint64) * np.uint64(top)) // np.uint64(count_ - 1)


def edge_rows(n, G):
    """The rows (< n) at which every integer column holds 0 or its width's maximum: both rows
    of a pair, the first and the last row of a tile, the first row of tile G (a workgroup's
    second tile), the table's last row and the row before it -- and, for the windows of the
    device test, row 0, the last row of tile 0, the first and the last row of the window
    [G * T + 101, 2 * G * T + 77) and the tile border inside its last tile."""
    T = TILE
    rows = [4098, 4099, T, 2 * T - 1, G * T, n - 1, n - 2,
            0, T - 1, G * T + 101, 2 * G * T + 76, 2 * G * T - 1, 2 * G * T]
    return sorted({r for r in rows if 0 <= r < n})


# float edges: -0.0, and the largest and the smallest magnitude an exact sum's quantum allows.
# v = m / 1024 with m < 2^24: |v| < 2^14, quantum 2^(14 - 61) (choose_exact_sum_scales); w = m / 4:
# |w| < 2^22, quantum 2^-39.  Every value is a normal float32 or a zero.
F_SCALE = dict(v=1024.0, w=4.0)
F_QUANTUM = dict(v=2.0 ** -47, w=2.0 ** -39)


def float_edges(name):
    big = float((1 << 24) - 1) / F_SCALE[name]
    q = F_QUANTUM[name]
    return [-0.0, big, -big, q, -q]  # (five: the small table has five edge rows)


def table_columns(n, G, seed=20):
    """name -> n values (uint64, float64 for v and w); see edge_rows"""
    rng = np.random.default_rng(seed)
    keys = dict(k8=spread(200, 255), k16=spread(1000, 65535), k32=spread(1000, TOP[32]),
                g3=np.array([0, 100, 255], np.uint64), l16=spread(1000, 65535)[::-1].copy(),
                p16=spread(1000, 65535))
    c = {}
    for name, values in keys.items():
        c[name] = values[rng.integers(0, len(values), n)]
    for name in ("a8", "a16", "a32", "b8", "b32"):
        c[name] = rng.integers(0, TOP[WIDTHS[name]], n, dtype=np.uint64, endpoint=True)
    for name in ("v", "w"):
        c[name] = rng.integers(0, 1 << 24, n).astype(np.float64) / F_SCALE[name]
    edges = edge_rows(n, G)
    listed = set(edges)
    for i, r in enumerate(edges):
        partner = r ^ 1
        for name, width in WIDTHS.items():
            if width == "f32":
                fe = float_edges(name)
                c[name][r] = fe[(i + (name == "w")) % len(fe)]
                continue
            top = np.uint64(TOP[width or 16])
            if name[0] == "a":
                here = top  # (a > c1 has to pass at every listed row)
            elif name[0] == "b":
                here = top if (i // 2) % 2 == 0 else np.uint64(0)
            else:
                here = top if i % 2 == 0 else np.uint64(0)
            c[name][r] = here
            # the other row of the pair shares the loaded word: the opposite end of the width
            # (a = 0 there: the row fails WHERE)
            if partner < n and partner not in listed:
                c[name][partner] = top - here
    return c
