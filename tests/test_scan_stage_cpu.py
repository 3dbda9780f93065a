"""The staging tile loop of evql_scan_agg without a GPU: config 3 over its
narrow and float32 copies compiles for gfx950 to the prefetching loop with WHERE alone per row,
an 8-byte tuple per passing row written to a ring of the wave in LDS, and the group update once
per 64 tuples; EVQL_SCAN_STAGE=0 gives the prefetching loop as it was; the shapes the rule
excludes compile to the same bytes either way; and a tuple's pack and unpack, restated on the
host from the layout the generated text states, return every field at both ends of its width.

The tuple holds COLUMNS (what the group key and the aggregate arguments read, as the bits of
their copies), not computed operands: a field is 8, 16 or 32 bits or a raw float32 word.  There
is no 64-bit field to restate -- a plan is admitted only if every column is read from a copy of
at most 32 bits, and what is computed from them is computed behind the ring."""
import re
import subprocess

import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B
from eventql_amd.plan import Plan, col, count, count_distinct, sum_

import scan_width_mixes as M
from test_flat_narrow_cpu import LLVM, audit, disassembly, tile_load_clusters
from test_scan_hot_path_cpu import NARROW_F32
from test_scan_prefetch_cpu import back_edge, code, loops

STAGE = "evql_stage_ring"  # the ring's name: in the text of a staging plan only
LDS_BYTES = 160 * 1024

k, a, b, v = [col(x) for x in "kabv"]
WHERE3 = (a > 30000) & (b < 30000)


@pytest.fixture
def switch(monkeypatch):
    monkeypatch.delenv("EVQL_SCAN_PREFETCH", raising=False)

    def set_(on):
        if on:
            monkeypatch.delenv("EVQL_SCAN_STAGE", raising=False)
        else:
            monkeypatch.setenv("EVQL_SCAN_STAGE", "0")
    return set_


def lds_bytes(obj, kernel="evql_scan_agg"):
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", obj], capture_output=True, text=True,
                           check=True).stdout
    for blk in notes.split("- .agpr_count")[1:]:
        if re.search(r"\.name:\s+(\w+)", blk).group(1) == kernel:
            return int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    raise AssertionError("no such kernel")


def test_config3_takes_the_staging_loop(built, tmp_path, switch):
    switch(True)
    text_on = E.plan_kernel_text(B.config3(), NARROW_F32)
    obj_on, on = code(tmp_path, "on", B.config3(), NARROW_F32)
    switch(False)
    text_off = E.plan_kernel_text(B.config3(), NARROW_F32)
    obj_off, off = code(tmp_path, "off", B.config3(), NARROW_F32)
    assert on != off and text_on != text_off
    assert STAGE in text_on and STAGE not in text_off
    assert M.MARKER in text_on and M.MARKER in text_off  # both are the prefetching loop
    # b:16 | k:16 | v:32 (scan columns a, b, k, v: a is read by WHERE alone)
    assert "struct alignas(8) EvqlStaged { u32 w[2]; };" in text_on
    assert "t.w[0] = f0 | (f1 << 16);" in text_on and "t.w[1] = f2;" in text_on
    vgprs, spill, scratch, flat = audit(obj_on)["evql_scan_agg"]
    lds = lds_bytes(obj_on)
    print("staging: %d VGPRs, %d B of LDS (prefetching loop: %d VGPRs, %d B)"
          % (vgprs, lds, audit(obj_off)["evql_scan_agg"][0], lds_bytes(obj_off)))
    assert (spill, scratch, flat) == (0, 0, 0)
    assert vgprs <= 89
    assert lds_bytes(obj_off) < lds <= LDS_BYTES
    ins = disassembly(obj_on)["evql_scan_agg"]
    assert [len(c) for c in tile_load_clusters(ins)] == [16, 16]
    with_test, without = loops(ins)
    assert len(with_test) == 1 and len(without) == 1
    c = without[0]
    later = [x[0] for x in tile_load_clusters(ins) if x[0] > c[0]]
    end = back_edge(ins, c, later[0] if later else len(ins))
    puts = [i for i in range(c[-1], end) if ins[i].startswith("ds_write_b64")]
    print("loop without zone test %d..%d, ds_write_b64 at %s" % (c[0], end, puts))
    assert len(puts) >= 8  # one per row of a step: 4 steps x 2 rows
    # the loop with zone test keeps the plain form: behind the table's initialisation, in front
    # of the kernel's first tile load, no 8-byte LDS store lies outside the staging loop
    first = min(with_test[0][0], c[0])
    assert [i for i, x in enumerate(ins) if i > first and x.startswith("ds_write_b64")] == puts


# wide: five 32-bit columns the prefetching loop admits (scan_width_mixes "five-32" with sums in
# place of its first-row column); the tuple is k32, b32, v, w = 16 bytes, 72 more than the LDS
# has left beside 4096 slots of 4 words
WIDE = dict(select=[col("k32"), sum_(col("b32")), sum_(col("v")), sum_(col("w"))], group_by=[col("k32")],
            where=(col("a32") > 5) & (col("b32") < 7), groups_hint=1000)
# twelve bytes (k32, b32, v) fit
FITS = dict(WIDE, select=[col("k32"), sum_(col("b32")), sum_(col("v")), count(1)])

# shape -> (plan, columns, is the prefetching loop in the text?)
EXCLUDED = {
    "no WHERE": (lambda: Plan(B.SCHEMA, select=[k, sum_(v), count(1), sum_(b), sum_(a)], group_by=[k],
                              groups_hint=1000), NARROW_F32, True),
    "first-row column": (lambda: Plan(B.SCHEMA, select=[k, sum_(v), count(1), b], group_by=[k], where=WHERE3,
                                      groups_hint=1000), NARROW_F32, True),
    "count_distinct": (lambda: Plan(B.SCHEMA, select=[k, sum_(v), count_distinct(b)], group_by=[k],
                                    where=WHERE3, groups_hint=1000), NARROW_F32, False),
    "tuple too wide": (lambda: Plan(M.SCHEMA, **WIDE), M.COPY_COLUMNS, True),
    "config2": (B.config2, NARROW_F32, False),
    "config3 over plain pages": (B.config3, B.PLAIN_COLUMNS, False),
}


@pytest.mark.parametrize("shape", sorted(EXCLUDED))
def test_excluded_shapes_do_not_know_the_switch(built, tmp_path, switch, shape):
    plan, columns, prefetching = EXCLUDED[shape]
    switch(True)
    text = E.plan_kernel_text(plan(), columns)
    assert STAGE not in text
    assert (M.MARKER in text) == prefetching, shape
    _, on = code(tmp_path, "on", plan(), columns)
    switch(False)
    _, off = code(tmp_path, "off", plan(), columns)
    assert on == off


def test_twelve_bytes_fit_and_sixteen_do_not(built, tmp_path, switch):
    switch(True)
    text = E.plan_kernel_text(Plan(M.SCHEMA, **FITS), M.COPY_COLUMNS)
    assert "struct alignas(4) EvqlStaged { u32 w[3]; };" in text and STAGE in text
    obj, _ = code(tmp_path, "fits", Plan(M.SCHEMA, **FITS), M.COPY_COLUMNS)
    vgprs, spill, scratch, flat = audit(obj)["evql_scan_agg"]
    assert (spill, scratch, flat) == (0, 0, 0)
    # the table (4 words x 4098 slots + 1) and 16 rings of 128 x 12 bytes
    assert 131144 + 16 * 128 * 12 <= lds_bytes(obj) <= LDS_BYTES
    assert 131144 + 16 * 128 * 16 > LDS_BYTES


def test_prefetch_off_switches_staging_off(built, monkeypatch):
    monkeypatch.setenv("EVQL_SCAN_PREFETCH", "0")
    monkeypatch.delenv("EVQL_SCAN_STAGE", raising=False)
    text = E.plan_kernel_text(B.config3(), NARROW_F32)
    assert STAGE not in text and M.MARKER not in text
    monkeypatch.setenv("EVQL_SCAN_STAGE", "0")
    assert E.plan_kernel_text(B.config3(), NARROW_F32) == text


# ---- pack and unpack, restated on the host ---------------------------------------------------
def layout_of(text):
    """(words, pack: word -> [(field, shift)], unpack: column -> (kind, word, shift)) as the
    generated text states them"""
    words = int(re.search(r"EvqlStaged \{ u32 w\[(\d+)\]; \};", text).group(1))
    pack = {}
    for w, rhs in re.findall(r"  t\.w\[(\d+)\] = (.*);", text):
        pack[int(w)] = [(int(f), int(sh or 0)) for f, sh in re.findall(r"f(\d+)(?: << (\d+))?", rhs)]
    unpack = {}
    for c, body in re.findall(r"u64 evql_stage_col(\d+)\(const EvqlStaged& t\) \{\n(.*?)\n\}", text, re.S):
        if "evql_f32_dec" in body:
            unpack[int(c)] = ("f32", int(re.search(r"t\.w\[(\d+)\]", body).group(1)), 0)
        elif ">>" in body:
            m = re.search(r"\(t\.w\[(\d+)\] >> (\d+)\) & 0xffffu", body)
            unpack[int(c)] = ("half", int(m.group(1)), int(m.group(2)))
        else:
            unpack[int(c)] = ("word", int(re.search(r"t\.w\[(\d+)\]", body).group(1)), 0)
    return words, pack, unpack


def pack(lay, fields):
    words, p, _ = lay
    out = []
    for w in range(words):
        x = 0
        for f, sh in p[w]:
            x |= (fields[f] << sh) & 0xffffffff
        out.append(x)
    return out


def unpack(lay, t, column):
    kind, w, sh = lay[2][column]
    if kind == "f32":
        with np.errstate(invalid="ignore"):
            return int(np.float64(np.uint32(t[w]).view(np.float32)).view(np.uint64))
    return (t[w] >> sh) & 0xffff if kind == "half" else t[w]


F32_EDGES = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x00800000]
F64_OF = {0x00000000: 0, 0x80000000: 0x8000000000000000, 0x7f800000: 0x7ff0000000000000,
          0xff800000: 0xfff0000000000000, 0x7fc12345: 0x7ff82468a0000000, 0xffc00001: 0xfff8000020000000,
          0x00800000: 0x3810000000000000}


def mix_plan(name):
    return Plan(M.SCHEMA, **M.BY_NAME[name].plan_kw(True))


# name -> (plan and columns, the staged columns and the widths of their copies)
TUPLES = {
    "config3": (lambda: (B.config3(), NARROW_F32), [("k", 16), ("b", 16), ("v", "f32")]),
    "k8-a8-b8-v": (lambda: (mix_plan("k8-a8-b8-v"), M.COPY_COLUMNS), [("k8", 8), ("b8", 8), ("v", "f32")]),
    "k16-a8-b32-v": (lambda: (mix_plan("k16-a8-b32-v"), M.COPY_COLUMNS), [("k16", 16), ("b32", 32), ("v", "f32")]),
    "k32-a32-b32": (lambda: (mix_plan("k32-a32-b32"), M.COPY_COLUMNS), [("k32", 32), ("a32", 32), ("b32", 32)]),
    "k32-a16-b8-w": (lambda: (mix_plan("k32-a16-b8-w"), M.COPY_COLUMNS), [("b8", 8), ("k32", 32), ("w", "f32")]),
}


@pytest.mark.parametrize("name", sorted(TUPLES))
def test_pack_then_unpack_returns_every_field(built, monkeypatch, name):
    monkeypatch.delenv("EVQL_SCAN_PREFETCH", raising=False)
    monkeypatch.delenv("EVQL_SCAN_STAGE", raising=False)
    make, fields = TUPLES[name]
    plan, columns = make()
    text = E.plan_kernel_text(plan, columns)
    lay = layout_of(text)
    column_of = {n: i for i, n in enumerate(plan.scan_columns)}
    # the layout's order: the fields of at most 16 bits by scan column, then the 32-bit ones
    fields = sorted(fields, key=lambda f: (f[1] in (32, "f32"), column_of[f[0]]))
    assert sorted(lay[2]) == sorted(column_of[n] for n, _ in fields), (name, lay)
    assert sorted(f for w in lay[1].values() for f, _ in w) == list(range(len(fields)))
    # two fields of at most 16 bits share a word; every other field has its own
    halves = sum(1 for _, w in fields if w in (8, 16))
    assert lay[0] == (halves + 1) // 2 + len(fields) - halves
    top = lambda w: 0xffffffff if w == "f32" else (1 << w) - 1
    # every field at its maximum while the others are 0, all 0, all at their maximum
    cases = [[0] * len(fields), [top(w) for _, w in fields]]
    for i, (_, w) in enumerate(fields):
        cases.append([top(w) if j == i else 0 for j in range(len(fields))])
    for i, (_, w) in enumerate(fields):
        for e in F32_EDGES if w == "f32" else []:
            cases.append([e if j == i else top(x) for j, (_, x) in enumerate(fields)])
    for values in cases:
        t = pack(lay, values)
        assert len(t) == lay[0] and all(0 <= x <= 0xffffffff for x in t)
        for (n, w), want in zip(fields, values):
            got = unpack(lay, t, column_of[n])
            if w == "f32":
                with np.errstate(invalid="ignore"):
                    widened = int(np.float64(np.uint32(want).view(np.float32)).view(np.uint64))
                assert got == widened, (name, n, hex(want), hex(got))
                if want in F64_OF:
                    assert got == F64_OF[want], (name, n, hex(want), hex(got))
            else:
                assert got == want, (name, n, values, t)
