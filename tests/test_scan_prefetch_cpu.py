"""The prefetching tile loop of evql_scan_agg without a GPU: config 3 over
its narrow and float32 copies compiles for gfx950 to a loop whose 16 loads are not waited for
until the tile in front of them is evaluated; EVQL_SCAN_PREFETCH=0 gives the loop that waits
directly behind its loads; the shapes the rule excludes compile to the same bytes either way;
and the two halves of the narrow accessors, restated on the host, compose to the old values.

Where the loops lie: config 3's WHERE prunes, so its kernel carries the tile loop twice
(tile_loop_twice).  The compiler lays the loop WITH zone test out first, so the prefetching
loop is found by what it is -- the one loop whose cluster no scalar load of a bitmap word
precedes -- not by its position."""
import re

import numpy as np
import pytest

from eventql_amd import bench_plans as B
from eventql_amd.plan import Plan, col, count, max_, sum_

from test_flat_narrow_cpu import compile_one, disassembly, tile_load_clusters
from test_scan_hot_path_cpu import NARROW_F32

k, a, b, v = [col(x) for x in "kabv"]
WHERE3 = (a > 30000) & (b < 30000)


@pytest.fixture
def switch(monkeypatch):
    def set_(on):
        if on:
            monkeypatch.delenv("EVQL_SCAN_PREFETCH", raising=False)
        else:
            monkeypatch.setenv("EVQL_SCAN_PREFETCH", "0")
    return set_


def code(tmp_path, name, plan, columns):
    d = tmp_path / name
    d.mkdir()
    obj = compile_one(d, plan, columns)
    with open(obj, "rb") as f:
        return obj, f.read()


def is_vmcnt(i):
    return i.startswith("s_waitcnt") and "vmcnt" in i


def loops(ins):
    """(clusters with zone test, clusters without): a zone test reads its bitmap word with a
    scalar one-dword load a few instructions ahead of the tile's loads"""
    with_test, without = [], []
    for c in tile_load_clusters(ins):
        ahead = ins[max(0, c[0] - 60):c[0]]
        (with_test if any(re.match(r"s_load_dword s\d+,", x) for x in ahead) else without).append(c)
    return with_test, without


def first_wait_behind(ins, c):
    """(distance in instructions, N) of the first s_waitcnt vmcnt(N) behind the cluster"""
    for i in range(c[-1] + 1, len(ins)):
        if is_vmcnt(ins[i]):
            return i - c[-1], int(re.search(r"vmcnt\((\d+)\)", ins[i]).group(1))
    raise AssertionError("no wait behind the cluster")


def back_edge(ins, c, end):
    """the tile loop's back edge: the first backward branch behind the cluster that jumps more
    than 1000 dwords (the probe loops inside the body jump a few hundred at most)"""
    for i in range(c[-1] + 1, end):
        m = re.match(r"s_c?branch\w* (\d+)$", ins[i])
        if m and int(m.group(1)) >= 32768 and 65536 - int(m.group(1)) > 1000:
            return i
    raise AssertionError("no back edge")


@pytest.fixture
def config3_on_off(built, tmp_path, switch):
    switch(True)
    obj_on, on = code(tmp_path, "on", B.config3(), NARROW_F32)
    switch(False)
    obj_off, off = code(tmp_path, "off", B.config3(), NARROW_F32)
    return (disassembly(obj_on)["evql_scan_agg"], on), (disassembly(obj_off)["evql_scan_agg"], off)


def test_the_loads_are_waited_for_behind_the_tile_they_overlap(config3_on_off):
    (ins, _), _ = config3_on_off
    with_test, without = loops(ins)
    assert [len(c) for c in with_test] == [16] and [len(c) for c in without] == [16]
    c = without[0]
    assert not [ins[i] for i in range(c[0], c[-1] + 1) if is_vmcnt(ins[i])]
    later = [x[0] for x in tile_load_clusters(ins) if x[0] > c[0]]
    end = back_edge(ins, c, later[0] if later else len(ins))
    atomics = [i for i in range(c[-1], end) if ins[i].startswith("global_atomic_")]
    assert atomics  # the HBM spill path is in the body
    # cold: the block of a global atomic (the HBM table's probe and its updates)
    cold = lambda i: any(abs(i - x) <= 16 for x in atomics)
    waits = [i for i in range(c[-1] + 1, end) if is_vmcnt(ins[i]) and not cold(i)]
    adds = [i for i in range(c[-1], end) if ins[i].startswith("ds_add_")]
    print("cluster %d..%d, back edge %d, last ds_add %d, waits %s"
          % (c[0], c[-1], end, adds[-1], [(i, ins[i]) for i in waits]))
    assert adds and waits
    # every wait for the cluster sits behind the last LDS update of the tile body: the copy
    assert min(waits) > adds[-1], [(i, ins[i]) for i in waits]
    assert any(x.startswith("v_mov_b32") for x in ins[min(waits):min(waits) + 4])


def test_the_loop_with_zone_test_keeps_its_form(config3_on_off):
    (ins, _), (ins_off, _) = config3_on_off
    for text in (ins, ins_off):
        with_test, _ = loops(text)
        assert len(with_test) == 1
        dist, n = first_wait_behind(text, with_test[0])
        assert dist <= 12 and n <= 15, (dist, n)


def test_the_switch_gives_the_waiting_loop(config3_on_off):
    (_, on), (ins, off) = config3_on_off
    assert on != off
    _, without = loops(ins)
    assert len(without) == 1
    dist, n = first_wait_behind(ins, without[0])
    assert dist <= 12 and n <= 15, (dist, n)


EXCLUDED = {
    "config3 over plain pages": (B.config3, B.PLAIN_COLUMNS),
    "ungrouped": (lambda: Plan(B.SCHEMA, select=[count(1), sum_(v), sum_(b), max_(k)], where=WHERE3),
                  NARROW_F32),
    "nullable column": (B.config3, [dict(c, dlevel_max=1) if c["name"] == "a" else c for c in NARROW_F32]),
    "two columns at unroll 8": (B.config2, NARROW_F32),
    "v on plain pages": (B.config3, [dict(c, narrow_bits=0) if c["name"] == "v" else c for c in NARROW_F32]),
}


@pytest.mark.parametrize("shape", sorted(EXCLUDED))
def test_excluded_shapes_do_not_know_the_switch(built, tmp_path, switch, shape):
    plan, columns = EXCLUDED[shape]
    switch(True)
    _, on = code(tmp_path, "on", plan(), columns)
    switch(False)
    _, off = code(tmp_path, "off", plan(), columns)
    assert on == off


# ---- the decode halves, restated on the host -------------------------------------------------
def old_x2(bits, mem, r):
    """evql_narrow_x2 / evql_f32_x2 before the split: rows r, r + 1 of the little-endian copy"""
    if bits == "f32":
        f = mem.view(np.float32)[r:r + 2]
        return [int(np.float64(x).view(np.uint64)) for x in f]
    w = mem.view({8: np.uint8, 16: np.uint16, 32: np.uint32}[bits])
    return [int(w[r]), int(w[r + 1])]


def load(bits, mem, r):
    """evql_narrow_ld / evql_f32_ld: the words as loaded (one dword for 8 and 16 bits)"""
    if bits in ("f32", 32):
        return [int(x) for x in mem.view(np.uint32)[r:r + 2]]
    if bits == 16:
        return [int(mem.view(np.uint32)[r // 2])]
    return [int(mem.view(np.uint16)[r // 2])]


def decode(bits, w):
    """evql_narrow_dec / evql_f32_dec"""
    if bits == "f32":
        return [int(np.float64(np.uint32(x).view(np.float32)).view(np.uint64)) for x in w]
    if bits == 32:
        return [w[0], w[1]]
    if bits == 16:
        return [w[0] & 0xffff, w[0] >> 16]
    return [w[0] & 0xff, w[0] >> 8]


@pytest.mark.parametrize("bits", [8, 16, 32, "f32"])
def test_decode_of_load_is_the_old_accessor(bits):
    rng = np.random.default_rng(5)
    if bits == "f32":
        edge = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
                         0x3f800000, 0x00800000], np.uint32)  # 0, -0.0, inf, -inf, quiet NaNs, 1, min normal
        vals = np.concatenate([edge, rng.random(56, np.float32).view(np.uint32)])
        mem = vals.view(np.uint8).copy()
    else:
        top = (1 << bits) - 1
        vals = np.concatenate([np.array([0, top, top, 0, 1, top - 1, 0xffff & top, 0], np.uint64),
                               rng.integers(0, top, 56, dtype=np.uint64, endpoint=True)])
        mem = vals.astype({8: np.uint8, 16: np.uint16, 32: np.uint32}[bits]).view(np.uint8).copy()
    for r in range(0, 64, 2):
        assert decode(bits, load(bits, mem, r)) == old_x2(bits, mem, r), (bits, r)
    if bits == "f32":
        with np.errstate(invalid="ignore"):
            got = [decode(bits, load(bits, mem, r)) for r in range(0, 8, 2)]
        assert got[0] == [0, 0x8000000000000000]
        assert got[1] == [0x7ff0000000000000, 0xfff0000000000000]
        assert got[2] == [0x7ff8000000000000, 0xfff8000000000000]
