"""Flat narrow copies and scalar page-table lookups without a GPU: the benchmark shapes and
their neighbours compile for gfx950 over the file's plain pages and over flat narrow arrays
(compile_only's `narrow_bits`) with no spilled VGPR, no scratch, no FLAT instruction and no
more VGPRs than the commit before this layout; and in config 3's evql_scan_agg a tile's
column loads go out back to back, with no wait for a page-table entry between them."""
import glob
import re
import subprocess

import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K
from eventql_amd.plan import Plan, col, count, lit, max_, min_, sum_

LLVM = "/opt/rocm/lib/llvm/bin"

SCHEMA = dict(B.SCHEMA, t=K.T_TIMESTAMP64)
PLAIN = B.PLAIN_COLUMNS + [dict(name="t", logical_type=K.COL_DATETIME,
                                storage_type=K.ENC_UINT64_LEB128)]
# what a table of benchmark size keeps: k < 1000, a, b < 65536 in 16 bits, u < 1e7 in 32
FLAT = [dict(c, narrow_bits=32 if c["name"] == "u" else 16)
        if c["storage_type"] == K.ENC_UINT64_PLAIN else c for c in PLAIN]
STR_PLAIN = B.STRING_KEY_COLUMNS
STR_FLAT = [dict(c, narrow_bits=16) if c["name"] == "a" else c for c in STR_PLAIN]
k, a, b, v, t = [col(x) for x in "kabvt"]
T0 = 1438055327000000


def _pruning():
    w = (t >= lit(T0, K.T_TIMESTAMP64)) & (t < lit(T0 + 10**9, K.T_TIMESTAMP64)) & (a > 30000)
    return Plan(SCHEMA, select=[k, sum_(v), count(1), sum_(b)], group_by=[k], where=w,
                groups_hint=1000)


PLANS = {
    "config2": B.config2,
    "config3": B.config3,
    "config4": B.config4,
    "ungrouped": lambda: Plan(SCHEMA, select=[count(1), sum_(a), min_(b), max_(b)],
                              where=(a > 30000) & (b < 30000)),
    "bare": lambda: Plan(SCHEMA, scan_select=[k, b + 1, v * 2.0], where=a > 30000),
    "pruning": _pruning,
}
SHAPES = {}
for _name, _plan in PLANS.items():
    SHAPES[_name + "/plain"] = (_plan, PLAIN)
    SHAPES[_name + "/flat16"] = (_plan, FLAT)
SHAPES["config4s/plain"] = (B.config4s, STR_PLAIN)
SHAPES["config4s/flat16"] = (B.config4s, STR_FLAT)

# VGPRs per kernel of the same shapes on the commit before this one (narrow copies as 16- /
# 32-bit bit-packed pages, page-table entries read with vector loads); DESIGN.md 6 has the
# table next to this commit's figures
PARENT_VGPRS = {
    "bare/flat16": {"evql_scan_count": 40, "evql_scan_emit": 104},
    "bare/plain": {"evql_scan_count": 38, "evql_scan_emit": 104},
    "config2/flat16": {"evql_scan_agg": 113},
    "config2/plain": {"evql_scan_agg": 122},
    "config3/flat16": {"evql_scan_agg": 99},
    "config3/plain": {"evql_scan_agg": 106},
    "config4/flat16": {"evql_scan_agg": 102, "evql_part_count": 44, "evql_part_scatter": 80, "evql_part_refine": 53, "evql_part_aggregate": 67},
    "config4/plain": {"evql_scan_agg": 92, "evql_part_count": 31, "evql_part_scatter": 78, "evql_part_refine": 53, "evql_part_aggregate": 67},
    "config4s/flat16": {"evql_scan_agg": 106, "evql_part_count": 38, "evql_part_scatter": 81, "evql_part_refine": 51, "evql_part_aggregate": 95},
    "config4s/plain": {"evql_scan_agg": 101, "evql_part_count": 32, "evql_part_scatter": 81, "evql_part_refine": 51, "evql_part_aggregate": 95},
    "pruning/flat16": {"evql_scan_agg": 113},
    "pruning/plain": {"evql_scan_agg": 120},
    "ungrouped/flat16": {"evql_scan_agg": 186},
    "ungrouped/plain": {"evql_scan_agg": 159},
}


def compile_one(tmp_path, plan, columns):
    assert E.compile_only(plan, columns, cache_dir=str(tmp_path)) > 4000
    objs = glob.glob(str(tmp_path) + "/*.hsaco")
    assert len(objs) == 1, objs
    return objs[0]


def disassembly(code_object):
    """kernel name -> its instructions, one text line each"""
    asm = subprocess.run([LLVM + "/llvm-objdump", "-d", code_object], capture_output=True,
                         text=True, check=True).stdout
    kernels, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return kernels


def audit(code_object):
    """kernel name -> (VGPRs, spilled VGPRs, scratch bytes, FLAT instructions)"""
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", code_object], capture_output=True,
                           text=True, check=True).stdout
    dis = disassembly(code_object)
    facts = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\w+)", blk).group(1)
        g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))  # noqa: E731
        flat = sum(1 for i in dis.get(name, []) if i.startswith("flat_"))
        facts[name] = (g("vgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"), flat)
    return facts


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_compiles_clean_and_no_fatter(built, tmp_path, shape):
    plan, columns = SHAPES[shape]
    facts = audit(compile_one(tmp_path, plan(), columns))
    assert facts
    for kernel, (vgprs, spill, scratch, flat) in sorted(facts.items()):
        print("%-16s %-20s vgpr %3d spill %d scratch %d flat %d" % (shape, kernel, vgprs, spill,
                                                                   scratch, flat))
        assert (spill, scratch, flat) == (0, 0, 0), (shape, kernel, facts[kernel])
        assert vgprs <= PARENT_VGPRS[shape][kernel], (shape, kernel, vgprs)


def tile_load_clusters(instructions):
    """Runs of streaming column loads: every column accessor of a tile loop loads
    non-temporally (`nt`), nothing else in the kernels does.  Loads fewer than 24
    instructions apart belong to one tile body (its 16 loads interleave with a few address
    computations each; the next tile body lies hundreds of instructions on)."""
    at = [i for i, ins in enumerate(instructions)
          if ins.startswith("global_load_") and ins.endswith(" nt")]
    clusters = []
    for i in at:
        if clusters and i - clusters[-1][-1] < 24:
            clusters[-1].append(i)
        else:
            clusters.append([i])
    return clusters


@pytest.mark.parametrize("form", ["plain", "flat16"])
def test_config3_tile_loads_issue_back_to_back(built, tmp_path, form):
    """4 columns x 4 unroll steps: the 16 column loads of a tile body follow each other with
    no s_waitcnt on vmcnt between the first and the last -- the page-table entries arrive
    through scalar loads (lgkmcnt), the flat arrays need none"""
    plan, columns = SHAPES["config3/" + form]
    ins = disassembly(compile_one(tmp_path, plan(), columns))["evql_scan_agg"]
    clusters = tile_load_clusters(ins)
    assert clusters and max(len(c) for c in clusters) == 16, [len(c) for c in clusters]
    for c in clusters:
        waits = [ins[i] for i in range(c[0], c[-1] + 1)
                 if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]
        assert not waits, (form, len(c), waits)
    # the page table is not read with vector loads any more: plain pages take one scalar
    # load per column and tile, flat arrays only for `v`
    body = ins[clusters[0][0] - 40:clusters[0][-1] + 1]
    scalar = [i for i in body if i.startswith("s_load_dwordx2")]
    assert len(scalar) == (4 if form == "plain" else 1), scalar


def test_flat_accessor_in_the_generated_text(built, tmp_path):
    """narrow_bits selects evql_narrow_x2 -- a distinct code object from both the plain pages
    and a bit-packed file column of the same width"""
    packed = [dict(c, storage_type=K.ENC_UINT32_BITPACKED, bits=16) if c["name"] in "kab" else c
              for c in B.PLAIN_COLUMNS]
    sizes = set()
    for columns in (PLAIN, FLAT, packed):
        d = tmp_path / ("c%d" % len(sizes))
        d.mkdir()
        with open(compile_one(d, B.config3(), columns), "rb") as f:
            sizes.add(f.read())
    assert len(sizes) == 3
