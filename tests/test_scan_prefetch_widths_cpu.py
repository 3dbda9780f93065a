"""Which column width mixes compile to the prefetching tile loop, without a GPU:
every plan of scan_width_mixes.py is compiled for gfx950 over the copies a resident table keeps
(compile_only's per-column `narrow_bits`), once with the prefetch allowed and once with
EVQL_SCAN_PREFETCH=0.

  PREFETCH     the text carries the rotating loop, the code object reports no scratch and no
               spilled VGPR, the loop without zone test issues one load per unroll step and
               column -- whatever the width: a 32-bit pair is one 8-byte load, an 8-bit pair
               one 2-byte load -- and the switch gives other bytes
  FALLS_BACK   the text carries the loop and the code object does report scratch: the runtime
               drops the prefetch (compile_plan_kernels)
  PLAIN_LOOP   no rotating loop in the text, and the switch changes nothing

Widening the mixes ends at the planner's unroll budget, not at the registers: five two-word
columns with three update words compile to 128 VGPRs without scratch, and a sixth column (or a
fourth update word next to five columns) takes unroll to 2, which the rule does not admit."""
import re

import pytest

import eventql_amd as E
from eventql_amd.plan import Plan

import scan_width_mixes as M
from test_flat_narrow_cpu import audit, compile_one, disassembly
from test_scan_prefetch_cpu import loops


def both(tmp_path, monkeypatch, mix, mode):
    """(plan, per switch setting: (text, code object path, its bytes))"""
    out = {}
    for tag in ("on", "off"):
        if tag == "on":
            monkeypatch.delenv("EVQL_SCAN_PREFETCH", raising=False)
        else:
            monkeypatch.setenv("EVQL_SCAN_PREFETCH", "0")
        plan = Plan(M.SCHEMA, **mix.plan_kw(mode == "exact"))
        d = tmp_path / ("%s-%s-%s" % (mix, mode, tag))
        d.mkdir()
        obj = compile_one(d, plan, M.COPY_COLUMNS)
        with open(obj, "rb") as f:
            out[tag] = (E.plan_kernel_text(plan, M.COPY_COLUMNS), obj, f.read())
    return plan, out


def define(text, name):
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def check_text(mix, plan, text):
    for i, name in enumerate(plan.scan_columns):
        assert M.accessor(name, i) in text, (mix, name, i)
    assert define(text, "EVQL_LCACHE") == mix.lcache
    assert define(text, "EVQL_TILE_ROWS") == (M.TILE if define(text, "EVQL_UNROLL") == 4 else M.TILE // 2)


def cases(mixes):
    return [pytest.param(m, mode, id="%s-%s" % (m, mode)) for m in mixes for mode in m.modes()]


@pytest.mark.parametrize("mix,mode", cases(M.PREFETCH))
def test_admitted_mixes_take_the_prefetching_loop_without_scratch(built, tmp_path, monkeypatch, mix, mode):
    plan, out = both(tmp_path, monkeypatch, mix, mode)
    ncols = len(plan.scan_columns)
    assert ncols >= 3
    text, obj, on = out["on"]
    off_text, off_obj, off = out["off"]
    assert M.MARKER in text and M.MARKER not in off_text
    assert define(text, "EVQL_UNROLL") == 4 and define(off_text, "EVQL_UNROLL") == 4
    check_text(mix, plan, text)
    check_text(mix, plan, off_text)
    for o in (obj, off_obj):
        vgprs, spill, scratch, flat = audit(o)["evql_scan_agg"]
        print("%-16s vgpr %3d spill %d scratch %d" % (mix, vgprs, spill, scratch))
        assert (spill, scratch, flat) == (0, 0, 0), (mix, vgprs, spill, scratch, flat)
    _, without = loops(disassembly(obj)["evql_scan_agg"])
    assert [len(c) for c in without] == [4 * ncols], (mix, [len(c) for c in without])
    assert on != off


def test_mixes_that_fall_back_do_report_scratch(built, tmp_path, monkeypatch):
    """(one test over the whole list: the list is empty as long as no admitted mix spills)"""
    for mix in M.FALLS_BACK:
        for mode in mix.modes():
            plan, out = both(tmp_path, monkeypatch, mix, mode)
            text, obj, _ = out["on"]
            assert M.MARKER in text
            check_text(mix, plan, text)
            _, spill, scratch, _ = audit(obj)["evql_scan_agg"]
            assert scratch > 0, (mix, spill, scratch)
            # ... and what the runtime compiles instead does not
            assert M.MARKER not in out["off"][0]
            _, spill, scratch, _ = audit(out["off"][1])["evql_scan_agg"]
            assert (spill, scratch) == (0, 0), (mix, spill, scratch)


@pytest.mark.parametrize("mix,mode", cases(M.PLAIN_LOOP))
def test_mixes_outside_the_rule_keep_the_plain_loop(built, tmp_path, monkeypatch, mix, mode):
    plan, out = both(tmp_path, monkeypatch, mix, mode)
    text, obj, on = out["on"]
    assert M.MARKER not in text
    check_text(mix, plan, text)
    assert text == out["off"][0] and on == out["off"][2]
    _, spill, scratch, _ = audit(obj)["evql_scan_agg"]
    assert (spill, scratch) == (0, 0), (mix, spill, scratch)
    flat_copies = all(M.WIDTHS[n] for n in plan.scan_columns)
    # the unroll budget, or a column without a flat copy: nothing else keeps these plans out
    assert (define(text, "EVQL_UNROLL") == 2) == flat_copies, mix


def test_the_lists_name_every_mix_once():
    names = [m.name for m in M.ALL]
    assert len(set(names)) == len(names)
    # both single-width mixes run with fast sums as well
    assert [m.name for m in M.ALL if m.fast] == ["k8-a8-b8-v", "k32-a32-b32-v"]
    widths = {M.WIDTHS[n] for m in M.PREFETCH for n in Plan(M.SCHEMA, **m.plan_kw()).scan_columns}
    assert widths == {8, 16, 32, "f32"}
