"""The float32 copy of a float32-exact FLOAT64 column without a GPU: the benchmark shapes with
`v` read through evql_f32_x2 (compile_only's narrow_bits=32 on a FLOAT_IEEE754 column) compile
for gfx950 with no spilled VGPR, no scratch, no FLAT instruction and no more VGPRs than with `v`
on the file's pages; config 3's tile loads still go out back to back; and the numpy model of
the representability rule that the GPU tests choose their inputs with is pinned."""
import numpy as np
import pytest

import eventql_amd as E
from eventql_amd import bench_plans as B, capi as K, synth

import narrow_float_model as M
from test_flat_narrow_cpu import audit, compile_one, disassembly, tile_load_clusters

# k < 1000, a, b < 65536 in 16 bits, u < 1e7 in 32: what a table of benchmark size keeps
NARROW = [dict(c, narrow_bits=32 if c["name"] == "u" else 16)
          if c["storage_type"] == K.ENC_UINT64_PLAIN else c for c in B.PLAIN_COLUMNS]
NARROW_F32 = [dict(c, narrow_bits=32) if c["name"] == "v" else c for c in NARROW]
PLANS = {"config2": B.config2, "config3": B.config3, "config4": B.config4}


@pytest.fixture(scope="module")
def compiled(built, tmp_path_factory):
    """(config, form) -> code object path, form 'plain' = v on the file's pages, 'f32' = copy"""
    out = {}
    for name, plan in PLANS.items():
        for form, columns in (("plain", NARROW), ("f32", NARROW_F32)):
            d = tmp_path_factory.mktemp("%s_%s" % (name, form))
            out[name, form] = compile_one(d, plan(), columns)
    return out


@pytest.mark.parametrize("config", sorted(PLANS))
def test_compiles_clean_and_no_fatter_than_plain_v(compiled, config):
    plain = audit(compiled[config, "plain"])
    f32 = audit(compiled[config, "f32"])
    assert f32 and sorted(f32) == sorted(plain)
    for kernel, (vgprs, spill, scratch, flat) in sorted(f32.items()):
        print("%-8s %-20s vgpr %3d (v plain: %3d) spill %d scratch %d flat %d"
              % (config, kernel, vgprs, plain[kernel][0], spill, scratch, flat))
        assert (spill, scratch, flat) == (0, 0, 0), (config, kernel, f32[kernel])
    assert f32["evql_scan_agg"][0] <= plain["evql_scan_agg"][0], (config, f32, plain)
    if config == "config3":
        assert f32["evql_scan_agg"][0] <= 93  # (v plain, as measured when the copy came in)


def test_config3_tile_loads_issue_back_to_back(compiled):
    """4 columns x 4 unroll steps: 16 streaming loads per tile body with no wait on vmcnt
    between them -- 12 dword loads of the 16-bit copies, 4 dwordx2 loads of the float32 copy"""
    ins = disassembly(compiled["config3", "f32"])["evql_scan_agg"]
    clusters = tile_load_clusters(ins)
    assert clusters and max(len(c) for c in clusters) == 16, [len(c) for c in clusters]
    for c in clusters:
        waits = [ins[i] for i in range(c[0], c[-1] + 1)
                 if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]
        assert not waits, (len(c), waits)
        if len(c) == 16:
            wide = [ins[i] for i in c if ins[i].startswith("global_load_dwordx2 ")]
            assert len(wide) == 4, [ins[i] for i in c]
            assert not [ins[i] for i in c if ins[i].startswith("global_load_dwordx4")]


@pytest.mark.parametrize("config", sorted(PLANS))
def test_a_code_object_of_its_own(compiled, config):
    with open(compiled[config, "plain"], "rb") as f, open(compiled[config, "f32"], "rb") as g:
        assert f.read() != g.read()


def test_nullable_or_integer_column_does_not_take_the_float_shape(built, tmp_path):
    """narrow_bits=32 on a nullable FLOAT column leaves the plan as it is"""
    nullable = [dict(c, dlevel_max=1) if c["name"] == "v" else c for c in NARROW]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    nullable_f32 = [dict(c, narrow_bits=32) if c["name"] == "v" else c for c in nullable]
    with open(compile_one(a, B.config3(), nullable), "rb") as f, \
            open(compile_one(b, B.config3(), nullable_f32), "rb") as g:
        assert f.read() == g.read()


# ---- the representability rule ----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.QUALIFYING))
def test_model_accepts(name):
    assert M.column_qualifies(np.array([1.5, M.QUALIFYING[name], -2.0]))


@pytest.mark.parametrize("name", sorted(M.DISQUALIFYING))
def test_model_refuses(name):
    x = np.array([1.5, M.DISQUALIFYING[name], -2.0])
    assert list(M.exact_f32_mask(x)) == [True, False, True]


def test_model_is_decided_on_the_bits():
    # a quiet NaN whose payload fits float32's 22 bits survives; the same with the sign set too
    assert M.column_qualifies(np.array([M.f64(0x7ffc000000000000), M.f64(0xfff8000000000000)]))
    # float32 denormals, exact as doubles, are refused: the largest and the smallest
    assert not M.exact_f32_mask(np.array([2.0 ** -127, 2.0 ** -149, -(2.0 ** -130)])).any()
    # beyond the range in either direction
    assert not M.exact_f32_mask(np.array([2.0 ** 128, -(2.0 ** 128), 2.0 ** -150, 1e300])).any()


def test_the_synthetic_v_qualifies():
    v = synth.table_columns(400_000)["v"]
    assert v.dtype == np.float64
    assert M.column_qualifies(v)
    assert v.max() < 16384.0 and v.min() >= 0.0
