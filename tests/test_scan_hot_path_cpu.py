"""The instruction work of evql_scan_agg's tile body without a GPU: the
benchmark shapes compile for gfx950 with the load geometry the other ISA tests pin, and the
vector instructions of the first tile body, the VGPRs and the exposed LDS round trips of the
probe stay at or below what the 32-bit window test, the branching one-entry accumulator cache
and the probe-ahead of a step's two rows reached."""
import pytest

from eventql_amd import bench_plans as B, capi as K

from test_flat_narrow_cpu import audit, compile_one, disassembly, tile_load_clusters

NARROW = [dict(c, narrow_bits=32 if c["name"] == "u" else 16)
          if c["storage_type"] == K.ENC_UINT64_PLAIN else c for c in B.PLAIN_COLUMNS]
NARROW_F32 = [dict(c, narrow_bits=32) if c["name"] == "v" else c for c in NARROW]

# shape -> (plan, columns, VALU bound of the first tile body, VGPR bound, VGPRs before)
# The commit before this one, measured with first_tile_body below and the same toolchain:
#   config3/f32    1103 VALU, 93 VGPRs     config3/plain  1164 VALU, 106 VGPRs
#   config2/narrow 2078 VALU, 99 VGPRs  (one cluster: the body runs to the end of the kernel)
SHAPES = {
    "config3/f32": (B.config3, NARROW_F32, 1064, 89, 93),
    "config3/plain": (B.config3, B.PLAIN_COLUMNS, 1114, 102, 106),
    "config2/narrow": (B.config2, NARROW, 2042, 91, 99),
}
PARENT_VALU = {"config3/f32": 1103, "config3/plain": 1164}


def first_tile_body(ins):
    """from the first streaming load of the kernel to the first load of the second tile body
    (or to the end, where the kernel has one)"""
    clusters = tile_load_clusters(ins)
    assert clusters
    return ins[clusters[0][0]:clusters[1][0]] if len(clusters) > 1 else ins[clusters[0][0]:]


@pytest.fixture(scope="module")
def compiled(built, tmp_path_factory):
    out = {}
    for shape, (plan, columns, _, _, _) in SHAPES.items():
        obj = compile_one(tmp_path_factory.mktemp(shape.replace("/", "_")), plan(), columns)
        out[shape] = (audit(obj)["evql_scan_agg"], disassembly(obj)["evql_scan_agg"])
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tile_body_work(compiled, shape):
    _, _, valu_bound, vgpr_bound, vgprs_before = SHAPES[shape]
    (vgprs, spill, scratch, flat), ins = compiled[shape]
    body = first_tile_body(ins)
    valu = sum(1 for i in body if i.startswith("v_"))
    print("%-15s VALU %4d (bound %d)  VGPRs %3d (bound %d, before %d)"
          % (shape, valu, valu_bound, vgprs, vgpr_bound, vgprs_before))
    assert (spill, scratch, flat) == (0, 0, 0)
    assert vgpr_bound <= vgprs_before and vgprs <= vgpr_bound
    assert valu <= valu_bound
    if shape in PARENT_VALU:
        assert valu_bound < PARENT_VALU[shape]


@pytest.mark.parametrize("shape", ["config3/f32", "config3/plain"])
def test_config3_load_geometry_stays(compiled, shape):
    _, ins = compiled[shape]
    clusters = tile_load_clusters(ins)
    assert [len(c) for c in clusters] == [16, 16]
    for c in clusters:
        assert not [ins[i] for i in range(c[0], c[-1] + 1)
                    if ins[i].startswith("s_waitcnt") and "vmcnt" in ins[i]]


@pytest.mark.parametrize("shape", ["config3/f32", "config3/plain"])
def test_config3_probe_round_trips(compiled, shape):
    """identity-slot reads that are waited for at once: one per row (8) before, at most one per
    step of two rows now"""
    body = first_tile_body(compiled[shape][1])
    exposed = sum(1 for x, y in zip(body, body[1:])
                  if x.startswith("ds_read_b64") and y.startswith("s_waitcnt lgkmcnt(0)"))
    assert exposed <= 4, exposed
