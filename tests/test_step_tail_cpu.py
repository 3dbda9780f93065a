"""The prologue and epilogue kernels of a step without a GPU: the
ahead-of-time kernels compile for gfx950 and k_table_init / k_table_tail keep no value in
scratch memory and spill no register."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
ROCM = os.environ.get("ROCM", "/opt/rocm")


def kernel_facts(code_object):
    """kernel name -> dict of the integer fields of its metadata note"""
    notes = subprocess.run([ROCM + "/lib/llvm/bin/llvm-readelf", "--notes", code_object],
                           capture_output=True, text=True, check=True).stdout
    facts = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\w+)", blk).group(1)
        facts[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}
    return facts


def test_step_kernels_compile_without_spills_or_scratch(tmp_path):
    out = str(tmp_path / "aot_kernels.hsaco")
    # the device half of the Makefile's aot_kernels.o rule
    subprocess.run([ROCM + "/bin/hipcc", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                    "-I" + ROCM + "/include", "-I" + os.path.join(ROOT, "include"),
                    "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", "-ffp-contract=off",
                    "--cuda-device-only", "--no-gpu-bundle-output", "-c",
                    os.path.join(CSRC, "aot_kernels.hip"), "-o", out], check=True)
    facts = kernel_facts(out)
    seen = []
    for name, f in sorted(facts.items()):
        if "k_table_tail" not in name and "k_table_init" not in name:
            continue
        seen.append(name)
        print("%s vgpr %d sgpr %d spill %d/%d scratch %d" % (
            name, f["vgpr_count"], f["sgpr_count"], f["vgpr_spill_count"], f["sgpr_spill_count"],
            f["private_segment_fixed_size"]))
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["private_segment_fixed_size"] == 0, (name, f)
    assert len(seen) == 2, seen
