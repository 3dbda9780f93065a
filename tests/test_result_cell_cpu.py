"""Where a select cell lives in a group record and how it is read (DESIGN.md 3.7,
csrc/result_cell.h), without a GPU: the classifier and the read as a stand-alone program under
AddressSanitizer + UBSan, the places that may hold a copy of either, and the kernels that read
cells compiled for gfx950 without scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eventql_amd", "csrc")
ROCM = os.environ.get("ROCM", "/opt/rocm")


def test_classifier_and_read_under_sanitizers(tmp_path):
    """tools/result_cell_check.cc: (word, count_word, is_mean) of every EVQL_AGG_*, the
    first-row cells, and cell_bits on hand-made records -- no device, no HIP runtime"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "result_cell_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tools", "result_cell_check.cc"),
                           os.path.join(CSRC, "result_cell.cc"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr[-2000:]


def sources(*suffixes):
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))
            if f.endswith(suffixes)}


def test_one_copy_of_each():
    cc = sources(".cc")
    # the NULL-key test of the read: in cell_bits alone
    null_key = {f for f, text in sources(".cc", ".h", ".hip").items() if "[0] == 2" in text}
    assert null_key == {"result_cell.h"}
    # the record word of an aggregate's state
    assert {f for f, text in cc.items() if "1 + kp.state_word_base() + " in text} == {"result_cell.cc"}
    # bare_column / first_row_cell are defined once
    for name in ("bool bare_column(", "bool first_row_cell(", "bool aggregate_cell("):
        assert [f for f, text in cc.items() if name in text] == ["result_cell.cc"], name
    # one digit-pass loop, one first-row gather, one pinned_reserve
    assert {f for f, text in cc.items() if "launch_sort_hist(" in text} == {"radix_sort.cc"}
    assert {f for f, text in cc.items() if "launch_gather_rows(" in text} == {"results.cc"}
    assert cc["results.cc"].count("launch_gather_rows(") == 1
    assert [f for f, text in cc.items() if "Status pinned_reserve(" in text] == ["results.cc"]
    # the mirrors are gone
    for f, text in sources(".cc", ".h", ".hip").items():
        assert "OrderKeySpec" not in text and "order_key_args" not in text, f


CELL_KERNELS = ("k_emit_fixed", "k_emit_str_bytes", "k_mat_fixed", "k_partial_sizes",
                "k_partial_tuple_bytes", "k_partial_data_bytes", "k_order_keys", "k_ord_key_perm",
                "k_mrg_cell_fixed", "k_mrg_cell_str_sizes", "k_mrg_cell_str_bytes", "k_sort_key_stats",
                "k_sort_hist", "k_sort_digit_scan", "k_sort_scatter")


def test_kernels_compile_without_scratch(tmp_path):
    out = str(tmp_path / "aot_kernels.hsaco")
    # the device half of the Makefile's aot_kernels.o rule, with the resource-usage remarks
    p = subprocess.run([ROCM + "/bin/hipcc", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                        "-I" + ROCM + "/include", "-I" + os.path.join(ROOT, "include"),
                        "--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics", "-ffp-contract=off",
                        "--cuda-device-only", "--no-gpu-bundle-output",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(CSRC, "aot_kernels.hip"), "-o", out],
                       capture_output=True, text=True, check=True)
    facts = {}
    name = None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            facts[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            facts[name][m.group(1).strip()] = int(m.group(2))
    for kernel in CELL_KERNELS:
        hits = [n for n in facts if re.search(r"\d" + kernel + "E", n)]
        assert len(hits) == 1, (kernel, hits)
        f = facts[hits[0]]
        print("%-24s vgpr %3d sgpr %3d lds %d scratch %d occupancy %d" % (
            kernel, f["VGPRs"], f["TotalSGPRs"], f["LDS Size"], f["ScratchSize"], f["Occupancy"]))
        assert f["ScratchSize"] == 0 and f["VGPRs Spill"] == 0 and f["SGPRs Spill"] == 0, (kernel, f)
        # (the occupancies of profiles/result_cell_kernel_resources.md: none fell)
        assert f["Occupancy"] >= (5 if kernel == "k_sort_scatter" else 8), (kernel, f)
