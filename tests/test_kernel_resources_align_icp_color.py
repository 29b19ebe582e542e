"""Register / private-memory budget of the colour-ICP kernels (texturefusion_amd/csrc/tf_align_icp_color.hip), checked at
build time in the manner of tests/test_kernel_resources_align_icp_gate.py.  k_cicp_rows is k_icp_rows / k_gated_rows with
three more scattered loads, the frame's colour word and a second row of sums: no private memory, two rows of 32 f64 per wave
of LDS (4096 B), at least four waves per SIMD.  Each VGPR ceiling is the first build's figure rounded up to the allocation
granule of 8: k_cicp_rows 69 -> 72 (both variants), k_cicp_lum 62 -> 64, k_cicp_grad 14 -> 16, k_cicp_begin 6 -> 8.  The map
kernels hold no LDS.  k_cicp_solve is k_calign_solve's function (al_solve_color, tf_align_rows.h): one workgroup whose lane 0
holds the joined 6 x 6 system in registers (176 VGPRs as built, which bounds nothing: what is checked is that none of its
arrays went to private memory; occupancy is no figure of a launch of one workgroup).  Only the figures the compiler reports,
and the files' text for what they share, are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup, min waves per SIMD)
BUDGET = {"k_cicp_begin": (8, 0, 0, 4), "k_cicp_lum": (64, 0, 0, 4), "k_cicp_grad": (16, 0, 0, 4),
          "k_cicp_rowsILb0": (72, 0, 4096, 4), "k_cicp_rowsILb1": (72, 0, 4096, 4), "k_cicp_solve": (176, 0, 4096, 0)}


def _usage(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"remark:\s+(VGPRs|SGPRs Spill|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).replace(" ", "_").split("_[")[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_colour_icp_kernels_stay_within_their_budget():
    usage = _usage("tf_align_icp_color.hip")
    assert len(usage) == len(BUDGET) and all("k_cicp_" in k for k in usage), sorted(usage)
    for frag, (max_vgpr, max_scratch, max_lds, min_waves) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 1, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["SGPRs_Spill"] == 0 and v["VGPRs_Spill"] == 0, "%s spills" % k
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS_Size"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS_Size"])
            assert v["Occupancy"] >= min_waves, "%s runs %d waves per SIMD" % (k, v["Occupancy"])


def test_the_colour_icp_shares_the_association_the_sums_and_the_frame_normal():
    col = open(os.path.join(CSRC, "tf_align_icp_color.hip")).read()
    code = col.split("#include <hip/hip_runtime.h>")[1]
    for inc in ('#include "tf_align_icp_rows.h"', '#include "tf_align_icp_normal.h"', '#include "tf_align_rows.h"'):
        assert inc in code
    # used, not restated: the point, bits 1 to 3, both rows' sums, the joined solve, the frame normal and the gate's bits
    for call in ("al_point(", "icp_assoc(", "al_row_sums(", "al_store_rows(", "al_solve_color(", "fn_taps(", "frame_normal(",
                 "fn_gate_bits("):
        assert call in code, call
    assert code.count("al_row_sums(") == 2
    assert "al_tile_sum(" not in code and "align_solve6" not in code and "align_update(" not in code
    assert "atomic" not in code  # no atomics of any kind in the code
    assert "al_solve_color(" in open(os.path.join(CSRC, "tf_align_color.hip")).read()
    # the frame normal's text exists once in the tree
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp", ".hpp")):
            text = open(os.path.join(CSRC, name)).read()
            if "FrameNormal frame_normal(" in text or "struct FnTaps" in text or "FnTaps fn_taps(" in text or "bool fn_in_range(" in text:
                found.append(name)
    assert found == ["tf_align_icp_normal.h"], found
    for name in ("tf_align_icp_gate.hip", "tf_align_icp_color.hip"):
        assert '#include "tf_align_icp_normal.h"' in open(os.path.join(CSRC, name)).read()
    # the kernels of the plain and the gated file are still counted in their own files; the other aligners do not know this one
    for name in ("tf_align_icp.hip", "tf_align_icp_gate.hip"):
        assert "k_cicp_" not in open(os.path.join(CSRC, name)).read()
    for name in ("tf_align.hip", "tf_align_color.hip", "tf_align_group.hip"):
        assert "icp" not in open(os.path.join(CSRC, name)).read().lower()
    assert "tf_align_icp_color.hip" in open(os.path.join(CSRC, "Makefile")).read()
