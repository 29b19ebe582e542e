"""Register / private-memory budget of the exposure-compensation kernels (texturefusion_amd/csrc/tf_align_exposure.hip),
checked at build time in the manner of tests/test_kernel_resources_align_icp_color.py.  k_ealign_rows is k_calign_rows and
k_ealign_proj_rows is k_cicp_rows, each with the compensated luma and a third row of sums: no private memory, no spills,
three rows of 32 f64 per wave of LDS (6144 B), at least four waves per SIMD.  Each VGPR ceiling is the first build's figure
rounded up to the allocation granule of 8: k_ealign_rows 120 -> 120, k_ealign_proj_rows 75 -> 80 (both variants),
k_ealign_begin 8 -> 8, k_ealign_cell 6 -> 8.  k_ealign_solve is one workgroup whose lane 0 holds the joined 6 x 6 system and
the eliminated pair in registers: what is checked is that none of its arrays went to private memory (occupancy is no figure
of a launch of one workgroup).  Only the figures the compiler reports, and the files' text for what they share, are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max LDS bytes per workgroup, min waves per SIMD); None: not checked
BUDGET = {"k_ealign_cell": (8, None, 4), "k_ealign_begin": (8, None, 4), "k_ealign_rowsE": (120, 6144, 4),
          "k_ealign_proj_rowsILb0": (80, 6144, 4), "k_ealign_proj_rowsILb1": (80, 6144, 4), "k_ealign_solve": (None, 6144, None)}


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
def test_exposure_kernels_stay_within_their_budget():
    usage = _usage("tf_align_exposure.hip")
    assert len(usage) == len(BUDGET) and all("k_ealign_" in k for k in usage), sorted(usage)  # the file's kernels and no others
    for frag, (max_vgpr, max_lds, min_waves) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 1, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["SGPRs_Spill"] == 0 and v["VGPRs_Spill"] == 0, "%s spills" % k
            if max_vgpr is not None:
                assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            if max_lds is not None:
                assert v["LDS_Size"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS_Size"])
            if min_waves is not None:
                assert v["Occupancy"] >= min_waves, "%s runs %d waves per SIMD" % (k, v["Occupancy"])


def _code(name):
    """the file's text without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_the_exposure_file_uses_the_shared_machinery():
    code = _code("tf_align_exposure.hip").split("#include <hip/hip_runtime.h>")[1]
    for inc in ('#include "tf_align_rows.h"', '#include "tf_align_icp_rows.h"', '#include "tf_align_icp_normal.h"',
                '#include "tf_align_exposure.h"'):
        assert inc in code
    # used, not restated: the SDF row, the association, the gate, the three rows' sums, the begin, the joined solve
    for call in ("al_sdf_row<true>(", "al_point(", "icp_assoc(", "fn_taps(", "frame_normal(", "fn_gate_bits(", "al_luma(",
                 "al_row_sums(", "al_exposure_row_sums(", "al_store_rows(", "al_begin(", "al_solve_color_exposure(", "align_walk("):
        assert call in code, call
    assert code.count("al_row_sums(") == 4 and code.count("al_exposure_row_sums(") == 2
    for none in ("al_tile_sum(", "al_tree_sum", "al_halve", "align_solve6", "align_update(", "al_decide(", "exposure_eliminate(",
                 "tri_sample", "atomic"):
        assert none not in code, none
    # the tree exists once and both tables go through it; the elimination is one header's, called from one place
    tree = _code("tf_align_tree.h")
    assert tree.count("double al_tree_sum(") == 1 and tree.count("al_tree_sum<") == 2 and tree.count("al_halve<16>") == 1
    assert "AlPairs al_exposure_pairs()" in tree
    rows = _code("tf_align_rows.h")
    assert '#include "tf_align_exposure_solve.h"' in rows and rows.count("exposure_eliminate(") == 1
    assert rows.count("void al_solve_color_exposure(") == 1 and rows.count("al_decide(c, a,") == 3  # pose, colour, exposure
    for part in ("al_fill_iter(", "al_count(", "al_keep_pose(", "al_fill_photo(", "al_fill_color_result("):
        assert part in rows.split("void al_solve_color_exposure(")[1], part
    solve = open(os.path.join(CSRC, "tf_align_exposure_solve.h")).read()
    assert "TF_AL_HD inline void exposure_eliminate(" in solve and "hip_runtime" not in solve  # host programs build it
    # the two aligners hand their calls over, the luma has one text
    for name in ("tf_align_color.hip", "tf_align_icp_color.hip"):
        text = _code(name)
        assert "exposure_on(v)" in text and "al_luma(" in text and "0.299f" not in text and "k_ealign_" not in text
    assert "tf_align_exposure.hip" in open(os.path.join(CSRC, "Makefile")).read()
