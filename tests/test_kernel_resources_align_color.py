"""Register / private-memory budget of the colour-aided alignment kernels (texturefusion_amd/csrc/tf_align_color.hip),
checked at build time like tests/test_kernel_resources_align.py.  k_calign_rows carries seven samples of SDF and intensity
(sixteen loads each) and two tiles' worth of sums: it is bound by chains of dependent loads and needs its waves, so the
budget is no private memory and at least four waves per SIMD (at most 128 VGPRs); the compiler reports 120 (116 before the row moved
into tf_align_rows.h: the same granule of 8).  Its LDS is two rows of 32 f64 per wave.  k_calign_solve is one workgroup of 256 threads whose lane 0 holds the
joined 6 x 6 system in registers (176 VGPRs as built, which bounds nothing: what is checked is that none of lane 0's arrays
went to private memory); its LDS is the 8 x 64 f64 table the eight groups' sums meet in."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_calign_begin": (8, 0, 0), "k_calign_rows": (120, 0, 4096), "k_calign_solve": (256, 0, 4096)}


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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_align_color_kernels_stay_within_their_budget():
    usage = _usage("tf_align_color.hip")
    kernels = [k for k in usage if "k_calign_" in k]
    assert len(kernels) == len(BUDGET), kernels
    assert not [k for k in usage if "k_align_" in k]  # tf_align.hip's three kernels stay the only ones of that name
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
    rows = [v for k, v in usage.items() if "k_calign_rows" in k][0]
    assert rows["Occupancy"] >= 4, rows


def test_the_sampler_and_the_tree_are_shared_not_copied():
    geo = open(os.path.join(CSRC, "tf_align.hip")).read()
    col = open(os.path.join(CSRC, "tf_align_color.hip")).read()
    rows = open(os.path.join(CSRC, "tf_align_rows.h")).read()
    assert '#include "tf_ray_devfn.h"' in rows and '#include "tf_align_tree.h"' in rows
    for text in (geo, col, rows):
        assert "bool tri_sample" not in text and "void al_halve(" not in text and "al_pairs()" not in text
    for text in (geo, col):
        assert '#include "tf_align_rows.h"' in text
        assert "al_row_sums(" in text and "al_tile_sum(" not in text  # through the one function that forms a row's sums
    code = col.split("#include <hip/hip_runtime.h>")[1]
    assert code.count("al_sdf_row<true>(") == 1 and "tri_sample_lum" not in code  # the SDF row's text, not a second copy
    assert "atomic" not in code  # no atomics of any kind in the code
