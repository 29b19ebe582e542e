"""Register / private-memory budget of the group alignment kernels (texturefusion_amd/csrc/tf_align_group.hip), checked at
build time in the manner of tests/test_kernel_resources_align.py.  k_galign_rows is k_align_rows' row (tf_align_rows.h) plus the frame's
table lookup and the three adds of the lever: the same budget, no private memory and at most 80 VGPRs, six waves per SIMD
(it builds at 76).  k_galign_solve is one workgroup of 256 threads per body whose lane 0 holds the 6 x 6 system in
registers; what is checked is that nothing of it went to private memory.  Its LDS is the 8 x 32 f64 table the eight
groups' sums meet in, the 32 f64 of the body's sums, and the small arrays of lane 0 the compiler moves there (5376 B as
built).  Only the figures the compiler reports are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_galign_begin": (8, 0, 0), "k_galign_rows": (80, 0, 2048), "k_galign_solve": (256, 0, 5376)}


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
def test_align_group_kernels_stay_within_their_budget():
    usage = _usage("tf_align_group.hip")
    kernels = [k for k in usage if "k_galign_" in k]
    assert len(kernels) == len(BUDGET), kernels
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
    rows = [v for k, v in usage.items() if "k_galign_rows" in k][0]
    assert rows["Occupancy"] >= 6, rows


def test_the_group_file_shares_the_sampler_the_tree_and_the_solve():
    text = open(os.path.join(CSRC, "tf_align_group.hip")).read()
    for inc in ('#include "tf_align_rows.h"', '#include "tf_align_group_solve.h"'):
        assert inc in text
    assert "bool tri_sample(" not in text and "tri_sample<" not in text and "al_sdf_row<false>(" in text
    # the row's sums, the solve launch's additions and the stop rules are called, not restated
    for call in ("al_row_sums(", "al_store_rows(", "al_add_rows(", "al_decide(", "align_update_about("):
        assert call in text, call
    assert "al_tile_sum(" not in text and "align_solve6(" not in text
    assert "atomic" not in text.split("#include <hip/hip_runtime.h>")[1]  # no atomics of any kind in the code
