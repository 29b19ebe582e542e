"""Register / private-memory budget of the projective-ICP kernels (texturefusion_amd/csrc/tf_align_icp.hip), checked at build
time in the manner of tests/test_kernel_resources_align_group.py.  k_icp_rows has no chunk cache and no eight-corner
samples: six scattered loads and the wave tree, so it has to stay inside k_align_rows' budget with room to spare -- at most
80 VGPRs, no private memory, six waves per SIMD (it builds at 63 VGPRs and eight waves).  k_icp_solve is k_align_solve's
function (al_solve_pose, tf_align_rows.h): one workgroup whose lane 0 holds the 6 x 6 system in registers; what is checked is that nothing of it went to private
memory.  Only the figures the compiler reports, and the file's includes, are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_icp_begin": (8, 0, 0), "k_icp_rows": (80, 0, 2048), "k_icp_solve": (256, 0, 5376)}


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
def test_align_icp_kernels_stay_within_their_budget():
    usage = _usage("tf_align_icp.hip")
    kernels = [k for k in usage if "k_icp_" in k]
    assert len(kernels) == len(BUDGET), kernels
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
    rows = [v for k, v in usage.items() if "k_icp_rows" in k][0]
    assert rows["Occupancy"] >= 6, rows


def test_the_icp_file_shares_the_tree_and_the_solve():
    text = open(os.path.join(CSRC, "tf_align_icp.hip")).read()
    assert '#include "tf_align_rows.h"' in text
    rows = open(os.path.join(CSRC, "tf_align_rows.h")).read()
    for inc in ('#include "tf_align_tree.h"', '#include "tf_align_solve.h"'):
        assert inc in rows
    # used, not restated: the row's sums, and the whole solve launch k_align_solve runs
    for call in ("al_point(", "al_row_sums(", "al_store_rows(", "al_solve_pose("):
        assert call in text, call
    assert "al_solve_pose(" in open(os.path.join(CSRC, "tf_align.hip")).read()
    assert "al_halve" not in text and "align_solve6" not in text and "al_tile_sum(" not in text and "align_update(" not in text
    assert "atomic" not in text.split("#include <hip/hip_runtime.h>")[1]  # no atomics of any kind in the code
    for name in ("tf_align.hip", "tf_align_color.hip", "tf_align_group.hip"):  # the other aligners do not know this one
        assert "icp" not in open(os.path.join(CSRC, name)).read().lower()
