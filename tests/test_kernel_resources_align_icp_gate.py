"""Register / private-memory budget of the gated projective-ICP kernels (texturefusion_amd/csrc/tf_align_icp_gate.hip),
checked at build time in the manner of tests/test_kernel_resources_align_icp.py.  k_gated_rows is k_icp_rows with four more
depth loads and the frame normal, and it is held to the project's own budget for k_icp_rows: at most 80 VGPRs, no private
memory, at most 2048 B of LDS, six waves per SIMD (it builds at 64 VGPRs and eight waves).  k_frame_normals has no sums: no
LDS at all.  Only the figures the compiler reports, and the files' text for what they share, are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_gated_rows": (80, 0, 2048), "k_frame_normals": (40, 0, 0)}


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
def test_gated_kernels_stay_within_their_budget():
    usage = _usage("tf_align_icp_gate.hip")
    assert len(usage) == len(BUDGET), sorted(usage)
    assert not [k for k in usage if "k_icp_" in k]  # tests/test_kernel_resources_align_icp.py counts those in its own file
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 1, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
    rows = [v for k, v in usage.items() if "k_gated_rows" in k][0]
    assert rows["Occupancy"] >= 6, rows


def test_the_two_rows_kernels_share_the_association_and_the_sums():
    gate = open(os.path.join(CSRC, "tf_align_icp_gate.hip")).read()
    icp = open(os.path.join(CSRC, "tf_align_icp.hip")).read()
    shared = open(os.path.join(CSRC, "tf_align_icp_rows.h")).read()
    for text in (gate, icp):
        assert '#include "tf_align_icp_rows.h"' in text
        # used, not restated: the point, bits 1 to 3, the row's sums
        for call in ("al_point(", "icp_assoc(", "al_row_sums(", "al_store_rows("):
            assert call in text, call
    assert "IcpAssoc icp_assoc(" in shared and "struct IcpRowsArgs" in shared and "struct IcpRowsArgs" not in icp
    assert "al_tile_sum(" not in gate and "align_solve6" not in gate
    assert "atomic" not in gate.split("#include <hip/hip_runtime.h>")[1]  # no atomics of any kind in the code
    assert "tf_align_icp_gate.hip" in open(os.path.join(CSRC, "Makefile")).read()
