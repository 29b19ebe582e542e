"""Register / private-memory budget of the depth-pyramid kernels (texturefusion_amd/csrc/tf_align_icp_pyramid.hip), checked at
build time in the manner of tests/test_kernel_resources_align_icp_gate.py.  k_depth_pyramid exchanges lanes and keeps
nothing: no private memory, no LDS; it builds at 13 VGPRs and is held to 16, the next multiple of 8.  k_pyramid_spread
(11 VGPRs) copies.  A pyramid level is evaluated by the rows kernels as they are, so this file holds no rows kernel: only
the figures the compiler reports, and the files' text for what they share, are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_depth_pyramid": (16, 0, 0), "k_pyramid_spread": (16, 0, 0)}


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
def test_pyramid_kernels_stay_within_their_budget():
    usage = _usage("tf_align_icp_pyramid.hip")
    assert len(usage) == len(BUDGET), sorted(usage)  # no rows kernel, no solve kernel: those are the other files'
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 1, "kernel %s not found" % frag
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
            assert v["Occupancy"] >= 8, v


def test_the_rows_kernels_are_used_not_restated():
    pyr = open(os.path.join(CSRC, "tf_align_icp_pyramid.hip")).read()
    icp = open(os.path.join(CSRC, "tf_align_icp.hip")).read()
    gate = open(os.path.join(CSRC, "tf_align_icp_gate.hip")).read()
    code = pyr.split("#include <hip/hip_runtime.h>")[1]
    # a level goes to k_icp_rows / k_gated_rows: the association and the sums stay where they are, in one text each ...
    for text in (icp, gate):
        for call in ("icp_assoc(", "al_row_sums("):
            assert call in text, call
    # ... and the new file has none of it: no association, no row sums, no tile tree, no solve
    for call in ("icp_assoc(", "al_row_sums(", "al_tile_sum(", "align_solve6", "al_point("):
        assert call not in code, call
    assert code.count("__global__") == 2
    assert '#include "tf_align_icp_pyramid.h"' in icp and "icp_pyramid_enqueue(" in icp and "align_level_image(" in icp
    assert "atomic" not in code and "__shared__" not in code  # no atomics of any kind, no LDS
    assert code.count("__shfl_xor(") == 3 and "__syncthreads" not in code  # one exchange text for the three levels
    assert "tf_align_icp_pyramid.hip" in open(os.path.join(CSRC, "Makefile")).read()
