"""Register / private-memory budget of the view-selection kernels (texturefusion_amd/csrc/tf_mrf.hip), checked at build
time like tests/test_kernel_resources.py: the line solver walks its line with one dependent round trip per node, and a
spilled loop variable would add another to every node without failing any parity test.  None of the kernels holds private
memory; the VGPR figures are what the kernels were built with."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane)
BUDGET = {"k_mrf_validate": (18, 0), "k_mrf_init": (12, 0), "k_mrf_linesE": (20, 0), "k_mrf_energy": (24, 0),
          "k_mrf_round_end": (6, 0),
          # the walk through the +a pointers (TF_MRF_WALK=pointers) and the walk over the line arrays (the default), per axis
          "k_mrf_phaseILi0E": (43, 0), "k_mrf_phaseILi1E": (43, 0), "k_mrf_phaseILi2E": (43, 0),
          "k_mrf_phase_linesILi0E": (50, 0), "k_mrf_phase_linesILi1E": (50, 0), "k_mrf_phase_linesILi2E": (50, 0)}


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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_view_selection_kernels_stay_within_their_budget():
    usage = _usage("tf_mrf.hip")
    kernels = [k for k in usage if "k_mrf_" in k]
    for k in kernels:  # every kernel of the file is budgeted
        assert any(frag in k for frag in BUDGET), "%s has no budget" % k
    for frag, (max_vgpr, max_scratch) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= 24576, "%s holds %d B of LDS" % (k, v["LDS"])
