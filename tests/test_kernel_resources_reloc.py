"""Register / private-memory budget of the relocalisation kernels (texturefusion_amd/csrc/tf_reloc.hip), checked at build time
in the manner of tests/test_kernel_resources_align_icp.py.  The three kernels are streaming integer reductions: the budgets
are the VGPR figures the compiler reports (22, 9 and 30) rounded up to the allocation granule of 8, no private memory and no
LDS.  The file's text is read for what the descriptor's exactness rests on: no atomics, and nothing summed in floating
point."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_reloc_describe": (24, 0, 0), "k_reloc_total": (16, 0, 0), "k_reloc_score": (32, 0, 0)}


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
def test_reloc_kernels_stay_within_their_budget():
    usage = _usage("tf_reloc.hip")
    kernels = [k for k in usage if "k_reloc_" in k]
    assert len(kernels) == len(BUDGET), kernels
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert len(hits) == 1, "kernel %s: %s" % (frag, sorted(hits))
        for k, v in hits.items():
            print(frag, v)
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
            assert v["Occupancy"] >= 8, v


def test_the_reloc_file_sums_integers_only_and_shares_the_score():
    text = open(os.path.join(CSRC, "tf_reloc.hip")).read()
    code = text.split("#include <hip/hip_runtime.h>")[1]
    assert '#include "tf_reloc_score.h"' in code and "reloc_score(" in code
    assert "reloc_grey_score" not in code and "18446744073709551616" not in code  # used, not restated
    assert "atomic" not in code  # no atomics of any kind in the code
    kernels = code.split("// the index as it lies in")[0]
    assert kernels.count("__global__") == len(BUDGET) and "__global__" not in code.split("// the index as it lies in")[1]
    # nothing of a pixel is accumulated in floating point: no float or double variable of a kernel is ever added to
    floats = set(re.findall(r"\b(?:float|double)\s+(\w+)\s*[=;,]", kernels))
    assert "z" in floats
    for name in floats:
        assert not re.search(r"\b%s\s*(\+=|-=|\*=)" % re.escape(name), kernels), name
        assert not re.search(r"\b%s\s*=\s*%s\s*[+\-]" % (re.escape(name), re.escape(name)), kernels), name
    # the other aligners and the renderer do not know this file
    for name in ("tf_align.hip", "tf_align_color.hip", "tf_align_group.hip", "tf_align_icp.hip", "tf_render.hip"):
        assert "k_reloc" not in open(os.path.join(CSRC, name)).read()
