"""Register / private-memory budget of the alignment kernels (texturefusion_amd/csrc/tf_align.hip), checked at build time
like tests/test_kernel_resources_render.py.  k_align_rows carries seven trilinear samples and the tile's 31 sums: the
budget is the raycaster's, no private memory and VGPRs at or below what gives six waves per SIMD (512 / 6 = 85, in
granules of 8: 80; it builds at 77).  k_align_solve is one workgroup of 256 threads whose lane 0 holds the 6 x 6 system in
registers (88 VGPRs as built; the budget of 256 is the most a 256-thread workgroup can be given and bounds nothing): what is
checked for this kernel is that nothing of lane 0's arrays went to private memory.  Its LDS, 5120 B as built, is the
8 x 32 f64 table the eight groups' sums meet in (2048 B) plus the small arrays of lane 0 the compiler moves there.
The kernels are calls into tf_align_rows.h, which all four aligners share: that its pieces exist once is checked here too."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max scratch bytes per lane, max LDS bytes per workgroup)
BUDGET = {"k_align_begin": (8, 0, 0), "k_align_rows": (80, 0, 2048), "k_align_solve": (256, 0, 5120)}


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
def test_align_kernels_stay_within_their_budget():
    usage = _usage("tf_align.hip")
    kernels = [k for k in usage if "k_align_" in k]
    assert len(kernels) == len(BUDGET), kernels
    for frag, (max_vgpr, max_scratch, max_lds) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= max_lds, "%s holds %d B of LDS" % (k, v["LDS"])
    rows = [v for k, v in usage.items() if "k_align_rows" in k][0]
    assert rows["Occupancy"] >= 6, rows


ALIGNERS = ("tf_align.hip", "tf_align_color.hip", "tf_align_group.hip", "tf_align_icp.hip")
SHARED = ("tf_align_rows.h", "tf_align_tree.h", "tf_align_solve.h", "tf_align_group_solve.h", "tf_ray_devfn.h", "tf_volume.h")
# a distinctive line of every shared piece: the tree's level and its table, the sampler, the 6 x 6 solve, the idle test,
# the level-finished mark, the stop rules, the solve launch's stride over the partial rows, the wave-order combine, the carver
PIECES = ("void al_halve(", "AlPairs al_pairs()", "bool tri_sample(", "bool align_solve6(", "(st & 1u) ||", "c.state & 0xFFu",
          "TF_ALIGN_SINGULAR", "TF_ALIGN_TOO_FEW", "TF_ALIGN_CONVERGED", "t += 8u", "k < kAlWaves; ++k", "L.take(count * sizeof(")


def _code(name):
    """the file's text without its // comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_the_sampler_is_shared_not_copied():
    ray = open(os.path.join(CSRC, "tf_ray.hip")).read()
    align = open(os.path.join(CSRC, "tf_align.hip")).read()
    assert '#include "tf_ray_devfn.h"' in ray and '#include "tf_align_rows.h"' in align
    assert '#include "tf_ray_devfn.h"' in open(os.path.join(CSRC, "tf_align_rows.h")).read()
    for text in (ray, align):
        assert "bool tri_sample(" not in text
    assert "atomic" not in align.split("#include <hip/hip_runtime.h>")[1]  # no atomics of any kind in the code
    assert "atomic" not in open(os.path.join(CSRC, "tf_align_rows.h")).read().split("#include <hip/hip_runtime.h>")[1]


def test_the_aligners_machinery_is_written_once():
    """every shared piece once in the headers, in no aligner's own file"""
    shared = "".join(_code(h) for h in SHARED)
    for piece in PIECES:
        assert shared.count(piece) == 1, piece
        for name in ALIGNERS:
            assert _code(name).count(piece) == 0, (name, piece)
    for name in ALIGNERS:
        assert '#include "tf_align_rows.h"' in _code(name), name
