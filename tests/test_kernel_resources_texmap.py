"""Register / private-memory budget of the resident TexMap's kernels (texturefusion_amd/csrc/tf_texmap.hip), checked at
build time like tests/test_kernel_resources_mrf.py.  No kernel of the file may hold private memory: each walks hash
tables with dependent loads, and a spilled probe variable would put a scratch round trip into every probe without
failing any parity test.  The VGPR ceilings are what the kernels were built with."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name fragment -> max VGPRs
BUDGET = {
    "k_tm_add_nodesE": 8,        # one chunk-hash probe and one atomic
    "k_tm_updateE": 20,          # two chunk-hash probes (edges) or the observation + cost probes of one column (thread 6)
    "k_tm_retractE": 9,          # a chunk-hash probe, then a cost-table probe
    "k_tm_wrong_mappingE": 8,    # one hash entry, its mesh record, one cost-table probe
    "k_tm_check_nodesE": 16,     # the entry's id unpacked and up to six neighbour probes, one after the other
    "k_tm_check_costsE": 6,      # one table entry, its node word and mesh state
    "k_tm_collect_allE": 13,     # one hash entry -> one record of the node list
    "k_tm_collect_idsE": 12,     # the same from a listed id
    "k_tm_countE": 13,           # a lane's cost-table probe per block of 64 rows
    "k_tm_scanE": 14,            # a thread's run of column lengths + the 1024-wide LDS scan
    "k_tm_fillE": 42,            # two passes over the rows (column maximum, then labels / costs / warm or cheapest-label start) + the neighbour lane
    "k_tm_rankE": 17,            # a key against a 256-key LDS tile at a time
    "k_tm_assignE": 10,          # one node: its solved label back to a keyframe index
    "k_tm_downloadE": 18,        # k_tm_count's walk, writing the entries out
    "k_tm_work_labelsE": 6,      # a work entry's label looked up in the keyframe cache table
    "k_tm_work_cutE": 3,         # one flag per work entry
}


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
def test_texmap_kernels_stay_within_their_budget():
    usage = _usage("tf_texmap.hip")
    kernels = [k for k in usage if "k_tm_" in k]
    assert len(kernels) >= len(BUDGET)
    for k in kernels:  # every kernel of the file is budgeted
        assert any(frag in k for frag in BUDGET), "%s has no budget" % k
    for frag, max_vgpr in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
            assert v["LDS"] <= 8192, "%s holds %d B of LDS" % (k, v["LDS"])


def test_new_kernels_live_in_their_own_file():
    """tf_mrf.hip keeps the solver's kernels only (tests/test_kernel_resources_mrf.py budgets every k_mrf_* of it)"""
    mrf = open(os.path.join(CSRC, "tf_mrf.hip")).read()
    assert "k_tm_" not in mrf
    tm = open(os.path.join(CSRC, "tf_texmap.hip")).read()
    for name in re.findall(r"__global__[^\n]*?void (\w+)\(", tm):
        assert name.startswith("k_tm_"), name
