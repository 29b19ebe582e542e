"""Load batches of the mesher and its filter, checked in the compiled kernels (hipcc cross-compiles without a GPU).

Both kernels are chains of dependent round trips to scattered cache lines; their source means several loads of a phase
to be in flight together.  A load under a lane-dependent condition is compiled behind that condition's branch and waited
for on its own: the kernel stays correct, passes every parity test, and is a few round trips slower -- this catches it.
(LOAD BATCHES.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

MESHER = "_ZN2tf6k_meshILi128ELb0E"             # k_mesh<128, false>: the product instance
FILTER = "_ZN2tf13k_mesh_filterILb1ELb0ELb0E"   # k_mesh_filter<true, false, false>: wave form, no patch stage


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel symbol -> its instructions (comments and directives dropped), from tf_mesh.hip compiled to assembly"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("asm") / "tf_mesh.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
           "--cuda-device-only", "-S", os.path.join(CSRC, "tf_mesh.hip"), "-o", out]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found, name = {}, None
    for line in open(out):
        code = line.split(";")[0].strip()
        m = re.match(r"(_ZN2tf\w+):$", code)
        if m:
            name = m.group(1)
            found[name] = []
        elif name and code and not code.startswith("."):
            found[name].append(code)
            if code.startswith("s_endpgm"):
                name = None
    return found


def _kernel(kernels, frag):
    hits = [k for k in kernels if k.startswith(frag)]
    assert len(hits) == 1, "kernel %s: %s" % (frag, hits)
    return kernels[hits[0]]


def _longest_run(code, op):
    """most `op` instructions issued without a wait for vector memory in between"""
    best = run = 0
    for ins in code:
        if ins.split()[0] == op:
            run += 1
            best = max(best, run)
        elif ins.startswith("s_waitcnt") and "vmcnt" in ins:
            run = 0
    return best


def test_mesher_stages_the_halo_as_one_batch(kernels):
    code = _kernel(kernels, MESHER)
    assert _longest_run(code, "global_load_dwordx4") >= 4, "the halo pairs (16 bytes each) are waited for one by one"


def test_mesher_reads_no_index_table_in_the_corner_pass(kernels):
    code = _kernel(kernels, MESHER)
    assert not [i for i in code if i.startswith("global_load_ushort")], "a 16-bit load: an index table, or a split colour load"


def test_filter_reads_the_corner_voxels_as_one_batch(kernels):
    code = _kernel(kernels, FILTER)
    assert _longest_run(code, "global_load_dwordx2") >= 4, "the neighbours' corner voxels (8 bytes each) are waited for one by one"
