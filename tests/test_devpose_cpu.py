"""The device-pose path without a GPU (tf_devpose.hip and the twins next to the bodies they call): the restatement of the
pose constants (tests/pose_consts_ref.py) against make_select_consts itself, bit for bit, and the register / private-memory
figures of the new kernels as the compiler reports them -- each twin beside its host-pose twin, from the same compile."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import pose_consts_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "texturefusion_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = shutil.which("g++") or shutil.which("c++")
GRANULE = 8  # VGPRs are allocated in blocks of eight on gfx950 (512 per SIMD lane, unified file)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_restatement_equals_make_select_consts(tmp_path):
    exe = str(tmp_path / "consts_print")
    cmd = [CXX, "-std=c++14", "-O2", "-Wall", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp_devpose", "consts_print.cpp"),
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [(name, res, p) for name, p in PR.poses().items() for res in PR.RESOLUTIONS]
    text = "".join(" ".join("%08x" % w for w in np.concatenate([[res], p]).astype(np.float32).view(np.uint32)) + "\n"
                   for _, res, p in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) == 6
    steps = set()
    for (name, res, p), line in zip(cases, lines):
        tok = line.split()
        assert len(tok) == 1 + PR.WORDS
        got = np.array([int(t, 16) for t in tok[1:]], np.uint32)
        want = PR.words(PR.consts(p, res))
        assert int(tok[0]) == PR.step_of(res), (name, res)
        assert np.array_equal(got, want), (name, float(res), np.flatnonzero(got != want))
        steps.add(int(tok[0]))
    assert steps == {1, 4}  # both branches of the resolution rule
    odd = PR.consts(PR.poses()["odd"], PR.RESOLUTIONS[0])
    assert np.signbit(odd["rot"][odd["rot"] == 0]).all()  # the negative zeros got through ...
    assert 0 < np.abs(odd["tc"]).max() < 1.2e-38          # ... and the denormal translation gave a denormal product


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
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def _one(usage, frag):
    hits = [v for k, v in usage.items() if frag in k]
    assert len(hits) == 1, (frag, sorted(usage))
    return hits[0]


# file -> [(device-pose twin, its host-pose twin as a mangled-name fragment)]; k_select's emit instance is <true>
TWINS = {
    "tf_kernels.hip": [("k_bbox_posed", "6k_bboxE"), ("k_select_posed", "k_selectILb1EE")],
    "tf_ray.hip": [("k_raycast_posed", "9k_raycastE")],
    "tf_align.hip": [("k_stage2_start", "k_align_begin")],
    "tf_align_icp.hip": [("k_track_start", "k_icp_begin")],
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(TWINS))
def test_device_pose_twins_cost_no_more_than_their_host_pose_twins(src):
    usage = _usage(src)
    for twin, host in TWINS[src]:
        t, h = _one(usage, twin), _one(usage, host)
        print(src, twin, t, host, h)
        assert t["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (twin, t["ScratchSize"])
        granules = lambda v: (v["VGPRs"] + GRANULE - 1) // GRANULE
        assert granules(t) <= granules(h), "%s: %d VGPRs, %s: %d" % (twin, t["VGPRs"], host, h["VGPRs"])
    if src == "tf_ray.hip":  # tests/test_raycast_cpu.py's budget: six waves per SIMD
        assert _one(usage, "k_raycast_posed")["VGPRs"] <= 80


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_constants_and_the_finish_kernel_own_no_private_memory():
    usage = _usage("tf_devpose.hip")
    kernels = sorted(k for k in usage if "k_pose_consts" in k or "k_track_finish" in k)
    assert len(kernels) == 2 and len(usage) == 2, sorted(usage)  # the file's only kernels
    for k in kernels:
        print(k, usage[k])
        assert usage[k]["ScratchSize"] == 0, "%s uses %d B/lane of private memory" % (k, usage[k]["ScratchSize"])
        assert usage[k]["VGPRs"] <= 64  # one wave each: anything up to eight waves' worth is free
