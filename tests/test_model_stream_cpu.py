"""The model stream's public surface and the build-time budget of its kernels (texturefusion_amd/csrc/tf_model.hip), without
a GPU: the header declares the entry points with the agreed signatures, the binding names them, the Makefile builds the
file, and every kernel of it holds no private memory and stays within the VGPR figures it was built with (resource remarks
only, as tests/test_kernel_resources_render.py reads them)."""
import os
import re
import shutil

import pytest

from tests.test_kernel_resources_render import _usage
from texturefusion_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SIGNATURES = {
    "tf_model_stream_reserve": "tf_volume* v, int64_t cap_vertices, int64_t cap_indices",
    "tf_model_stream_update_device": "tf_volume* v",
    "tf_model_stream_update": "tf_volume* v, int64_t* n_vertices, int64_t* n_indices",
    "tf_model_stream_get": "tf_volume* v, const float** d_vertices, const uint32_t** d_indices, const uint32_t** d_counts, "
                           "int64_t* cap_vertices, int64_t* cap_indices",
    "tf_model_stream_stats": "tf_volume* v, int64_t out[4]",
    "tf_model_stream_release": "tf_volume* v",
    "tf_model_stream_time": "tf_volume* v, double us[4]",  # (the measurement aid beside the six)
}

# kernel name fragment -> (max VGPRs, max scratch bytes per lane): the figures of the build that was measured
BUDGET = {"k_model_list": (12, 0), "k_model_rank": (12, 0), "k_model_place": (14, 0), "k_model_scan": (82, 0), "k_model_write": (45, 0)}


def test_header_declares_the_six_entry_points():
    text = open(os.path.join(ROOT, "include", "tf_fusion.h")).read()
    for name, args in SIGNATURES.items():
        m = re.search(r"TF_API int %s\(([^;]*)\);" % name, text)
        assert m, "%s is not declared" % name
        assert " ".join(m.group(1).split()) == args, "%s(%s)" % (name, " ".join(m.group(1).split()))
        assert name in capi.SYMBOLS, "%s is missing from capi.SYMBOLS" % name
        assert hasattr(capi.Volume, name[3:]), "capi.Volume has no %s" % name[3:]


def test_makefile_builds_tf_model():
    mk = open(os.path.join(ROOT, "texturefusion_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "tf_model.hip" in srcs
    assert "tf_model.hip" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_model_kernels_stay_within_their_budget():
    usage = _usage("tf_model.hip")
    kernels = [k for k in usage if "k_model_" in k]
    assert len(kernels) == len(BUDGET), kernels
    for k in kernels:  # every kernel of the file is budgeted
        assert any(frag in k for frag in BUDGET), "%s has no budget" % k
    for frag, (max_vgpr, max_scratch) in BUDGET.items():
        hits = {k: v for k, v in usage.items() if frag in k}
        assert hits, "kernel %s not found" % frag
        for k, v in hits.items():
            assert v["ScratchSize"] <= max_scratch, "%s uses %d B/lane of private memory" % (k, v["ScratchSize"])
            assert v["VGPRs"] <= max_vgpr, "%s uses %d VGPRs (budget %d)" % (k, v["VGPRs"], max_vgpr)
