"""The voxel update (K-A) on hand-built chunks at its arithmetic edges (tests/ka_inputs.py; tests/test_ka_cpu.py proves on
the CPU that every case hits the edge it names), device against oracle, bit for bit: needsUpdate flags, out_quality, sdf,
weight and colour of every listed chunk -- through tf_integrate in its six (colour, quality, flag) instances, through
tf_integrate_depth_group_host, and through the fused frame (k_frame's own instance of the body, the kernel the benchmark
times), where the chunk lists and the dirty sets are compared too.

No tolerance.  One exception: in case G (the only one that may store NaNs, tests/test_ka_cpu.py::test_no_nan_outside_g) a
stored NaN equals a stored NaN whatever its sign and payload -- x86 produces the negative default NaN, the GPU the positive
one -- and only at exactly the voxels where the oracle has one."""
import numpy as np
import pytest

from oracle import api as O
from tests import ka_inputs as KI
from tests import ka_ref as KR
from tests.util import sorted_ids
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu

MODES = ((False, False), (True, False), (True, True))  # (colour, quality)


def _pair(c):
    ov = O.Volume(c.res, O.camera_from(c.cam), O.Integrator(*c.ig))
    gv = capi.Volume(c.res, c.cam, max_chunks=4096, max_list=4096, max_coarse=1 << 14, atlas_w=1920, atlas_h=720)
    gv.set_truncation(*[float(v) for v in c.ig[:4]])
    gv.set_weight(float(c.ig[4]))
    return ov, gv


def _preset(c, ov, gv):
    for i, cid in enumerate(c.ids):
        s, w, col = c.chunk(i)
        ov.set_chunk(cid, s, w, col)
        gv.set_chunk(cid, s, w, col)


def _assert_same_chunks(c, ov, gv, ids, what):
    nan_ok = c.name in KI.NAN_ALLOWED
    ids = np.asarray(ids, np.int32).reshape(-1, 3)
    gs, gw, gc = gv.get_chunks(ids)
    for i, cid in enumerate(ids):
        s, w, col = ov.get_chunk(cid)
        assert KR.same_floats(s, gs[i], nan_ok), "%s: sdf differs in chunk %s" % (what, cid)
        assert KR.same_floats(w, gw[i], nan_ok), "%s: weight differs in chunk %s" % (what, cid)
        assert np.array_equal(col, gc[i]), "%s: colour differs in chunk %s" % (what, cid)


@pytest.mark.parametrize("name", KI.ALL)
def test_integrate_all_six_instances(gpu_required, name):
    c = KI.cases()[name]
    ov, gv = _pair(c)
    try:
        for flag in (1, 0):
            for colour, quality in MODES:
                what = "%s flag %d colour %d quality %d" % (name, flag, colour, quality)
                ov.reset()
                gv.reset()
                _preset(c, ov, gv)
                rgba, q = (c.rgba if colour else None), (c.quality if quality else None)
                on, gn = np.zeros(len(c.ids), np.uint8), np.zeros(len(c.ids), np.uint8)
                oq = ov.integrate(c.depths[0], rgba, q, c.poses[0], c.ids, on, flag, -1)
                gv.frame_upload(c.depths[0], rgba, q)
                gq = gv.integrate(c.poses[0], c.ids, gn, flag, colour, quality)
                assert np.array_equal(on, gn), what + ": needsUpdate flags"
                if colour:
                    assert np.array_equal(oq.view(np.uint32), gq.view(np.uint32)), what + ": out_quality %s vs %s" % (oq, gq)
                _assert_same_chunks(c, ov, gv, c.ids, what)
    finally:
        gv.close()
        ov.close()


@pytest.mark.parametrize("name", [n for n in KI.ALL if n[0] in "ABCDEFGJ"])
def test_depth_group_host(gpu_required, name):
    """J: 1, 2 and 6 frames; A - G: a group of one"""
    c = KI.cases()[name]
    ov, gv = _pair(c)
    try:
        for flag in (1, 0):
            ov.reset()
            gv.reset()
            _preset(c, ov, gv)
            on, gn = np.zeros(len(c.ids), np.uint8), np.zeros(len(c.ids), np.uint8)
            for dep, pose in zip(c.depths, c.poses):  # the oracle: one depth-only integrate per frame
                ov.integrate(dep, None, None, pose, c.ids, on, flag, -1)
            gv.integrate_depth_group_host(c.depths, np.stack([p.reshape(12) for p in c.poses]), c.ids, gn, flag)
            assert np.array_equal(on, gn), "%s flag %d: needsUpdate flags" % (name, flag)
            _assert_same_chunks(c, ov, gv, c.ids, "%s group of %d, flag %d" % (name, len(c.poses), flag))
    finally:
        gv.close()
        ov.close()


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "depth"])
@pytest.mark.parametrize("name", KI.FUSED)
def test_fused_frame(gpu_required, name, colour):
    """tf_integrate_frame against the oracle's integrate_frame: the selection finds the preset chunks by itself
    (tests/test_ka_cpu.py::test_fused_selection_finds_the_preset_chunks), creates others around them and parks what it
    does not update"""
    c = KI.cases()[name]
    ov, gv = _pair(c)
    try:
        _preset(c, ov, gv)
        rgba = c.rgba if colour else None
        nv, ns = ov.integrate_frame(c.depths[0], rgba, c.poses[0])
        gv.frame_upload(c.depths[0], rgba, None)
        gv.integrate_frame(c.poses[0], colour)
        gv.sync()
        st = gv.stats()
        assert (st.n_selected, st.n_updated) == (ns, nv)
        ids = sorted_ids(ov.list_chunks())
        assert np.array_equal(ids, sorted_ids(gv.list_chunks())), "chunk lists"
        assert np.array_equal(sorted_ids(ov.dirty()), sorted_ids(gv.dirty())), "dirty sets"
        _assert_same_chunks(c, ov, gv, ids, "%s fused" % name)
    finally:
        gv.close()
        ov.close()
