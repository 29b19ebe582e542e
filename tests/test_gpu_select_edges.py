"""The chunk selection (K-B + K-C: bbox_body, probe, select_body, k_scan, k_acquire, and the posed twins k_bbox_posed /
k_select_posed) on hand-built frames at its decision edges (tests/select_inputs.py; tests/test_select_cpu.py proves on the
CPU that every case hinges on the decision it names), device against oracle, through the three forms of the selection:

  call by call   frame_upload + prepare (k_bbox, k_select<false>, k_scan, k_acquire): ids AND order, newChunkFlag, n_coarse
  fused          integrate_frame (the selection roles of the frame kernel): n_selected, n_updated, n_coarse, the surviving
                 chunk set and every chunk's contents
  posed          integrate_frame_posed_device, the pose in a device buffer: as the fused form

No tolerance anywhere: integers and raw bits.  One handle per camera, resolution and pool size, reset between cases; one
test runs a sequence of frames with boxes that are not nested on a single handle per flow (stale bounding-box keys, a stale
second selection set); the last holds the contract of DESIGN.md for frames without a finite box, for which the oracle is not
the reference."""
import numpy as np
import pytest

from oracle import api as O
from tests import select_inputs as SI
from tests.util import HipBuffer, assert_chunks_equal, sorted_ids
from texturefusion_amd import capi

pytestmark = pytest.mark.gpu

CAP = 1 << 13  # chunks and list entries: the longest list has 2507, the sequence leaves 5274 chunks behind
FLOWS = ("prepare", "fused", "posed")


@pytest.fixture(scope="module")
def pairs(gpu_required):
    """(camera, resolution, large grid) -> (oracle volume, device volume), made on first use"""
    made = {}

    def get(c):
        big = c.n_coarse is not None and c.n_coarse[1] > 1 << 14
        key = (c.cam, float(c.res), big)
        if key not in made:
            ov = O.Volume(c.res, O.camera_from(c.cam), O.Integrator(*c.ig))
            kw = {} if big else dict(max_coarse=1 << 14)  # (the scan sizes need the default, 1 << 20)
            gv = capi.Volume(c.res, c.cam, max_chunks=CAP, max_list=CAP, atlas_w=1920, atlas_h=720, **kw)
            made[key] = (ov, gv)
        ov, gv = made[key]
        ov.reset()
        gv.reset()
        return ov, gv

    yield get
    for ov, gv in made.values():
        gv.close()
        ov.close()


def _cell_buf(pose):
    c = capi.DevicePose()
    c.pose[:] = [float(x) for x in np.asarray(pose, np.float32).reshape(12)]
    c.valid = 1
    return HipBuffer(64).from_host(np.frombuffer(bytes(c), np.uint8))


def _oracle_counts(c):
    ids, nc = O.select(c.depth, O.camera_from(c.cam), O.Integrator(*c.ig), c.pose, c.res)
    return len(ids), nc


def _device_frame(gv, c, flow):
    """one frame through `flow`; -> (ids, newChunkFlag) of the call-by-call form, None of the others (waited for)"""
    if flow == "prepare":
        gv.frame_upload(c.depth, None, None)
        return gv.prepare(c.pose, cap=CAP)
    if flow == "fused":
        gv.frame_upload(c.depth, None, None)
        gv.integrate_frame(c.pose, False)
        gv.sync()
        return None
    d_depth, cell = HipBuffer(c.depth.nbytes).from_host(c.depth), _cell_buf(c.pose)
    try:
        gv.integrate_frame_posed_device(d_depth.ptr, 0, cell.ptr)
        gv.sync()
    finally:
        d_depth.free()
        cell.free()
    return None


def _frame_both(ov, gv, c, flow, contents=True):
    """one frame through the oracle and the device; everything the flow lets one compare"""
    what = "%s, %s" % (c.name, flow)
    n_sel, n_coarse = _oracle_counts(c)
    if flow == "prepare":
        oids, onew = ov.prepare(c.depth, c.pose, cap=CAP)
        gids, gnew = _device_frame(gv, c, flow)
        assert len(oids) == n_sel
        assert gids.shape == oids.shape and np.array_equal(gids, oids), what + ": ids or order"
        assert np.array_equal(gnew, onew), what + ": newChunkFlag"
        st = gv.stats()
        assert (st.n_coarse, st.n_selected) == (n_coarse, n_sel), what
    else:
        nv, ns = ov.integrate_frame(c.depth, None, c.pose)
        _device_frame(gv, c, flow)
        assert ns == n_sel
        st = gv.stats()
        assert (st.n_selected, st.n_updated, st.n_coarse) == (ns, nv, n_coarse), what
    ids = sorted_ids(ov.list_chunks())
    assert np.array_equal(ids, sorted_ids(gv.list_chunks())), what + ": chunk sets"
    if contents:
        assert_chunks_equal(ov, gv, ids, what)
    return n_sel


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("name", SI.SMALL + SI.SCAN)
def test_selection_equals_the_oracle(pairs, name, flow):
    c = SI.case(name)
    ov, gv = pairs(c)
    n = _frame_both(ov, gv, c, flow)
    assert c.n_selected[0] <= n <= c.n_selected[1]
    if flow == "prepare":  # the same frame again: no chunk is new any more, the list and n_coarse stay (keys re-armed)
        _frame_both(ov, gv, c, flow, contents=False)


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("res", [SI.RES5, SI.RES20], ids=["5mm", "20mm"])
def test_a_sequence_on_one_handle(pairs, res, flow):
    """large, small, shifted, large, small elsewhere, shifted: a set that met the keys of its last frame would give the
    small frames a larger n_coarse; a second selection set that kept its list would show in n_selected and the chunk set"""
    seq = SI.sequence(res)
    ov, gv = pairs(seq[0])
    for k, c in enumerate(seq):
        _frame_both(ov, gv, c, flow, contents=(k == len(seq) - 1))


@pytest.mark.parametrize("flow", FLOWS)
def test_a_grid_and_a_list_that_fit_exactly(gpu_required, flow):
    """the capacity tests are strict: a grid of exactly max_coarse blocks and a list of exactly max_list entries fit, one
    block or one entry less of room is TF_ERR_CAPACITY (that such an error leaves no trace: tests/test_gpu_parity.py)"""
    c = SI.case("scan_small")
    n_sel, n_coarse = _oracle_counts(c)
    for room, text in (((n_coarse, n_sel), None), ((n_coarse - 1, n_sel), "candidate grid full"), ((n_coarse, n_sel - 1), "visible list full")):
        ov = O.Volume(c.res, O.camera_from(c.cam), O.Integrator(*c.ig))
        gv = capi.Volume(c.res, c.cam, max_chunks=1 << 10, max_coarse=room[0], max_list=room[1], atlas_w=1920, atlas_h=720)
        try:
            if text is None:
                _frame_both(ov, gv, c, flow)
            else:
                with pytest.raises(capi.TFError) as e:
                    _device_frame(gv, c, flow)
                assert e.value.code == capi.TF_ERR_CAPACITY and text in str(e.value)
                gv.sync()  # (cleared)
                assert len(gv.list_chunks()) == 0
        finally:
            gv.close()
            ov.close()


def _state(gv):
    ids = sorted_ids(gv.list_chunks())
    s, w, col = gv.get_chunks(ids)
    return dict(ids=ids.tobytes(), sdf=s.tobytes(), weight=w.tobytes(), color=col.tobytes(), dirty=sorted_ids(gv.dirty()).tobytes())


@pytest.mark.parametrize("flow", FLOWS)
@pytest.mark.parametrize("name", SI.UNDEFINED)
def test_a_frame_without_a_finite_box(pairs, name, flow):
    """such a frame selects nothing or reports TF_ERR_CAPACITY, leaves the volume as it was, and the
    next ordinary frame on the handle gives the oracle's list and n_coarse.  The oracle never sees the frame"""
    c = SI.case(name)
    before, after = SI.sequence(c.res)[0], SI.sequence(c.res)[2]
    ov, gv = pairs(c)
    _frame_both(ov, gv, before, "fused")
    state = _state(gv)
    assert len(state["ids"]) > 0
    try:
        got = _device_frame(gv, c, flow)
        st = gv.stats()
        assert st.n_selected == 0, "a list of %d" % st.n_selected
        assert got is None or (len(got[0]) == 0 and len(got[1]) == 0)
        print("%s, %s: nothing selected, n_coarse %d" % (name, flow, st.n_coarse))
    except capi.TFError as e:
        assert e.code == capi.TF_ERR_CAPACITY, e
        print("%s, %s: %s" % (name, flow, e))
    now = _state(gv)
    for k in state:
        assert now[k] == state[k], "%s changed" % k
    _frame_both(ov, gv, after, flow)
    _frame_both(ov, gv, before, flow)  # (the fused forms: the other selection set)
