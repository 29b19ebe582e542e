"""The census of tests/select_inputs.py, on the CPU: every hand-built frame of the chunk selection hinges on the decisions it
names.  For every small case the restatement (tests/select_ref.py) equals the oracle's tfo_select in ids, order and n_coarse;
every mutant the case names gives another list or another n_coarse; every mutant of the table is killed by a case that names
it; the events the restatement records (probes on a rounding tie, probes behind the camera, probes on pixels 1, 2, W-2, W-1)
reach the minima the case states.  The scan-size cases are held against the oracle's n_coarse, and their lists against the
tiles of 256 blocks they must touch.

`ge_band` stays in the table: floats that put a signed distance exactly on either edge of the band exist
(select_inputs._on_band_edge finds them while the cases are built and fails if it cannot).

No GPU.  tests/test_gpu_select_edges.py runs the same cases through the device."""
import numpy as np
import pytest

from oracle import api as O
from tests import select_inputs as SI
from tests import select_ref as SR


def _oracle(c):
    return O.select(c.depth, O.camera_from(c.cam), O.Integrator(*c.ig), c.pose, c.res)


def _ref(c, mutant=None):
    return SR.select(c.depth, c.cam, c.ig, c.pose, c.res, mutant)


def test_the_case_tables_are_complete():
    assert tuple(SI.small_cases()) == SI.SMALL and tuple(SI.scan_cases()) == SI.SCAN and tuple(SI.undefined_cases()) == SI.UNDEFINED
    for c in SI.small_cases().values():
        assert set(c.kills) <= set(SR.MUTANTS) and set(c.minima) <= set(SR.EVENTS), c.name
        assert c.cam.width % 8 == 0 and c.depth.shape == (c.cam.height, c.cam.width) and c.depth.dtype == np.float32


@pytest.mark.parametrize("name", SI.SMALL)
def test_restatement_equals_oracle_and_named_mutants_change_the_result(name):
    c = SI.case(name)
    oids, onc = _oracle(c)
    ids, nc, ev = _ref(c)
    assert nc == onc, "n_coarse %d, oracle %d" % (nc, onc)
    assert ids.shape == oids.shape and np.array_equal(ids, oids), "ids or order"
    assert c.n_selected[0] <= len(oids) <= c.n_selected[1], len(oids)
    for k, least in c.minima.items():
        assert ev[k] >= least, "%s: %d events, at least %d wanted" % (k, ev[k], least)
    for m in c.kills:
        mids, mnc, _ = _ref(c, m)
        assert mnc != onc or not np.array_equal(mids, oids), "mutant %s survives" % m


def test_every_mutant_is_killed_by_a_case_that_names_it():
    named = set()
    for c in SI.small_cases().values():
        named |= set(c.kills)
    assert named == set(SR.MUTANTS), sorted(set(SR.MUTANTS) - named)


def test_the_step_rule_is_the_reference_s_on_both_sides_of_10_mm():
    F = np.float32
    assert SR.step_rule(F(0.01))[0] == 4 and SR.step_rule(np.nextafter(F(0.01), F(1)))[0] == 1
    assert SR.step_rule(F(0.01), "float_step_rule")[0] == 1  # what the f32(0.01) case is there to exclude
    assert SR.step_rule(SI.RES20)[0] == 1 and SR.step_rule(SI.RES8)[0] == 4 and SR.step_rule(SI.RES_2_7)[0] == 4 and SR.step_rule(SI.RES_2_6)[0] == 1


@pytest.mark.parametrize("name", ["band_upper", "band_lower", "band_20mm"])
def test_a_signed_distance_sits_exactly_on_the_band_s_edge(name):
    """the chunk that `>=` would add has a valid probe whose float32 signed distance equals dtp (-dtn) bit for bit"""
    c = SI.case(name)
    ids, _, _ = _ref(c)
    more, _, _ = _ref(c, "ge_band")
    extra = sorted(set(map(tuple, more.tolist())) - set(map(tuple, ids.tolist())))
    assert extra and set(map(tuple, ids.tolist())) <= set(map(tuple, more.tolist()))
    on_edge = 0
    for cid in extra:
        t = SR.chunk_probes(c.depth, c.cam, c.ig, c.pose, c.res, cid)
        edge = -t["dtn"] if name == "band_lower" else t["dtp"]
        on_edge += int(np.count_nonzero(t["valid"] & (t["sd"] == edge)))
    assert on_edge >= 1


def _tiles_touched(c, oids, onc):
    mn, mx = O.bbox(c.depth, O.camera_from(c.cam), c.pose, c.res)
    step = SR.step_rule(c.res)[0]
    dims = [(int(mx[a]) + 1 - (int(mn[a]) - 1)) // step + 1 for a in range(3)]
    assert dims[0] * dims[1] * dims[2] == onc
    b = (oids.astype(np.int64) - (mn.astype(np.int64) - 1)) // step
    cb = (b[:, 0] * dims[1] + b[:, 1]) * dims[2] + b[:, 2]
    return np.unique(cb), np.unique(cb // 256), (onc + 255) // 256


@pytest.mark.parametrize("name", SI.SCAN)
def test_scan_sizes(name):
    c = SI.case(name)
    oids, onc = _oracle(c)
    assert c.n_coarse[0] <= onc <= c.n_coarse[1], onc
    assert c.n_selected[0] <= len(oids) <= c.n_selected[1], len(oids)
    blocks, tiles, n_tiles = _tiles_touched(c, oids, onc)
    if name in ("scan_255", "scan_256", "scan_257"):  # the last block of the column holds chunks: lane 254 / 255 of tile 0, lane 0 of tile 1
        assert blocks[-1] == onc - 1 and len(blocks) >= 10
    if n_tiles > 64:  # first, middle and last tiles
        assert tiles[0] == 0 and tiles[-1] >= n_tiles - 8 and np.any((tiles > n_tiles // 3) & (tiles < 2 * n_tiles // 3)), tiles
        assert len(tiles) >= 10
    if name == "scan_278_tiles":  # the tiles a workgroup takes second
        assert n_tiles > 257 and np.count_nonzero(tiles >= 256) >= 3, tiles


@pytest.mark.parametrize("res", [SI.RES5, SI.RES20], ids=["5mm", "20mm"])
def test_the_sequence_s_boxes_are_not_nested(res):
    seq = SI.sequence(res)
    assert len(seq) >= 4
    boxes = [O.bbox(c.depth, O.camera_from(c.cam), c.pose, c.res) for c in seq]
    for (amn, amx), (bmn, bmx) in zip(boxes[:-1], boxes[1:]):
        a_in_b = np.all(amn >= bmn) and np.all(amx <= bmx)
        b_in_a = np.all(bmn >= amn) and np.all(bmx <= amx)
        assert not a_in_b and not b_in_a
    counts = [_oracle(c) for c in seq]
    assert all(len(ids) >= 50 for ids, _ in counts)
    assert len({nc for _, nc in counts}) >= 3


@pytest.mark.parametrize("name", SI.UNDEFINED)
def test_undefined_frames_have_no_representable_box(name):
    """why the oracle is not the reference there: a corner of the box is NaN, stays at its +-1e8 start value (whose chunk
    index overflows an int at 5 mm; at 20 mm it fits, and min > max is a plain empty box), or is infinite / 1e30"""
    c = SI.case(name)
    if name == "nan_20mm":
        lo, hi = SR.bbox(c.depth, c.cam, c.pose, c.res)
        assert all(l > h for l, h in zip(lo, hi))
        assert _ref(c)[1] == 0 and _oracle(c)[1] == 0
    else:
        with pytest.raises(SR.Undefined):
            SR.bbox(c.depth, c.cam, c.pose, c.res)


def test_infinite_pixels_under_the_identity_pose_are_ignored_by_the_box():
    c, base = SI.case("inf_ignored"), SI.case("slant_5mm")
    assert np.count_nonzero(np.isinf(c.depth)) == 2
    for a, b in zip(SR.bbox(c.depth, c.cam, c.pose, c.res), SR.bbox(base.depth, base.cam, base.pose, base.res)):
        assert a == b
