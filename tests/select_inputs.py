"""Hand-built frames for the chunk selection (K-B + K-C) at its decision edges, shared by tests/test_select_cpu.py (which
proves, with tests/select_ref.py and the oracle, that every case hinges on the decisions it names) and
tests/test_gpu_select_edges.py (which runs them through the three device forms of the selection): the GPU tests cannot
drift to inputs the census never saw.

numpy + texturefusion_amd.synth + tests/select_ref.py only: no oracle, no GPU.

A case is a `Case`: camera, resolution, pose, depth, the mutants of tests/select_ref.py it must kill (another list or
another n_coarse than the oracle's) and the least event counts the restatement must record on it.  40 x 32 cameras.

  slant_5mm        depth = 0.3 + 0.02 j + 0.01 i under a camera with non-integral intrinsics (the reference truncates them:
                   33, 31, 19, 15), identity pose: step 4, probes on pixel 1, 2, W-2, W-1 of both axes
  slant_10mm       the same at f32(0.01): (double)res > 0.01 is false, the step stays 4
  slant_20mm       the same at 0.02: step 1, the sqrt(3) diagonal, the scaled negative truncation
  slant_rot        slant_5mm under pose_euler(0.35, 0.2, 0.1, (0.1, -0.05, 0.2))
  bad_8mm          the slanted frame with 10 % zeros, a NaN, a -0.1, three columns of 1.45 (just under far = 1.5) and two rows
                   of 0.26 (just over near = 0.25), under the rotated pose at 8 mm: probes with pz <= 0
  away_20mm        a camera turned away, pose_euler(3.0, 0.1, 0.0, (0, 0, 0.3)) at 20 mm: the box lies behind the camera
  planes           res = 2^-7, identity pose, fx = fy = 32, cx = cy = 16.5: chunk z-index 4 starts exactly at near = 0.25 and
                   index 24 at far = 1.5; depth 0.27 in the upper half, 1.52 in the lower
  ties, ties_fx65  res = 2^-7, fx = fy = 17 (65), cx = cy = 16, identity rotation with t_z = -2^-8 (the probes' pz get even
                   numerators), depth 0.3 with every third row 0.55: probes with u or v exactly on .5
  band_upper,      the slanted plane under `planes`' camera and resolution (identity pose, dyadic origins) with one pixel set so
  band_lower       that the signed distance of one probe of a chunk that no other probe selects equals dtp (the band's far
                   edge), respectively -dtn (its near edge), exactly: the builder searches the unselected chunks next to
                   the list and the floats around pz + dtp / pz - dtn, and asserts that `>=` there adds the chunk.
                   band_20mm: the same at step 1 (res 2^-6), upper edge
  zeros_5mm,       an all-zero frame: nothing at 5 mm; at 20 mm the box of the 0.2 offsets is probed and the reference
  zeros_20mm       selects 16 chunks (depth 0 lies in the band of the chunks around the camera; near = 0.05 admits all of
                   them, under near = 0.25 there are 8)
  wall_5mm         a flat wall at 0.6 m without holes: the box is built from depth + 0.2 only and misses the wall itself
  inf_ignored      slant_5mm with a +inf and a -inf pixel under the identity pose: they back-project to NaN on every axis
                   (0 * inf) and are ignored by the box, the list differs only through the pixels themselves

Scan sizes (no restatement; the oracle alone): frames whose box gives n_coarse <= 64, exactly 255, 256 and 257, just above
64 * 256 and just above 256 * 256, for k_scan's tiles of 256 blocks, its look-back rounds of 64 tiles and a workgroup's
second tile.  scan_255 .. scan_257 are columns of 1 x 1 x n blocks at f32(0.01): a narrow camera (fx = fy = 200) sees an
all-zero frame, whose back-projection (the 0.2 offset) stays inside one chunk in x and y, and the one pixel on the optical
axis lies 82 m away.  The chunks along the axis all read that pixel, and at tens of metres the truncation distance is
metres wide, so every chunk from the near plane (76 m, to keep the list short) to the column's last block is selected: the
last lanes of tile 0 and, in scan_257, the single block of tile 1.  (At 5 mm the last block would lie wholly behind the
band: it starts up to two chunks in front of the chunk of depth + 0.2, 0.08 m at the most, against 0.05 m of dtn.)  The two
large ones are a 0.5 m wall with a strip at 0.75 m and far pixels towards three corners; their lists touch tiles from the
first to the last few, in the larger one tiles beyond 256 (a workgroup's second tile).  scan_small is `ties_fx65`.

Frames the reference leaves undefined (UNDEFINED; it casts an out-of-range float to int): all NaN, +inf, -inf and 1e30
pixels under the rotated and under the identity pose, and a single 1e30 pixel on the truncated principal point (19, 15)
under the identity pose, which leaves x and y alone and puts the box's far corner beyond any chunk index on z only.  The
oracle is not the reference for them; the device's contract is in DESIGN.md."""
import dataclasses
import functools

import numpy as np

from tests import select_ref as SR
from texturefusion_amd import synth

F = np.float32
W, H = 40, 32
IG = (F(0.0019), F(0.00152), F(0.001504), F(6.0), F(1.0))  # MobileFusion::initChiselMap
CAM_FRAC = synth.Camera(W, H, 33.7, 31.2, 19.6, 15.4, 0.25, 1.5)
CAM_PLANES = synth.Camera(W, H, 32.0, 32.0, 16.5, 16.5, 0.25, 1.5)
CAM_TIES = synth.Camera(W, H, 17.0, 17.0, 16.0, 16.0, 0.1, 1.5)
CAM_TIES65 = synth.Camera(W, H, 65.0, 65.0, 16.0, 16.0, 0.1, 1.5)
CAM_NARROW = synth.Camera(W, H, 200.0, 200.0, 20.0, 16.0, 76.0, 200.0)
CAM_WIDE = synth.Camera(W, H, 33.0, 33.0, 19.5, 15.5, 0.05, 8.0)
RES5, RES8, RES10, RES20 = F(0.005), F(0.008), F(0.01), F(0.02)
RES_2_7, RES_2_6 = F(2.0 ** -7), F(2.0 ** -6)
ROTATED = synth.pose_euler(0.35, 0.2, 0.1, (0.1, -0.05, 0.2))
AWAY = synth.pose_euler(3.0, 0.1, 0.0, (0.0, 0.0, 0.3))
BORDERS = dict(x1=1, x2=1, xw2=1, xw1=1, y1=1, y2=1, yh2=1, yh1=1)


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    cam: synth.Camera
    res: np.float32
    pose: np.ndarray
    depth: np.ndarray
    kills: tuple = ()
    minima: dict = dataclasses.field(default_factory=dict)  # event of select_ref.EVENTS -> least count
    n_selected: tuple = (1, 1 << 30)                        # the oracle's count lies in [lo, hi]
    n_coarse: tuple = None                                  # scan sizes: the oracle's n_coarse lies in [lo, hi]
    ig: tuple = IG


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def _pose_t(t):
    p = synth.pose_identity()
    p[:, 3] = t
    return p


def _pose_id():
    return synth.pose_identity()


def slanted():
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (0.3 + 0.02 * j + 0.01 * i).astype(F)


def bad_depths():
    d = slanted()
    rng = np.random.Generator(np.random.PCG64(7))
    d[rng.random(d.shape) < 0.10] = 0.0
    d[:, 30:33] = 1.45
    d[20:22, :] = 0.26
    d[5, 7] = np.nan
    d[9, 11] = -0.1
    return d


def planes_depth():
    d = np.full((H, W), 0.27, F)
    d[H // 2:] = 1.52
    return d


def ties_depth():
    d = np.full((H, W), 0.3, F)
    d[::3] = 0.55
    return d


def with_pixels(depth, pixels):
    d = depth.copy()
    for (i, j), v in pixels.items():
        d[i, j] = v
    return d


NONFINITE = {(6, 9): np.inf, (17, 25): -np.inf, (25, 14): 1e30}


def _on_band_edge(cam, res, pose, base, upper):
    """`base` with one pixel moved so that one probe of one chunk has sd == dtp (upper) or sd == -dtn exactly, and the list
    gains that chunk if the band's comparisons admit equality.  Tried in order: the unselected neighbours of the selected
    chunks (one chunk in x and y, a block's depth in z), their valid probes, the float pz + edge and its two neighbours"""
    ids, _, _ = SR.select(base, cam, IG, pose, res)
    have = {tuple(c) for c in ids.tolist()}
    step = SR.step_rule(res)[0]
    near = []
    for c in ids.tolist():
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in range(-step, step + 1):
                    n = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if n not in have and n not in near:
                        near.append(n)
    for cid in near:
        t = SR.chunk_probes(base, cam, IG, pose, res, cid)
        if not t["depth_valid"]:
            continue
        for l in range(8):
            if not t["valid"][l]:
                continue
            pz, edge = t["pz"][l], (t["dtp"] if upper else -t["dtn"])
            d0 = F(pz + edge)
            for d in (d0, np.nextafter(d0, F(10)), np.nextafter(d0, F(-10))):
                if F(d - pz) != edge:
                    continue
                depth = with_pixels(base, {(int(t["Y"][l]), int(t["X"][l])): d})
                a = SR.select(depth, cam, IG, pose, res)
                b = SR.select(depth, cam, IG, pose, res, "ge_band")
                if cid not in {tuple(c) for c in a[0].tolist()} and cid in {tuple(c) for c in b[0].tolist()}:
                    return depth
    raise AssertionError("no float puts a signed distance on the band's edge")


@functools.lru_cache(maxsize=None)
def small_cases():
    """name -> Case: the cases the restatement runs on"""
    eye = synth.pose_identity()
    rounding = ("trunc", "plus_half", "no_int_intrinsics", "border0", "border_hi", "coarse_trunc")
    c = [
        Case("slant_5mm", CAM_FRAC, RES5, eye, slanted(), rounding + ("no_margin", "no_offset", "swap_dtn"), BORDERS, (2000, 3000)),
        Case("slant_10mm", CAM_FRAC, RES10, eye, slanted(), rounding + ("float_step_rule",), _without(BORDERS, "x2")),
        Case("slant_20mm", CAM_FRAC, RES20, eye, slanted(), ("no_depth_valid", "no_margin", "no_offset"), _without(BORDERS, "x2", "yh2")),
        Case("slant_rot", CAM_FRAC, RES5, ROTATED, slanted(), rounding, BORDERS),
        Case("bad_8mm", CAM_FRAC, RES8, ROTATED, bad_depths(), ("no_depth_valid", "border0", "border_hi", "coarse_trunc"),
             dict(pz_le0=30)),
        Case("away_20mm", CAM_FRAC, RES20, AWAY, slanted(), ("no_depth_valid", "border0", "border_hi"), dict(pz_le0=30)),
        Case("planes", CAM_PLANES, RES_2_7, eye, planes_depth(), ("ge_near_far",)),
        Case("ties", CAM_TIES, RES_2_7, _pose_t((0.0, 0.0, -2.0 ** -8)), ties_depth(), ("half_away",), dict(tie=200)),
        Case("ties_fx65", CAM_TIES65, RES_2_7, _pose_t((0.0, 0.0, -2.0 ** -8)), ties_depth(), (), dict(tie=20)),
        Case("band_upper", CAM_PLANES, RES_2_7, eye, _on_band_edge(CAM_PLANES, RES_2_7, eye, slanted(), True), ("ge_band",)),
        Case("band_lower", CAM_PLANES, RES_2_7, eye, _on_band_edge(CAM_PLANES, RES_2_7, eye, slanted(), False), ("ge_band",)),
        Case("band_20mm", CAM_PLANES, RES_2_6, eye, _on_band_edge(CAM_PLANES, RES_2_6, eye, slanted(), True), ("ge_band",)),
        Case("zeros_5mm", CAM_WIDE, RES5, eye, np.zeros((H, W), F), (), {}, (0, 0)),
        Case("zeros_20mm", CAM_WIDE, RES20, eye, np.zeros((H, W), F), (), {}, (16, 16)),
        Case("wall_5mm", CAM_FRAC, RES5, eye, np.full((H, W), 0.6, F), ("no_offset",), {}, (0, 0)),
        Case("inf_ignored", CAM_FRAC, RES5, eye, with_pixels(slanted(), {(6, 9): np.inf, (17, 25): -np.inf}), (), {}, (2000, 3000)),
    ]
    return {x.name: x for x in c}


COLUMN_POSE = _pose_t((0.041, 0.041, 0.0))


def _column(z_far):
    """an empty (all-zero) frame with the pixel on the optical axis at z_far"""
    return with_pixels(np.zeros((H, W), F), {(16, 20): z_far})


def _hall(z_far):
    """a wall at 0.5 m, a strip at 0.75 m in its middle, and pixels towards three corners at z_far"""
    d = np.full((H, W), 0.5, F)
    d[12:20, :] = 0.75
    return with_pixels(d, {(3, 3): z_far, (3, W - 4): z_far, (H - 4, 3): z_far})


@functools.lru_cache(maxsize=None)
def scan_cases():
    """name -> Case with the n_coarse its box must give (tests/test_select_cpu.py holds them against the oracle)"""
    eye = synth.pose_identity()
    c = [
        Case("scan_small", CAM_TIES65, RES_2_7, _pose_t((0.0, 0.0, -2.0 ** -8)), ties_depth(), n_coarse=(8, 64), n_selected=(50, 4000)),
        Case("scan_255", CAM_NARROW, RES10, COLUMN_POSE, _column(81.3), n_coarse=(255, 255), n_selected=(200, 4000)),
        Case("scan_256", CAM_NARROW, RES10, COLUMN_POSE, _column(81.7), n_coarse=(256, 256), n_selected=(200, 4000)),
        Case("scan_257", CAM_NARROW, RES10, COLUMN_POSE, _column(82.0), n_coarse=(257, 257), n_selected=(200, 4000)),
        Case("scan_71_tiles", CAM_WIDE, RES5, eye, _hall(4.4), n_coarse=(64 * 256 + 1, 72 * 256), n_selected=(200, 4000)),
        Case("scan_278_tiles", CAM_WIDE, RES5, eye, _hall(7.1), n_coarse=(256 * 256 + 1, 280 * 256), n_selected=(200, 4000)),
    ]
    return {x.name: x for x in c}


@functools.lru_cache(maxsize=None)
def undefined_cases():
    """name -> Case: frames without a finite, representable box"""
    eye = synth.pose_identity()
    c = [
        Case("nan_5mm", CAM_FRAC, RES5, eye, np.full((H, W), np.nan, F)),
        Case("nan_20mm", CAM_FRAC, RES20, eye, np.full((H, W), np.nan, F)),
        Case("nonfinite_rot", CAM_FRAC, RES5, ROTATED, with_pixels(slanted(), NONFINITE)),
        Case("nonfinite_eye", CAM_FRAC, RES5, eye, with_pixels(slanted(), NONFINITE)),
        Case("huge_on_axis", CAM_FRAC, RES5, eye, with_pixels(slanted(), {(15, 19): 1e30})),
    ]
    return {x.name: x for x in c}


SMALL = ("slant_5mm", "slant_10mm", "slant_20mm", "slant_rot", "bad_8mm", "away_20mm", "planes", "ties", "ties_fx65", "band_upper",
         "band_lower", "band_20mm", "zeros_5mm", "zeros_20mm", "wall_5mm", "inf_ignored")
SCAN = ("scan_small", "scan_255", "scan_256", "scan_257", "scan_71_tiles", "scan_278_tiles")
UNDEFINED = ("nan_5mm", "nan_20mm", "nonfinite_rot", "nonfinite_eye", "huge_on_axis")


def sequence(res):
    """Frames for ONE handle (CAM_FRAC at `res`) whose boxes are not nested in either direction: large, small, shifted,
    large, small elsewhere, shifted -- each of the two selection sets serves three times, and a set that kept the keys of
    its last frame would give the small frames a box that is too large"""
    near = np.full((H, W), 0.3, F)
    near[10:22, 12:28] = 0.55  # (the wall itself lies in front of the box of depth + 0.2; the patch is inside it)
    frames = [("large", _pose_id(), slanted()), ("small", _pose_t((1.5, -1.2, 0.4)), near), ("shifted", ROTATED, slanted()),
              ("large again", _pose_id(), slanted()), ("small elsewhere", _pose_t((-1.4, 1.1, -0.1)), near), ("shifted again", ROTATED, slanted())]
    return [Case("sequence %d: %s" % (k, what), CAM_FRAC, F(res), pose, depth) for k, (what, pose, depth) in enumerate(frames)]


def case(name):
    for table in (small_cases, scan_cases, undefined_cases):
        if name in table():
            return table()[name]
    raise KeyError(name)
