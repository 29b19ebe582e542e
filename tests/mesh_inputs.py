"""Hand-built neighbourhoods for the marching-cubes mesher (k_mesh_filter + k_mesh, tf_mesh.hip), one decision per case,
each with its known answer.  Pure numpy: no GPU, no oracle -- tests/test_mesh_edges_cpu.py proves on the oracle that the
inputs sit where they claim, tests/test_gpu_mesh_edges.py puts the same cases on the device.

A case is a neighbourhood (`Hood`: a centre chunk and some of its 26 neighbours, addressed by voxel coordinates relative
to the centre's origin) and what the centre's mesh must be (`Expect`).  The answer is built, not computed by a second
mesher: the field says which lattice points are negative, the case says by hand which cells are unobserved (`dead`) and
which (cell, edge) pairs fail their validity test (`bad`), and `predict` only walks the triangle table over that --
triangles in cell order, vertices in edge-slot order, the LAST emitting cell of a slot owning its vertex
(ChunkManager.cpp:836-897).  The one piece of arithmetic restated here is the vertex position (`vertex`).

Families (letters as in the test modules): A every cube case with exact counts, B vertex ownership, C edge validity
thresholds, D vertex arithmetic and colour, E adjacency flags, F the mesh store at its capacities, G the filter."""
import os
import re

import numpy as np

F = np.float32
RES5 = F(0.005)
RES10 = F(0.01)

CORNER = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGE = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
ALL27 = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
PLUS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
COLOUR = (30, 60, 90, 3)


def table():
    """the packed triangle table the oracle and the device share: 256 rows of 16 edge ids, -1 = end"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "mc_table.inc")
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", open(path).read())]
    assert len(words) == 256
    return [[(-1 if ((w >> (4 * j)) & 0xF) == 0xF else (w >> (4 * j)) & 0xF) for j in range(16)] for w in words]


_TABLE = table()
TRIANGLES = [sum(e >= 0 for e in row) // 3 for row in _TABLE]


def edge_slot(x, y, z, e):
    """slot of edge e of cell (x, y, z) in the 9 x 9 x 9 x 3 edge grid: axis + 3 (bx + 9 by + 81 bz)"""
    bx = x + (e in (1, 5, 9, 10))
    by = y + (e in (2, 6, 10, 11))
    bz = z + (e in (4, 5, 6, 7))
    ax = 2 if e >= 8 else (e & 1)
    return ax + 3 * (bx + 9 * by + 81 * bz)


def slot_of(axis, b):
    return axis + 3 * (b[0] + 9 * b[1] + 81 * b[2])


_SLOT_CELLS = {}
for _z in range(8):
    for _y in range(8):
        for _x in range(8):
            for _e in range(12):
                _SLOT_CELLS.setdefault(edge_slot(_x, _y, _z, _e), []).append(((_x, _y, _z), _e))


def slot_cells(m):
    """the (up to four) cells of the chunk around edge slot m, ascending, each with its name for the edge"""
    return list(_SLOT_CELLS.get(m, []))


def cells_with_corner(g):
    """the cells of the chunk (0..7 per axis) that have lattice point g as a corner"""
    return {(x, y, z) for x in (g[0] - 1, g[0]) for y in (g[1] - 1, g[1]) for z in (g[2] - 1, g[2])
            if 0 <= x < 8 and 0 <= y < 8 and 0 <= z < 8}


def bad_slot(m):
    """edge slot m fails for every cell around it (a test on the nearer corner alone: weight, gradient norm, product)"""
    return set(slot_cells(m))


def bad_cells(cells):
    """every edge of these cells fails (a test that depends on the cell: the outside partners of its corner)"""
    return {(c, e) for c in cells for e in range(12)}


def predict(neg, dead=(), bad=()):
    """neg[z, y, x] over the 9^3 lattice -> (used slots ascending, their owners (cell, edge), indices u32)"""
    dead, bad = set(dead), set(bad)
    owner, tris = {}, []
    for z in range(8):
        for y in range(8):
            for x in range(8):
                if (x, y, z) in dead:
                    continue
                case = sum(int(neg[z + c[2], y + c[1], x + c[0]]) << k for k, c in enumerate(CORNER))
                row = _TABLE[case]
                for t in range(0, 15, 3):
                    if row[t] < 0:
                        break
                    tri = (row[t + 2], row[t + 1], row[t])  # (s2, s1, s0), ChunkManager.cpp:914-916
                    if any(((x, y, z), e) in bad for e in tri):
                        continue
                    for e in tri:
                        m = edge_slot(x, y, z, e)
                        owner[m] = ((x, y, z), e)  # the last writer wins
                        tris.append(m)
    slots = sorted(owner)
    rank = {m: i for i, m in enumerate(slots)}
    return slots, [owner[m] for m in slots], np.array([rank[m] for m in tris], np.uint32)


def vertex(cid, res, cell, e, s0, s1):
    """tf_mesh.hip pass 2 (ChunkManager.cpp:757-762, :662, :872-877) in float32, operation by operation"""
    res, s0, s1 = F(res), F(s0), F(s1)
    half = res * F(0.5)
    tt = s0 / (s0 - s1)
    out = np.empty(3, np.float32)
    for a in range(3):
        p0 = F(CORNER[EDGE[e][0]][a]) * res
        p1 = F(CORNER[EDGE[e][1]][a]) * res
        ev = p0 + tt * (p1 - p0)
        org = F(8 * int(cid[a])) * res
        origin = org + (F(cell[a]) * res + half)
        out[a] = ev + origin
    return out


def colour_of(col4):
    """ChunkManager.cpp:808-824: sums / 255 / count, white when the count is 0"""
    if int(col4[3]) == 0:
        return np.ones(3, np.float32)
    return np.array([(F(int(c)) / F(255.0)) / F(int(col4[3])) for c in col4[:3]], np.float32)


class Hood:
    """a centre chunk and the listed ones of its neighbours; voxels are addressed by g = (x, y, z) relative to the centre's
    origin, -8..15 per axis; a chunk that is not there reads as sdf 999"""

    def __init__(self, centre, present=ALL27, sdf=0.01, weight=60.0, colour=COLOUR):
        self.c = tuple(int(v) for v in centre)
        self.ch = {}
        for d in present:
            self.ch[tuple(self.c[a] + d[a] for a in range(3))] = [
                np.full(512, sdf, np.float32), np.full(512, weight, np.float32), np.tile(np.array(colour, np.uint16), 512)]
        assert self.c in self.ch

    def _at(self, g):
        return tuple(self.c[a] + (g[a] >> 3) for a in range(3)), (g[0] & 7) + 8 * (g[1] & 7) + 64 * (g[2] & 7)

    def set(self, g, sdf=None, w=None, col=None):
        key, i = self._at(g)
        if sdf is not None:
            self.ch[key][0][i] = sdf
        if w is not None:
            self.ch[key][1][i] = w
        if col is not None:
            self.ch[key][2][4 * i:4 * i + 4] = col
        return self

    def fill(self, fn):
        """sdf = fn(gx, gy, gz) (arrays) over every chunk that is there"""
        zz, yy, xx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
        for key, f in self.ch.items():
            o = [8 * (key[a] - self.c[a]) for a in range(3)]
            f[0][:] = np.asarray(fn(xx + o[0], yy + o[1], zz + o[2]), np.float32).reshape(512)
        return self

    def sdf(self, g):
        key, i = self._at(g)
        return self.ch[key][0][i] if key in self.ch else F(999.0)

    def colour(self, g):
        key, i = self._at(g)
        return self.ch[key][2][4 * i:4 * i + 4]

    def neg(self):
        n = np.zeros((9, 9, 9), bool)
        for z in range(9):
            for y in range(9):
                for x in range(9):
                    n[z, y, x] = self.sdf((x, y, z)) < 0
        return n

    def chunks(self):
        return {k: tuple(a.copy() for a in f) for k, f in self.ch.items()}


class Expect:
    """the centre's mesh: None for verts / indices / colours / adj = not stated; key: the chunk is in allMeshes"""

    def __init__(self, nv, nt, verts=None, indices=None, colours=None, adj=None, key=None, owners=None):
        self.nv, self.nt, self.verts, self.indices, self.colours, self.adj = nv, nt, verts, indices, colours, adj
        self.key = (nv > 0) if key is None else key
        self.owners = owners
        self.name = ""  # the case's name where several share a step


def expect(hood, res=RES5, dead=(), bad=(), key=None, colours=False, adj=None):
    slots, owners, idx = predict(hood.neg(), dead, bad)
    verts = np.zeros((len(slots), 3), np.float32)
    cols = np.zeros((len(slots), 3), np.float32)
    for i, (cell, e) in enumerate(owners):
        g0 = tuple(cell[a] + CORNER[EDGE[e][0]][a] for a in range(3))
        g1 = tuple(cell[a] + CORNER[EDGE[e][1]][a] for a in range(3))
        s0, s1 = hood.sdf(g0), hood.sdf(g1)
        verts[i] = vertex(hood.c, res, cell, e, s0, s1)
        cols[i] = colour_of(hood.colour(g1 if abs(s0) > abs(s1) else g0))
    return Expect(len(slots), len(idx) // 3, verts, idx, cols if colours else None, adj, key, owners)


NONE = Expect(0, 0)


def check(exp, mesh, what):
    """mesh: None (not in allMeshes) or dict(verts, indices, colors, adj)"""
    if not exp.key:
        assert mesh is None, "%s: a mesh where none is expected (%d vertices)" % (what, len(mesh["verts"]))
        return
    assert mesh is not None, "%s: no mesh, expected %d vertices / %d triangles" % (what, exp.nv, exp.nt)
    got = (len(mesh["verts"]), len(mesh["indices"]) // 3)
    assert got == (exp.nv, exp.nt), "%s: (nv, nt) = %s, expected %s" % (what, got, (exp.nv, exp.nt))
    if exp.verts is not None and exp.nv:
        diff = np.flatnonzero((mesh["verts"].view(np.uint32) != exp.verts.view(np.uint32)).any(axis=1))
        assert len(diff) == 0, "%s: vertex %d is %s, expected %s (owner %s)" % (
            what, diff[0], mesh["verts"][diff[0]], exp.verts[diff[0]], exp.owners[diff[0]] if exp.owners else "?")
    if exp.indices is not None and exp.nt:
        assert np.array_equal(mesh["indices"], exp.indices), "%s: indices differ" % what
    if exp.colours is not None and exp.nv:
        assert np.array_equal(mesh["colors"].view(np.uint32), exp.colours.view(np.uint32)), "%s: colours differ" % what
    if exp.adj is not None:
        assert list(mesh["adj"]) == list(exp.adj), "%s: adjacency flags %s, expected %s" % (what, list(mesh["adj"]), exp.adj)


class Step:
    """upload `chunks` (only those that changed since the step before), finalize `ids` with needs = 1, update_meshes
    (compress_meshes too when `compress`), then every key of `expect` must hold its answer; `only`: the keys of
    allMeshes are exactly these"""

    def __init__(self, what, chunks, ids, expect, only=None, compress=False):
        self.what, self.chunks, self.ids, self.expect, self.only, self.compress = what, chunks, ids, expect, only, compress


def apply_step(step, volumes, cache):
    """cache: what the volumes hold (key -> arrays), kept by the caller across the steps of one scene"""
    for key, f in step.chunks.items():
        old = cache.get(key)
        if old is not None and all(a.tobytes() == b.tobytes() for a, b in zip(old, f)):
            continue
        cache[key] = f
        for v in volumes:
            v.set_chunk(np.array(key, np.int32), *f)
    ids = np.array(step.ids, np.int32).reshape(-1, 3)
    for v in volumes:
        v.finalize(ids, np.ones(len(ids), np.uint8), np.zeros(len(ids), np.uint8))


def check_step(step, meshes, who):
    """meshes: key -> mesh dict of every chunk in allMeshes"""
    for key, exp in step.expect.items():
        check(exp, meshes.get(key), "%s, %s %s, chunk %s" % (who, step.what, exp.name, key))
    if step.only is not None:
        assert set(meshes) == set(step.only), "%s, %s: allMeshes holds %s, expected %s" % (
            who, step.what, sorted(meshes), sorted(step.only))


# ---------------------------------------------------------------------------------------------------------------
# A. every cube case, exact counts: sdf = +-a on a random sign lattice, everything observed, every cut edge valid
# ---------------------------------------------------------------------------------------------------------------
A_SEEDS = (1, 2, 3, 4, 5, 6)
A_AMPL = 0.004


def case_a(seed, centre=(0, 0, 0), res=RES5):
    rng = np.random.default_rng(seed)
    sign = rng.integers(0, 2, (24, 24, 24)) * 2 - 1  # [z + 8, y + 8, x + 8]
    hood = Hood(centre).fill(lambda x, y, z: sign[z + 8, y + 8, x + 8] * A_AMPL)
    return hood, expect(hood, res)


def a_counts(hood):
    """(triangles, vertices, cube cases) from the signs alone: table counts per cell, sign-changing lattice edges"""
    n = hood.neg()
    cases = [sum(int(n[z + c[2], y + c[1], x + c[0]]) << k for k, c in enumerate(CORNER))
             for z in range(8) for y in range(8) for x in range(8)]
    nv = int((n[:, :, 1:] != n[:, :, :-1]).sum() + (n[:, 1:, :] != n[:, :-1, :]).sum() + (n[1:, :, :] != n[:-1, :, :]).sum())
    return sum(TRIANGLES[c] for c in cases), nv, set(cases)


def case_checkerboard(centre=(0, 0, 0)):
    """the largest mesh a chunk can have: every lattice edge cut, 3 * 8 * 81 = 1944 vertices"""
    hood = Hood(centre).fill(lambda x, y, z: (((x + y + z) & 1) * 2 - 1) * A_AMPL)
    return hood, expect(hood)


# ---------------------------------------------------------------------------------------------------------------
# B. who owns a vertex: a plane across one axis, one edge, every set of emitting cells
# ---------------------------------------------------------------------------------------------------------------
B_CENTRE = (0, 0, 0)
B_CUT = 3.87  # the plane lies between lattice points 3 and 4 of the axis, nearer to 3


def b_base(axis, others):
    """lattice base point of the edge: 3 along the axis, `others` on the two remaining axes (ascending axis order)"""
    b = list(others)
    b.insert(axis, 3)
    return tuple(b)


def b_kill_corner(axis, base, cell):
    """the corner of `cell` that is diagonal to the edge in both other axes, at the far end along the axis: not on the
    edge, not a gradient partner of the edge's nearer corner, and a corner of no other cell around the edge"""
    k = [0, 0, 0]
    for a in range(3):
        k[a] = 4 if a == axis else (base[a] + 1 if cell[a] == base[a] else base[a] - 1)
    return tuple(k)


def b_hood(axis, res=RES5):
    return Hood(B_CENTRE).fill(lambda x, y, z: ((x, y, z)[axis] + 0.5 - B_CUT) * float(res))


def b_subsets(axis, others):
    """-> [(emitters, Step)] for every non-empty subset of the cells around the edge, and the edge's slot"""
    base = b_base(axis, others)
    m = slot_of(axis, base)
    cells = slot_cells(m)
    out = []
    for mask in range(1, 1 << len(cells)):
        hood = b_hood(axis)
        keep = [c for i, c in enumerate(cells) if (mask >> i) & 1]
        dead = set()
        for i, (cell, e) in enumerate(cells):
            if not (mask >> i) & 1:
                k = b_kill_corner(axis, base, cell)
                hood.set(k, sdf=999.0)
                dead |= cells_with_corner(k)
        exp = expect(hood, dead=dead)
        what = "B axis %d edge %s emitters %s" % (axis, base, [c for c, e in keep])
        out.append((keep, Step(what, hood.chunks(), [hood.c], {hood.c: exp})))
    return m, cells, out


B_BORDERS = [(0, 4), (8, 4), (4, 0), (4, 8), (0, 0), (8, 8), (0, 8), (8, 0)]


def b_candidates(axis, others, res=RES5):
    """the vertex as each cell around the edge would round it"""
    hood = b_hood(axis, res)
    out = []
    for cell, e in slot_cells(slot_of(axis, b_base(axis, others))):
        g0 = tuple(cell[a] + CORNER[EDGE[e][0]][a] for a in range(3))
        g1 = tuple(cell[a] + CORNER[EDGE[e][1]][a] for a in range(3))
        out.append(vertex(hood.c, res, cell, e, hood.sdf(g0), hood.sdf(g1)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# C. edge validity: one negative voxel V in a positive field (an octahedron: 6 vertices, 8 triangles, one per cell
#    around V), V the nearer corner of all six edges unless the case says otherwise
# ---------------------------------------------------------------------------------------------------------------
NEG = -0.004
V3 = (3, 3, 3)
ABOVE_50 = np.nextafter(F(50.0), F(np.inf))
BELOW_1 = np.nextafter(F(1.0), F(0.0))
ABOVE_1 = np.nextafter(F(1.0), F(np.inf))


def step_of(v, axis, d):
    g = list(v)
    g[axis] += d
    return tuple(g)


def neighbours6(v):
    return [step_of(v, a, d) for a in range(3) for d in (-1, 1)]


def slots_at(v):
    """the six edge slots that end in lattice point v (those inside the chunk's edge grid)"""
    out = []
    for a in range(3):
        for d in (-1, 0):
            b = step_of(v, a, d)
            if all(0 <= b[i] <= 8 for i in range(3)) and b[a] <= 7:
                out.append(slot_of(a, b))
    return out


ALONE = [(0, 0, 0)]


def iso(centre=(0, 0, 0), v=V3, present=ALONE, **kw):
    return Hood(centre, present, **kw).set(v, sdf=NEG)


def cells_where_offset(v, axis, o):
    """the cells around v in which v sits at offset o along the axis"""
    return {c for c in cells_with_corner(v) if v[axis] - c[axis] == o}


def c_cases():
    """-> [(name, hood, Expect)], every hood at its own centre"""
    out = []
    k = [0]

    def centre():
        k[0] += 1
        return (4 * k[0] - 60, 3 * (k[0] % 5) - 4, -2 - (k[0] % 3))

    def add(name, hood, **kw):
        out.append((name, hood, expect(hood, **kw)))

    all6 = set().union(*[bad_slot(m) for m in slots_at(V3)])
    # weight of the nearer corner: > 50
    add("weight 50", iso(centre()).set(V3, w=50.0), bad=all6)
    add("weight above 50", iso(centre()).set(V3, w=ABOVE_50))
    h = iso(centre()).set(V3, w=ABOVE_50)
    for g in neighbours6(V3):
        h.set(g, w=50.0)
    add("near above 50, far 50", h)
    h = iso(centre()).set(V3, w=50.0)
    for g in neighbours6(V3):
        h.set(g, w=ABOVE_50)
    add("near 50, far above 50", h, bad=all6)
    # a tie |s0| == |s1|: corner e0 of the CELL's edge decides, and the cells around an edge name its ends differently
    for d in (1, -1):
        light = step_of(V3, 0, d)
        h = iso(centre()).set(light, sdf=-NEG, w=50.0)
        m = slot_of(0, V3 if d > 0 else light)
        bad = {(c, e) for c, e in slot_cells(m) if tuple(c[a] + CORNER[EDGE[e][0]][a] for a in range(3)) == light}
        assert len(bad) == 2
        add("tie, light corner at %+d" % d, h, bad=bad)
        h = iso(centre()).set(light, sdf=-NEG)  # (both heavy: the tie alone changes nothing)
        add("tie, both heavy, at %+d" % d, h)
    # the three outside partners, both cube offsets: < 1
    for axis in range(3):
        for o in (0, 1):
            for where in ("chunk", "face", "absent"):
                v = list(V3)
                if where != "chunk":
                    v[axis] = 7 if o else 0
                v = tuple(v)
                p, q = step_of(v, axis, 1 if o else -1), step_of(v, axis, -1 if o else 1)
                lost = cells_where_offset(v, axis, o)
                d = [0, 0, 0]
                d[axis] = 1 if o else -1
                if where == "absent":
                    h = iso(centre(), v)
                    dead = cells_with_corner(p)  # (o = 1: the cells that reach into the missing chunk)
                    add("partner axis %d offset %d in a missing chunk" % (axis, o), h, dead=dead, bad=bad_cells(lost))
                    continue
                for val in (F(1.0), BELOW_1):
                    h = iso(centre(), v, ALONE + ([tuple(d)] if where == "face" else [])).set(p, sdf=val).set(q, sdf=0.6)  # (0.6: the gradient stays below 100 res)
                    add("partner axis %d offset %d in the %s at %r" % (axis, o, where, float(val)), h,
                        bad=bad_cells(lost) if val == F(1.0) else ())
    # gradient norm: only x differs, |xp - xm| == 100 res passes, the next float fails
    lim = RES5 * F(100.0)
    xm = F(0.25)
    for name, dx in (("at", lim), ("above", np.nextafter(lim, F(np.inf)))):
        xp = xm + dx
        assert F(xp - xm) == dx and xp < 1 and float(xp) - float(xm) == float(dx)
        h = iso(centre()).set(step_of(V3, 0, -1), sdf=xm).set(step_of(V3, 0, 1), sdf=xp)
        add("gradient norm %s 100 res" % name, h, bad=all6 if name == "above" else ())
    # observed: a far corner of one cell at 1 / just above
    far = (4, 4, 4)
    add("far corner 1.0", iso(centre()).set(far, sdf=1.0))
    add("far corner above 1.0", iso(centre()).set(far, sdf=ABOVE_1), dead=cells_with_corner(far))
    # zeros: neither positive nor negative, a product that is not < 0
    for z in (0.0, -0.0):
        g = step_of(V3, 0, 1)
        add("corner %r" % z, iso(centre()).set(g, sdf=z), bad=bad_slot(slot_of(0, V3)))
    h = Hood(centre(), ALONE)
    for c in CORNER:
        h.set(tuple(3 + c[a] for a in range(3)), sdf=0.0)
    add("a cell of zeros", h)
    add("a cell of positives", Hood(centre(), ALONE))
    h = Hood(centre(), ALONE, sdf=0.0)
    add("a chunk of zeros", h)
    # products: denormal (a vertex), underflowing to zero (none), denormal corner values
    g = step_of(V3, 0, 1)
    add("product denormal", iso(centre()).set(V3, sdf=-1e-20).set(g, sdf=1e-20))
    add("product underflows", iso(centre()).set(V3, sdf=-1e-23).set(g, sdf=1e-23), bad=bad_slot(slot_of(0, V3)))
    add("corner denormal", iso(centre()).set(V3, sdf=-1e-40))
    add("both denormal", iso(centre()).set(V3, sdf=-1e-40).set(g, sdf=3e-41), bad=bad_slot(slot_of(0, V3)))
    return out


# ---------------------------------------------------------------------------------------------------------------
# D. vertex arithmetic and colour
# ---------------------------------------------------------------------------------------------------------------
APART = [(x, y, z) for z in (2, 5) for y in (2, 5) for x in (2, 5)]  # isolated voxels that share no neighbour either, all partners in the chunk
EVEN_INTERIOR = [(x, y, z) for z in (2, 4, 6) for y in (2, 4, 6) for x in (2, 4, 6)]
BIG = (1 << 20) - 2  # chunk ids are 21 bits per axis: -2^20 .. 2^20 - 1, and the face neighbours must be ids too
D_IDS = [(0, 0, 0), (-1, -3, -2), (BIG, -BIG, BIG - 1), (-BIG, BIG, 5)]


def d_cases(res):
    """t near 0 and near 1 by turns: |s0| is 10^4 times |s1| and the reverse, at chunk ids 0, small negative, +-(2^20 - 2)"""
    out = []
    for cid in D_IDS:
        h = Hood(cid, ALONE)
        for i, v in enumerate(APART):
            near, far = (-4e-7, 0.004) if i & 1 else (-0.004, 4e-7)
            h.set(v, sdf=near)
            for g in neighbours6(v):
                h.set(g, sdf=far)
        out.append(("t near 0 / 1 at %s" % (cid,), h, expect(h, res)))
    return out


D_COLOURS = [(123, 45, 6, 0), (0, 0, 0, 1), (65535, 65535, 65535, 1), (65535, 1, 30000, 65535), (255, 510, 765, 3)]


def d_colour_case(centre=(2, -7, 1)):
    """count 0 (white), count 1 with sums 0 and 65535, count 65535; V is the nearer corner of its six edges"""
    h = Hood(centre, ALONE)
    for v, col in zip(EVEN_INTERIOR, D_COLOURS):
        h.set(v, sdf=NEG, col=col)
    return "colour counts", h, expect(h, colours=True)


# ---------------------------------------------------------------------------------------------------------------
# E. adjacency flags (Mesh.cpp:52-83: floor((p - org) / res) <= 0 / >= 8 per axis)
# ---------------------------------------------------------------------------------------------------------------
def _e_hood(k, centre, sdf):
    axis = k >> 1
    v = list(V3)
    v[axis] = 7 if k & 1 else 1
    d = [0, 0, 0]
    d[axis] = 1 if k & 1 else -1
    return Hood(centre, ALONE + [tuple(d)]).set(tuple(v), sdf=sdf)


def e_flag_alone(k, centre):
    """one crossing a quarter cell inside face k (t = 0.25 from lattice point 0, or 0.75 from 7), every other vertex
    more than a cell away from every face -> only flag k"""
    h = _e_hood(k, centre, -0.03)  # |-0.03| = 3 x 0.01: the crossings sit a quarter from the neighbours
    adj = [0] * 6
    adj[k] = 1
    return "flag %d alone" % k, h, expect(h, adj=adj)


def e_id(k, j):
    return (4 * j * j - 30 + 300 * k, 3 * j - 10, 13 - 5 * j)


def e_half(k, j):
    """the same with the crossing at t = 0.5: the unrounded coordinate is exactly 1 / 8 cells from the origin, and one
    rounding decides floor() -- no answer stated for the flag, the oracle decides"""
    h = _e_hood(k, e_id(k, j), -0.01)
    return "flag %d, t = 0.5, chunk %s" % (k, h.c), h, expect(h)


def e_exchange():
    """-> [Step, Step]: pairs (A, B = A + x); A's mesh touches its +x face.  B has a mesh away from its faces / a mesh that
    is emptied in the second step / none.  After CompressMeshes flag +x of A == flag -x of B wherever B is in allMeshes."""
    hoods = []
    for i in range(3):
        h = Hood((10 * i, 0, 0), [(0, 0, 0), (1, 0, 0)]).set((7, 3, 3), sdf=-0.03)
        if i < 2:
            h.set((8 + 3, 3, 3), sdf=NEG)  # (3, 3, 3) of B
        hoods.append(h)
    ids = [h.c for h in hoods] + [step_of(h.c, 0, 1) for h in hoods]
    have = [(0, 0, 0), (10, 0, 0), (20, 0, 0), (1, 0, 0), (11, 0, 0)]

    def chunks():
        out = {}
        for h in hoods:
            out.update(h.chunks())
        return out

    first = Step("E exchange, first meshing", chunks(), ids, {}, only=have)
    hoods[1].set((8 + 3, 3, 3), sdf=0.01)
    exp = {h.c: Expect(6, 8, adj=[0, 1, 0, 0, 0, 0]) for h in hoods}
    exp[(1, 0, 0)] = Expect(6, 8, adj=[1, 0, 0, 0, 0, 0])
    exp[(11, 0, 0)] = Expect(0, 0, adj=[1, 0, 0, 0, 0, 0], key=True)
    exp[(21, 0, 0)] = NONE
    return [first, Step("E exchange, B emptied, compressed", chunks(), ids, exp, only=have, compress=True)]


# ---------------------------------------------------------------------------------------------------------------
# F. the mesh store at its capacities: isolated negative voxels on the even lattice (no two share a cell), the -x / -y
#    / -z neighbours present and positive: interior (6, 8), on one face (5, 4), on an edge (4, 2), at the corner (3, 1)
# ---------------------------------------------------------------------------------------------------------------
F_PRESENT = [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
EVEN = [(x, y, z) for z in (0, 2, 4, 6) for y in (0, 2, 4, 6) for x in (0, 2, 4, 6)]
F_KINDS = {n: [v for v in EVEN if sum(c == 0 for c in v) == n] for n in range(4)}  # by the number of zero coordinates
F_ADDS = {0: (6, 8), 1: (5, 4), 2: (4, 2), 3: (3, 1)}
# (nv, nt) -> (interior, face, edge, corner) voxels; blocks of 64 / 64: exactly full, one vertex past, triangles exactly
# full with room in the vertices, one triangle past
F_MIXES = {(64, 64): (4, 8, 0, 0), (65, 62): (5, 3, 5, 0), (48, 64): (8, 0, 0, 0), (51, 65): (8, 0, 0, 1)}
F_FIT = {(64, 64): True, (65, 62): False, (48, 64): True, (51, 65): False}


def f_case(counts, centre):
    h = Hood(centre, F_PRESENT)
    for kind, n in enumerate(counts):
        assert n <= len(F_KINDS[kind])
        if n:
            for v in F_KINDS[kind][::len(F_KINDS[kind]) // n][:n]:
                h.set(v, sdf=NEG)
    return h, expect(h)


def f_centre(want):
    i = list(F_MIXES).index(want)
    return (7 * i - 9, 2 - 4 * i, 3 * i)


def f_steps():
    """-> [Step, Step]: the four capacity cases; then a smaller field into the chunk that went past the vertices and an
    empty field into the chunk that was exactly full (it stays in allMeshes, without vertices)"""
    chunks, ids, exp = {}, [], {}
    for want, mix in F_MIXES.items():
        h, e = f_case(mix, f_centre(want))
        assert (e.nv, e.nt) == want, (want, e.nv, e.nt)
        chunks.update(h.chunks())
        ids.append(h.c)
        exp[h.c] = e
    first = Step("F capacities", chunks, ids, exp)
    chunks, exp = dict(chunks), dict(exp)
    h, e = f_case((2, 0, 0, 0), f_centre((65, 62)))
    chunks.update(h.chunks())
    exp[h.c] = e
    h = Hood(f_centre((64, 64)), F_PRESENT)
    chunks.update(h.chunks())
    exp[h.c] = Expect(0, 0, key=True)
    return [first, Step("F shrunk and emptied", chunks, ids, exp)]


# ---------------------------------------------------------------------------------------------------------------
# G. the filter: a chunk can have a vertex only if the 9^3 corner voxels hold an observed positive sdf, a negative
#    sdf and a weight above 50; the classes' only occurrence is one voxel of a +x / +y / +z neighbour
# ---------------------------------------------------------------------------------------------------------------
def g_positions(d):
    """lattice points of the centre that neighbour d contributes: coordinate 8 along the displaced axes; along the others
    mid-face, one coordinate 0, all 0"""
    free = [a for a in range(3) if not d[a]]
    out = []
    for zeros in range(len(free) + 1):
        g = [8 if d[a] else (3, 4, 5)[a] for a in range(3)]
        for a in free[:zeros]:
            g[a] = 0
        out.append(tuple(g))
    return out


G_CLASSES = ("negative", "positive", "heavy", "heavy at 50")


def g_case(cls, g, centre):
    """the class's only voxel at lattice point g of the centre (coordinate 9: one layer beyond what the centre's cells
    and the filter read)"""
    if cls == "negative":
        h = Hood(centre).set(g, sdf=NEG)
    elif cls == "positive":
        h = Hood(centre, sdf=-0.01).set(g, sdf=-NEG)
    else:
        h = Hood(centre, weight=50.0).set(g, sdf=NEG, w=ABOVE_50 if cls == "heavy" else 50.0)
    if max(g) > 8 or cls == "heavy at 50":
        return h, NONE
    return h, expect(h)


def g_class_steps(cls):
    """-> [Step]: every position of every + neighbour, and one layer beyond, side by side"""
    chunks, ids, exp = {}, [], {}
    k = 0
    for d in PLUS:
        for g in g_positions(d) + [tuple(9 if d[a] else (3, 4, 5)[a] for a in range(3))]:
            h, e = g_case(cls, g, (4 * (k % 6) - 10, 4 * ((k // 6) % 6) - 10, 3))
            k += 1
            chunks.update(h.chunks())
            ids.append(h.c)
            exp[h.c] = e
    return [Step("G class %s" % cls, chunks, ids, exp)]


def g_stale_steps():
    """the centre's only negative corner appears in a + neighbour that is re-uploaded while the centre alone is finalized,
    and disappears again the same way: nothing / a mesh / an empty mesh that stays in allMeshes"""
    hoods = [Hood((6 * i - 20, 2, 2)) for i in range(len(PLUS))]

    def step(what, exp):
        chunks = {}
        for h in hoods:
            chunks.update(h.chunks())
        return Step("G stale: " + what, chunks, [h.c for h in hoods], exp)

    steps = [step("nothing yet", {h.c: NONE for h in hoods})]
    for h, d in zip(hoods, PLUS):
        h.set(g_positions(d)[0], sdf=NEG)
    steps.append(step("appears", {h.c: expect(h) for h in hoods}))
    for h, d in zip(hoods, PLUS):
        h.set(g_positions(d)[0], sdf=0.01)
    steps.append(step("gone", {h.c: Expect(0, 0, key=True) for h in hoods}))
    return steps


def lone_chunk_fields(seed=7):
    """chunk contents from families A, C and F and the filter's classes, each meant for a chunk without neighbours"""
    rng = np.random.default_rng(seed)
    col = np.tile(np.array(COLOUR, np.uint16), 512)
    pool = []
    for s in range(4):
        sign = rng.integers(0, 2, 512) * 2 - 1
        pool.append(((sign * A_AMPL).astype(np.float32), np.full(512, 60.0, np.float32), col))
    for w in (50.0, ABOVE_50):
        pool.append(iso().set(V3, w=w).chunks()[(0, 0, 0)])
    h = Hood((0, 0, 0), ALONE)
    for v in F_KINDS[0][:8]:
        h.set(v, sdf=NEG)
    pool.append(h.chunks()[(0, 0, 0)])
    pool.append(Hood((0, 0, 0), ALONE).chunks()[(0, 0, 0)])                                    # all positive
    pool.append(Hood((0, 0, 0), ALONE, weight=50.0).set(V3, sdf=NEG).chunks()[(0, 0, 0)])      # no heavy voxel
    pool.append(Hood((0, 0, 0), ALONE, sdf=999.0).chunks()[(0, 0, 0)])                         # nothing observed
    pool.append(iso().set((4, 4, 4), sdf=ABOVE_1).chunks()[(0, 0, 0)])
    return pool


def g_forms_scene(n=1536, every=22):
    """n centre chunks three apart along every axis (no two share a face neighbour: 7 n distinct dirty ids, and room for a
    + 1 neighbour between them).  Most are lone chunks with contents in rotation; every `every`-th is the centre of a
    filter cluster (g_case: the class's only voxel in a + neighbour, at every position of g_class_steps, and one layer
    beyond) whose 26 neighbours are uploaded but not finalized.  -> Step with the clusters' known answers"""
    pool = lone_chunk_fields()
    ids = [(3 * (i % 16) - 24, 3 * ((i // 16) % 16) - 24, 3 * (i // 256)) for i in range(n)]
    chunks = {cid: pool[i % len(pool)] for i, cid in enumerate(ids)}
    clusters = [(cls, g) for cls in G_CLASSES[:3] for d in PLUS
                for g in g_positions(d) + [tuple(9 if d[a] else (3, 4, 5)[a] for a in range(3))]]
    assert every * len(clusters) <= n
    exp = {}
    for k, (cls, g) in enumerate(clusters):
        h, e = g_case(cls, g, ids[every * k])
        e = Expect(e.nv, e.nt, e.verts, e.indices, owners=e.owners)  # (a fresh one: NONE is shared)
        e.name = "cluster %s at %s" % (cls, g)
        chunks.update(h.chunks())
        exp[h.c] = e
    return Step("G forms", chunks, ids, exp)


G_BLOCK = (16, 16, 13)


def g_block_scene(every=4):
    """a solid block of chunks with a tilted, wavy sheet through every one of them: the same sheet in every chunk layer
    (a height between lattice planes 1 and 6, shifted from layer to layer), so that every chunk of the block survives the
    filter.  The height is constant over `every` x `every` voxels: a sparser field, less work per chunk.  -> (chunks, ids)"""
    nx, ny, nz = G_BLOCK
    col = np.tile(np.array(COLOUR, np.uint16), 512)
    w = np.full(512, 60.0, np.float32)
    zz, yy, xx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    chunks, ids = {}, []
    for cz in range(nz):
        for cy in range(ny):
            for cx in range(nx):
                gx, gy = (xx + 8 * cx) // every * every, (yy + 8 * cy) // every * every
                h = 3.6 + 2.0 * np.sin(0.05 * gx + 0.3 * cz) * np.cos(0.04 * gy)
                sdf = ((zz + 0.5 - h) * 0.005).clip(-0.02, 0.02).astype(np.float32).reshape(512)
                chunks[(cx, cy, cz)] = (sdf, w, col)
                ids.append((cx, cy, cz))
    return chunks, ids


# ---------------------------------------------------------------------------------------------------------------
# pool placement: a volume deals its slots in 64 stripes by a hash of the chunk id (chunk_acquire, tf_devfn.h), and its
# dirty list holds as many ids as its pool: a scene is known to fit the volume its test creates
# ---------------------------------------------------------------------------------------------------------------
def fits(steps, max_chunks):
    keys = set()
    for s in steps:
        keys |= set(s.chunks)
        dirty = {tuple(step_of(i, a, d)) for i in s.ids for a in range(3) for d in (-1, 1)} | set(s.ids)
        if len(dirty) > max_chunks:
            return False
    from tests.test_gpu_mesh_halo_edges import _stripe  # (the one restatement of chunk_acquire's hash; imported late:
    per = [0] * 64                                       # building the cases needs neither the oracle nor the library)
    for k in keys:
        per[_stripe(k)] += 1
    return max(per) <= max_chunks // 64


class Scene:
    def __init__(self, steps, max_chunks=1 << 8, res=RES5, **volume):
        self.steps, self.max_chunks, self.res, self.volume = steps, max_chunks, res, volume


def _side_by_side(what, cases):
    chunks, ids, exp = {}, [], {}
    for name, hood, e in cases:
        for k, f in hood.chunks().items():
            assert k not in chunks, "hoods overlap at %s" % (k,)
            chunks[k] = f
        ids.append(hood.c)
        exp[hood.c] = e
        e.name = name
    return [Step(what, chunks, ids, exp)]


SCENE_NAMES = ["A seed %d" % s for s in A_SEEDS] + ["A overflow pool", "F checkerboard"] + \
    ["B axis %d %s" % (a, w) for a in range(3) for w in ("interior", "borders")] + \
    ["C", "D res 5", "D res 10", "E alone", "E half", "E exchange", "F capacities"] + \
    ["G class %s" % c for c in G_CLASSES] + ["G stale"]
_SCENES = {}


def scene(name):
    if not _SCENES:
        _SCENES.update(scenes())
    return _SCENES[name]


def scenes():
    """name -> Scene, the cases both test modules run"""
    out = {}
    for seed in A_SEEDS:
        h, e = case_a(seed)
        out["A seed %d" % seed] = Scene([Step("A seed %d" % seed, h.chunks(), [h.c], {h.c: e})],
                                        mesh_max_vertices=2240, mesh_max_triangles=2560)
    h, e = case_a(A_SEEDS[0])
    out["A overflow pool"] = Scene([Step("A in the overflow pool", h.chunks(), [h.c], {h.c: e})],
                                   mesh_max_vertices=64, mesh_max_triangles=64, mesh_overflow_blocks=16)
    h, e = case_checkerboard()
    out["F checkerboard"] = Scene([Step("F checkerboard", h.chunks(), [h.c], {h.c: e})],
                                  mesh_max_vertices=64, mesh_max_triangles=64, mesh_overflow_blocks=16)
    for axis in range(3):
        steps = [s for keep, s in b_subsets(axis, (4, 4))[2]]
        out["B axis %d interior" % axis] = Scene(steps)
        steps = []
        for others in B_BORDERS:
            steps += [s for keep, s in b_subsets(axis, others)[2]]
        out["B axis %d borders" % axis] = Scene(steps)
    out["C"] = Scene(_side_by_side("C", c_cases()), max_chunks=1 << 10)
    out["D res 5"] = Scene(_side_by_side("D", d_cases(RES5) + [d_colour_case()]))
    out["D res 10"] = Scene(_side_by_side("D", d_cases(RES10)), res=RES10)
    steps = _side_by_side("E alone", [e_flag_alone(k, (5 * k - 12, 3, -4)) for k in range(6)])
    steps[0].compress = True
    out["E alone"] = Scene(steps)
    steps = _side_by_side("E half", [e_half(k, j) for k in range(6) for j in range(8)])
    steps[0].compress = True
    out["E half"] = Scene(steps, max_chunks=1 << 10)
    out["E exchange"] = Scene(e_exchange())
    out["F capacities"] = Scene(f_steps(), mesh_max_vertices=64, mesh_max_triangles=64, mesh_overflow_blocks=16)
    for cls in G_CLASSES:
        out["G class %s" % cls] = Scene(g_class_steps(cls), max_chunks=1 << 12)
    out["G stale"] = Scene(g_stale_steps(), max_chunks=1 << 12)
    return out
