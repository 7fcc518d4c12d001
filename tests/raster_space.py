"""The renderer space ("Raster space"): cases that put every coverage rule, draw path and boundary of
csrc/render.hip on the 1/256-px lattice, a scalar reference written from the header comment of render.hip and from pmn_hip.h (NOT from
render_ref.py), and one checker.  Test infrastructure: nothing in the product imports it.

The lattice.  The camera is E = I, K = diag(1/256, 1/256, 1); the world vertex (X z, Y z, z) then projects to exactly (X, Y) in units of
1/256 px whenever X z and Y z are exact float32 numbers: pc = the vertex itself, q.x = X z / 256, q.x / q.z = X / 256 is representable,
so the IEEE quotient is that number in float32 and in float64, and rintf(u * 256) = X.  Two domains are used: z a power of two in
2^-3 .. 2^5 with |X|, |Y| <= 2^22 + 1, and z = m / 8 with |X| m < 2^24 (8 <= m <= 1023 where |X| <= 2^13).  Every vertex a case plans
is checked for this when it is made, and check_plan() compares the plan with render_ref.project in both precisions.  The integers that
coverage is decided on are therefore the test's own, the float32 and float64 oracles agree on every pixel by construction, and NO pixel
is left out of any comparison.

Conditions the reference asserts on every case: the projection is exact; every exact c_i = b_i / z_i is far below float32 overflow; at
every pixel the two nearest candidates differ in exact depth by more than a relative 2^-20, or are the same snapped vertices and z in the
same vertex order (their depth bits are then equal and the lower index wins).  2^-20 is far above the depth bound, so a float32 z-buffer
and an exact one pick the same winner.

Depth bound.  There are seven roundings on the way to a triangle's depth: each c_i takes four (two int64-to-float conversions and two
divisions) in parallel, the sum two adds, the reciprocal one; all terms are non-negative, nothing cancels, the error is 7 u + O(u^2)
with u = 2^-24.  Asserted: |depth - exact| <= 8 * 2^-24 * exact.  A point's depth is pc.z bit for bit."""
from __future__ import annotations

import dataclasses
import functools
import math
from fractions import Fraction

import numpy as np

import render_ref as RR

GUARD = 1 << 22            # units of 1/256 px, drawn up to and including this
MAX_BOX = 64               # PMN_RASTER_MAX_BOX
SPLAT_MAX_RADIUS = 32      # PMN_SPLAT_MAX_RADIUS
MAX_BOXES = (0, 1, 1 << 40)  # every mesh case is drawn with each: the default split, everything on the worklist, nothing on it
DEPTH_BOUND = Fraction(8, 1 << 24)
SEPARATION = Fraction(1, 1 << 20)
K = np.diag([1 / 256, 1 / 256, 1]).astype(np.float32)
E = np.eye(4, dtype=np.float32)
CAM = np.concatenate((K.reshape(9), E[:3, :4].reshape(12))).astype(np.float32)
SUBNORMAL = float(np.float32(2.0 ** -149))


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    h: int
    w: int
    vertices: np.ndarray                 # [n,3] float32: the mesh's vertices or the cloud's points
    plan: list                           # per vertex (X, Y, state): what the projection must give
    faces: np.ndarray | None = None      # [m,3] int32; None: a cloud
    radius_px: float = 0.0
    radius_world: float = 0.0
    claims: dict = dataclasses.field(default_factory=dict)

    @property
    def id(self):
        return self.name.replace(" ", "-").replace("/", ":")


class Builder:
    """Collects vertices on the lattice (at) or as raw float32 triples with the state they must get (raw), and faces."""

    def __init__(self):
        self.v, self.plan, self.f = [], [], []

    def at(self, X, Y, z=1.0):
        assert z > 0 and float(np.float32(z)) == z, z
        X, Y, z = int(X), int(Y), float(z)
        xyz = np.float32([X * z, Y * z, z])  # the double products are exact; the condition is that their float32 roundings are too
        assert Fraction(float(xyz[0])) == X * Fraction(z) and Fraction(float(xyz[1])) == Y * Fraction(z), (X, Y, z)
        self.v.append(xyz)
        self.plan.append((X, Y, 0) if max(abs(X), abs(Y)) <= GUARD else (0, 0, 2))
        return len(self.v) - 1

    def raw(self, x, y, z, state):
        self.v.append(np.float32([x, y, z]))
        self.plan.append((0, 0, state))
        return len(self.v) - 1

    def tri(self, a, b, c, z=1.0):
        """A face on three new vertices; a, b, c are (X, Y) at depth ``z`` or (X, Y, z)."""
        self.f.append([self.at(*p) if len(p) == 3 else self.at(p[0], p[1], z) for p in (a, b, c)])
        return len(self.f) - 1

    def mesh(self, name, h, w, **claims):
        return Case(name, h, w, np.asarray(self.v, np.float32).reshape(-1, 3), list(self.plan), np.asarray(self.f, np.int32).reshape(-1, 3),
                    claims=claims)

    def cloud(self, name, h, w, radius_px=0.0, radius_world=0.0, **claims):
        return Case(name, h, w, np.asarray(self.v, np.float32).reshape(-1, 3), list(self.plan), None, radius_px, radius_world, claims)


def check_plan(case):
    """The projection is exact: render_ref.project returns the planned X, Y and state in float32 and in float64."""
    want = np.asarray(case.plan, np.int64).reshape(-1, 3)
    for T in (np.float32, np.float64):
        _, X, Y, state = RR.project(case.vertices, CAM, T)
        assert np.array_equal(X, want[:, 0]) and np.array_equal(Y, want[:, 1]) and np.array_equal(state, want[:, 2]), (case.name, T)


def attributes(case, seed=0, flat=None):
    """(colors [n,3] uint8, normals [n,3] float32 world) per vertex or point: seeded random, a fifth of the normals zero; ``flat``: one
    colour everywhere."""
    rng = np.random.default_rng(seed)
    n = len(case.vertices)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8) if flat is None else np.full((n, 3), flat, np.uint8)
    nrm = rng.integers(-4, 5, (n, 3)).astype(np.float32) / np.float32(4)
    nrm[rng.random(n) < 0.2] = 0
    return col, nrm


# ---- the scalar reference -------------------------------------------------------------------------------------------------------------

def _vertex(v):
    """(state, X, Y, z) of a float32 world vertex under CAM, as render.hip's header states r_project: pc is the vertex; NOT DRAWN
    (state 1) unless pc is finite and pc.z > 0; X = pc.x / pc.z in 1/256 px, state 2 unless |X|, |Y| <= 2^22."""
    x, y, z = (float(c) for c in v)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z) and z > 0):
        return 1, 0, 0, None
    X, Y = Fraction(x) / Fraction(z), Fraction(y) / Fraction(z)
    assert X.denominator == 1 and Y.denominator == 1 and max(abs(X), abs(Y)) < 1 << 24, "off the lattice"
    assert (x == 0 and y == 0) or z >= 2.0 ** -100, "x / 256 must not underflow"
    if abs(X) > GUARD or abs(Y) > GUARD:
        return 2, 0, 0, None
    return 0, int(X), int(Y), Fraction(z)


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


class Reference:
    """covered[t]: the set of (py, px) primitive t writes; hits, index [h,w]; depth [h,w] of Fractions (0 where nothing is drawn);
    boxes[t] = (width, height) of a drawn triangle's clipped box; incidences = (pixel, edge) pairs with w_i == 0 on the triangle's
    boundary on a top-left edge, on another edge, and pixels with two at once."""

    def __init__(self, case):
        self.h, self.w = case.h, case.w
        self.covered, self.boxes, self.cand = {}, {}, {}
        self.count = [0, 0, 0]
        self.incidences = [0, 0, 0]

    def put(self, t, py, px, depth, signature):
        self.covered[t].add((py, px))
        self.cand.setdefault((py, px), []).append((depth, t, signature))

    def finish(self, separated=True):
        h, w = self.h, self.w
        self.hits = np.zeros((h, w), np.int64)
        self.index = np.full((h, w), -1, np.int64)
        self.depth = np.zeros((h, w), object)
        for (py, px), c in self.cand.items():
            c.sort(key=lambda e: (e[0], e[1]))
            self.hits[py, px] = len(c)
            self.depth[py, px], self.index[py, px] = c[0][0], c[0][1]
            if separated and len(c) > 1:
                assert c[1][0] - c[0][0] > SEPARATION * c[0][0] or (c[0][2] is not None and c[0][2] == c[1][2]), \
                    ("two candidates too close in depth", py, px, c[0][1], c[1][1])
        del self.cand
        return self

    def counters(self, max_box=0):
        """(behind / non-finite / bad index, outside the band, zero area, boxes above max_box)"""
        cap = MAX_BOX if max_box == 0 else max_box
        return tuple(self.count) + (sum(bw * bh > cap for bw, bh in self.boxes.values()),)


def reference_mesh(case):
    """Per face: a bad index or a vertex of state 1 -> counter 0, else a vertex of state 2 -> counter 1, else area == 0 -> counter 2;
    else every centre of the clipped box with all s w_i > 0, or = 0 on a top-left edge, is covered at depth 1 / sum((s w_i / s area) /
    z_i), exactly.  Per-pixel loops over Python ints and Fractions; kept once per case."""
    if "ref" in case.__dict__:
        return case.ref
    ref = Reference(case)
    h, w = case.h, case.w
    verts = [_vertex(v) for v in case.vertices]
    nv = len(verts)
    for t, idx in enumerate(case.faces.tolist()):
        if any(i < 0 or i >= nv for i in idx):
            ref.count[0] += 1
            continue
        st = [verts[i] for i in idx]
        if any(s[0] == 1 for s in st):
            ref.count[0] += 1
            continue
        if any(s[0] == 2 for s in st):
            ref.count[1] += 1
            continue
        (X0, Y0, z0), (X1, Y1, z1), (X2, Y2, z2) = (s[1:] for s in st)
        area = _orient(X0, Y0, X1, Y1, X2, Y2)
        if area == 0:
            ref.count[2] += 1
            continue
        s = 1 if area > 0 else -1
        edges = ((X1, Y1, X2, Y2), (X2, Y2, X0, Y0), (X0, Y0, X1, Y1))  # edge i runs v1->v2, v2->v0, v0->v1
        top_left = [s * (e[3] - e[1]) < 0 or (e[3] == e[1] and s * (e[2] - e[0]) > 0) for e in edges]
        px0, px1 = max(-(-min(X0, X1, X2) // 256), 0), min(max(X0, X1, X2) // 256, w - 1)  # ceil and floor of the box, clipped
        py0, py1 = max(-(-min(Y0, Y1, Y2) // 256), 0), min(max(Y0, Y1, Y2) // 256, h - 1)
        ref.covered[t] = set()
        if px0 > px1 or py0 > py1:
            continue
        ref.boxes[t] = (px1 - px0 + 1, py1 - py0 + 1)
        zs = (z0, z1, z2)
        flat = z0 == z1 == z2 and 1 / z0 < 1 << 100
        signature = ((X0, Y0, z0), (X1, Y1, z1), (X2, Y2, z2))
        for py in range(py0, py1 + 1):
            for px in range(px0, px1 + 1):
                ws = [s * _orient(e[0], e[1], e[2], e[3], 256 * px, 256 * py) for e in edges]
                if min(ws) < 0:
                    continue
                zeros = [i for i in range(3) if ws[i] == 0]
                for i in zeros:
                    ref.incidences[0 if top_left[i] else 1] += 1
                ref.incidences[2] += len(zeros) == 2
                if not all(top_left[i] for i in zeros):
                    continue
                if flat:
                    depth = z0
                else:
                    c = [Fraction(ws[i], s * area) / zs[i] for i in range(3)]
                    assert max(c) < 1 << 100, ("a c_i near float32 overflow", t, py, px)
                    depth = 1 / sum(c)
                ref.put(t, py, px, depth, signature)
    case.ref = ref.finish()
    return case.ref


def reference_points(case):
    """The nearest pixel ((X + 128) >> 8, (Y + 128) >> 8) always and, with r > 0, every pixel with (256 px - X)^2 + (256 py - Y)^2 <=
    Rq^2, Rq = rintf(r * 256) (half to even), r = radius_px or min(radius_world * K_00 / pc.z, 32); depth = pc.z, index = the point's."""
    if "ref" in case.__dict__:
        return case.ref
    ref = Reference(case)
    h, w = case.h, case.w
    for t, v in enumerate(case.vertices):
        state, X, Y, z = _vertex(v)
        if state:
            ref.count[state - 1] += 1
            continue
        ref.covered[t] = set()
        if case.radius_world > 0:
            rw = Fraction(float(np.float32(case.radius_world)))
            for q in (rw, z):  # powers of two: (radius_world * K_00) / pc.z is exact in float32
                assert q.numerator == 1 or q.denominator == 1 and q.numerator & (q.numerator - 1) == 0
            r = min(rw * Fraction(float(CAM[0])) / z, SPLAT_MAX_RADIUS)
        else:
            r = Fraction(float(np.float32(case.radius_px)))
        Rq = round(r * 256)  # Fraction: half to even
        pixels = {((Y + 128) // 256, (X + 128) // 256)}
        for py in range(-(-(Y - Rq) // 256), (Y + Rq) // 256 + 1):
            for px in range(-(-(X - Rq) // 256), (X + Rq) // 256 + 1):
                if r > 0 and (256 * px - X) ** 2 + (256 * py - Y) ** 2 <= Rq * Rq:
                    pixels.add((py, px))
        for py, px in pixels:
            if 0 <= py < h and 0 <= px < w:
                ref.covered[t].add((py, px))
                ref.cand.setdefault((py, px), []).append((z, t, (X, Y, z)))
    case.ref = ref.finish(separated=False)  # a point's depth is exact in float32: equal depths are ties, the lowest index wins
    return case.ref


def reference(case):
    return reference_points(case) if case.faces is None else reference_mesh(case)


# ---- the float32 / float64 oracle of render_ref on a case -----------------------------------------------------------------------------

def oracle(case, dtype=np.float32, colors=None, normals=None, shade=False, rr=RR, max_box=0):
    """dict(depth [h,w] dtype, index, counters, rgb, normal) of render_ref (or a mutated copy ``rr``) on the case."""
    if case.faces is None:
        o = rr.splat_points(case.vertices, CAM, case.h, case.w, dtype, radius_px=case.radius_px, radius_world=case.radius_world)
        o["counters"] = tuple(o["counters"]) + (0, 0)
    else:
        o = rr.raster_triangles(case.vertices, case.faces, CAM, case.h, case.w, dtype, MAX_BOX if max_box == 0 else max_box)
    o["depth"] = o["depth"].astype(dtype)
    o["rgb"], o["normal"] = rr.resolve(o["depth"], o["index"], CAM, case.vertices, case.faces, dtype, colors, normals, shade)
    return o


# ---- the checker ----------------------------------------------------------------------------------------------------------------------

def check(case, got, ref, o32=None, max_box=0, stats=None):
    """A list of failures (empty: passed).  ``got``: dict(depth [h,w] float32, index [h,w], counters [4], rgb | None, normal | None).
    ``o32``: the float32 oracle's dict; then depth, index, rgb and normal must be byte-equal to it on every pixel.  ``stats``, if a
    dict, receives 'differ' (pixels that differ from o32) and 'depth' (worst depth error over its bound)."""
    fails = []
    mesh = case.faces is not None
    depth = np.asarray(got["depth"])
    index = np.asarray(got["index"]).astype(np.int64)
    if depth.dtype != np.float32:
        fails.append(f"depth is {depth.dtype}")
        depth = depth.astype(np.float32)
    bad = index != ref.index
    if bad.any():
        py, px = np.argwhere(bad)[0]
        fails.append(f"index differs on {int(bad.sum())} px, first ({py}, {px}): got {index[py, px]}, reference {ref.index[py, px]}")
    want = tuple(ref.counters(max_box)) if mesh else tuple(ref.count[:2]) + (0, 0)
    if tuple(int(c) for c in got["counters"][:4]) != want:
        fails.append(f"counters {tuple(int(c) for c in got['counters'][:4])}, reference {want}")
    miss = index < 0
    if (depth[miss].view(np.uint32) != 0).any():
        fails.append("a missed pixel holds a depth other than +0")
    for k in ("rgb", "normal"):
        if got.get(k) is not None and np.asarray(got[k])[miss].view(np.uint8).any():
            fails.append(f"a missed pixel holds a non-zero {k}")
    worst = 0.0
    for py, px in np.argwhere(~miss & ~bad):
        exact, d = ref.depth[py, px], Fraction(float(depth[py, px]))
        if mesh:
            worst = max(worst, float(abs(d - exact) / (DEPTH_BOUND * exact)))
        elif d != exact:
            fails.append(f"point depth at ({py}, {px}) is {float(d)!r}, pc.z is {float(exact)!r}")
            break
    if worst > 1:
        fails.append(f"triangle depth error is {worst:.3f} x the bound 8 * 2^-24 relative")
    differ = 0
    if o32 is not None:
        d32 = o32["depth"].astype(np.float32)
        differ = int(((index != o32["index"]) | (depth.view(np.uint32) != d32.view(np.uint32))).sum())
        if differ:
            fails.append(f"depth / index differ from the float32 oracle's bytes on {differ} px")
        for k in ("rgb", "normal"):
            if got.get(k) is not None and np.asarray(got[k]).tobytes() != o32[k].tobytes():
                n = int((np.asarray(got[k]).reshape(case.h, case.w, -1).view(np.uint8) != o32[k].reshape(case.h, case.w, -1).view(np.uint8)).any(2).sum())
                differ = max(differ, n)
                fails.append(f"{k} differs from the float32 oracle's bytes on {n} px")
    if stats is not None:
        stats["differ"] = max(stats.get("differ", 0), differ)
        stats["depth"] = max(stats.get("depth", 0.0), worst)
    return fails


check_mesh = check_points = check


# ---- triangles: the families ----------------------------------------------------------------------------------------------------------

RING16 = [(2, 0), (2, 1), (2, 2), (1, 2), (0, 2), (-1, 2), (-2, 2), (-2, 1), (-2, 0), (-2, -1), (-2, -2), (-1, -2), (0, -2), (1, -2),
          (2, -2), (2, -1)]
FAN_STEP = 384  # 1.5 px: rim vertices on centres and on half pixels
FAN_HUBS = {"on-centre": 0, "half-pixel": 128, "off-centre": 77}


@functools.lru_cache(None)
def fans():
    """Per fan: (together, [each triangle alone], inside [h,w] bool: the centres strictly inside the square outline)."""
    out = []
    h, w = 9, 10
    for n in (8, 16):
        ring = RING16[::16 // n]
        for hub_name, off in FAN_HUBS.items():
            hx = hy = 4 * 256 + off
            rim = [(hx + FAN_STEP * dx, hy + FAN_STEP * dy) for dx, dy in ring]
            py, px = np.mgrid[0:h, 0:w] * 256
            inside = (np.abs(px - hx) < 2 * FAN_STEP) & (np.abs(py - hy) < 2 * FAN_STEP)
            for winding in (1, -1):
                name = f"fan of {n} {hub_name} winding {winding:+d}"
                tris = [((hx, hy), rim[i], rim[(i + 1) % n])[::winding] for i in range(n)]
                b = Builder()
                singles = []
                for i, t in enumerate(tris):
                    b.tri(*t)
                    one = Builder()
                    one.tri(*t)
                    singles.append(one.mesh(f"{name} triangle {i}", h, w))
                out.append((b.mesh(name, h, w), singles, inside))
    return out


def _snap(rng, v):
    u = rng.random(v.shape)
    return np.where(u < 0.4, (v + 128) // 256 * 256, np.where(u < 0.7, (v + 64) // 128 * 128, v))


@functools.lru_cache(None)
def soup():
    """About 1000 fronto-parallel triangles, triangle t at z = (8 + t) / 8, a large share of the vertices on pixel centres and half
    pixels, so that hundreds of centres lie exactly on edges and on vertices."""
    rng = np.random.default_rng(1)
    b = Builder()
    for t in range(1000):
        centre = rng.integers(-256, 33 * 256, 2)
        p = np.clip(_snap(rng, centre + rng.integers(-768, 769, (3, 2))), -(1 << 13), 1 << 13)
        b.tri(*(tuple(q) for q in p.tolist()), z=(8 + t) / 8)
    return b.mesh("soup", 33, 33)


@functools.lru_cache(None)
def perspective():
    """Tilted triangles with three different z = m / 8; triangle k takes its m from 40 k + 8 .. 40 k + 47, so no two intersect."""
    rng = np.random.default_rng(2)
    b = Builder()
    for k in range(24):
        p = _snap(rng, rng.integers(-512, 34 * 256 - 512, (3, 2)))
        m = 40 * k + 8 + rng.choice(40, 3, replace=False)
        b.tri(*((int(q[0]), int(q[1]), int(mm) / 8) for q, mm in zip(p, m)))
    return b.mesh("perspective", 33, 33)


@functools.lru_cache(None)
def degenerates():
    b = Builder()
    claims = {"zero": [], "sliver": [], "corner": []}
    claims["zero"].append(b.tri((0, 0), (300, 300), (900, 900)))                      # collinear, distinct
    claims["zero"].append(b.tri((256, 512), (256, 512), (1000, 90)))                  # two equal vertices
    a, c = b.at(512, 512), b.at(1500, 700)
    b.f.append([a, a, c])                                                              # a repeated index
    claims["zero"].append(len(b.f) - 1)
    for p in (((10, 10), (2000, 30), (1000, 21)), ((300, 1), (300, 2500), (301, 1200)), ((260, 260), (500, 505), (400, 403))):
        claims["sliver"].append(b.tri(*p, z=2.0))                                      # area != 0, no centre inside
    n = 0
    for sx in (1, -1):          # a right angle at a pixel centre, the triangle in each of the four quadrants, both windings:
        for sy in (1, -1):      # only the one whose corner is its own top-left vertex covers it
            for winding in (1, -1):
                cx, cy = 256 * (3 + 3 * (n % 4)), 256 * (3 + 4 * (n // 4))
                claims["corner"].append(b.tri(*((cx, cy), (cx + sx * 100, cy), (cx, cy + sy * 100))[::winding], z=4.0))
                n += 1
    return b.mesh("degenerates", 12, 16, **claims)


@functools.lru_cache(None)
def not_drawn():
    b = Builder()
    G = GUARD

    def face(v, z=1.0):  # v with two ordinary vertices
        b.f.append([v, b.at(256, 256, z), b.at(1024, 512, z)])
        return len(b.f) - 1
    claims = {"behind": [], "band": [], "drawn": []}
    claims["drawn"].append(b.tri((100, 100), (2000, 300), (700, 1900), z=8.0))
    for z in (0.0, -0.0, -1.0, -SUBNORMAL):
        claims["behind"].append(face(b.raw(0.0, 0.0, z, 1)))
    for xyz in ((np.nan, 0, 1), (0, np.nan, 1), (0, 0, np.nan), (np.inf, 0, 1), (0, -np.inf, 1), (0, 0, np.inf), (0, 0, -np.inf)):
        claims["behind"].append(face(b.raw(*xyz, 1)))
    # a positive subnormal z is in front of the camera and finite: the vertex (0, 0, 2^-149) is DRAWN, at X = Y = 0.  The far edge
    # lies on y - x = 256 and runs through centres, where the vertex's weight is 0 (c_0 = 0 exactly, the depth is the other
    # vertices'); no centre lies strictly between that edge and the apex, and the reference asserts that the apex pixel itself is
    # not covered (there c_0 would overflow in float32 and not in float64; on the other side of the apex it is covered).
    claims["subnormal"] = []
    for p, q, z in (((-512, -256), (768, 1024), 1.0), ((768, 1024), (-256, 0), 2.0)):
        b.f.append([b.raw(0.0, 0.0, SUBNORMAL, 0), b.at(*p, z), b.at(*q, z)])
        claims["subnormal"].append(len(b.f) - 1)
    for z in (2.0, 0.125):
        claims["drawn"].append(b.tri((G, -300), (-300, -300), (-300, G), z=z))        # |X|, |Y| == 2^22: drawn
        claims["drawn"].append(b.tri((-G, 2000), (2000, 2000), (2000, -G), z=z * 2))
        claims["band"].append(b.tri((G + 1, -300), (-300, -300), (-300, G), z=z))     # 2^22 + 1: counter 1
        claims["band"].append(b.tri((G, -300), (-300, -300), (-300, -(G + 1)), z=z))
    b.f.append([b.raw(0.0, 0.0, -2.0, 1), b.at(G + 1, 0, 1.0), b.at(256, 256)])        # behind AND out of band: counter 0 only
    claims["behind"].append(len(b.f) - 1)
    b.f.append([b.at(G + 1, 0, 1.0), b.at(256, 256), b.raw(np.nan, 0.0, 1.0, 1)])
    claims["behind"].append(len(b.f) - 1)
    nv = len(b.v)
    for bad in ([-1, 0, 1], [0, nv, 1], [0, 1, 2 ** 31 - 1], [-2 ** 31, 0, 1]):
        b.f.append(bad)
        claims["behind"].append(len(b.f) - 1)
    return b.mesh("not drawn", 9, 9, **claims)


VIEWS = [(1, 1), (1, 70), (70, 1), (5, 65), (9, 64), (4, 63)]
STRIPS = [(1, 16384), (16384, 1)]


@functools.lru_cache(None)
def clipping():
    """Per view: triangles straddling each border and corner, wholly outside on each side, and one containing the whole view."""
    out = []
    for h, w in VIEWS:
        b = Builder()
        R, B = 256 * (w - 1), 256 * (h - 1)   # the last column's and row's centres
        mx, my = R // 2, B // 2
        m = iter(range(8, 64))
        z = lambda: next(m) / 8
        for cx, cy in ((0, my), (R, my), (mx, 0), (mx, B)):                             # borders
            b.tri((cx - 400, cy - 300), (cx + 350, cy + 10), (cx - 20, cy + 380), z=z())
        for cx, cy in ((0, 0), (R, 0), (0, B), (R, B)):                                 # corners
            b.tri((cx - 300, cy - 400), (cx + 380, cy - 20), (cx + 10, cy + 350), z=z())
        outside = [b.tri((-900, my - 300), (-300, my), (-700, my + 300), z=z()),        # px1 < 0 <= px0
                   b.tri((R + 900, my - 300), (R + 1, my), (R + 700, my + 300), z=z()),  # px0 > w - 1
                   b.tri((mx - 300, -900), (mx, -1), (mx + 300, -700), z=z()),
                   b.tri((mx - 300, B + 900), (mx, B + 255), (mx + 300, B + 700), z=z()),
                   b.tri((-257, -257), (-1, -200), (-200, -1), z=z())]
        whole = b.tri((-1024, -1024), (2 * R + 2048, -1024), (-1024, 2 * B + 2048), z=z())
        out.append(b.mesh(f"clipping {h}x{w}", h, w, outside=outside, whole=whole))
    return out


@functools.lru_cache(None)
def strips():
    """The 16384-pixel limit the guard band is designed around: one triangle from band edge to band edge over a one-row / one-column view."""
    G = GUARD
    a, b = Builder(), Builder()
    a.tri((-G, -256), (G, -256), (0, G), z=2.0)
    b.tri((-256, -G), (G, 0), (-256, G), z=0.5)
    return [a.mesh("strip 1x16384", 1, 16384), b.mesh("strip 16384x1", 16384, 1)]


BOX_WIDTHS, BOX_HEIGHTS = (1, 7, 8, 9, 17), (1, 7, 8, 9, 63, 64, 65, 129)


@functools.lru_cache(None)
def box_matrix():
    """Per width a case with one triangle per height whose clipped bounding box is exactly width x height; with max_box = 1 all but
    the 1 x 1 box take the worklist path: tile and slice tails (a tile is 8 x 8, a slice every 64th row of tiles)."""
    out = []
    for bw in BOX_WIDTHS:
        b = Builder()
        want = []
        for j, bh in enumerate(BOX_HEIGHTS):
            x0, y0 = 3 + 5 * j, (129 - bh) // 2 if bh < 129 else 0
            X0, X1 = 256 * x0 - 100, 256 * (x0 + bw - 1) + 50
            Y0, Y1 = 256 * y0 - 30, 256 * (y0 + bh - 1) + 99
            want.append((b.tri((X0, Y0), (X1, Y0), ((X0 + X1) // 2, Y1), z=(8 + j) / 8), (bw, bh)))
        out.append(b.mesh(f"boxes of width {bw}", 129, 70, boxes=want))
    return out


WORKLIST_LENGTHS = (1, 63, 64, 65, 257, 1100)


@functools.lru_cache(None)
def worklists():
    """n triangles with a 9 x 9 box (81 > 64 pixels: the worklist at the default max_box) with 0, 1 or 2 small or undrawable triangles
    between them, so that a wave's ballot holds a partial set at varying lanes.  1100 x 8 slices = 8800 items exceed the 8192 waves of
    raster_large_kernel: its stride loop takes a second round."""
    out = []
    for n in WORKLIST_LENGTHS:
        b = Builder()
        large = []
        for i in range(n):
            slot, layer = i % 98, i // 98
            X, Y = 256 * (9 * (slot % 7) + 1), 256 * (9 * (slot // 7) + 1)
            large.append(b.tri((X, Y), (X + 2048, Y + layer), (X + 3 * layer, Y + 2048), z=(8 + layer) / 8))
            for k in range(i % 3):
                kind = (i + k) % 5
                if kind == 0:
                    b.tri((X + 200, Y + 200), (X + 600, Y + 250), (X + 300, Y + 590), z=(40 + layer) / 8)  # small: a 2 x 2 box
                elif kind == 1:
                    b.f.append([b.raw(0.0, 0.0, -1.0, 1), b.at(X, Y), b.at(X + 256, Y)])
                elif kind == 2:
                    b.tri((GUARD + 1, 0, 1.0), (X, Y, 1.0), (X, Y + 256, 1.0))
                elif kind == 3:
                    b.tri((X, Y), (X + 256, Y + 256), (X + 512, Y + 512))
                else:
                    b.f.append([b.at(X, Y), -1, b.at(X + 256, Y)])
        out.append(b.mesh(f"worklist of {n}", 129, 70, large=large))
    return out


@functools.lru_cache(None)
def zbuffer():
    """The same triangle at indices i < j (on separate, equal vertices) with another between them, and with the two copies swapped;
    a nearer triangle with the higher index; a nearer one with the lower index."""
    out = []
    T = ((300, 200), (2500, 700), (900, 2600))
    for name in ("copies", "copies swapped"):
        b = Builder()
        first = [b.at(*p, 2.0) for p in T]
        second = [b.at(*p, 2.0) for p in T]
        if name.endswith("swapped"):
            first, second = second, first
        b.f.append(first)
        b.tri((100, 1500), (2800, 1400), (1500, 2900), z=4.0)
        b.f.append(second)
        b.tri((1000, 100), (2000, 2000), (200, 1200), z=1.0)       # nearer, higher index
        b.tri((2000, 100), (2900, 2900), (1200, 1500), z=8.0)      # farther, higher index
        out.append(b.mesh(name, 12, 12, copies=(0, 2)))
    return out


def mesh_cases():
    """Every mesh case (the fans together; their single triangles are drawn by their own test)."""
    return ([f[0] for f in fans()] + [soup(), perspective(), degenerates(), not_drawn()] + clipping() + strips() + box_matrix() +
            worklists() + zbuffer())


def permuted(case, seed=0):
    """(the case with its faces or points permuted, perm): primitive i of the new case is primitive perm[i] of the old one."""
    perm = np.random.default_rng(seed).permutation(len(case.vertices) if case.faces is None else len(case.faces))
    if case.faces is None:
        c = dataclasses.replace(case, name=case.name + " permuted", vertices=np.ascontiguousarray(case.vertices[perm]),
                                plan=[case.plan[i] for i in perm], claims={})
    else:
        c = dataclasses.replace(case, name=case.name + " permuted", faces=np.ascontiguousarray(case.faces[perm]), claims={})
    c.__dict__.pop("ref", None)
    return c, perm


# ---- points: the families -------------------------------------------------------------------------------------------------------------

def _nearest_values(n):
    return [-129, -128, -1, 0, 127, 128, 129, 256 * (n - 1) + 127, 256 * (n - 1) + 128]


@functools.lru_cache(None)
def nearest():
    """(X + 128) >> 8 on both sides of every threshold, for negative X too, and at the last column and row: all 81 combinations, once
    with equal depths (the lowest index wins a pixel) and once with distinct ones."""
    h, w = 4, 5
    out = []
    for name in ("equal depths", "distinct depths"):
        b = Builder()
        for i, Y in enumerate(_nearest_values(h)):
            for j, X in enumerate(_nearest_values(w)):
                b.at(X, Y, 1.0 if name[0] == "e" else (8 + (37 * (9 * i + j)) % 81) / 8)
        out.append(b.cloud(f"nearest pixel {name}", h, w))
    return out


RADII_PX = (127 / 256, 127.5 / 256, 128.5 / 256, 129.5 / 256, 0.5, 1.0, 5.0, 32.0)


def _disc_points(b, h, w, Rq, z):
    R, B = 256 * (w - 1), 256 * (h - 1)
    mx, my = (w // 2) * 256, (h // 2) * 256
    spots = [(mx, my), (mx + 128, my), (mx, my - 128), (mx + 128, my + 128), (mx + 77, my - 33),          # centre, half pixels, general
             (-Rq // 2, my), (R + Rq // 2, my), (mx, -Rq // 2), (mx, B + Rq // 2),                       # clipped at every border
             (-Rq // 2, -Rq // 2), (R + Rq // 3, -Rq // 2), (-Rq // 3, B + Rq // 2), (R + Rq // 2, B + Rq // 2),  # and corner
             (-Rq, my), (-Rq - 1, my), (mx, B + Rq), (mx, B + Rq + 1), (R + Rq, B), (R + Rq + 1, B)]     # just touching, just not
    for X, Y in spots:
        b.at(X, Y, z())


@functools.lru_cache(None)
def radii():
    """radius_px on both sides of the Rq < 128 branch and of rintf's ties, and Rq = 1280, where (+-3, +-4) px lie exactly on the disc."""
    out = []
    for r in RADII_PX:
        Rq = round(Fraction(float(np.float32(r))) * 256)
        n = 2 * math.ceil(r) + 5
        b = Builder()
        m = iter(range(8, 200))
        _disc_points(b, n, n + 1, Rq, lambda: next(m) / 8)
        out.append(b.cloud(f"radius_px {r * 256:g}/256", n, n + 1, radius_px=r, Rq=Rq))
    return out


@functools.lru_cache(None)
def radius_world():
    """K_00 = 2^-8, z and radius_world powers of two: r = radius_world * K_00 / z is exact.  Below the clamp, exactly at
    PMN_SPLAT_MAX_RADIUS and above it."""
    out = []
    for rw in (4096.0, 8192.0, 16384.0):
        b = Builder()
        zs = iter([1.0, 2.0, 0.5, 4.0, 0.25] * 8)
        _disc_points(b, 69, 70, 4096, lambda: next(zs))
        want = sorted({min(Fraction(rw) / 256 / Fraction(z), SPLAT_MAX_RADIUS) for z in (1.0, 2.0, 0.5, 4.0, 0.25)})
        out.append(b.cloud(f"radius_world {rw:g}", 69, 70, radius_world=rw, radii=want))
    return out


CLOUD_SIZES = (1, 63, 64, 65, 257, 1000)


@functools.lru_cache(None)
def clouds():
    """n points (one block, a wave and its neighbours, several blocks) with a 1-px disc, and some behind, non-finite and out of band."""
    out = []
    for n in CLOUD_SIZES:
        rng = np.random.default_rng(n)
        m = 8 + rng.permutation(1016)  # distinct depths: no two different points tie
        b = Builder()
        for i in range(n):
            u = i % 23
            if n > 1 and u == 5:
                b.raw(1.0, 2.0, float(rng.choice([0.0, -0.0, -3.0])), 1)
            elif n > 1 and u == 11:
                b.raw(*rng.permutation([np.nan, 1.0, 1.0]).tolist(), 1) if i % 2 else b.raw(np.inf, 0.0, 1.0, 1)
            elif n > 1 and u == 17:
                b.at(GUARD + 1, 0, 1.0) if i % 2 else b.at(300, -(GUARD + 1), 0.5)
            else:
                X, Y = _snap(rng, rng.integers(-512, 33 * 256 + 512, 2))
                b.at(int(X), int(Y), int(m[i]) / 8)
        out.append(b.cloud(f"cloud of {n}", 33, 33, radius_px=1.0))
    return out


@functools.lru_cache(None)
def ties():
    """Equal-depth points on one pixel (different sub-pixel positions): the lower index wins; a nearer point with a higher index wins."""
    b = Builder()
    for X, Y, z in ((512, 512, 2.0), (520, 500, 2.0), (512, 512, 2.0), (600, 480, 4.0), (1024, 1024, 2.0), (1030, 1000, 1.0),
                    (1536, 512, 1.0), (1500, 530, 2.0), (1536, 512, 1.0)):
        b.at(X, Y, z)
    return [b.cloud("ties nearest", 8, 8), b.cloud("ties radius 1", 8, 8, radius_px=1.0)]


def point_cases():
    return nearest() + radii() + radius_world() + clouds() + ties()


def lattice_cases():
    """The cases resolve is run on: small meshes and clouds whose every covered pixel has interpolated attributes."""
    return [fans()[0][0], perspective(), degenerates(), not_drawn(), zbuffer()[0]] + clipping() + [radii()[5], clouds()[3], ties()[1]]
