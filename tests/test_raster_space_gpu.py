"""GPU checks of the renderer space (tests/raster_space.py; DESIGN.md section 16, "Raster space"): every case through
render.Renderer (and ops.raster_resolve where a raw call is needed) against the scalar reference and, byte for byte, the float32 oracle
of tests/render_ref.py.  tests/test_raster_space.py has shown on the CPU that the cases hold what they claim, that the reference and
the oracle agree on every pixel of every case in float32 and float64, and that the checker reports eight planted defects; a failure
here is the kernels' (or the stated definition's).

Gates (raster_space.check): index equal to the exact reference on EVERY pixel (no pixel is excluded anywhere); missed pixels hold depth
+0, index -1, rgb 0, normal 0; counters equal, counter 3 being the reference's count of boxes above the call's max_box; triangle depth
within 8 * 2^-24 relative of the exact depth (seven roundings, no cancellation); point depth = pc.z bit for bit; depth, index, rgb and
normal byte-equal to the float32 oracle.  Mesh cases are drawn with max_box 0 (the default 64), 1 and 2^40: equal planes.  Each test
prints the pixels that differ from the float32 oracle (0 required) and the worst depth error over its bound."""
import numpy as np
import pytest
import torch

import raster_space as S

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests selected but no ROCm device is visible"
    return torch.device("cuda")


def _up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_RENDERER = []


def _renderer():
    from patchmatchnet_amd import render
    if not _RENDERER:
        _RENDERER.append(render.Renderer(_dev()))
    return _RENDERER[0]


def _draw(case, max_box=0, colors=None, normals=None, shade=True, rgb=True, normal=True):
    r = _renderer()
    dev = r.device
    v, col, nrm = _up(case.vertices, dev), _up(colors, dev), _up(normals, dev)
    if case.faces is None:
        out = r.render_points(v, S.K, S.E, case.h, case.w, col, nrm, case.radius_px, case.radius_world, shade, rgb, normal)
    else:
        out = r.render_mesh(v, _up(case.faces, dev), S.K, S.E, case.h, case.w, col, nrm, shade, rgb, normal, max_box)
    host = [None if t is None else t.cpu().numpy().copy() for t in out]
    return dict(depth=host[0], index=host[1], rgb=host[2], normal=host[3], counters=host[4].tolist())


def _run(case, stats, seed=0):
    """The case with attributes, at every max_box if it is a mesh: all gates, and the planes equal across max_box."""
    ref = S.reference(case)
    col, nrm = S.attributes(case, seed)
    o32 = S.oracle(case, np.float32, col, nrm, True)
    first = None
    for max_box in (S.MAX_BOXES if case.faces is not None else (0,)):
        got = _draw(case, max_box, col, nrm)
        fails = S.check(case, got, ref, o32, max_box, stats)
        assert not fails, (case.name, max_box, fails)
        first = first or got
        assert got["depth"].tobytes() == first["depth"].tobytes() and got["index"].tobytes() == first["index"].tobytes(), (case.name, max_box)
        assert got["counters"][:3] == first["counters"][:3]
    return first


def _report(name, stats):
    print(f"{name}: {stats.get('differ', 0)} px differ from the float32 oracle (0 required), worst depth error / bound "
          f"{stats.get('depth', 0.0):.3f} (1 allowed)")
    assert stats.get("differ", 0) == 0 and stats.get("depth", 0.0) <= 1


@pytest.mark.parametrize("fan", S.fans(), ids=lambda f: f[0].id)
def test_top_left_rule_on_fans(fan):
    """Every triangle of the fan alone covers the reference's set; together they cover every centre inside the outline exactly once."""
    together, singles, inside = fan
    stats = {}
    hits = np.zeros((together.h, together.w), np.int64)
    for n, c in enumerate(singles):
        got = _draw(c, S.MAX_BOXES[n % 3], rgb=False, normal=False)
        fails = S.check(c, got, S.reference(c), S.oracle(c), S.MAX_BOXES[n % 3], stats)
        assert not fails, (c.name, fails)
        covered = {(int(py), int(px)) for py, px in np.argwhere(got["index"] >= 0)}
        assert covered == S.reference(c).covered[0], c.name
        hits += got["index"] >= 0
    assert (hits[inside] == 1).all() and hits.max() == 1 and np.array_equal(hits, S.reference(together).hits)
    _run(together, stats)
    _report(together.name, stats)


MESHES = ([S.soup(), S.perspective(), S.degenerates(), S.not_drawn()] + S.clipping() + S.strips() + S.box_matrix() + S.worklists() +
          S.zbuffer())


@pytest.mark.parametrize("case", MESHES, ids=lambda c: c.id)
def test_mesh_case_on_both_paths(case):
    stats = {}
    got = _run(case, stats)
    if "large" in case.claims:
        assert got["counters"][3] == len(case.claims["large"])
    _report(case.name, stats)


@pytest.mark.parametrize("case", S.point_cases(), ids=lambda c: c.id)
def test_point_case(case):
    stats = {}
    _run(case, stats)
    _report(case.name, stats)


@pytest.mark.parametrize("case", [S.soup(), S.perspective(), S.worklists()[4], S.box_matrix()[4], S.clouds()[5], S.radii()[6]],
                         ids=lambda c: c.id)
def test_permuted_primitives_map_back(case):
    """No two different primitives tie in these cases: a permutation gives the same depth bytes and, mapped back, the same winners."""
    stats = {}
    a = _draw(case, rgb=False, normal=False)
    for seed in (1, 2):
        p, perm = S.permuted(case, seed)
        b = _run(p, stats, seed)
        assert a["depth"].tobytes() == b["depth"].tobytes()
        assert np.array_equal(np.where(b["index"] >= 0, perm[np.maximum(b["index"], 0)], -1), a["index"])
    _report(case.name, stats)


def test_equal_depth_ties_go_to_the_lower_index():
    stats = {}
    for case in S.zbuffer() + S.ties() + [S.nearest()[0]]:
        got = _run(case, stats)
        p, perm = S.permuted(case, 5)
        b = _run(p, stats)
        assert b["depth"].tobytes() == got["depth"].tobytes()
        if "copies" in case.claims:
            i, j = case.claims["copies"]
            assert (got["index"] == i).any() and not (got["index"] == j).any()
    _report("ties", stats)


VARIANTS = [dict(colors=c, normals=n, shade=s) for c in ("random", None) for n in ("random", None) for s in (True, False)] + \
           [dict(colors="random", normals="random", shade=True, rgb=False), dict(colors="random", normals="random", shade=True, normal=False),
            dict(colors="random", normals=None, shade=False, rgb=False, normal=False), dict(colors=255, normals="random", shade=True),
            dict(colors=77, normals=None, shade=True), dict(colors="random", normals="zero", shade=True)]


@pytest.mark.parametrize("case", S.lattice_cases(), ids=lambda c: c.id)
def test_resolve_variants(case):
    """Vertex normals or the face's own, colours or mid-grey, shaded or not, rgb and normal each absent, flat colours (r_byte's half-up
    rounding of colour x Lambert), all-zero normals (the normal plane is zero and nothing is shaded)."""
    stats = {}
    ref = S.reference(case)
    for n, var in enumerate(VARIANTS):
        col, nrm = S.attributes(case, n, flat=var["colors"] if isinstance(var["colors"], int) else None)
        col = None if var["colors"] is None else col
        nrm = None if var["normals"] is None else np.zeros_like(nrm) if var["normals"] == "zero" else nrm
        want_rgb, want_normal = var.get("rgb", True), var.get("normal", True)
        got = _draw(case, S.MAX_BOXES[n % 3], col, nrm, var["shade"], want_rgb, want_normal)
        assert (got["rgb"] is None) == (not want_rgb) and (got["normal"] is None) == (not want_normal)
        o32 = S.oracle(case, np.float32, col, nrm, var["shade"])
        fails = S.check(case, got, ref, o32, S.MAX_BOXES[n % 3], stats)
        assert not fails, (case.name, var, fails)
        if var["normals"] == "zero":
            assert not got["normal"].any()
        if case.faces is None and nrm is not None and want_normal:
            zero = (got["index"] >= 0) & ~nrm[np.maximum(got["index"], 0)].any(-1)
            assert not got["normal"][zero].any()
            if col is not None and want_rgb:
                assert np.array_equal(got["rgb"][zero], col[got["index"][zero]])  # no normal, no shading: the point's own bytes
    _report(case.name, stats)


@pytest.mark.parametrize("case", S.clipping() + [S.strips()[0], S.radii()[5]], ids=lambda c: c.id)
def test_resolve_rewrites_every_pixel(case):
    """ops.raster_resolve on outputs pre-filled with a sentinel: every pixel is rewritten, the tails of the 64 x 4 blocks included,
    for drawn keys and for untouched ones."""
    from patchmatchnet_amd import ops
    dev = _dev()
    h, w = case.h, case.w
    col, nrm = S.attributes(case, 9)
    o32 = S.oracle(case, np.float32, col, nrm, True)
    v, f = _up(case.vertices, dev), _up(case.faces, dev)
    for drawn in (True, False):
        keys = torch.full((h, w), -1, dtype=torch.int64, device=dev)
        counters = torch.zeros(4, dtype=torch.int32, device=dev)
        if drawn and f is not None:
            ops.raster_triangles(v, f, S.CAM, keys, counters, torch.zeros(len(case.faces), dtype=torch.int32, device=dev))
        elif drawn:
            ops.splat_points(v, S.CAM, keys, counters, case.radius_px, case.radius_world)
        depth = torch.full((h, w), -7.0, device=dev)
        index = torch.full((h, w), -99, dtype=torch.int32, device=dev)
        rgb = torch.full((h, w, 3), 0xAB, dtype=torch.uint8, device=dev)
        normal = torch.full((h, w, 3), -7.0, device=dev)
        ops.raster_resolve(keys, S.CAM, v, f, depth, index, _up(col, dev), _up(nrm, dev), True, rgb, normal)
        got = dict(depth=depth.cpu().numpy(), index=index.cpu().numpy(), rgb=rgb.cpu().numpy(), normal=normal.cpu().numpy())
        if drawn:
            for k in got:
                assert got[k].tobytes() == o32[k].astype(got[k].dtype).tobytes(), (case.name, k)
        else:
            assert (got["depth"].view(np.uint32) == 0).all() and (got["index"] == -1).all() and not got["rgb"].any() and \
                (got["normal"].view(np.uint32) == 0).all(), case.name
    print(f"{case.name}: every pixel of {h} x {w} rewritten, 0 px differ from the float32 oracle")
