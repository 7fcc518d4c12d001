"""CPU checks of the camera space (tests/camera_space.py): the reference alone -- its float32 restatement against the same operations
in float64 -- meets every condition tests/test_camera_space_gpu.py leans on: the six pivot patterns of the projection's inverse are
all reached, each by two samples; per rig the float32 and float64 restatements agree on which hypotheses are in front of the source
camera but for <= 1 % of the samples, and <= 1 % lie where they could not; every rig holds its stated share of samples inside the
source map, on its border, outside it and behind the camera; and a CPU port of the kernel's Gauss-Jordan shows which rig catches
which negated swap.  The position errors of the float32 restatement are printed per rig (`-s`): `dtu` is what the suite has been
living with, the others are the conditioning the rigs add."""
import numpy as np
import pytest

import camera_space as CS
import ref64 as R


def test_table_holds_what_the_issue_lists():
    rigs = CS.rigs()
    assert tuple(rigs) == CS.RIG_NAMES
    for rig in rigs.values():
        assert rig.intrinsics.dtype == np.float32 and rig.extrinsics.dtype == np.float32
        assert rig.intrinsics.shape == (rig.B, rig.V, 3, 3) and rig.extrinsics.shape == (rig.B, rig.V, 4, 4)
        assert len(rig.ratios) == rig.V and rig.ratios[0] == (1.0, 1.0)
        for a in (rig.intrinsics, rig.extrinsics, rig.depth_min, rig.depth_max):
            assert np.isfinite(a).all()
        for c in CS.warp_cases(rig.name):
            assert np.isfinite(c.P).all() and np.isfinite(c.depth).all() and (c.depth > 0).all()
        # rotations are rotations, last rows are (0, 0, 0, 1)
        Rm = rig.extrinsics[:, :, :3, :3].astype(np.float64)
        assert np.abs(Rm @ Rm.transpose(0, 1, 3, 2) - np.eye(3)).max() < 1e-6
        assert (rig.extrinsics[:, :, 3] == np.float32([0, 0, 0, 1])).all()
    two = [r for r in rigs.values() if r.B == 2]
    assert two and all(not np.array_equal(r.extrinsics[0], r.extrinsics[1]) and not np.array_equal(r.intrinsics[0], r.intrinsics[1])
                       for r in two)
    assert {2, 11} <= {r.V for r in rigs.values()}
    assert {1, 3, 4} <= {r.nstages for r in rigs.values()}
    assert any(r.scale0 != 0.125 for r in rigs.values())
    counts = [r.nstages * r.B * (r.V - 1) for r in rigs.values()]
    assert any(c > 64 and c % 64 for c in counts), counts
    # far_origin is unit's first sample seen from a world origin ~2.3e3 away; mixed has what its name says
    assert np.abs(rigs["far_origin"].extrinsics[0, :, :3, 3]).max() > 1e3
    m = rigs["mixed"]
    K = m.intrinsics[0]
    assert (K[:, 0, 0] != K[:, 1, 1]).all() and (K[:, 0, 1] != 0).all()
    W0, H0 = CS.W_MAP / m.scale0, CS.H_MAP / m.scale0
    assert all(not (W0 / 3 < k[0, 2] < 2 * W0 / 3) or not (H0 / 3 < k[1, 2] < 2 * H0 / 3) for k in K)
    sizes = [m.map_size(v) for v in range(1, m.V)]
    assert any(hs < CS.H_MAP and ws < CS.W_MAP for hs, ws in sizes) and any(hs > CS.H_MAP and ws > CS.W_MAP for hs, ws in sizes)
    w = rigs["wide"]
    assert float(w.depth_max[0] / w.depth_min[0]) == 40.0
    C = [-(w.extrinsics[0, v, :3, :3].astype(np.float64).T @ w.extrinsics[0, v, :3, 3]) for v in range(w.V)]
    base = max(np.linalg.norm(c - C[0]) for c in C[1:])
    assert 0.2 * w.depth_min[0] < base <= w.depth_min[0] / 3.0 + 1e-6


def test_pivot_patterns_all_six_each_twice():
    seen = {}
    for rig in CS.rigs().values():
        for s, scale in enumerate(rig.scales()):
            P = CS.stage_proj(rig, scale, np.float32)
            for b in range(rig.B):
                seen.setdefault(CS.pivot_pattern(P[b, 0]), set()).add((rig.name, b))
    assert set(seen) == set(CS.PATTERNS), sorted(seen)
    for pat, where in sorted(seen.items()):
        print(f"pivot pattern {pat[:2]}: {len(where)} (rig, b), e.g. {sorted(where)[:3]}")
        assert len(where) >= 2, (pat, where)
    # the turned rig gives the pattern each of its rotations was chosen for, and the swaps that go with it
    rig = CS.rigs()["turned"]
    P = CS.stage_proj(rig, rig.scale0, np.float32)
    for b, (pat, _kind, _params) in enumerate(CS.TURNS):
        assert CS.pivot_pattern(P[b, 0]) == pat, (b, pat)
        assert CS.swaps(P[b, 0]) == tuple((c, p) for c, p in enumerate(pat) if c != p)
    assert {k: len(v) for k, v in CS.pivot_cases().items()} == {p: 2 for p in CS.PATTERNS}
    assert CS.pivot_pattern(CS.stage_proj(CS.rigs()["dtu"], 0.125, np.float32)[0, 0]) == (0, 1, 2, 3)  # what the suite had


def test_pivot_pattern_is_the_inverse_the_reference_computes():
    """The port of the kernel's Gauss-Jordan passes test (b)'s gate on every sample of `turned` (so the gate can be met, by these
    operations), and its pivots are pivot_pattern's."""
    rig = CS.rigs()["turned"]
    P = CS.stage_proj(rig, rig.scale0, np.float32)
    for b in range(rig.B):
        ratio, ok = CS.inverse_gate(CS.gauss_jordan_port(P[b, 0]), P[b, 0])
        print(f"turned b={b} pattern {CS.pivot_pattern(P[b, 0])[:2]}: port of the kernel's inverse at {ratio:.3f} of its bound")
        assert ok, (b, ratio)


def test_every_negated_swap_is_caught():
    """Negating one `sw` of the kernel exchanges two rows where the pivot search asked for none (and leaves them where it asked).
    An exchange of whole rows of [A | I] is a legal row operation, so this breaks the inverse only through the pivot it leaves on
    the diagonal: a zero (row 3 in columns 0..2, and the entries a turned camera's zeros put there) or a small one.  For each of the
    six conditions the port with that condition negated must fail test (b)'s gate on at least one of its samples."""
    rig = CS.rigs()["turned"]
    P = CS.stage_proj(rig, rig.scale0, np.float32)
    for cond in CS.SW_CONDITIONS:
        caught = []
        for b in range(rig.B):
            ratio, ok = CS.inverse_gate(CS.gauss_jordan_port(P[b, 0], negate=cond), P[b, 0])
            if not ok:
                caught.append((b, CS.pivot_pattern(P[b, 0])[:2], ratio))
        print(f"sw{cond} negated: caught by turned b = {[c[0] for c in caught]} (patterns {sorted({c[1] for c in caught})})")
        assert caught, cond


@pytest.mark.parametrize("name", CS.RIG_NAMES)
def test_front_test_is_stable_and_classes_are_present(name):
    rig = CS.rigs()[name]
    cases = CS.warp_cases(name)
    total = sum(c.pos64[2].size for c in cases)
    disagree = sum(int((c.pos64[2] != c.pos32[2]).sum()) for c in cases) / total
    near = sum(int(c.near.sum()) for c in cases) / total
    assert disagree <= 0.01, disagree
    assert near <= 0.01, near
    share = {k: 0 for k in CS.CLASSES}
    for c in cases:
        for k, m in CS.classify(c.pos64[0], c.pos64[1], c.pos64[2], c.hs, c.ws).items():
            share[k] += int(m.sum())
    share = {k: v / total for k, v in share.items()}
    print(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()) + f"; front disagrees {disagree:.2e}, near 1e-3 {near:.2e}")
    assert rig.shares, name
    for k, least in rig.shares.items():
        assert least >= 0.02 and share[k] >= least, (name, k, share[k], least)
    if name == "ring":
        assert set(rig.shares) == set(CS.CLASSES)
        pz = np.concatenate([c.pos64[3].ravel() for c in cases])
        assert (pz < -1.0).any() and ((pz > 1e-3) & (pz < 0.3)).any()  # hypotheses on both sides of the front test ...
        far = max(float(max(np.abs(c.pos64[0][c.pos64[2]]).max(), np.abs(c.pos64[1][c.pos64[2]]).max())) for c in cases)
        print(f"ring: farthest front position {far:.3e} px")
        assert far > 5e4, far  # ... and positions of 1e4 - 1e5 px (a 32-pixel window of depth 4.5 over pz = 1e-3; more at larger maps)
    if name == "mixed":  # behind-camera hypotheses on a source map smaller than the reference's
        assert any((c.hs < c.h and c.ws < c.w) and (~c.pos64[2]).mean() > 0.1 for c in cases)


@pytest.mark.parametrize("name", CS.RIG_NAMES)
def test_reference_position_errors_are_printed(name):
    """float32 restatement vs float64, in source pixels: through the projections (what test (a) gates the kernel against) and
    through the warp chain on one projection (test (c)); and, per ramp channel, the sampled values."""
    rig = CS.rigs()[name]
    for s, scale in enumerate(rig.scales()):
        e = CS.projection_error(CS.projections(rig, scale, np.float32), rig, s)
        print(f"REFERENCE {name} stage {s} (scale {scale:g}): float32 projections move a pixel by at most {e:.3e} px")
        assert np.isfinite(e)
    cases = CS.warp_cases(name)
    e = max(CS.position_error(c.pos32, c.pos64, c.hs, c.ws, ~c.near) for c in cases)
    v = np.max([np.abs(c.ref32 - c.want)[:, :, ~c.near[0]].max(axis=(0, 2)) if c.near.shape[0] == 1 else
                np.abs(c.ref32 - c.want).transpose(1, 0, 2, 3, 4)[:, ~c.near].max(axis=1) for c in cases], axis=0)
    print(f"REFERENCE {name} warp: float32 positions within {e:.3e} px, sampled ramps (x, y, 1) within {v[0]:.3e} {v[1]:.3e} {v[2]:.3e}")
    assert np.isfinite(e) and np.isfinite(v).all()


def test_positions_wrap_ref64_and_ramps_show_positions():
    """positions() is ref64.warp_positions; sampling the ramps at an inside position returns the position and a weight of one, and a
    behind-camera hypothesis samples nothing on a source map of any size.  The reference's own sentinel (w, h, 1) lands ON the last
    texel of a smaller map, with the weight (1 - (ws-1)/(w-1)) (1 - (hs-1)/(h-1)): what test (c) on the device would see."""
    c = [c for c in CS.warp_cases("mixed") if c.stage == 0 and c.view == 1][0]
    ix, iy, front = CS.positions(c.P[0], c.depth[0], c.h, c.w, c.hs, c.ws, np.float64)
    jx, jy = R.warp_positions(c.P[0], c.depth[0], c.h, c.w, c.hs, c.ws)
    assert np.array_equal(ix, jx) and np.array_equal(iy, jy)
    cl = CS.classify(ix, iy, front, c.hs, c.ws)
    got = R.bilinear(CS.ramps(c.hs, c.ws), ix, iy)
    m = cl["inside"]
    assert m.any() and np.abs(got[0][m] - ix[m]).max() < 1e-12 and np.abs(got[1][m] - iy[m]).max() < 1e-12
    assert np.abs(got[2][m] - 1.0).max() < 1e-12
    assert c.hs < c.h and c.ws < c.w and (~front).any()
    assert (got[:, ~front] == 0.0).all() and (got[:, cl["outside"]] == 0.0).all()
    sx, sy = c.w * (c.ws - 1) / (c.w - 1), c.h * (c.hs - 1) / (c.h - 1)
    assert sx < c.ws and sy < c.hs
    kx, ky = R.warp_positions(c.P[0], c.depth[0], c.h, c.w, c.hs, c.ws, sentinel=(sx, sy))
    leak = (1.0 - (c.ws - 1) / (c.w - 1)) * (1.0 - (c.hs - 1) / (c.h - 1))
    assert np.abs(R.bilinear(CS.ramps(c.hs, c.ws), kx, ky)[2][~front] - leak).max() < 1e-12 and leak > 0.25
