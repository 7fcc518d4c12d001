"""The numpy model of moving least squares (tests/mls_ref.py, the host form of pmn_knn_mls) against an independent solver route and
against properties, on the CPU: the GPU test (tests/test_mls_gpu.py) holds the kernel to this model bit for bit, so the model itself
has to be right."""
import numpy as np
import pytest

import cloud_normals_ref as R
import knn_ref as K
import mls_ref as M

BIG = 1000.0
SPHERE_RADIUS, SHEET_RADIUS = 3.0, 5.0   # about three spacings of either cloud: the sphere's 1500 points lie 0.9 apart, the sheet's 1.4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("degree", (1, 2))
def test_a_planar_lattice_does_not_move(degree):
    """Axis-aligned lattice in z = 3: every delta has z = 0, so the xz, yz and zz moments and covariance entries are exactly 0, the
    rotations (0, 2) and (1, 2) are skipped, the normal is exactly (0, 0, 1), n . c is exactly 0 and no coordinate moves by one bit.
    (The xy entry is exactly 0 only where the neighbourhood is symmetric: a corner's is not.)"""
    pts = M.planar_lattice()
    for k in (8, 16, 32):
        r = M.mls(None, pts, k, 3.5, same_cloud=True, degree=degree)
        assert (r["status"] == degree).all()
        assert (r["A"][:, [2, 4, 5]] == 0.0).all() and (r["t"] == 0.0).all() and (r["A"][:, 1] == 0.0).any()
        assert np.array_equal(r["normal"], np.tile(np.float32([0, 0, 1]), (len(pts), 1)))
        assert np.array_equal(_bits(r["position"]), _bits(pts)) and (r["displacement"] == 0.0).all()


def test_smoothing_a_noisy_sphere_brings_it_closer_to_the_sphere():
    pts, centre, radius = M.noisy_sphere()
    rms_in = np.sqrt((M.sphere_distance(pts, centre, radius) ** 2).mean())
    for k in (16, 32):
        for degree in (1, 2):
            r = M.mls(None, pts, k, SPHERE_RADIUS, same_cloud=True, degree=degree)
            rms_out = np.sqrt((M.sphere_distance(r["position"], centre, radius) ** 2).mean())
            print(f"k {k} degree {degree}: rms {rms_in:.4f} -> {rms_out:.4f}")
            assert rms_out < rms_in, (k, degree)


def test_the_quadric_has_less_inward_bias_than_the_plane():
    """The reason degree 2 exists: a plane fitted to a patch of a sphere lies inside it."""
    pts, centre = R.sphere_cloud(noise=0.0)
    for k in (16, 32):
        bias = {}
        for degree in (1, 2):
            r = M.mls(None, pts, k, SPHERE_RADIUS, same_cloud=True, degree=degree)
            assert (r["status"] == degree).all()
            bias[degree] = M.sphere_distance(r["moved"], centre, 10.0).mean()
        print(f"k {k}: mean distance to the sphere, degree 1 {bias[1]:.3e}, degree 2 {bias[2]:.3e}")
        assert bias[1] < 0.0 and abs(bias[2]) < abs(bias[1])


def test_status_counts():
    one = np.array([[1.0, 2.0, 3.0]], np.float32)
    two = np.array([[1.0, 2.0, 3.0], [1.5, 2.0, 3.0]], np.float32)
    for pts in (one, two, K.axis_cloud()):
        for degree in (1, 2):
            r = M.mls(None, pts, 8, BIG, same_cloud=True, degree=degree)
            assert (r["status"] == 0).all() and np.array_equal(_bits(r["position"]), _bits(pts))
            assert not r["normal"].any() and not r["displacement"].any()
    # far queries with nothing in range
    sheet = R.sheet_cloud()
    far = K.far_queries(sheet)
    r = M.mls(far, sheet, 16, SHEET_RADIUS, degree=2)
    nothing = r["count"] == 0
    assert nothing.sum() >= 13 and (r["status"][nothing] == 0).all() and np.array_equal(_bits(r["position"][nothing]), _bits(far[nothing]))
    assert (r["status"] == 2).sum() > 30   # ... and the near ones are fitted
    # fewer than six members: the plane, never the quadric
    sphere = R.sphere_cloud()[0]
    r = M.mls(None, sphere, 4, SPHERE_RADIUS, same_cloud=True, degree=2)     # m = 5
    assert set(np.unique(r["status"])) <= {0, 1} and (r["status"] == 1).sum() > 1400
    r = M.mls(None, sphere, 5, SPHERE_RADIUS, same_cloud=True, degree=2)     # m = 6
    assert (r["status"] == 2).sum() > 1000
    r = M.mls(None, sphere[:5], 8, BIG, same_cloud=True, degree=2)
    assert (r["count"] == 4).all() and (r["status"] == 1).all()
    r = M.mls(K.far_queries(sphere)[:60], sphere, 5, SPHERE_RADIUS, degree=2)  # a separate query is no member: m = count
    assert (r["status"][r["count"] < 6] < 2).all()
    # a radius far beyond the neighbourhood: a and b are tiny, the pivots of the second-order columns fail, the plane stands
    r = M.mls(None, sphere, 16, BIG, same_cloud=True, degree=2)
    assert (r["status"] == 1).all()


@pytest.mark.parametrize("k", (16, 32))
def test_the_model_against_eigh_and_lstsq(k):
    """Wherever the model takes the step of the degree asked for and the independent route's (l1 - l0) / l2 >= 1e-3, the model's
    position must agree with the independent route (centred covariance, numpy.linalg.eigh, numpy.linalg.lstsq in unscaled
    coordinates).  Measured here, in float64 before the output is rounded: the largest difference of a coordinate is 1.14e-13 on the
    sphere (coordinates up to 660, where one float64 ulp is 1.14e-13: the two routes differ by the last rounding of q + delta) and
    1.42e-14 on the sheet (coordinates up to 60), at k = 16 and 32 and both degrees.  The tolerance is 1e-12, about 8 times the
    largest difference seen.  The float32 output adds its own rounding, which is the floor: at most half a float32 ulp of the
    coordinate.  No point of either cloud drops out for a small gap (0.00 % at k = 16 and k = 32; the smallest gaps are 0.13 on the
    sphere and 0.026 on the sheet); at most 1 % may."""
    for name, pts, radius in (("sphere", R.sphere_cloud()[0], SPHERE_RADIUS), ("sheet", R.sheet_cloud(), SHEET_RADIUS)):
        for degree in (1, 2):
            r = M.mls(None, pts, k, radius, same_cloud=True, degree=degree)
            moved, values = M.mls_independent(None, pts, k, radius, same_cloud=True, degree=degree)
            taken = r["status"] == degree
            ok = taken & (R.gap(values) >= 1e-3)
            left_out = int((taken & ~ok).sum())
            d64 = np.abs(r["moved"] - moved)[ok].max()
            half_ulp = np.spacing(np.abs(r["position"][ok])).astype(np.float64) / 2.0
            d32 = np.abs(r["position"][ok].astype(np.float64) - moved[ok])
            print(f"{name} k {k} degree {degree}: {int(ok.sum())} compared, {left_out} left out, float64 {d64:.3e}, float32 {d32.max():.3e}")
            assert taken.sum() >= 0.98 * len(pts) and left_out <= 0.01 * len(pts), (name, degree)
            assert d64 <= 1e-12, (name, degree)
            assert (d32 <= half_ulp + 1e-12).all(), (name, degree)
