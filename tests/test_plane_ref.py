"""CPU checks of tests/plane_ref.py, the numpy statement of plane segmentation, on the reference alone: the cases
of tests/test_plane_gpu.py contain what they are meant to contain.  The two recovery caps (at least 95 % of the planted points, at most
1 % of the others) are conditions on the scene and the seed, not on the code under test."""
import math

import numpy as np
import pytest

import plane_ref as R


@pytest.fixture(scope="module")
def planted():
    pts, planted, plane, normals = R.planted_scene(0)
    return pts, planted, plane, normals, R.segment_plane(pts, 2.0 * R.PLANTED_S, seed=0)


def _shares(res, planted):
    return res["inliers"][planted].mean(), res["inliers"][~planted].mean()


def test_planted_scene_is_recovered(planted):
    pts, mark, plane, normals, res = planted
    assert 3900 <= len(pts) <= 4100 and mark.sum() == 2200
    r = pts.astype(np.float64) @ plane[:3] + plane[3]
    assert np.abs(r[mark]).max() <= R.PLANTED_S * (1.0 + 1e-4)      # bounded noise: float32 rounding adds less than 1e-6
    assert (np.abs(r[~mark]) <= 2.0 * R.PLANTED_S).mean() < 0.01   # the others really are off the plane
    got, others = _shares(res, mark)
    print(f"seed 0: {got:.4f} of the planted points, {others:.4f} of the others, refits {res['refits']}, rmse {res['rmse']:.5f}")
    # achieved with seed 0 and with seed 5: 1.0000 of the planted points, 0.0044 of the others (the winning draw already holds every
    # planted point; its refit drops clutter and is rejected)
    assert got >= 0.95 and others <= 0.01
    assert res["count"] == res["inliers"].sum() and res["counts"][res["hypothesis"]] == res["counts"].max()
    assert abs(abs(res["plane"][:3] @ plane[:3]) - 1.0) < 1e-4
    # the rmse from the ten sums is the rmse of the residuals (cancellation: 2^-53 * count * extent^2 against count * rmse^2)
    rr = pts.astype(np.float64)[res["inliers"]] @ res["plane"][:3] + res["plane"][3]
    assert abs(res["rmse"] - math.sqrt(np.mean(rr * rr))) < 1e-9
    # another seed meets the caps too (tests/test_plane_gpu.py relies on it)
    got, others = _shares(R.segment_plane(pts, 2.0 * R.PLANTED_S, seed=5), mark)
    print(f"seed 5: {got:.4f} of the planted points, {others:.4f} of the others")
    assert got >= 0.95 and others <= 0.01


def test_normal_angle_removes_inliers_with_foreign_normals(planted):
    pts, mark, plane, normals, res = planted
    with_n = R.segment_plane(pts, 2.0 * R.PLANTED_S, seed=0, normals=normals, normal_angle=20.0)
    assert with_n["inliers"][mark].mean() >= 0.95
    assert with_n["inliers"][~mark].sum() < res["inliers"][~mark].sum()


def test_points_exactly_on_the_threshold_count():
    pts, planes, normals, active, thr, min_cos = R.score_case(257, 64)
    p = pts.astype(np.float64)
    rows = [h for h in range(0, 64, 3) if h % 7 != 1]
    on = sum(int((np.abs(p[:, 2] + planes[h, 3]) == thr).sum()) for h in rows)
    assert on > 50  # r == threshold exactly, many times
    h = rows[0]
    inside = np.abs(p[:, 2] + planes[h, 3]) < thr
    exact = np.abs(p[:, 2] + planes[h, 3]) == thr
    assert R.score(pts, planes[h:h + 1], thr)[0] == inside.sum() + exact.sum() and exact.sum() > 0
    assert R.score(pts, planes[h:h + 1], 0.0)[0] == (p[:, 2] + planes[h, 3] == 0.0).sum()
    # non-finite rows score 0; zero normals fail the normal test; an all-zero mask leaves nothing
    bad = [h for h in range(1, 64, 7)]
    assert not np.isfinite(planes[bad]).all(1).any() and (R.score(pts, planes[bad], 100.0) == 0).all()
    assert (normals == 0).all(1).sum() > 5
    zero = (normals == 0).all(1)
    assert R.score(pts[zero], planes[h:h + 1], thr, normals[zero], None, min_cos)[0] == 0 < R.score(pts[zero], planes[h:h + 1], thr)[0]
    assert (R.score(pts, planes, thr, active=np.zeros(257, np.uint8)) == 0).all()
    assert 0 < R.score(pts, planes, thr, active=active).sum() < R.score(pts, planes, thr).sum()


def test_invalid_hypotheses():
    pts = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [1, 0, 0], [0, 1, 0]], np.float32)
    planes = R.hypotheses(pts, np.array([[0, 0, 3], [3, 4, 3], [0, 1, 2], [0, 3, 4], [4, 3, 0]]))
    assert np.isnan(planes[:3]).all()  # a repeated index (twice), three collinear points
    assert np.array_equal(planes[3], [0.0, 0.0, 1.0, 0.0]) and np.array_equal(planes[4], [0.0, 0.0, 1.0, 0.0])  # the sign rule
    assert np.array_equal(R.sign_rule([-0.5, 0.5, 0.1]), [0.5, -0.5, -0.1])  # a tie of magnitudes goes to the lowest axis
    with pytest.raises(ValueError):
        R.segment_plane(pts[:3], 0.1, hypotheses=16)  # collinear: every hypothesis is invalid
    with pytest.raises(ValueError):
        R.segment_plane(pts[:2], 0.1, hypotheses=16)


def test_tie_case_has_a_tie_and_the_lowest_index_wins():
    pts = R.tie_case()
    res = R.segment_plane(pts, 0.25, hypotheses=64, seed=0)
    c = res["counts"]
    assert c.max() == 8 and (c == 8).sum() >= 2 and res["hypothesis"] == int(np.flatnonzero(c == 8)[0])
    assert np.array_equal(res["plane"][:3], [0.0, 0.0, 1.0]) and res["plane"][3] == 0.0 and res["count"] == 8


def test_rejected_refit_case():
    pts, thr = R.rejected_refit_case()
    res = R.segment_plane(pts, thr, hypotheses=1024, seed=0)
    assert res["count"] == 42 and res["rejected"] and res["refits"] == 0
    assert np.array_equal(res["plane"][:3], [0.0, 0.0, 1.0]) and res["plane"][3] == 0.0
    centre, _ = R.frame(pts)
    _, sums, _ = R.inliers_and_sums(pts, res["plane"], thr, centre=centre)
    assert R.inliers_and_sums(pts, R.refit(sums, centre), thr, centre=centre)[1][0] < 42


def test_two_plane_scene():
    pts, which = R.two_planes()
    res = R.segment_planes(pts, 2.0 * R.PLANTED_S, max_planes=4, min_inliers=200, seed=0)
    assert len(res["counts"]) == 2 and res["planes"].shape == (2, 4)  # the third best plane is below min_inliers
    lab = res["labels"]
    assert (lab[which == 0] == 0).mean() >= 0.95 and (lab[which == 1] == 1).mean() >= 0.95 and (lab[which == -1] >= 0).mean() < 0.1
    assert abs(res["planes"][0][2]) > 0.999 and abs(res["planes"][1][0]) > 0.999
    assert res["counts"] == [int((lab == 0).sum()), int((lab == 1).sum())]
    one = R.segment_planes(pts, 2.0 * R.PLANTED_S, max_planes=1, min_inliers=200, seed=0)
    assert np.array_equal(one["labels"] == 0, lab == 0)


def test_the_sum_cases_qualify_for_bit_equality(planted):
    pts, mark, plane, normals, res = planted
    centre, extent = R.frame(pts)
    assert R.qualifies(pts, res["inliers"], centre, extent)
    p2, thr = R.rejected_refit_case()
    c2, e2 = R.frame(p2)
    assert R.qualifies(p2, np.ones(len(p2), bool), c2, e2)
    # a term 2^-100 of its bound does not qualify (such a case is compared with the derived bound instead)
    tiny = np.array([[0, 0, 0], [1, 1, 1]], np.float32)
    assert not R.qualifies(tiny, np.ones(2, bool), [2.0 ** -100] * 3, [1.0] * 3)
