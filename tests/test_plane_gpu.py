"""GPU checks of plane segmentation (pmn_plane_score, pmn_plane_inliers, pointcloud.plane_score / plane_inliers / segment_plane /
segment_planes) against the brute-force numpy float64 statement of tests/plane_ref.py.

The definition is exact: every inlier decision is taken on un-contracted float64 values that numpy reproduces bit for bit, the counts are
integers, and the ten sums are exact up to one rounding, which math.fsum is too -- so counts, masks, sums, plane coefficients, labels,
winner indices and refit counts are compared with np.array_equal: no tolerance.  (A sum whose terms fall below 2^-80 of its bound would
be compared with (n + 2) * 2^-53 * sum |term| instead; tests/test_plane_ref.py shows that no case here needs it.)  What the cases contain
is asserted on the reference alone by tests/test_plane_ref.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import plane_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 63, 64, 65, 257, 4099)
HS = (1, 63, 64, 65, 1000, 4096)


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _planted():
    return R.planted_scene(0)


@functools.lru_cache(maxsize=None)
def _two():
    return R.two_planes()


def _score(pts, planes, thr, normals=None, active=None, min_cos=0.0):
    from patchmatchnet_amd import pointcloud as PC
    got = PC.plane_score(_dev(pts), _dev(planes, np.float64), thr, None if normals is None else _dev(normals),
                         None if active is None else _dev(active, np.uint8), min_cos)
    assert got.dtype == torch.int32 and got.shape == (len(planes),)
    return got.cpu().numpy()


@pytest.mark.parametrize("n", NS)
def test_counts_are_the_reference(n):
    for H in HS:
        pts, planes, normals, active, thr, min_cos = R.score_case(n, H)
        assert np.array_equal(_score(pts, planes, thr), R.score(pts, planes, thr)), (n, H)
        want = R.score(pts, planes, thr, normals, active, min_cos)
        got = _score(pts, planes, thr, normals, active, min_cos)
        assert np.array_equal(got, want), (n, H, int((got != want).sum()))
        assert np.array_equal(_score(pts, planes, thr, normals, active, min_cos), got)  # a second run gives the same bits
    pts, planes, normals, active, thr, min_cos = R.score_case(n, 65)
    assert np.array_equal(_score(pts, planes, thr, active=active), R.score(pts, planes, thr, active=active))
    assert np.array_equal(_score(pts, planes, thr, normals, None, min_cos), R.score(pts, planes, thr, normals, None, min_cos))
    # min_cos == 0: the test on the normals does not exist, zero normals count
    assert np.array_equal(_score(pts, planes, thr, normals, None, 0.0), R.score(pts, planes, thr))
    assert not _score(pts, planes, thr, active=np.zeros(n, np.uint8)).any()
    assert np.array_equal(_score(pts, planes, 0.0), R.score(pts, planes, 0.0))
    assert np.array_equal(_score(pts, planes, 0.0, normals, active, 1.0), R.score(pts, planes, 0.0, normals, active, 1.0))


def test_more_rows_than_one_call_takes_and_a_second_stream():
    from patchmatchnet_amd import pointcloud as PC
    pts, planes, normals, active, thr, min_cos = R.score_case(257, 4097)
    want = R.score(pts, planes, thr, normals, active, min_cos)
    assert np.array_equal(_score(pts, planes, thr, normals, active, min_cos), want)
    d = [_dev(pts), _dev(planes, np.float64), _dev(normals), _dev(active, np.uint8)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        got = PC.plane_score(d[0], d[1], thr, d[2], d[3], min_cos)
        mask, sums = PC.plane_inliers(d[0], [0.0, 0.0, 1.0, -0.5], thr, d[2], d[3], min_cos)
    s.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    m2, s2 = PC.plane_inliers(d[0], [0.0, 0.0, 1.0, -0.5], thr, d[2], d[3], min_cos)
    assert torch.equal(mask, m2) and torch.equal(sums, s2)


def _check_inliers(pts, plane, thr, normals=None, active=None, min_cos=0.0):
    from patchmatchnet_amd import pointcloud as PC
    centre, extent = R.frame(pts, active)
    want_mask, want, mags = R.inliers_and_sums(pts, plane, thr, normals, active, min_cos, centre)
    assert R.qualifies(pts, want_mask, centre, extent)
    args = (_dev(pts), plane, thr, None if normals is None else _dev(normals), None if active is None else _dev(active, np.uint8), min_cos)
    c, e = PC.plane_frame(args[0], args[4])
    assert np.array_equal(c, centre) and np.array_equal(e, extent)
    mask, sums = PC.plane_inliers(*args)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want_mask)
    got = sums.cpu().numpy()
    print(f"n {len(pts)}: {int(got[0])} inliers, sums differ from fsum in {int((got != want).sum())} of 10")
    assert np.array_equal(got, want), (got, want)
    again = PC.plane_inliers(*args, return_mask=False)
    assert again[0] is None and torch.equal(again[1], sums)  # a second run, and no mask: the same bits
    return int(got[0])


def test_inlier_masks_and_exact_sums():
    pts, planted, plane, normals = _planted()
    thr = 2.0 * R.PLANTED_S
    assert _check_inliers(pts, plane, thr) > 2000
    rng = np.random.default_rng(3)
    active = (rng.random(len(pts)) < 0.6).astype(np.uint8)
    assert _check_inliers(pts, plane, thr, normals, active, float(np.cos(np.radians(20.0)))) > 1000
    assert _check_inliers(pts, [0.0, 0.0, 1.0, -50.0], thr) == 0             # no inlier: ten zeros
    assert _check_inliers(pts, plane, thr, active=np.zeros(len(pts), np.uint8) + (np.arange(len(pts)) == 7)) <= 1
    p2, t2 = R.rejected_refit_case()
    assert _check_inliers(p2, [0.0, 0.0, 1.0, 0.0], t2) == 42                 # 32 of them exactly on the threshold
    for n in (1, 63, 64, 65, 1025, 4099):                                     # sizes around a lane, a wave and a workgroup
        pts, planes, normals, active, thr, min_cos = R.score_case(n, 4)
        _check_inliers(pts, [0.0, 0.0, 1.0, 0.25], thr)
        _check_inliers(pts, [0.6, 0.0, 0.8, 0.125], 1.0, normals, None, min_cos)


def _same(got, want):
    assert np.array_equal(got["plane"], want["plane"]) and got["plane"].dtype == np.float64, (got["plane"], want["plane"])
    assert got["inliers"].dtype == torch.bool and np.array_equal(got["inliers"].cpu().numpy(), want["inliers"])
    assert (got["count"], got["hypothesis"], got["refits"]) == (want["count"], want["hypothesis"], want["refits"])
    assert got["rmse"] == want["rmse"]


def test_segment_plane_is_the_reference():
    from patchmatchnet_amd import pointcloud as PC
    pts, planted, plane, normals = _planted()
    d, dn = _dev(pts), _dev(normals)
    s = R.PLANTED_S
    first = PC.segment_plane(d, 2.0 * s, seed=0)
    _same(first, R.segment_plane(pts, 2.0 * s, seed=0))
    _same(PC.segment_plane(d, 2.0 * s, seed=0), first | {"inliers": first["inliers"].cpu().numpy()})  # the same seed twice
    other = PC.segment_plane(d, 2.0 * s, seed=5)
    _same(other, R.segment_plane(pts, 2.0 * s, seed=5))
    m = other["inliers"].cpu().numpy()
    assert other["hypothesis"] != first["hypothesis"] and m[planted].mean() >= 0.95 and m[~planted].mean() <= 0.01
    # a tight threshold, where refits are accepted (one, then a rejected one; three), and the normal test
    accepted = []
    for seed in (0, 1):
        want = R.segment_plane(pts, s, seed=seed)
        _same(PC.segment_plane(d, s, seed=seed), want)
        accepted.append(want["refits"])
    assert max(accepted) >= 2 and min(accepted) >= 1
    _same(PC.segment_plane(d, 2.0 * s, seed=0, normals=dn, normal_angle=20.0),
          R.segment_plane(pts, 2.0 * s, seed=0, normals=normals, normal_angle=20.0))
    active = (np.arange(len(pts)) % 3 != 0).astype(np.uint8)
    _same(PC.segment_plane(d, 2.0 * s, seed=2, hypotheses=300, refine=1, active=_dev(active, np.uint8)),
          R.segment_plane(pts, 2.0 * s, seed=2, hypotheses=300, refine=1, active=active))
    # the tie goes to the lowest index; the refit that loses inliers is rejected
    tie = R.tie_case()
    want = R.segment_plane(tie, 0.25, hypotheses=64, seed=0)
    assert (want["counts"] == want["counts"].max()).sum() >= 2
    _same(PC.segment_plane(_dev(tie), 0.25, hypotheses=64, seed=0), want)
    rej, thr = R.rejected_refit_case()
    want = R.segment_plane(rej, thr, seed=0)
    assert want["rejected"] and want["refits"] == 0
    _same(PC.segment_plane(_dev(rej), thr, seed=0), want)


def test_segment_planes_is_the_reference():
    from patchmatchnet_amd import pointcloud as PC
    pts, which = _two()
    thr = 2.0 * R.PLANTED_S
    want = R.segment_planes(pts, thr, max_planes=4, min_inliers=200, seed=0)
    got = PC.segment_planes(_dev(pts), thr, max_planes=4, min_inliers=200, seed=0)
    assert len(want["counts"]) == 2 and got["counts"] == want["counts"]
    assert got["labels"].dtype == torch.int64 and np.array_equal(got["labels"].cpu().numpy(), want["labels"])
    assert got["planes"].dtype == np.float64 and np.array_equal(got["planes"], want["planes"])
    for g, w in zip(got["results"], want["results"]):
        _same(g, w)
    again = PC.segment_planes(_dev(pts), thr, max_planes=4, min_inliers=200, seed=0)
    assert torch.equal(again["labels"], got["labels"]) and np.array_equal(again["planes"], got["planes"])
    planted, _, _, _ = _planted()
    one = PC.segment_planes(_dev(planted), thr, max_planes=1, min_inliers=100, seed=0)
    assert np.array_equal(one["labels"].cpu().numpy() == 0, R.segment_plane(planted, thr, seed=0)["inliers"])
    none = PC.segment_planes(_dev(planted), thr, max_planes=3, min_inliers=4000, seed=0)
    assert none["counts"] == [] and none["planes"].shape == (0, 4) and bool((none["labels"] == -1).all())


def test_default_threshold_is_two_spacings():
    from patchmatchnet_amd import pointcloud as PC
    pts = _two()[0]
    d = _dev(pts)
    thr = PC.PLANE_THRESHOLD_SPACINGS * PC.cloud_spacing(d)
    a, b = PC.segment_plane(d, seed=1), PC.segment_plane(d, thr, seed=1)
    assert np.array_equal(a["plane"], b["plane"]) and torch.equal(a["inliers"], b["inliers"])


def test_icp_sums_survive_the_shared_header():
    """pmn_icp_accumulate now takes its digits from csrc/exact_sum.hpp: one small cloud against tests/tnt_ref.py within that
    reference's bound, (n + 2) * 2^-53 * sum |term| (tests/test_tnt_score_gpu.py)."""
    import tnt_ref as T
    from patchmatchnet_amd import pointcloud as PC, registration as RG
    target = np.ascontiguousarray(T.synthetic_scene(0)["gt"][::30])
    rng = np.random.default_rng(1)
    src = (target[rng.integers(0, len(target), 333)].astype(np.float64) + T.TAU * rng.standard_normal((333, 3))).astype(np.float32)
    pose = T.rigid(T.rotation((2.0, -1.0, 0.5), 1.5), (0.004, -0.003, 0.002))
    centre = T.bbox_centre(target)
    want, mag = T.icp_sums(src, target, pose, centre, 80 * T.TAU)
    grid = PC.build_grid(_dev(target), 0.3)
    got = RG.icp_accumulate(_dev(src), grid, pose, centre, 80 * T.TAU).cpu().numpy()
    assert got.shape == (17,) and got[0] == want[0] > 100
    assert (np.abs(got - want) <= (want[0] + 2) * 2.0 ** -53 * mag).all(), (got, want)


def test_argument_checks_return_their_codes_without_launching():
    from patchmatchnet_amd import _lib
    L = _lib.lib()
    ARG, SHAPE = -1, -2
    assert L.pmn_error_string(SHAPE).decode().startswith("unsupported shape")
    n = 100
    xyz, nrm = torch.zeros(n, 3, device=DEV), torch.zeros(n, 3, device=DEV)
    planes, counts = torch.zeros(8, 4, dtype=torch.float64, device=DEV), torch.full((8,), -7, dtype=torch.int32, device=DEV)
    x, q, p, c = xyz.data_ptr(), nrm.data_ptr(), planes.data_ptr(), counts.data_ptr()
    nan, inf = float("nan"), float("inf")

    def score(xyz=x, normals=q, n=n, planes=p, H=8, thr=0.1, min_cos=0.0, counts=c):
        return L.pmn_plane_score(xyz, normals, None, n, planes, H, thr, min_cos, counts, None)

    for kw in (dict(xyz=None), dict(planes=None), dict(counts=None), dict(n=0), dict(n=2 ** 31 - 64), dict(thr=-0.1), dict(thr=nan),
               dict(thr=inf), dict(min_cos=-0.1), dict(min_cos=1.5), dict(min_cos=nan), dict(normals=None, min_cos=0.5)):
        assert score(**kw) == ARG, kw
    for H in (0, -1, 4097):
        assert score(H=H) == SHAPE, H
    sums, mask = torch.full((10,), -7.0, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    words = _lib.plane_scratch(n)
    scratch = torch.zeros(words, dtype=torch.int64, device=DEV)
    d3, d4 = ctypes.c_double * 3, ctypes.c_double * 4

    def inl(xyz=x, normals=q, n=n, plane=(0, 0, 1, 0), thr=0.1, min_cos=0.0, centre=(0, 0, 0), extent=(1, 1, 1), scr=scratch.data_ptr(),
            words=words, sums=sums.data_ptr()):
        return L.pmn_plane_inliers(xyz, normals, None, n, d4(*plane) if plane else None, thr, min_cos, d3(*centre) if centre else None,
                                   d3(*extent) if extent else None, scr, words, mask.data_ptr(), sums, None)

    for kw in (dict(xyz=None), dict(plane=None), dict(centre=None), dict(extent=None), dict(scr=None), dict(sums=None), dict(n=0),
               dict(n=2 ** 31 - 64), dict(thr=-1.0), dict(thr=nan), dict(min_cos=2.0), dict(normals=None, min_cos=0.5),
               dict(plane=(0, nan, 1, 0)), dict(plane=(0, 0, 1, inf)), dict(centre=(0, inf, 0)), dict(extent=(1, -1, 1)),
               dict(extent=(1, nan, 1)), dict(words=words - 1)):
        assert inl(**kw) == ARG, kw
    assert inl(extent=(1e300, 1, 1)) == SHAPE
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((sums == -7.0).all())  # nothing was launched
    assert score() == 0 and inl() == 0
    torch.cuda.synchronize()
    assert bool((counts == n).all()) and sums[0].item() == n


def test_wrapper_checks_raise():
    from patchmatchnet_amd import PmnError, pointcloud as PC
    pts = _dev(R.tie_case())
    n = pts.shape[0]
    planes = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
    nrm = torch.zeros(n, 3, device=DEV)
    bad_calls = [
        lambda: PC.plane_score(pts.cpu(), planes, 0.1),
        lambda: PC.plane_score(pts, planes.cpu(), 0.1),
        lambda: PC.plane_score(pts, planes.float(), 0.1),
        lambda: PC.plane_score(pts, planes[:, :3], 0.1),
        lambda: PC.plane_score(pts, planes[:0], 0.1),
        lambda: PC.plane_score(pts, planes, -1.0),
        lambda: PC.plane_score(pts, planes, float("nan")),
        lambda: PC.plane_score(pts, planes, 0.1, min_cos=0.5),
        lambda: PC.plane_score(pts, planes, 0.1, normals=nrm, min_cos=1.5),
        lambda: PC.plane_score(pts, planes, 0.1, normals=nrm[:5]),
        lambda: PC.plane_score(pts, planes, 0.1, normals=nrm.double()),
        lambda: PC.plane_score(pts, planes, 0.1, active=torch.ones(n, device=DEV)),
        lambda: PC.plane_score(pts, planes, 0.1, active=torch.ones(n + 1, dtype=torch.bool, device=DEV)),
        lambda: PC.plane_score(pts, planes, 0.1, active=torch.ones(n, dtype=torch.bool)),
        lambda: PC.plane_inliers(pts, [0, 0, 1], 0.1),
        lambda: PC.plane_inliers(pts, [0, 0, 1, float("inf")], 0.1),
        lambda: PC.plane_inliers(pts, [0, 0, 1, 0], 0.1, centre=[0, 0, 0]),
        lambda: PC.plane_inliers(pts, [0, 0, 1, 0], 0.1, centre=[0, 0, 0], extent=[1, -1, 1]),
        lambda: PC.plane_inliers(pts, [0, 0, 1, 0], 0.1, scratch=torch.empty(3, dtype=torch.int64, device=DEV)),
        lambda: PC.plane_inliers(pts, [0, 0, 1, 0], 0.1, active=torch.zeros(n, dtype=torch.bool, device=DEV)),  # no active point
        lambda: PC.plane_hypotheses(np.zeros((4, 3))),
        lambda: PC.segment_plane(pts, 0.1, hypotheses=0),
        lambda: PC.segment_plane(pts, 0.1, seed=-1),
        lambda: PC.segment_plane(pts, 0.1, refine=-1),
        lambda: PC.segment_plane(pts, 0.1, normal_angle=10.0),
        lambda: PC.segment_plane(pts, 0.1, normals=nrm, normal_angle=100.0),
        lambda: PC.segment_plane(pts[:2].contiguous(), 0.1),                                   # fewer than 3 points
        lambda: PC.segment_plane(pts, 0.1, active=torch.arange(n, device=DEV) < 2),            # fewer than 3 active points
        lambda: PC.segment_plane(_dev([[0, 0, 0], [1, 1, 1], [2, 2, 2]]), 0.1, hypotheses=16),  # every hypothesis is invalid
        lambda: PC.segment_planes(pts, 0.1, max_planes=0),
        lambda: PC.segment_planes(pts, 0.1, min_inliers=0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(PmnError):
            call()
            pytest.fail(f"call {i} was accepted")
    got = PC.plane_hypotheses(R.tie_case()[None, :3])  # the product's host code on its own
    assert np.array_equal(got, R.hypotheses(R.tie_case(), [[0, 1, 2]]))
