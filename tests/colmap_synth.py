"""Seeded synthetic COLMAP sparse models (binary cameras.bin / images.bin / points3D.bin) for the COLMAP import tests.

``write_model`` is a small writer of COLMAP's binary format; ``make_model`` builds a model from a seed; ``write_case`` puts the model
and tiny JPEGs under ``<root>/sparse`` and ``<root>/images``.  Named cases (``CASES``) are what tests/golden/colmap_reference.npz
pins; ``large_case`` is the ~300-image model of the GPU test and scripts/colmap_import_bench.py.  No reference imports.
"""
from __future__ import annotations

import hashlib
import math
import os
import struct
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MODEL_IDS = {"SIMPLE_PINHOLE": (0, 3), "PINHOLE": (1, 4), "SIMPLE_RADIAL": (2, 4), "RADIAL": (3, 5), "OPENCV": (4, 8),
             "OPENCV_FISHEYE": (5, 8), "FULL_OPENCV": (6, 12), "FOV": (7, 5), "SIMPLE_RADIAL_FISHEYE": (8, 4),
             "RADIAL_FISHEYE": (9, 5), "THIN_PRISM_FISHEYE": (10, 12)}


def write_model(sparse_dir: str, cameras: Sequence[Tuple[int, str, int, int, Sequence[float]]],
                images: Sequence[Tuple[int, Sequence[float], Sequence[float], int, str, np.ndarray]],
                points: Sequence[Tuple[int, Sequence[float], Sequence[int], float, np.ndarray]]) -> None:
    """cameras: (id, model name, width, height, params); images: (id, qvec, tvec, camera_id, name, point3D ids per keypoint, -1 =
    untriangulated); points: (id, xyz, rgb, error, track [(image_id, point2D_idx)])."""
    os.makedirs(sparse_dir, exist_ok=True)
    with open(os.path.join(sparse_dir, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for cid, model, w, h, params in cameras:
            mid, n = MODEL_IDS[model]
            assert len(params) == n
            f.write(struct.pack("<iiQQ", cid, mid, w, h) + struct.pack("<" + "d" * n, *params))
    with open(os.path.join(sparse_dir, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name, pids in images:
            f.write(struct.pack("<idddddddi", iid, *q, *t, cid) + name.encode() + b"\x00")
            pts = np.zeros(len(pids), [("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            pts["x"] = np.arange(len(pids)) * 0.5 + 0.25
            pts["y"] = np.arange(len(pids)) * 0.25 + 0.5
            pts["id"] = pids
            f.write(struct.pack("<Q", len(pids)) + pts.tobytes())
    with open(os.path.join(sparse_dir, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(points)))
        for pid, xyz, rgb, err, track in points:
            track = np.asarray(track, np.int32).reshape(-1, 2)
            f.write(struct.pack("<QdddBBBd", pid, *xyz, *rgb, err) + struct.pack("<Q", len(track)) + track.astype("<i4").tobytes())


def _quat_look_at(center: np.ndarray, target: np.ndarray, rng) -> Tuple[np.ndarray, np.ndarray]:
    """(qvec w,x,y,z, tvec) of a camera at ``center`` looking at ``target`` (+z forward), with a small random roll."""
    z = target - center
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) + 0.1 * rng.standard_normal(3)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])  # world -> camera rows
    return rot_to_quat(R), -R @ center


def rot_to_quat(R: np.ndarray) -> np.ndarray:
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    return q / np.linalg.norm(q)


def make_model(seed: int, n_images: int, n_points: int, keypoints: int, mean_track: float, camera_models: Sequence[str] = ("PINHOLE",),
               image_ids: Optional[Sequence[int]] = None, disjoint_pair: Optional[Tuple[int, int]] = None,
               duplicate_in: Optional[int] = None, point_at_center_of: Optional[int] = None, width: int = 64, height: int = 48):
    """A random model: cameras on a ring around the origin looking at it, points in a ball around the origin, tracks of 2 or more
    images (Poisson around ``mean_track``), every image padded with untriangulated keypoints up to ``keypoints`` and shuffled.
    Options (case B): image ids in the given (non-contiguous, unsorted) order, one image pair (by position) that shares no point,
    one point observed twice by one image, one point placed exactly at one image's camera centre."""
    rng = np.random.default_rng(seed)
    cameras = []
    for c, model in enumerate(camera_models):
        f, cx, cy = 60.0 + 5 * c + rng.uniform(0, 1), width / 2 + rng.uniform(-1, 1), height / 2 + rng.uniform(-1, 1)
        n = MODEL_IDS[model][1]
        if model.startswith("SIMPLE") or model.startswith("RADIAL"):
            params = [f, cx, cy] + list(rng.uniform(-0.01, 0.01, n - 3))
        else:
            params = [f, f * 1.01, cx, cy] + list(rng.uniform(-0.01, 0.01, n - 4))
        cameras.append((c + 1, model, width, height, params))
    ids = list(image_ids) if image_ids is not None else list(range(1, n_images + 1))
    poses = []
    for i in range(n_images):
        a = 2 * math.pi * i / n_images * 0.35 + rng.uniform(-0.02, 0.02)
        center = np.array([8 * math.sin(a), rng.uniform(-0.5, 0.5), -8 * math.cos(a)])
        poses.append(_quat_look_at(center, rng.uniform(-0.3, 0.3, 3), rng))
    xyz = rng.uniform(-2, 2, (n_points, 3))
    tracks: List[np.ndarray] = []
    for p in range(n_points):
        L = int(min(n_images, max(2, rng.poisson(mean_track))))
        t = np.sort(rng.choice(n_images, L, replace=False))
        if disjoint_pair is not None and disjoint_pair[0] in t and disjoint_pair[1] in t:
            t = t[t != disjoint_pair[1]]  # (still >= 2 images: it held both members of the pair)
        tracks.append(t)
    if point_at_center_of is not None:
        from patchmatchnet_amd import colmap as C  # the centre exactly as the import computes it (-R^T t from qvec / tvec)
        q, t = poses[point_at_center_of]
        e = np.zeros((4, 4))
        e[:3, :3] = C.rotation_from_quaternion([float(v) for v in q])
        e[:3, 3] = t
        xyz[0] = C.camera_center(e)
        other = (point_at_center_of + 1) % n_images
        tracks[0] = np.sort(np.array([point_at_center_of, other]))
    per_image: List[List[int]] = [[] for _ in range(n_images)]
    point_ids = rng.permutation(np.arange(1, 3 * n_points + 1))[:n_points] + 100  # sparse, unordered ids
    for p, t in enumerate(tracks):
        for i in t:
            per_image[i].append(int(point_ids[p]))
    if duplicate_in is not None and per_image[duplicate_in]:
        per_image[duplicate_in].append(per_image[duplicate_in][0])
    images, obs = [], {}
    for i in range(n_images):
        pids = per_image[i] + [-1] * max(0, keypoints - len(per_image[i]))
        pids = rng.permutation(np.asarray(pids, np.int64))
        q, t = poses[i]
        cam = cameras[i % len(cameras)][0]
        images.append((ids[i], [float(v) for v in q], [float(v) for v in t], cam, "img_%03d.jpg" % i, pids))
        for k, pid in enumerate(pids):
            if pid != -1:
                obs.setdefault(int(pid), []).append((ids[i], k))
    points = [(int(point_ids[p]), [float(v) for v in xyz[p]], [int(v) for v in rng.integers(0, 256, 3)], 0.5,
               obs.get(int(point_ids[p]), [])) for p in rng.permutation(n_points)]
    return cameras, images, points


CASES: Dict[str, dict] = {
    "A": dict(model=dict(seed=11, n_images=10, n_points=600, keypoints=400, mean_track=4.0),
              args=dict(num_src_images=-1, theta0=5.0, sigma1=1.0, sigma2=10.0)),
    "B": dict(model=dict(seed=12, n_images=9, n_points=300, keypoints=180, mean_track=3.5,
                         camera_models=("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "OPENCV"), image_ids=[7, 3, 12, 5, 40, 1, 9, 22, 15],
                         disjoint_pair=(1, 6), duplicate_in=4, point_at_center_of=2),
              args=dict(num_src_images=4, theta0=3.0, sigma1=2.0, sigma2=8.0)),
}


def large_case() -> dict:
    """~300 images, ~100k points, mean track length ~6 (the GPU test's and the import benchmark's model)."""
    return dict(seed=13, n_images=300, n_points=100000, keypoints=2400, mean_track=6.0)


def write_images(image_dir: str, images, seed: int = 0) -> None:
    from PIL import Image as PilImage
    os.makedirs(image_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    for im in images:
        arr = rng.integers(0, 256, (24, 32, 3), dtype=np.uint8)
        PilImage.fromarray(arr).save(os.path.join(image_dir, im[4]))


def write_case(root: str, model_kw: dict) -> str:
    """<root>/sparse/*.bin and <root>/images/*; returns the sha256 of the three model files (what the golden was computed on)."""
    cams, imgs, pts = make_model(**model_kw)
    write_model(os.path.join(root, "sparse"), cams, imgs, pts)
    write_images(os.path.join(root, "images"), imgs, seed=model_kw.get("seed", 0))
    return model_digest(os.path.join(root, "sparse"))


def model_digest(sparse_dir: str) -> str:
    h = hashlib.sha256()
    for name in ("cameras.bin", "images.bin", "points3D.bin"):
        with open(os.path.join(sparse_dir, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def oracle_scores(model, theta0: float, sigma1: float, sigma2: float) -> np.ndarray:
    """numpy float64 restatement of the reference's scores by per-point pair enumeration: every observation of image i (in the
    image's order) of a point also observed by an image j > i adds its term to score[i, j] -- np.add.at adds them in that order."""
    from patchmatchnet_amd import colmap as C
    extr = [C.extrinsic_matrix(im) for im in model.images]
    centers = np.stack([C.camera_center(e) for e in extr])
    obs_ptr, obs_pt, trk_ptr, trk_img = C.view_selection_inputs(model)
    N = len(model.images)
    img = np.repeat(np.arange(N), np.diff(obs_ptr))
    lens = trk_ptr[obs_pt + 1] - trk_ptr[obs_pt]
    rep_i, rep_p = np.repeat(img, lens), np.repeat(obs_pt, lens)
    starts = np.repeat(trk_ptr[obs_pt], lens)
    offs = np.arange(len(rep_i)) - np.repeat(np.cumsum(lens) - lens, lens)
    rep_j = trk_img[starts + offs].astype(np.int64)
    keep = rep_j > rep_i
    i, j, p = rep_i[keep], rep_j[keep], rep_p[keep]
    ci, cj, x = centers[i], centers[j], model.xyz[p]
    a, b = ci - x, cj - x
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
        na = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        nb = np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])
        theta = (180 / np.pi) * np.arccos(dot / na / nb)
        s = np.where(theta <= theta0, sigma1, sigma2)
        term = np.exp(-(theta - theta0) * (theta - theta0) / (2 * s ** 2))
    score = np.zeros((N, N))
    np.add.at(score, (i, j), term)
    iu = np.triu_indices(N, 1)
    score[(iu[1], iu[0])] = score[iu]
    return score
