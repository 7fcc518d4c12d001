"""COLMAP sparse models in, MVSNet layout out (reference colmap_input.py), and back to a COLMAP dense workspace (reference
colmap_output.py).

    read_model(<input>/sparse)              cameras.bin / images.bin / points3D.bin (COLMAP's binary format)
    import_model(input, output, ...)        cams/%08d_cam.txt, pair.txt, images/%08d.jpg: what eval.py reads
    export_workspace(input, results, out)   images/, stereo/{depth,confidence}_maps/*.geometric.bin, stereo/*.cfg, sparse/*.txt

Host geometry is numpy float64 with the reference's semantics (intrinsics from its per-model parameter table, distortion ignored
unless import_model(undistort=True) / colmap_input.py --undistort resamples the pictures into pinhole cameras first: undistort.py;
extrinsics from qvec / tvec; depth range = the 1 % / 99 % order statistics of the camera-space z of every observation).  The one hot
path, the pairwise view-selection scores, runs on the GPU (pmn_view_scores through ops.view_scores); there is no CPU fallback.
"""
from __future__ import annotations

import os
import shutil
import struct
import time
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

# COLMAP's camera models: id -> (name, parameter names).  Only f / fx / fy / cx / cy are used (the reference ignores distortion)
# unless the import undistorts (undistort.py reads the rest).
CAMERA_MODELS: Dict[int, Tuple[str, Tuple[str, ...]]] = {
    0: ("SIMPLE_PINHOLE", ("f", "cx", "cy")),
    1: ("PINHOLE", ("fx", "fy", "cx", "cy")),
    2: ("SIMPLE_RADIAL", ("f", "cx", "cy", "k")),
    3: ("RADIAL", ("f", "cx", "cy", "k1", "k2")),
    4: ("OPENCV", ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")),
    5: ("OPENCV_FISHEYE", ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4")),
    6: ("FULL_OPENCV", ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")),
    7: ("FOV", ("fx", "fy", "cx", "cy", "omega")),
    8: ("SIMPLE_RADIAL_FISHEYE", ("f", "cx", "cy", "k")),
    9: ("RADIAL_FISHEYE", ("f", "cx", "cy", "k1", "k2")),
    10: ("THIN_PRISM_FISHEYE", ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "sx1", "sy1")),
}
CAMERA_MODEL_IDS = {name: mid for mid, (name, _) in CAMERA_MODELS.items()}

POINT2D_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("point3d_id", "<i8")])


class ColmapFormatError(ValueError):
    """A malformed COLMAP model: the message names the file and the record."""


class Camera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: Tuple[float, ...]


class Image(NamedTuple):
    id: int
    qvec: Tuple[float, float, float, float]
    tvec: Tuple[float, float, float]
    camera_id: int
    name: str
    points2d: np.ndarray  # POINT2D_DTYPE [n]: x, y, point3D_id (-1 = not triangulated)

    @property
    def point3d_ids(self) -> np.ndarray:
        return self.points2d["point3d_id"]


class Model(NamedTuple):
    cameras: Dict[int, Camera]
    images: List[Image]           # in images.bin order (= the output index)
    point_ids: np.ndarray         # int64 [P], ascending
    xyz: np.ndarray               # float64 [P, 3], row k = point point_ids[k]


class _Reader:
    def __init__(self, path: str) -> None:
        self.path = path
        with open(path, "rb") as f:
            self.buf = f.read()
        self.pos = 0

    def take(self, n: int, what: str) -> memoryview:
        if n < 0 or self.pos + n > len(self.buf):
            raise ColmapFormatError(f"{self.path}: truncated in {what} (needs {n} bytes at offset {self.pos}, file has "
                                    f"{len(self.buf)})")
        view = memoryview(self.buf)[self.pos:self.pos + n]
        self.pos += n
        return view

    def unpack(self, fmt: str, what: str) -> tuple:
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt), what))


def read_cameras_bin(path: str) -> Dict[int, Camera]:
    r = _Reader(path)
    (n,) = r.unpack("Q", "the camera count")
    cameras: Dict[int, Camera] = {}
    for k in range(n):
        cam_id, model_id, width, height = r.unpack("iiQQ", f"camera record {k}")
        if model_id not in CAMERA_MODELS:
            raise ColmapFormatError(f"{path}: camera record {k} (camera_id {cam_id}) has unknown camera model id {model_id}")
        name, pnames = CAMERA_MODELS[model_id]
        params = r.unpack("d" * len(pnames), f"camera record {k} (camera_id {cam_id}) parameters")
        cameras[cam_id] = Camera(cam_id, name, width, height, tuple(params))
    return cameras


def read_images_bin(path: str) -> List[Image]:
    r = _Reader(path)
    (n,) = r.unpack("Q", "the image count")
    images: List[Image] = []
    for k in range(n):
        head = r.unpack("idddddddi", f"image record {k}")
        img_id, qvec, tvec, cam_id = head[0], head[1:5], head[5:8], head[8]
        end = r.buf.find(b"\x00", r.pos)
        if end < 0:
            raise ColmapFormatError(f"{path}: truncated in image record {k} (image_id {img_id}): name without terminator")
        name = bytes(r.take(end - r.pos, f"image record {k} name")).decode("utf-8")
        r.take(1, f"image record {k} name")
        (npts,) = r.unpack("Q", f"image record {k} ({name}) point count")
        pts = np.frombuffer(r.take(POINT2D_DTYPE.itemsize * npts, f"image record {k} ({name}) 2-D points"), POINT2D_DTYPE)
        images.append(Image(img_id, tuple(qvec), tuple(tvec), cam_id, name, pts))
    return images


def read_points3d_bin(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(point ids int64 [P] ascending, xyz float64 [P,3]).  The tracks are skipped: the view selection reads the images' lists."""
    r = _Reader(path)
    (n,) = r.unpack("Q", "the point count")
    offs = np.empty(n, np.int64)
    buf, pos = r.buf, r.pos
    rec = struct.Struct("<Q")
    for k in range(n):
        if pos + 51 > len(buf):
            raise ColmapFormatError(f"{path}: truncated in point record {k} (needs 51 bytes at offset {pos}, file has {len(buf)})")
        offs[k] = pos
        (tl,) = rec.unpack_from(buf, pos + 43)
        pos += 51 + 8 * tl
        if pos > len(buf):
            raise ColmapFormatError(f"{path}: truncated in point record {k} track ({tl} entries)")
    head = np.frombuffer(buf, np.uint8)[offs[:, None] + np.arange(32)].copy() if n else np.empty((0, 32), np.uint8)
    ids = head[:, :8].copy().view("<u8")[:, 0].astype(np.int64)
    xyz = head[:, 8:32].copy().view("<f8").reshape(n, 3)
    order = np.argsort(ids, kind="stable")
    ids, xyz = ids[order], np.ascontiguousarray(xyz[order])
    if n and (np.diff(ids) == 0).any():
        dup = int(ids[np.flatnonzero(np.diff(ids) == 0)[0]])
        raise ColmapFormatError(f"{path}: point3D_id {dup} appears twice")
    return ids, xyz


def read_model(sparse_dir: str) -> Model:
    cameras = read_cameras_bin(os.path.join(sparse_dir, "cameras.bin"))
    images = read_images_bin(os.path.join(sparse_dir, "images.bin"))
    ids, xyz = read_points3d_bin(os.path.join(sparse_dir, "points3D.bin"))
    for im in images:
        if im.camera_id not in cameras:
            raise ColmapFormatError(f"{os.path.join(sparse_dir, 'images.bin')}: image {im.name} (image_id {im.id}) uses "
                                    f"camera_id {im.camera_id}, which cameras.bin does not define")
        pid = im.point3d_ids
        pid = pid[pid != -1]
        pos = np.searchsorted(ids, pid)
        bad = (pos >= len(ids)) | (ids[np.minimum(pos, max(len(ids) - 1, 0))] != pid) if len(ids) else np.ones(len(pid), bool)
        if bad.any():
            raise ColmapFormatError(f"{os.path.join(sparse_dir, 'images.bin')}: image {im.name} (image_id {im.id}) references "
                                    f"point3D_id {int(pid[np.flatnonzero(bad)[0]])}, which points3D.bin does not contain")
    return Model(cameras, images, ids, xyz)


# ---- host geometry ------------------------------------------------------------------------------------------------------------

def intrinsic_matrix(cam: Camera) -> np.ndarray:
    """3x3 float64 K from the model's f / fx / fy / cx / cy (distortion parameters are ignored, as in the reference, unless the import runs
    with undistort=True: it then passes the undistorted PINHOLE camera here)."""
    p = dict(zip(CAMERA_MODELS[CAMERA_MODEL_IDS[cam.model]][1], cam.params))
    fx, fy = (p["f"], p["f"]) if "f" in p else (p["fx"], p["fy"])
    return np.array([[fx, 0, p["cx"]], [0, fy, p["cy"]], [0, 0, 1]])


def rotation_from_quaternion(q: Sequence[float]) -> np.ndarray:
    """COLMAP's (w, x, y, z) unit quaternion -> 3x3 rotation, in Python float arithmetic."""
    w, x, y, z = q
    return np.array([
        [1 - 2 * y ** 2 - 2 * z ** 2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
        [2 * x * y + 2 * w * z, 1 - 2 * x ** 2 - 2 * z ** 2, 2 * y * z - 2 * w * x],
        [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2]])


def extrinsic_matrix(im: Image) -> np.ndarray:
    e = np.zeros((4, 4))
    e[:3, :3] = rotation_from_quaternion(im.qvec)
    e[:3, 3] = im.tvec
    e[3, 3] = 1
    return e


def camera_center(e: np.ndarray) -> np.ndarray:
    return -np.matmul(e[:3, :3].transpose(), e[:3, 3:4])[:, 0]


def depth_index(n: int) -> Tuple[int, int]:
    """Indices of the relaxed depth range in the n sorted depths: the float64 products n * .01 / n * .99, truncated."""
    return int(n * .01), int(n * .99)


def depth_ranges(model: Model, extrinsics: Sequence[np.ndarray]) -> List[Tuple[float, float]]:
    """Per image the 1 % / 99 % order statistics of the camera-space z of its observations (duplicates kept)."""
    out = []
    for im, e in zip(model.images, extrinsics):
        pid = im.point3d_ids
        pid = pid[pid != -1]
        if len(pid) == 0:
            raise ColmapFormatError(f"image {im.name} (image_id {im.id}) has no triangulated point: its depth range is undefined")
        p = model.xyz[np.searchsorted(model.point_ids, pid)]
        hom = np.concatenate([p, np.ones((len(p), 1))], axis=1)
        zs = np.sort(hom @ e[2])
        a, b = depth_index(len(zs))
        out.append((float(zs[a]), float(zs[b])))
    return out


def view_selection_inputs(model: Model):
    """CSR lists of pmn_view_scores: (obs_ptr int64 [N+1], obs_pt int32, trk_ptr int64 [P+1], trk_img int32)."""
    N, P = len(model.images), len(model.point_ids)
    per_image = []
    for im in model.images:
        pid = im.point3d_ids
        per_image.append(np.searchsorted(model.point_ids, pid[pid != -1]).astype(np.int32))
    counts = np.array([len(a) for a in per_image], np.int64)
    obs_ptr = np.zeros(N + 1, np.int64)
    np.cumsum(counts, out=obs_ptr[1:])
    obs_pt = np.concatenate(per_image) if N else np.empty(0, np.int32)
    img = np.repeat(np.arange(N, dtype=np.int64), counts)
    # distinct (point, image) pairs, sorted by point then image
    key = np.unique(obs_pt.astype(np.int64) * max(N, 1) + img)
    trk_pt, trk_img = key // max(N, 1), (key % max(N, 1)).astype(np.int32)
    trk_ptr = np.zeros(P + 1, np.int64)
    np.cumsum(np.bincount(trk_pt, minlength=P), out=trk_ptr[1:])
    return obs_ptr, obs_pt.astype(np.int32), trk_ptr, trk_img


def select_views(score: np.ndarray, num_src_images: int) -> List[List[Tuple[int, float]]]:
    """Per image the num_src_images best-scored images, best first (np.argsort reversed: ties and NaN sort as in the reference;
    with num_src_images < 0 every image, itself included, is listed)."""
    n = score.shape[0]
    k = n if num_src_images < 0 else num_src_images
    return [[(int(j), score[i, j]) for j in np.argsort(score[i])[::-1][:k]] for i in range(n)]


# ---- writers ------------------------------------------------------------------------------------------------------------------

def write_cam_file(path: str, extrinsic: np.ndarray, intrinsic: np.ndarray, depth_min: float, depth_max: float) -> None:
    lines = ["extrinsic\n"]
    lines += ["".join(str(extrinsic[r, c]) + " " for c in range(4)) + "\n" for r in range(4)]
    lines += ["\nintrinsic\n"]
    lines += ["".join(str(intrinsic[r, c]) + " " for c in range(3)) + "\n" for r in range(3)]
    lines += ["\n%f %f \n" % (depth_min, depth_max)]
    with open(path, "w") as f:
        f.writelines(lines)


def write_pair_file(path: str, view_sel: List[List[Tuple[int, float]]]) -> None:
    with open(path, "w") as f:
        f.write("%d\n" % len(view_sel))
        for i, sel in enumerate(view_sel):
            f.write("%d\n%d " % (i, len(sel)) + "".join("%d %f " % (j, s) for j, s in sel) + "\n")


def copy_images(image_dir: str, out_dir: str, names: Sequence[str], convert_format: bool = False) -> None:
    """images/<name> -> out_dir/%08d.jpg in the given order.  Every image first goes to a temporary name in out_dir and is renamed
    only after all of them are there: with out_dir == image_dir a source already called %08d.jpg is never overwritten before it has
    been copied.  convert_format re-encodes through PIL as JPEG quality 95 (the quality cv2.imwrite defaults to; the bytes are
    PIL's, not OpenCV's)."""
    os.makedirs(out_dir, exist_ok=True)
    tmp = []
    for i, name in enumerate(names):
        t = os.path.join(out_dir, ".pmn_import_%08d.tmp" % i)
        src = os.path.join(image_dir, name)
        if convert_format:
            from PIL import Image as PilImage
            with PilImage.open(src) as im:
                im.convert("RGB").save(t, "JPEG", quality=95)
        else:
            shutil.copyfile(src, t)
        tmp.append(t)
    for i, t in enumerate(tmp):
        os.replace(t, os.path.join(out_dir, "%08d.jpg" % i))


def undistort_images(image_dir: str, out_dir: str, names: Sequence[str], cameras: Sequence[Camera], dst_cameras: Sequence[Camera],
                     device) -> float:
    """images/<name> -> out_dir/%08d.jpg, each picture resampled from cameras[i] into dst_cameras[i] on the GPU (ops.undistort_image)
    and written as JPEG quality 95 through PIL, with copy_images' temporary-name protocol.  Decoding and encoding run on a small
    thread pool; every GPU call is made from this thread.  Returns the device time of the resampling in seconds, summed over the
    images."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image as PilImage
    from . import ops
    os.makedirs(out_dir, exist_ok=True)

    def decode(i: int) -> np.ndarray:
        with PilImage.open(os.path.join(image_dir, names[i])) as im:
            arr = np.array(im.convert("RGB"), dtype=np.uint8)  # (a copy: PIL's buffer is read-only)
        cam = cameras[i]
        if arr.shape[:2] != (cam.height, cam.width):
            raise ColmapFormatError(f"image {names[i]} is {arr.shape[1]} x {arr.shape[0]} but its camera (camera_id {cam.id}) is "
                                    f"{cam.width} x {cam.height}: it cannot be undistorted with that camera")
        return arr

    def encode(i: int, arr: np.ndarray) -> str:
        t = os.path.join(out_dir, ".pmn_import_%08d.tmp" % i)
        PilImage.fromarray(arr).save(t, "JPEG", quality=95)
        return t

    n, ahead, device_ms, tmp = len(names), 4, 0.0, []
    with ThreadPoolExecutor(max_workers=min(8, max(1, os.cpu_count() or 1))) as pool, torch.cuda.device(device):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        decoded = {i: pool.submit(decode, i) for i in range(min(ahead, n))}
        for i in range(n):
            arr = decoded.pop(i).result()
            if i + ahead < n:
                decoded[i + ahead] = pool.submit(decode, i + ahead)
            img = torch.from_numpy(arr).to(device)
            start.record()
            out = ops.undistort_image(img, cameras[i], dst_cameras[i])
            stop.record()
            host = out.cpu().numpy()  # (synchronises: the events are complete)
            device_ms += start.elapsed_time(stop)
            tmp.append(pool.submit(encode, i, host))
        tmp = [t.result() for t in tmp]
    for i, t in enumerate(tmp):
        os.replace(t, os.path.join(out_dir, "%08d.jpg" % i))
    return device_ms / 1e3


def _warn_ignored_distortion(model: Model) -> None:
    from . import undistort as U
    names = sorted({cam.model for cam in model.cameras.values() if U.has_distortion(cam)})
    if names:
        import sys
        print(f"colmap import: the model has cameras with non-zero distortion parameters ({', '.join(names)}) and they are ignored: "
              "the pictures must already be undistorted, or pass --undistort", file=sys.stderr)


def import_model(input_folder: str, output_folder: str = "", num_src_images: int = -1, theta0: float = 5, sigma1: float = 1,
                 sigma2: float = 10, convert_format: bool = False, device: str = "cuda:0", undistort: bool = False,
                 blank_pixels: float = 0.0, min_scale: float = 0.2, max_scale: float = 2.0, max_image_size: int = -1) -> Dict[str, float]:
    """<input>/sparse + <input>/images -> <output>/cams, <output>/pair.txt, <output>/images.  Returns the wall time of each phase
    in seconds (read, prepare, view_scores = device time of pmn_view_scores, write).

    ``undistort``: for a raw model (cameras with distortion, pictures as taken).  One ideal PINHOLE camera is computed per COLMAP
    camera (undistort.undistorted_camera with blank_pixels / min_scale / max_scale / max_image_size), every picture is resampled into
    it on the GPU and written as JPEG quality 95, and the cam files carry the undistorted intrinsics; extrinsics, depth ranges and
    pair.txt do not depend on the intrinsics.  The result gains "undistort", the device time of the resampling summed over the images.
    Without it the distortion parameters are ignored, as in the reference (one line on stderr says so when any is non-zero)."""
    import torch
    from . import ops
    output_folder = output_folder or input_folder
    if not os.path.isdir(input_folder):
        raise ValueError(f"invalid input folder {input_folder!r}")
    if not os.path.isdir(output_folder):
        raise ValueError(f"invalid output folder {output_folder!r}")
    times: Dict[str, float] = {}
    t = time.perf_counter()
    model = read_model(os.path.join(input_folder, "sparse"))
    times["read"] = time.perf_counter() - t

    t = time.perf_counter()
    if undistort:
        from . import undistort as U
        und = {cid: U.undistorted_camera(cam, blank_pixels, min_scale, max_scale, max_image_size) for cid, cam in model.cameras.items()}
        intr = {cid: intrinsic_matrix(cam) for cid, cam in und.items()}
    else:
        intr = {cid: intrinsic_matrix(cam) for cid, cam in model.cameras.items()}
        _warn_ignored_distortion(model)
    extr = [extrinsic_matrix(im) for im in model.images]
    ranges = depth_ranges(model, extr)
    centers = np.stack([camera_center(e) for e in extr]) if extr else np.zeros((0, 3))
    csr = view_selection_inputs(model)
    dev = torch.device(device)
    up = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (centers, model.xyz) + csr]
    times["prepare"] = time.perf_counter() - t

    N = len(model.images)
    if N:
        with torch.cuda.device(dev):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            score_dev = ops.view_scores(*up, theta0, sigma1, sigma2)
            stop.record()
            score = score_dev.cpu().numpy()
            times["view_scores"] = start.elapsed_time(stop) / 1e3
    else:
        score = np.zeros((0, 0))
        times["view_scores"] = 0.0

    t = time.perf_counter()
    view_sel = select_views(score, num_src_images)
    cam_dir = os.path.join(output_folder, "cams")
    os.makedirs(cam_dir, exist_ok=True)
    for i, im in enumerate(model.images):
        write_cam_file(os.path.join(cam_dir, "%08d_cam.txt" % i), extr[i], intr[im.camera_id], *ranges[i])
    write_pair_file(os.path.join(output_folder, "pair.txt"), view_sel)
    if undistort:
        times["undistort"] = undistort_images(os.path.join(input_folder, "images"), os.path.join(output_folder, "images"),
                                              [im.name for im in model.images], [model.cameras[im.camera_id] for im in model.images],
                                              [und[im.camera_id] for im in model.images], dev)
    else:
        copy_images(os.path.join(input_folder, "images"), os.path.join(output_folder, "images"), [im.name for im in model.images],
                    convert_format)
    times["write"] = time.perf_counter() - t
    return times


# ---- export: MVSNet layout + depth / confidence maps -> COLMAP dense workspace ----------------------------------------------

def rotation_matrix_to_quaternion(rot: np.ndarray) -> List[float]:
    """(w, x, y, z), w >= 0, of a rotation matrix by Bar-Itzhack's method: the eigenvector of the largest eigenvalue of the symmetric
    4x4 matrix built from the entries.  The entries' sums are taken in the matrix's own dtype (float32 when it comes from a camera
    file) and the eigen-decomposition in float64."""
    r = np.asarray(rot)
    m = np.zeros((4, 4))
    m[0, 0] = r[0, 0] - r[1, 1] - r[2, 2]
    m[1, 1] = r[1, 1] - r[0, 0] - r[2, 2]
    m[2, 2] = r[2, 2] - r[0, 0] - r[1, 1]
    m[3, 3] = r[0, 0] + r[1, 1] + r[2, 2]
    m[1, 0] = r[0, 1] + r[1, 0]
    m[2, 0] = r[0, 2] + r[2, 0]
    m[2, 1] = r[1, 2] + r[2, 1]
    m[3, 0] = r[2, 1] - r[1, 2]
    m[3, 1] = r[0, 2] - r[2, 0]
    m[3, 2] = r[1, 0] - r[0, 1]
    vals, vecs = np.linalg.eigh(m / 3.0, UPLO="L")
    v = vecs[:, int(np.argmax(vals))]
    q = np.array([v[3], v[0], v[1], v[2]])
    if q[0] < 0:
        q = -q
    return [q[0], q[1], q[2], q[3]]


def export_workspace(input_folder: str, results_folder: str = "", output_folder: str = "", normal_maps: bool = False,
                     device: str = "cuda:0", normals_radius: int = 2, normals_depth_thres: float = 0.01) -> None:
    """MVSNet-layout input (cams/, images/, pair.txt) + eval.py results (depth_est/, confidence/ as .pfm or .bin) -> a COLMAP dense
    workspace: images/, stereo/{depth,confidence}_maps/<image>.geometric.bin, stereo/patch-match.cfg, stereo/fusion.cfg, and a
    PINHOLE text model with no points in sparse/.  Views are listed in ascending id order.

    ``normal_maps``: additionally stereo/normal_maps/<image>.geometric.bin for every image -- COLMAP's stereo_fusion opens one per
    image of fusion.cfg -- computed on ``device`` from the exported depth map (ops.depth_normals) with the cam
    file's intrinsics scaled to the map's size as eval.py scales them.  Needs a ROCm device (checked before anything is written);
    without the flag the export is host-only and stereo/normal_maps/ stays empty, as the reference leaves it."""
    from PIL import Image as PilImage
    from .data_io import read_cam_file, read_map, read_pair_file, save_bin
    if normal_maps:
        import torch
        from ._lib import PmnError
        if torch.device(device).type != "cuda" or not torch.cuda.is_available():
            raise PmnError(f"--normal_maps needs a ROCm GPU (pmn_depth_normals has no CPU fallback): device {device!r} is not one, "
                           "or none is visible; nothing was written")
        from . import ops
    results_folder = results_folder or input_folder
    output_folder = output_folder or input_folder
    for what, d in (("input", input_folder), ("results", results_folder), ("output", output_folder)):
        if not os.path.isdir(d):
            raise ValueError(f"invalid {what} folder {d!r}")
    for sub in ("images", "sparse", "stereo", "stereo/confidence_maps", "stereo/consistency_graphs", "stereo/depth_maps",
                "stereo/normal_maps"):
        os.makedirs(os.path.join(output_folder, sub), exist_ok=True)
    shutil.copytree(os.path.join(input_folder, "images"), os.path.join(output_folder, "images"), dirs_exist_ok=True)

    depth_dir, conf_dir = os.path.join(results_folder, "depth_est"), os.path.join(results_folder, "confidence")
    for image_file in sorted(os.listdir(os.path.join(input_folder, "images"))):
        stem = os.path.splitext(image_file)[0]
        for src_dir, kind in ((depth_dir, "depth_maps"), (conf_dir, "confidence_maps")):
            src = next((os.path.join(src_dir, stem + ext) for ext in (".pfm", ".bin")
                        if os.path.isfile(os.path.join(src_dir, stem + ext))), None)
            if src is None:
                raise FileNotFoundError(f"no {kind[:-5]} map for image {image_file} in {src_dir}")
            dst = os.path.join(output_folder, "stereo", kind, image_file + ".geometric.bin")
            if src.endswith(".bin"):
                shutil.copyfile(src, dst)
            else:
                save_bin(dst, np.ascontiguousarray(read_map(src)))
            if normal_maps and kind == "depth_maps":
                depth = np.ascontiguousarray(read_map(src), np.float32)
                depth = depth.reshape(depth.shape[0], depth.shape[1])
                with PilImage.open(os.path.join(input_folder, "images", image_file)) as im:
                    w0, h0 = im.width, im.height
                K, _, _ = read_cam_file(os.path.join(input_folder, "cams", stem + "_cam.txt"))
                K[0] *= depth.shape[1] / w0  # eval.py's _scan_cameras: the intrinsics at the MAP's size
                K[1] *= depth.shape[0] / h0
                nrm = ops.depth_normals(torch.from_numpy(depth).to(device), K, normals_radius, normals_depth_thres)
                save_bin(os.path.join(output_folder, "stereo", "normal_maps", image_file + ".geometric.bin"),
                         np.ascontiguousarray(nrm.permute(1, 2, 0).cpu().numpy()))

    cameras, images = [], []
    for cam_file in sorted(os.listdir(os.path.join(input_folder, "cams"))):
        stem = cam_file.split("_")[0]
        vid, im_file = int(stem), stem + ".jpg"
        with PilImage.open(os.path.join(input_folder, "images", im_file)) as im:
            width, height = im.width, im.height
        K, E, _ = read_cam_file(os.path.join(input_folder, "cams", cam_file))
        cameras.append((vid, width, height, [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]))
        images.append((vid, rotation_matrix_to_quaternion(E[0:3, 0:3]), list(E[0:3, 3]), im_file))
    names = {vid: name for vid, _, _, name in images}
    pairs = read_pair_file(os.path.join(input_folder, "pair.txt"))

    with open(os.path.join(output_folder, "stereo", "patch-match.cfg"), "w") as f:
        for ref, src in pairs:
            f.write(names[ref] + "\n" + ", ".join(names[s] for s in src) + "\n")
    with open(os.path.join(output_folder, "stereo", "fusion.cfg"), "w") as f:
        f.writelines(",".join(names[v] for v in [ref] + src) + "\n" for ref, src in pairs)
    sparse = os.path.join(output_folder, "sparse")
    with open(os.path.join(sparse, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        f.write("# Number of cameras: {}\n".format(len(cameras)))
        f.writelines("{} PINHOLE {} {} {} {} {} {}\n".format(vid, w, h, *p) for vid, w, h, p in cameras)
    with open(os.path.join(sparse, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n")
        f.write("#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        f.write("# Number of images: {}, mean observations per image: 0\n".format(len(images)))
        f.writelines("{} {} {} {} {} {} {} {} {} {}\n\n".format(vid, *q, *t, vid, name) for vid, q, t, name in images)
    with open(os.path.join(sparse, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        f.write("#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        f.write("# Number of points: 0, mean track length: 0")
