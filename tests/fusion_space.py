"""The fusion kernel space: one row per call of pmn_fuse_view / pmn_fuse_view_merged (FuseRow) and of pmn_pack_points /
pmn_pack_points_normals (PackRow) at the edges where such kernels go wrong -- image sizes on, one past and below the 32x8 tile,
sources smaller and larger than the reference, strides larger than the maps, slots out of order, 0 .. PMN_MAX_FUSE_SRC sources,
every side of geo_mask_thres, source cameras that see nothing / stand behind the surface / project into the one-pixel bands around the
image / overflow the fixed-point remap, holes and non-finite depths on either side, confidence on its threshold; for the packer pixel
counts around PMN_PACK_PIX and the 1024-pixel block, block counts around the scan's 1024-block chunk, empty and full masks, capacity
met and missed by one, a non-zero cursor, two views, colours on the truncation boundaries, both rotation strides.

Plain helper module (no tests here): tests/test_fusion_space.py checks the table on the CPU (coverage of every edge, the reference
tests/fusion_ref64.py against oracle/fusion_oracle.py, the fragile-share cap), tests/test_fusion_space_gpu.py runs every row on the
device.  ``python tests/fusion_space.py`` prints the fragile share of every row.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache
from typing import Dict, List, Tuple

import numpy as np

import fusion_ref64 as R64
import synth

THRESHOLDS = (1.0, 0.01, 0.5)  # geo_pixel_thres, geo_depth_thres, photo_thres (geo_mask_thres is the row's)
CLAIM_SENTINEL = 0xAA          # fill of the claim bytes no view owns


@dataclass(frozen=True)
class FuseRow:
    name: str
    H: int = 40
    W: int = 72
    n_src: int = 5
    src_sizes: Tuple[Tuple[int, int], ...] = ()  # (h, w) of every source; () = the reference's size
    mask_thres: int = 1
    prefill: bool = False   # a second merged pass with ``claimed`` pre-filled randomly
    slot_pad: int = 0       # floats added to slot_stride
    claim_pad: int = 0      # bytes added to claim_stride
    reorder: bool = False   # the reference in the LAST slot, the sources in descending slots
    camera: str = ""        # source 0 (and 1): away | behind | bands | huge
    bad_ref: bool = False   # reference depth with 0, negative, NaN and +inf pixels
    bad_src: bool = False   # every source depth with the same
    conf_tie: bool = False  # confidence exactly photo_thres on some pixels
    rel_tie: bool = False   # source 0 stands in the reference camera; its depths put ``rel`` exactly on geo_depth_thres or one ulp below
    spikes: bool = False    # single-pixel depth steps (x 1.03) in the sources: the claim's own depth test rejects
    step: float = 0.08      # angle between neighbouring cameras
    seed: int = 0

    @property
    def id(self) -> str:
        return self.name

    @property
    def friendly(self) -> bool:
        return not (self.camera or self.bad_ref or self.bad_src or self.rel_tie)


MIXED = ((40, 72), (24, 44), (30, 54), (36, 64))


def _fuse_rows() -> List[FuseRow]:
    R = [
        # image sizes and tile positions (32x8 tiles)
        FuseRow("1x1", H=1, W=1, n_src=1),
        FuseRow("2x3", H=2, W=3, n_src=2, prefill=True),
        FuseRow("8x32-exact-tile", H=8, W=32, n_src=2),
        FuseRow("9x33-one-past", H=9, W=33, n_src=3, mask_thres=2),
        FuseRow("7x31-one-short", H=7, W=31, n_src=2),
        FuseRow("40x72", prefill=True),
        # source sizes, strides, slot order
        FuseRow("mixed-sizes", H=30, W=54, n_src=4, src_sizes=MIXED, mask_thres=2, prefill=True, seed=1),
        FuseRow("mixed-sizes-padded-reordered", H=30, W=54, n_src=4, src_sizes=MIXED, mask_thres=2, slot_pad=37, claim_pad=13,
                reorder=True, prefill=True, seed=2),
        FuseRow("padded", H=9, W=33, n_src=3, slot_pad=1, claim_pad=1, seed=3),
        FuseRow("reordered", H=17, W=40, n_src=5, reorder=True, mask_thres=3, seed=4),
        # number of sources
        FuseRow("nsrc0-thres0", n_src=0, mask_thres=0),
        FuseRow("nsrc0-thres1", n_src=0, mask_thres=1),
        FuseRow("nsrc1", n_src=1, H=20, W=35),
        FuseRow("nsrc32", n_src=32, H=24, W=40, mask_thres=20, step=0.01, prefill=True),
        FuseRow("nsrc32-thres32", n_src=32, H=9, W=33, mask_thres=32, step=0.01, seed=5),
        # geo_mask_thres
        FuseRow("thres0", mask_thres=0, H=16, W=40, seed=6),
        FuseRow("thres-nsrc", mask_thres=5, H=16, W=40, step=0.03, seed=7),
        FuseRow("thres-nsrc-plus-1", mask_thres=6, H=16, W=40, step=0.03, seed=8),
        # source cameras
        FuseRow("camera-away", camera="away", seed=9),
        FuseRow("camera-behind", camera="behind", seed=10),
        FuseRow("camera-bands", camera="bands", prefill=True, seed=11),
        FuseRow("camera-bands-9x33", H=9, W=33, n_src=2, camera="bands", seed=12),
        FuseRow("camera-huge-focal", camera="huge", seed=13),
        # depth and confidence values
        FuseRow("bad-ref", bad_ref=True, seed=14),
        FuseRow("bad-src", bad_src=True, prefill=True, seed=15),
        FuseRow("bad-both-mixed", H=30, W=54, n_src=4, src_sizes=MIXED, bad_ref=True, bad_src=True, claim_pad=5, seed=16),
        FuseRow("conf-tie", conf_tie=True, H=16, W=40, seed=17),
        FuseRow("rel-tie", rel_tie=True, n_src=2, seed=20),
        # merged: a depth edge under a claim
        FuseRow("spikes", spikes=True, prefill=True, seed=18),
        FuseRow("spikes-mixed", H=30, W=54, n_src=4, src_sizes=MIXED, spikes=True, mask_thres=2, seed=19),
    ]
    return R


FUSE_ROWS = _fuse_rows()


def _rot_y(a: float) -> np.ndarray:
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float64)


@lru_cache(maxsize=None)
def _depth(K: bytes, E: bytes, h: int, w: int, seed: int) -> np.ndarray:
    Km = np.frombuffer(K, np.float32).reshape(1, 1, 3, 3)
    Em = np.frombuffer(E, np.float32).reshape(1, 1, 4, 4)
    return synth.render_scene(1, h, w, seed=seed, all_depths=True, cameras=(Km, Em))[3][0].numpy().astype(np.float32)


def _sprinkle(rng, d: np.ndarray) -> np.ndarray:
    """0, negative, NaN and +inf pixels (about 3 % each; on a map too small for that, one of each as far as the pixels go)."""
    d = d.copy()
    flat = d.reshape(-1)
    k = max(1, flat.size * 3 // 100)
    idx = rng.permutation(flat.size)
    for j, v in enumerate((0.0, None, np.nan, np.inf)):
        sel = idx[j * k:(j + 1) * k]
        flat[sel] = -flat[sel] if v is None else v
    return d


def _rel_ties(d_ref: np.ndarray, thr: np.float32) -> np.ndarray:
    """A source depth map for a source standing in the reference camera (the sample at an integer position is the source depth
    itself, and it comes back as depth_rep unchanged): where a float32 exists that makes |depth_rep - d_ref| / d_ref, in float32,
    exactly ``thr`` (even pixels) or the float32 below ``thr`` (odd pixels) it is that value, elsewhere d_ref."""
    out = d_ref.copy()
    want = np.where((np.arange(d_ref.size) % 2 == 0).reshape(d_ref.shape), thr, np.nextafter(thr, np.float32(0.0))).astype(np.float32)
    cand = (d_ref * (np.float32(1.0) + thr)).astype(np.float32)
    for _ in range(64):
        cand = np.nextafter(cand, np.float32(0.0))
    for _ in range(128):
        hit = (np.abs(cand - d_ref) / d_ref).astype(np.float32) == want
        out[hit] = cand[hit]
        cand = np.nextafter(cand, np.float32(np.inf))
    return out


@lru_cache(maxsize=None)
def scene(row: FuseRow) -> Dict:
    """The row's inputs: maps float32 [V,F] flat slots, sizes per slot, ref_slot, src_slots, mats, thresholds, views (the dicts
    oracle.fusion_oracle.fuse_view takes, reference first), claim_room (bytes per claim slot), prefilled (the random claim bytes of
    the second pass, sentinel outside every view)."""
    from patchmatchnet_amd import fusion
    rng = np.random.default_rng(1000 + row.seed)
    n = row.n_src
    sizes = [(row.H, row.W)] + [tuple(row.src_sizes[i]) if row.src_sizes else (row.H, row.W) for i in range(n)]
    views = []
    for i, (h, w) in enumerate(sizes):
        intr, extr = synth.synthetic_cameras(n + 1, h, w, step=row.step)
        K, E = intr[0, i].astype(np.float32), extr[0, i].astype(np.float32)
        Kd, Ed = K, E  # the camera the depth map is rendered in
        if row.camera and i == 1:
            if row.camera == "away":     # in front of the camera still, far outside its image
                E = (_rot_y(1.2) @ E.astype(np.float64)).astype(np.float32)
            elif row.camera == "behind":  # the whole surface behind the camera, its projections inside the image
                E = (np.diag([-1.0, 1.0, -1.0, 1.0]) @ E.astype(np.float64)).astype(np.float32)
            elif row.camera == "bands":  # a longer focal length: the projected grid reaches just past all four borders
                K = K.copy()
                K[0, 0] *= np.float32(1.05)
                K[1, 1] *= np.float32(1.05)
                Kd = K
            elif row.camera == "huge":
                K = K.copy()
                K[0, 0] = K[1, 1] = np.float32(1e9)
        if row.rel_tie and i == 1:
            K, E = views[0]["intrinsics"], views[0]["extrinsics"]
            Kd, Ed = K, E
        if row.camera == "behind" and i == 2:  # part of the surface behind this one
            E = (_rot_y(1.5) @ E.astype(np.float64)).astype(np.float32)
        d = _depth(Kd.tobytes(), Ed.tobytes(), h, w, row.seed) + rng.standard_normal((h, w)).astype(np.float32) * np.float32(0.02)
        d = d.astype(np.float32)
        c = (0.4 + 0.6 * rng.random((h, w))).astype(np.float32)
        if row.rel_tie and i == 1:
            d = _rel_ties(views[0]["depth"], np.float32(THRESHOLDS[1]))
        if row.spikes and i > 0:
            d[1::3, 1::3] *= np.float32(1.03)
        if (row.bad_ref and i == 0) or (row.bad_src and i > 0):
            d = _sprinkle(rng, d)
        if row.conf_tie and i == 0:
            c.reshape(-1)[::3] = np.float32(THRESHOLDS[2])
        views.append(dict(depth=d, confidence=c, intrinsics=K, extrinsics=E))
    V = n + 1
    slot_of = [V - 1 - i for i in range(V)] if row.reorder else list(range(V))
    slot_sizes = [None] * V
    for i, s in enumerate(slot_of):
        slot_sizes[s] = sizes[i]
    F = max(2 * h * w for h, w in sizes) + row.slot_pad
    maps = np.full((V, F), np.nan, np.float32)  # padding and the room behind a smaller view: NaN, read by no correct kernel
    for i, s in enumerate(slot_of):
        h, w = sizes[i]
        maps[s, :h * w] = views[i]["depth"].reshape(-1)
        maps[s, h * w:2 * h * w] = views[i]["confidence"].reshape(-1)
    mats = fusion.camera_block(views[0]["intrinsics"], views[0]["extrinsics"], [(v["intrinsics"], v["extrinsics"]) for v in views[1:]])
    room = max(h * w for h, w in sizes) + row.claim_pad
    prefilled = np.full((V, room), CLAIM_SENTINEL, np.uint8)
    for s, (h, w) in enumerate(slot_sizes):
        prefilled[s, :h * w] = (rng.random(h * w) < 0.3).astype(np.uint8)
    return dict(maps=maps, sizes=slot_sizes, ref_slot=slot_of[0], src_slots=slot_of[1:], mats=mats,
                thresholds=(THRESHOLDS[0], THRESHOLDS[1], row.mask_thres, THRESHOLDS[2]), views=views, claim_room=room,
                prefilled=prefilled)


def empty_claims(row: FuseRow) -> np.ndarray:
    """The claim bytes before a scan's first view: 0 inside every view's h*w, the sentinel behind it and in the stride padding."""
    sc = scene(row)
    c = np.full(sc["prefilled"].shape, CLAIM_SENTINEL, np.uint8)
    for s, (h, w) in enumerate(sc["sizes"]):
        c[s, :h * w] = 0
    return c


@lru_cache(maxsize=None)
def reference(row: FuseRow) -> Dict:
    """fusion_ref64 on the row, computed once: the view and the merged results on empty (and, for ``prefill`` rows, pre-filled) claims."""
    sc = scene(row)
    args = (sc["maps"], sc["sizes"], sc["ref_slot"], sc["src_slots"])
    view = R64.fuse_view_ref(*args, sc["mats"], sc["thresholds"])
    out = dict(view=view, merged=R64.merge_ref(view, *args, sc["thresholds"], empty_claims(row)))
    if row.prefill:
        out["merged_prefilled"] = R64.merge_ref(view, *args, sc["thresholds"], sc["prefilled"])
    return out


def fragile_share(row: FuseRow) -> Tuple[int, int]:
    """(fragile (pixel, source) entries, all entries) of the row."""
    f = reference(row)["view"]["fragile"]
    return int(f.sum()), int(f.size)


# ---- the packer ---------------------------------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class PackRow:
    name: str
    H: int
    W: int
    mask: str = "p5"            # zeros | ones | p01 | p5 | last
    float_image: bool = False
    normals: bool = False
    rot_stride: int = 3
    capacity: str = "exact"     # exact: cursor0 + total; short: one less (the view is refused); roomy: 100 more
    cursor0: int = 0
    second: Tuple[int, int, str] = ()  # a second view (H, W, mask) packed behind the first
    seed: int = 0

    @property
    def id(self) -> str:
        return self.name


def _pack_rows() -> List[PackRow]:
    R = []
    # pixel counts around PMN_PACK_PIX (4) and the 1024-pixel block; every record form at the small ones
    for i, n in enumerate((1, 3, 4, 5, 1023, 1024, 1025)):
        R.append(PackRow(f"n{n}-ones", 1, n, mask="ones", float_image=bool(i & 1), normals=bool(i & 2), rot_stride=3 + (i & 1), seed=i))
        R.append(PackRow(f"n{n}-p5", 1, n, mask="p5", float_image=not (i & 1), normals=not (i & 2), rot_stride=4 - (i & 1),
                         capacity="roomy", cursor0=i, seed=10 + i))
    R += [
        # masks
        PackRow("zeros", 33, 65, mask="zeros", float_image=True, seed=20),
        PackRow("zeros-cursor", 5, 7, mask="zeros", normals=True, cursor0=9, seed=21),
        PackRow("last-only", 33, 65, mask="last", seed=22),
        PackRow("last-only-1025", 1, 1025, mask="last", normals=True, float_image=True, seed=23),
        PackRow("p01", 40, 72, mask="p01", normals=True, rot_stride=4, seed=24),
        PackRow("p5-float-normals-stride4", 40, 72, float_image=True, normals=True, rot_stride=4, seed=25),
        PackRow("p5-float-normals-stride3", 40, 72, float_image=True, normals=True, rot_stride=3, seed=26),
        # capacity and cursor
        PackRow("short-by-one", 40, 72, capacity="short", seed=27),
        PackRow("short-by-one-cursor-normals", 9, 33, capacity="short", cursor0=17, normals=True, float_image=True, seed=28),
        PackRow("short-ones-1", 1, 1, mask="ones", capacity="short", seed=29),
        PackRow("cursor", 40, 72, cursor0=1000, seed=30),
        PackRow("two-views", 40, 72, second=(31, 57, "p5"), cursor0=3, float_image=True, seed=31),
        PackRow("two-views-normals-second-short", 9, 33, second=(40, 72, "ones"), normals=True, capacity="short", seed=32),
        # block counts around the scan's 1024-block chunk (the carry between chunks)
        PackRow("blocks1024", 1024, 1024, seed=33),
        PackRow("blocks1025", 1, 2 ** 20 + 1, seed=34),
        PackRow("blocks1025-last-only", 1, 2 ** 20 + 1, mask="last", seed=35),
    ]
    return R


PACK_ROWS = _pack_rows()


def _mask(rng, kind: str, n: int) -> np.ndarray:
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    if kind == "last":
        m = np.zeros(n, np.uint8)
        m[-1] = 1
        return m
    m = (rng.random(n) < {"p01": 0.01, "p5": 0.5}[kind]).astype(np.uint8)
    return m * rng.integers(1, 256, n).astype(np.uint8)  # any non-zero byte keeps the pixel


def colour_pool() -> np.ndarray:
    """Float colours in [0, 1] on the boundaries of (im * 255).astype(uint8): 0, 1, k/255 and its two float32 neighbours."""
    ks = np.array([1, 2, 3, 17, 64, 85, 127, 128, 170, 200, 254, 255], np.float32)
    v = (ks / np.float32(255.0)).astype(np.float32)
    pool = np.concatenate([[np.float32(0.0), np.float32(1.0)], v, np.nextafter(v, np.float32(0.0)), np.nextafter(v, np.float32(1.0))])
    return pool[(pool >= 0) & (pool <= 1)].astype(np.float32)


def pack_view(rng, H: int, W: int, kind: str, float_image: bool, normals: bool) -> Dict:
    n = H * W
    xyz = rng.standard_normal((H, W, 3)).astype(np.float32) * np.float32(300.0)
    if float_image:
        pool = colour_pool()
        image = np.where(rng.random((H, W, 3)) < 0.5, pool[rng.integers(0, len(pool), (H, W, 3))], rng.random((H, W, 3))).astype(np.float32)
    else:
        image = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    out = dict(mask=_mask(rng, kind, n).reshape(H, W), xyz=xyz, image=image)
    if normals:
        nrm = rng.standard_normal((3, H, W)).astype(np.float32)
        nrm /= np.maximum(np.linalg.norm(nrm, axis=0, keepdims=True), np.float32(1e-6))
        nrm[:, rng.random((H, W)) < 0.2] = 0.0  # invalid normals stay exactly zero
        out["normals"] = nrm.astype(np.float32)
    return out


def pack_inputs(row: PackRow) -> Dict:
    """views (one or two dicts of mask uint8 [H,W], xyz, image, normals), rotation float32 [3,3] or [4,4], expected record bytes per
    view, totals, capacity."""
    rng = np.random.default_rng(2000 + row.seed)
    views = [pack_view(rng, row.H, row.W, row.mask, row.float_image, row.normals)]
    if row.second:
        views.append(pack_view(rng, row.second[0], row.second[1], row.second[2], row.float_image, row.normals))
    rot = None
    if row.normals:
        rot = rng.standard_normal((row.rot_stride, row.rot_stride)).astype(np.float32)
    want = [pack_reference(v, rot) for v in views]
    totals = [len(w) for w in want]
    capacity = row.cursor0 + sum(totals) + {"exact": 0, "short": -1, "roomy": 100}[row.capacity]
    return dict(views=views, rotation=rot, want=want, totals=totals, capacity=capacity)


def pack_reference(view: Dict, rot) -> np.ndarray:
    """The records of one view in numpy, uint8 [M, 15 or 27]: boolean index in row-major order; x y z [nx ny nz] r g b; float colours
    as (im * 255).astype(uint8); normals (r0 cx + r1 cy) + r2 cz in float32."""
    keep = view["mask"].reshape(-1) != 0
    cols = [np.ascontiguousarray(view["xyz"].reshape(-1, 3)[keep]).view(np.uint8).reshape(-1, 12)]
    if "normals" in view:
        c = view["normals"].reshape(3, -1)[:, keep]
        r = np.asarray(rot, np.float32)
        world = np.stack([(r[k, 0] * c[0] + r[k, 1] * c[1]) + r[k, 2] * c[2] for k in range(3)], 1).astype(np.float32)
        cols.append(np.ascontiguousarray(world).view(np.uint8).reshape(-1, 12))
    im = view["image"].reshape(-1, 3)[keep]
    cols.append((im * 255).astype(np.uint8) if im.dtype == np.float32 else im)
    return np.concatenate(cols, 1)


if __name__ == "__main__":
    tot = [0, 0]
    for row_ in FUSE_ROWS:
        a_, b_ = fragile_share(row_)
        tot[0] += a_
        tot[1] += b_
        print("%-32s %6d of %8d  %.2e" % (row_.id, a_, b_, a_ / max(b_, 1)))
    print("%-32s %6d of %8d  %.2e" % ("table", tot[0], tot[1], tot[0] / tot[1]))
