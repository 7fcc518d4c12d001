"""How far two surfaces lie from each other, on the GPU: the yardstick for anything that changes a mesh.

    python compare_mesh.py --a before.ply --b after.ply [--spacing S] [--seed N] [--max_dist D] [--report FILE.json]

Per direction (a -> b, b -> a) it prints the count, mean, RMS, median, 95th percentile and maximum of the distances from the source to
the target, and the symmetric Hausdorff distance (the larger of the two maxima).  The queries of a direction are points drawn on the
source's triangles --spacing apart (meshops.sample_surface) or, with --spacing 0 or for a file without faces, its vertices.  The
distance is the exact point-to-triangle distance (meshops.point_mesh_distance) where the target has faces, else the distance to its
nearest point (pointcloud.nn_distance); both are capped at --max_dist (default: twice the diagonal of the two files' common bounding box,
which no distance reaches).  One process on one ROCm GPU; torchrun is not supported."""
import argparse
import sys

import cloud_tool


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Distances between two PLY meshes or clouds on a ROCm GPU, in both directions. Single process "
                                            "on one GPU; torchrun is not supported.")
    p.add_argument("--a", required=True, help="PLY mesh or cloud")
    p.add_argument("--b", required=True, help="PLY mesh or cloud")
    p.add_argument("--spacing", type=float, default=0.0, help="draw the queries on the source's triangles this far apart (0: its vertices)")
    p.add_argument("--seed", type=int, default=0, help="seed of --spacing's points")
    p.add_argument("--max_dist", type=float, default=None, help="cap of the distances (default: twice the common bounding box's diagonal)")
    p.add_argument("--report", default="", help="also write the figures to this JSON file")
    p.add_argument("--device", default="cuda:0")
    return p


def statistics(d) -> dict:
    """count, mean, rms, median, p95 and max of a float64 tensor of distances (numpy's median and linear-interpolated percentile)."""
    import torch
    n = int(d.numel())
    s = torch.sort(d).values
    pos = 0.95 * (n - 1)
    lo = int(pos)
    hi = min(lo + 1, n - 1)
    return {"count": n, "mean": float(d.mean()), "rms": float(torch.sqrt((d * d).mean())),
            "median": float((s[(n - 1) // 2] + s[n // 2]) / 2), "p95": float(s[lo] + (s[hi] - s[lo]) * (pos - lo)), "max": float(s[-1])}


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if cloud_tool.refuse_torchrun("compare_mesh.py"):
        return 2
    import torch

    from patchmatchnet_amd import PmnError, meshops, pointcloud as PC, render
    if args.spacing < 0:
        raise PmnError("--spacing must be >= 0")
    models = {}
    for name, path in (("a", args.a), ("b", args.b)):
        m = render.read_ply_model(path)
        v = torch.from_numpy(m["vertices"]).to(args.device).contiguous()
        if v.shape[0] < 1:
            raise PmnError(f"{path}: no vertices")
        f = None if m["faces"] is None or len(m["faces"]) == 0 else torch.from_numpy(m["faces"]).to(args.device).contiguous()
        models[name] = (path, v, f)
    both = torch.cat([models["a"][1], models["b"][1]])
    diagonal = float((both.max(0).values.double() - both.min(0).values.double()).norm())
    max_dist = args.max_dist if args.max_dist is not None else max(2.0 * diagonal, 1.0)
    if not max_dist > 0:
        raise PmnError("--max_dist must be positive")
    out = {"a": args.a, "b": args.b, "spacing": args.spacing, "seed": args.seed, "max_dist": max_dist}
    for src, dst in (("a", "b"), ("b", "a")):
        _, sv, sf = models[src]
        _, tv, tf = models[dst]
        sampled = args.spacing > 0 and sf is not None
        query = meshops.sample_surface(sv, sf, spacing=args.spacing, seed=args.seed)[0] if sampled else sv
        if query.shape[0] < 1:
            raise PmnError(f"{models[src][0]}: --spacing {args.spacing} draws no point on it; use a smaller spacing")
        if tf is not None:
            d = meshops.point_mesh_distance(query, meshops.build_face_grid(tv, tf), max_dist)
        else:
            d = PC.nn_distance(query, PC.build_grid(tv, PC.default_cell(tv)), max_dist)
        st = statistics(d)
        st.update({"queries": "samples" if sampled else "vertices", "target": "triangles" if tf is not None else "points"})
        out[f"{src}_to_{dst}"] = st
        print("%s -> %s (%s to %s): count %d, mean %.9g, rms %.9g, median %.9g, p95 %.9g, max %.9g"
              % (src, dst, st["queries"], st["target"], st["count"], st["mean"], st["rms"], st["median"], st["p95"], st["max"]))
    out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"])
    print("hausdorff: %.9g" % out["hausdorff"])
    if args.report:
        cloud_tool.write_report(args.report, out)
    return 0


if __name__ == "__main__":
    from patchmatchnet_amd import PmnError
    try:
        sys.exit(main())
    except PmnError as e:
        sys.exit("compare_mesh.py: " + str(e))
