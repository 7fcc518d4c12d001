"""What the command-line tools at the repository root share: the refusals, the job list, reading a cloud, writing
the kept points, side files and the loop over the files with its JSON report.  A new cloud tool keeps its docstring, parser, argument
checks, per-file function, report fields and printed lines and takes the rest from here; clean_cloud.py is the shortest example.
Importing this module imports neither torch nor patchmatchnet_amd: a tool can refuse its arguments with no device visible."""
import json
import os
import sys


def fail(tool: str, msg) -> int:
    """One line on stderr, `<tool>: <msg>` with the white space collapsed; returns the exit code 2."""
    print(f"{tool}: " + " ".join(str(msg).split()), file=sys.stderr)
    return 2


def refuse_torchrun(tool: str) -> bool:
    """True, after the refusal is printed, when the process runs under torchrun."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print(f"{tool}: single process, single GPU -- running under torchrun (WORLD_SIZE > 1) is not supported", file=sys.stderr)
        return True
    return False


def read_scan_list(path: str):
    """The scans of a list file: one per line, blank lines and surrounding white space dropped."""
    if not os.path.isfile(path):
        raise ValueError(f"invalid scan list file: {path}")
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def jobs(args, source_name: str, result_name: str, single_only: str = ""):
    """[(source, destination, scan)] of --input / --output / --scan_list: <input>/<scan>/<source_name> -> <output or input>/<scan>/
    <result_name> per scan of the list, or the one pair with scan "".  ValueError where the arguments do not name existing files, and
    with ``single_only`` as the message when it is given together with a scan list (flags that name one file)."""
    if args.scan_list:
        if not os.path.isdir(args.input):
            raise ValueError(f"--scan_list needs --input to be a folder, got {args.input}")
        scans = read_scan_list(args.scan_list)
        if single_only:
            raise ValueError(single_only)
        out = [(os.path.join(args.input, s, source_name), os.path.join(args.output or args.input, s, result_name), s) for s in scans]
    else:
        if not args.output:
            raise ValueError("--output is required for a single file")
        out = [(args.input, args.output, "")]
    for src, _, _ in out:
        if not os.path.isfile(src):
            raise ValueError(f"no such file: {src}")
    return out


def load_cloud(src: str, min_points: int = 1, mesh_hint: str = "", few_points_msg=None):
    """ply.read_ply_model(src); PmnError for a mesh (``mesh_hint`` says what to use instead) and for fewer than ``min_points`` points
    (``few_points_msg`` says why that many)."""
    from patchmatchnet_amd import ply
    from patchmatchnet_amd._lib import PmnError
    model = ply.read_ply_model(src)
    if model["faces"] is not None:
        raise PmnError(f"{src}: a mesh ({len(model['faces'])} faces), not a cloud" + ("; " + mesh_hint if mesh_hint else ""))
    n = len(model["vertices"])
    if n < min_points:
        raise PmnError(f"{src}: no points" if few_points_msg is None else f"{src}: {n} points; {few_points_msg}")
    return model


def device_of(args, device):
    """The device of the earlier files, or --device for the first: called once everything that can be refused without the GPU has been."""
    import torch
    return torch.device(args.device) if device is None else device


def upload(array, dtype, device):
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(array, dtype)).to(device)


def write_kept(dst: str, model, keep, colors=None, normals=None, vertices=None) -> None:
    """Writes the points of ``model`` under the mask ``keep``, unchanged and in order: white where the file had no colours, normals
    when it had them.  ``colors`` / ``normals`` / ``vertices``, one row per point of the file, take the place of the file's."""
    import numpy as np
    from patchmatchnet_amd import ply
    if colors is None:
        colors = model["colors"] if model["colors"] is not None else np.full((len(keep), 3), 255, np.uint8)
    if normals is None:
        normals = model["normals"]
    if vertices is None:
        vertices = model["vertices"]
    ply.write_ply(dst, vertices[keep], colors[keep], None if normals is None else normals[keep])


def save_side_file(path: str, saver) -> None:
    """``saver(path)`` after the folder of ``path`` exists."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    saver(path)


def write_report(path: str, report: dict) -> None:
    def dump(p):
        with open(p, "w") as f:
            json.dump(report, f, indent=1)
    save_side_file(path, dump)


def run(tool: str, jobs, per_file, settings: dict, report_path: str, also_catch=()) -> int:
    """The loop over the files: ``per_file(*job, device)`` returns (its report entry, the device in use), the device is None for
    the first file.  A PmnError (or one of ``also_catch``) ends the run with fail(); what earlier files wrote stays.  The report
    {"abi", **settings, "files"} is written to ``report_path``, when given, after the last file succeeded."""
    from patchmatchnet_amd import _lib
    files, device = [], None
    try:
        for job in jobs:
            one, device = per_file(*job, device)
            files.append(one)
    except (_lib.PmnError, *also_catch) as e:
        return fail(tool, e)
    if report_path:
        write_report(report_path, {"abi": _lib.ABI_VERSION, **settings, "files": files})
    return 0
