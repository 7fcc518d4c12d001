"""cloud_tool.py, what the command-line tools at the repository root share: the job list, reading a cloud, writing the kept points, the
refusals of the five cloud tools that come from it and the loop with its report.  None of it needs a GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cloud_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("clean_cloud", "cloud_normals", "mesh_cloud", "cluster_cloud", "segment_cloud")
TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))


def _args(**kw):
    return argparse.Namespace(**{"input": "", "output": "", "scan_list": "", **kw})


def test_jobs_of_a_single_file(tmp_path):
    src = tmp_path / "a.ply"
    src.write_bytes(b"")
    assert cloud_tool.jobs(_args(input=str(src), output="b.ply"), "fused.ply", "x.ply") == [(str(src), "b.ply", "")]
    with pytest.raises(ValueError, match="^--output is required for a single file$"):
        cloud_tool.jobs(_args(input=str(src)), "fused.ply", "x.ply")
    with pytest.raises(ValueError, match="^no such file: .*missing.ply$"):
        cloud_tool.jobs(_args(input=str(tmp_path / "missing.ply"), output="b.ply"), "fused.ply", "x.ply")


def test_jobs_of_a_scan_list(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("scan1  \n\n  scan 2\t\n")
    assert cloud_tool.read_scan_list(str(lst)) == ["scan1", "scan 2"]
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    for s in ("scan1", "scan 2"):
        os.makedirs(os.path.join(data, s))
        open(os.path.join(data, s, "in.ply"), "w").close()
    want = [(os.path.join(data, s, "in.ply"), os.path.join(out, s, "res.ply"), s) for s in ("scan1", "scan 2")]
    assert cloud_tool.jobs(_args(input=data, output=out, scan_list=str(lst)), "in.ply", "res.ply") == want
    under_input = cloud_tool.jobs(_args(input=data, scan_list=str(lst)), "in.ply", "res.ply")  # no --output: next to the sources
    assert [d for _, d, _ in under_input] == [os.path.join(data, s, "res.ply") for s in ("scan1", "scan 2")]
    with pytest.raises(ValueError, match="^no such file: .*scan1.fused.ply$"):
        cloud_tool.jobs(_args(input=data, scan_list=str(lst)), "fused.ply", "res.ply")
    with pytest.raises(ValueError, match="^--scan_list needs --input to be a folder, got .*list.txt$"):
        cloud_tool.jobs(_args(input=str(lst), scan_list=str(lst)), "in.ply", "res.ply")
    with pytest.raises(ValueError, match="^invalid scan list file: .*none.txt$"):
        cloud_tool.jobs(_args(input=data, scan_list=str(tmp_path / "none.txt")), "in.ply", "res.ply")
    # a flag that names one file is refused after the list is known to exist and before its scans are looked for
    with pytest.raises(ValueError, match="^one file only$"):
        cloud_tool.jobs(_args(input=data, scan_list=str(lst)), "fused.ply", "res.ply", single_only="one file only")
    with pytest.raises(ValueError, match="^invalid scan list file"):
        cloud_tool.jobs(_args(input=data, scan_list=str(tmp_path / "none.txt")), "in.ply", "res.ply", single_only="one file only")


def test_load_cloud(tmp_path):
    from patchmatchnet_amd import ply
    from patchmatchnet_amd._lib import PmnError
    path = str(tmp_path / "m.ply")
    ply.write_ply_mesh(path, *TRIANGLE)
    with pytest.raises(PmnError, match=r"m.ply: a mesh \(1 faces\), not a cloud; use the other tool$"):
        cloud_tool.load_cloud(path, mesh_hint="use the other tool")
    with pytest.raises(PmnError, match=r"m.ply: a mesh \(1 faces\), not a cloud$"):
        cloud_tool.load_cloud(path)
    for n in (0, 2, 5):
        ply.write_ply(str(tmp_path / f"{n}.ply"), np.arange(3 * n, dtype=np.float32).reshape(n, 3), np.zeros((n, 3), np.uint8))
    with pytest.raises(PmnError, match="0.ply: no points$"):
        cloud_tool.load_cloud(str(tmp_path / "0.ply"))
    with pytest.raises(PmnError, match="2.ply: 2 points; a plane needs 3$"):
        cloud_tool.load_cloud(str(tmp_path / "2.ply"), min_points=3, few_points_msg="a plane needs 3")
    model = cloud_tool.load_cloud(str(tmp_path / "5.ply"), min_points=3, few_points_msg="a plane needs 3")
    assert model["faces"] is None and np.array_equal(model["vertices"], np.arange(15, dtype=np.float32).reshape(5, 3))


def test_write_kept(tmp_path):
    from patchmatchnet_amd import ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((6, 3)).astype(np.float32)
    c = rng.integers(0, 255, (6, 3)).astype(np.uint8)
    n = rng.standard_normal((6, 3)).astype(np.float32)
    keep = np.array([True, False, True, False, False, True])
    dst = str(tmp_path / "sub" / "out.ply")
    os.makedirs(tmp_path / "sub")

    def written(model, **kw):
        cloud_tool.write_kept(dst, model, keep, **kw)
        return ply.read_ply_model(dst)

    m = written({"vertices": v, "colors": c, "normals": n})
    assert m["faces"] is None and np.array_equal(m["vertices"], v[keep])
    assert np.array_equal(m["colors"], c[keep]) and np.array_equal(m["normals"], n[keep])
    m = written({"vertices": v, "colors": None, "normals": n})
    assert m["colors"].shape == (3, 3) and (m["colors"] == 255).all() and np.array_equal(m["normals"], n[keep])
    m = written({"vertices": v, "colors": c, "normals": None})
    assert m["normals"] is None and np.array_equal(m["colors"], c[keep])
    other_c, other_n = (255 - c).astype(np.uint8), -n
    m = written({"vertices": v, "colors": c, "normals": n}, colors=other_c)
    assert np.array_equal(m["colors"], other_c[keep]) and np.array_equal(m["normals"], n[keep])
    m = written({"vertices": v, "colors": None, "normals": None}, normals=other_n)
    assert np.array_equal(m["normals"], other_n[keep]) and (m["colors"] == 255).all() and np.array_equal(m["vertices"], v[keep])


def test_side_files_make_their_folder(tmp_path):
    path = str(tmp_path / "a" / "b" / "labels.npy")
    cloud_tool.save_side_file(path, lambda p: np.save(p, np.arange(3)))
    assert np.array_equal(np.load(path), np.arange(3))
    cloud_tool.write_report(str(tmp_path / "c" / "r.json"), {"b": 1, "a": [2]})
    assert (tmp_path / "c" / "r.json").read_text() == '{\n "b": 1,\n "a": [\n  2\n ]\n}'


def _refusal_cases(tmp_path):
    """(name, argv, environment, word of the message) of the refusals every cloud tool takes from cloud_tool.py."""
    from patchmatchnet_amd import ply
    cloud, mesh, out = str(tmp_path / "fused.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "out.ply")
    ply.write_ply(cloud, np.eye(5, 3, dtype=np.float32), np.zeros((5, 3), np.uint8))
    ply.write_ply_mesh(mesh, *TRIANGLE)
    return out, [("missing", ["--input", str(tmp_path / "missing.ply"), "--output", out], {}, "no such file: "),
                 ("mesh", ["--input", mesh, "--output", out], {}, "a mesh (1 faces), not a cloud"),
                 ("torchrun", ["--input", cloud, "--output", out], {"WORLD_SIZE": "2"}, "torchrun (WORLD_SIZE > 1) is not supported"),
                 ("no output", ["--input", cloud], {}, "--output is required for a single file"),
                 ("no list", ["--input", str(tmp_path), "--output", str(tmp_path / "o"), "--scan_list", str(tmp_path / "none.txt")], {},
                  "invalid scan list file: ")]


@pytest.mark.parametrize("tool", TOOLS)
def test_shared_refusals(tool, tmp_path, monkeypatch, capsys):
    """In the tool's own main(): exit code 2, nothing on stdout, one line on stderr that starts with the tool's name, no output file and
    no device."""
    module = __import__(tool)
    out, cases = _refusal_cases(tmp_path)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    for name, argv, env, word in cases:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            assert module.main(argv) == 2, name
        got = capsys.readouterr()
        assert got.out == "", (name, got.out)
        lines = got.err.splitlines()
        assert len(lines) == 1 and lines[0].startswith(tool + ".py: ") and word in lines[0], (name, got.err)
        assert not os.path.exists(out) and not os.path.exists(tmp_path / "o"), name


@pytest.mark.parametrize("tool", TOOLS)
def test_refusal_as_a_process(tool, tmp_path):
    """The same through the command line, for the exit code: under torchrun, which a tool refuses before it imports anything."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK")}
    env.update(WORLD_SIZE="2", HIP_VISIBLE_DEVICES="")
    out = str(tmp_path / "out.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, tool + ".py"), "--input", str(tmp_path / "fused.ply"), "--output", out],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 2 and r.stdout == "", (r.returncode, r.stdout)
    assert r.stderr == f"{tool}.py: single process, single GPU -- running under torchrun (WORLD_SIZE > 1) is not supported\n"
    assert not os.path.exists(out)


def test_importing_the_tools_imports_no_gpu_code():
    code = ("import sys, cloud_tool, " + ", ".join(TOOLS) + "; "
            "sys.exit(any(m == 'torch' or m.startswith('patchmatchnet_amd') for m in sys.modules))")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, timeout=120).returncode == 0


def test_a_failure_part_way_through_a_list(tmp_path, monkeypatch, capsys):
    import clean_cloud
    from patchmatchnet_amd._lib import ABI_VERSION, PmnError
    scans = ("s1", "s2", "s3")
    for s in scans:
        os.makedirs(tmp_path / "data" / s)
        (tmp_path / "data" / s / "fused.ply").write_bytes(b"")
    (tmp_path / "list.txt").write_text("\n".join(scans) + "\n")
    report = tmp_path / "rep" / "report.json"
    argv = ["--input", str(tmp_path / "data"), "--output", str(tmp_path / "out"), "--scan_list", str(tmp_path / "list.txt"),
            "--report", str(report), "--k", "7"]
    seen = []

    def clean_file(src, dst, args, device, fail_at=2):
        assert device == (None if not seen else "the device")  # the first file's device is handed to the later ones
        seen.append(src)
        if len(seen) == fail_at:
            raise PmnError(f"{src}:\n  refused  on purpose")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        open(dst, "w").close()
        return {"input": src, "output": dst}, "the device"

    monkeypatch.setattr(clean_cloud, "clean_file", clean_file)
    assert clean_cloud.main(argv) == 2
    got = capsys.readouterr()
    assert got.out == "" and got.err == f"clean_cloud.py: {tmp_path / 'data' / 's2' / 'fused.ply'}: refused on purpose\n"
    assert len(seen) == 2 and os.path.isfile(tmp_path / "out" / "s1" / "fused_clean.ply")  # what the first scan wrote stays
    assert not os.path.exists(tmp_path / "out" / "s2") and not os.path.exists(report) and not os.path.exists(report.parent)

    del seen[:]
    monkeypatch.setattr(clean_cloud, "clean_file", lambda *a: clean_file(*a, fail_at=0))
    assert clean_cloud.main(argv) == 0
    rep = json.loads(report.read_text())
    assert list(rep) == ["abi", "method", "k", "std_ratio", "radius", "min_neighbors", "cell", "max_dist", "files"]
    assert rep["abi"] == ABI_VERSION and (rep["method"], rep["k"], rep["radius"]) == ("statistical", 7, None)
    assert rep["files"] == [{"input": str(tmp_path / "data" / s / "fused.ply"), "output": str(tmp_path / "out" / s / "fused_clean.ply")}
                            for s in scans]
    assert report.read_text().startswith('{\n "abi": ')  # indent=1
