"""What the PLY readers and writers do, file by file (CPU only).  A corpus of tiny files is assembled from bytes spelled out here and
every file goes through every reader: pointcloud.read_ply_vertices, tsdf.read_ply_mesh and render.read_ply_model.  Each (file, reader)
pair has one recorded outcome: the exact arrays (values, dtype, shape, None versus array) or the exception type with the message
fragment the other IO tests match (the file's name, plus the few words they look for).  The writers are compared with whole files:
header text plus struct.pack of the body.  The functions are imported under the names the tools use (fusion / tsdf / pointcloud /
render), so the test does not depend on where the format is implemented.

The outcomes differ between the readers on purpose: read_ply_mesh reads only what write_ply_mesh writes and
does not range-check the faces, read_ply_vertices wants ``vertex`` first and ignores everything after it, read_ply_model reads faces
from little-endian files only.  fusion.write_ply writes coloured clouds only, so the cloud writer is checked for the two coloured
layouts and the mesh writer for all four."""
import itertools
import struct

import numpy as np
import pytest

from patchmatchnet_amd import fusion, pointcloud, render, tsdf
from patchmatchnet_amd._lib import PmnError

V = np.array([[0.5, -1.0, 2.0], [3.0, 4.25, -5.0], [0.001, 7.0, 8.0]], np.float32)
N = np.array([[0.0, 0.0, 1.0], [0.6, -0.8, 0.0], [-1.0, 0.0, 0.0]], np.float32)
C = np.array([[255, 0, 7], [1, 2, 3], [200, 100, 50]], np.uint8)
F = np.array([[0, 1, 2], [2, 1, 0]], np.int32)
LAYOUTS = [(c, n) for c in (False, True) for n in (False, True)]  # (colors, normals)
XYZ = "property float x\nproperty float y\nproperty float z\n"
NXYZ = "property float nx\nproperty float ny\nproperty float nz\n"
RGB = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
FACE = "element face %d\nproperty list uchar int vertex_indices\n"
LE = "ply\nformat binary_little_endian 1.0\n"


def _head(n, colors, normals, nf=None, start=LE):
    return (start + "element vertex %d\n" % n + XYZ + (NXYZ if normals else "") + (RGB if colors else "") +
            (FACE % nf if nf is not None else "") + "end_header\n").encode("ascii")


def _vertices(n, colors, normals, order="<"):
    body = b""
    for i in range(n):
        body += struct.pack(order + "3f", *V[i]) + (struct.pack(order + "3f", *N[i]) if normals else b"") + \
            (struct.pack("3B", *C[i]) if colors else b"")
    return body


def _faces(faces, index="i"):
    return b"".join(struct.pack("<B3" + index, 3, *(int(k) for k in f)) for f in faces)


class Ok:
    """The arrays a reader returns: vertices, faces (None: a cloud, or a mesh without faces), colors, normals."""

    def __init__(self, vertices, faces=None, colors=None, normals=None):
        self.vertices, self.faces, self.colors, self.normals = vertices, faces, colors, normals


class Err:
    def __init__(self, *fragments):
        self.fragments = fragments


def _same(got, want, dtype):
    if want is None:
        assert got is None
        return
    assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == np.shape(want), (got, want)
    assert got.tobytes() == np.ascontiguousarray(want, dtype).tobytes()


def _check(reader, path, want):
    kind = {"vertices": ValueError, "mesh": ValueError, "model": PmnError}[reader]
    call = {"vertices": pointcloud.read_ply_vertices, "mesh": tsdf.read_ply_mesh, "model": render.read_ply_model}[reader]
    if isinstance(want, Err):
        with pytest.raises(kind) as e:
            call(str(path))
        assert type(e.value) is kind
        for fragment in (path.name,) + want.fragments:
            assert fragment in str(e.value), (fragment, str(e.value))
        return
    got = call(str(path))
    if reader == "vertices":  # positions only
        _same(got, want.vertices, np.float32)
        assert got.flags["C_CONTIGUOUS"]
        return
    if reader == "mesh":  # a tuple; the faces are always an array
        assert isinstance(got, tuple) and len(got) == 4
        v, f, c, n = got
        _same(f, np.zeros((0, 3), np.int32) if want.faces is None else want.faces, np.int32)
    else:  # a dict; no faces is None
        assert sorted(got) == ["colors", "faces", "normals", "vertices"]
        v, f, c, n = got["vertices"], got["faces"], got["colors"], got["normals"]
        _same(f, want.faces, np.int32)
    _same(v, want.vertices, np.float32)
    _same(c, want.colors, np.uint8)
    _same(n, want.normals, np.float32)


def _corpus():
    """name -> (bytes, {reader: outcome})."""
    files = {}
    # the four layouts the library writes, as a cloud and as a mesh, with 0, 1 and 3 vertices and 0 and 2 faces
    for (colors, normals), n in itertools.product(LAYOUTS, (0, 1, 3)):
        tag = "%d%d_%d" % (colors, normals, n)
        full = Ok(V[:n], None, C[:n] if colors else None, N[:n] if normals else None)
        files["cloud" + tag] = (_head(n, colors, normals) + _vertices(n, colors, normals),
                                {"vertices": Ok(V[:n]), "mesh": Err(), "model": full})
        for faces in (F[:0], F) if n == 3 else (F[:0],):
            mesh = Ok(V[:n], faces if len(faces) else None, full.colors, full.normals)
            files["mesh%s_%d" % (tag, len(faces))] = (_head(n, colors, normals, len(faces)) + _vertices(n, colors, normals) + _faces(faces),
                                                      {"vertices": Ok(V[:n]), "mesh": mesh, "model": mesh})
    # ascii: a comment, trailing blanks on header lines, a colour column that is skipped
    text = "ply\nformat ascii 1.0  \ncomment by hand\nelement vertex 3\t\n" + XYZ + "property uchar red \nend_header\n" + \
        "".join("%r %r %r %d\n" % (float(v[0]), float(v[1]), float(v[2]), c[0]) for v, c in zip(V, C))
    files["ascii"] = (text.encode(), {"vertices": Ok(V), "mesh": Err(), "model": Ok(V)})
    files["ascii0"] = (b"ply\nformat ascii 1.0\nelement vertex 0\n" + XYZ.encode() + b"end_header\n",
                       {"vertices": Ok(V[:0]), "mesh": Err(), "model": Ok(V[:0])})
    files["ascii_mesh"] = ((text + "3 0 1 2\n").replace("end_header", (FACE % 1) + "end_header").encode(),
                           {"vertices": Ok(V), "mesh": Err(), "model": Err("binary_little_endian")})
    # big-endian: read as positions by both cloud readers; double x, z before y, colours and normals skipped
    big = b"".join(struct.pack(">dfffB", v[0], 7.0, v[2], v[1], 200) for v in V)
    files["big"] = (b"ply\nformat binary_big_endian 1.0\nelement vertex 3\nproperty double x\nproperty float nx\nproperty float z\n"
                    b"property float y\nproperty uchar red\nend_header\n" + big, {"vertices": Ok(V), "mesh": Err(), "model": Ok(V)})
    files["big_faces"] = (b"ply\nformat binary_big_endian 1.0\nelement vertex 3\n" + XYZ.encode() + (FACE % 1).encode() + b"end_header\n" +
                          _vertices(3, False, False, ">") + struct.pack(">B3i", 3, 0, 1, 2),
                          {"vertices": Ok(V), "mesh": Err(), "model": Err("binary_little_endian")})
    # further scalar properties: double positions, diffuse colours, an alpha, an obj_info line; float colours are no colours
    body = b"".join(struct.pack("<3d4B", *(float(t) for t in v), *c, 255) for v, c in zip(V, C))
    files["double_diffuse"] = ((LE + "obj_info scanner 7\nelement vertex 3\nproperty double x\nproperty double y\nproperty double z\n"
                                "property uchar diffuse_red\nproperty uchar diffuse_green\nproperty uchar diffuse_blue\nproperty uchar alpha\n"
                                "end_header\n").encode() + body, {"vertices": Ok(V), "mesh": Err(), "model": Ok(V, None, C)})
    body = b"".join(struct.pack("<6f", *v, *(c / np.float32(255))) for v, c in zip(V, C))
    files["float_colors"] = ((LE + "element vertex 3\n" + XYZ + "property float red\nproperty float green\nproperty float blue\nend_header\n")
                             .encode() + body, {"vertices": Ok(V), "mesh": Err(), "model": Ok(V)})
    # a library mesh with a comment after the format line: the mesh reader compares the header with what it writes
    files["comment_mesh"] = (_head(3, True, False, 2, LE + "comment made by a scanner\n") + _vertices(3, True, False) + _faces(F),
                             {"vertices": Ok(V), "mesh": Err(), "model": Ok(V, F, C)})
    # a library mesh with blanks at the end of every header line (no carriage returns)
    spaced = _head(3, True, True, 2).decode().replace("\n", " \t\n").encode()
    files["trailing_blanks"] = (spaced + _vertices(3, True, True) + _faces(F),
                                {"vertices": Ok(V), "mesh": Ok(V, F, C, N), "model": Ok(V, F, C, N)})
    # elements around the vertices
    edges = "element edge 2\nproperty int a\nproperty ushort b\n"
    files["edge_between"] = ((LE + "element vertex 3\n" + XYZ + edges + FACE % 2 + "end_header\n").encode() + _vertices(3, False, False) +
                             struct.pack("<iHiH", 0, 1, 1, 2) + _faces(F), {"vertices": Ok(V), "mesh": Err(), "model": Ok(V, F)})
    files["camera_first"] = ((LE + "element camera 1\nproperty float focal\nelement vertex 3\n" + XYZ + "end_header\n").encode() +
                             struct.pack("<f", 50.0) + _vertices(3, False, False),
                             {"vertices": Err("camera"), "mesh": Err(), "model": Err()})
    # faces
    files["uint_faces"] = (_head(3, False, False, 2).replace(b"uchar int", b"uchar uint") + _vertices(3, False, False) + _faces(F, "I"),
                           {"vertices": Ok(V), "mesh": Err(), "model": Ok(V, F)})
    files["quad"] = (_head(3, False, False, 1) + _vertices(3, False, False) + struct.pack("<B4i", 4, 0, 1, 2, 0),
                     {"vertices": Ok(V), "mesh": Err(), "model": Err()})
    far = np.array([[0, 1, 3], [2, 1, 0]], np.int32)  # vertex 3 does not exist: only the model reader checks the range
    files["index_out_of_range"] = (_head(3, False, False, 2) + _vertices(3, False, False) + _faces(far),
                                   {"vertices": Ok(V), "mesh": Ok(V, far), "model": Err()})
    for bad in ("property list uchar ushort vertex_indices", "property list int int vertex_indices",
                "property list uchar int vertex_indices\nproperty list uchar float texcoord"):
        files["faces_%d" % len(files)] = (_head(3, False, False, 1).replace(b"property list uchar int vertex_indices", bad.encode()) +
                                          _vertices(3, False, False) + bytes(32), {"vertices": Ok(V), "mesh": Err(), "model": Err("cannot be read")})
    # headers no reader accepts
    files["list_in_vertex"] = ((LE + "element vertex 1\n" + XYZ + "property list uchar int seen_by\nend_header\n").encode() +
                               _vertices(1, False, False) + struct.pack("<Bi", 1, 4), {"vertices": Err(), "mesh": Err(), "model": Err()})
    files["unknown_type"] = ((LE + "element vertex 1\n" + XYZ + "property half w\nend_header\n").encode() + bytes(14),
                             {"vertices": Err(), "mesh": Err(), "model": Err()})
    files["no_z"] = ((LE + "element vertex 1\nproperty float x\nproperty float y\nend_header\n").encode() + bytes(8),
                     {"vertices": Err("'z'"), "mesh": Err(), "model": Err()})
    files["no_end_header"] = ((LE + "element vertex 1\n" + XYZ).encode(), {"vertices": Err(), "mesh": Err(), "model": Err()})
    files["not_ply"] = (b"P6\n1 1\n255\n000", {"vertices": Err(), "mesh": Err(), "model": Err()})
    # truncated bodies
    files["short_cloud"] = (_head(3, True, False) + _vertices(2, True, False) + bytes(7),
                            {"vertices": Err(), "mesh": Err(), "model": Err()})
    files["short_mesh"] = (_head(3, True, False, 2) + _vertices(3, True, False) + _faces(F)[:-1],
                           {"vertices": Ok(V), "mesh": Err(), "model": Err()})
    return files


CORPUS = _corpus()


@pytest.mark.parametrize("reader", ["vertices", "mesh", "model"])
@pytest.mark.parametrize("name", list(CORPUS))
def test_readers(tmp_path, name, reader):
    blob, outcomes = CORPUS[name]
    path = tmp_path / (name + ".ply")
    path.write_bytes(blob)
    assert sorted(outcomes) == ["mesh", "model", "vertices"]
    _check(reader, path, outcomes[reader])


def test_corpus_covers_the_sizes():
    assert len(CORPUS) == len(set(CORPUS)) and len(CORPUS) >= 12 + 16 + 20
    assert {"cloud11_0", "cloud00_1", "mesh01_3_2", "mesh10_3_0", "mesh11_0_0"} <= set(CORPUS)


@pytest.mark.parametrize("n", [0, 2])
def test_writers_byte_for_byte(tmp_path, n):
    path = str(tmp_path / "out" / "w.ply")  # the writers create the folder
    blob = lambda: open(path, "rb").read()
    for normals in (False, True):  # clouds are written with colours
        want = _head(n, True, normals) + _vertices(n, True, normals)
        fusion.write_ply(path, V[:n], C[:n], N[:n] if normals else None)
        assert blob() == want
        assert fusion.ply_header(n, normals) == _head(n, True, normals)
        rec = fusion.ply_records(V[:n], C[:n], N[:n] if normals else None)
        assert rec.dtype == (fusion.PLY_VERTEX_NORMALS if normals else fusion.PLY_VERTEX) and rec.tobytes() == _vertices(n, True, normals)
    for colors, normals in LAYOUTS:
        for faces in (F[:0], F) if n else (F[:0],):  # two vertices: faces 0 1 1 / 1 0 0 stay in range
            faces = np.minimum(faces, 1)
            want = _head(n, colors, normals, len(faces)) + _vertices(n, colors, normals) + _faces(faces)
            tsdf.write_ply_mesh(path, V[:n], faces, C[:n] if colors else None, N[:n] if normals else None)
            assert blob() == want
            assert tsdf.mesh_header(n, len(faces), colors, normals) == _head(n, colors, normals, len(faces))
    # streamed records: the header of a coloured cloud for the total, or the bare records
    chunks = [fusion.ply_records(V[:1], C[:1]), fusion.ply_records(V[:0], C[:0]), fusion.ply_records(V[1:n + 1], C[1:n + 1])]
    assert fusion.write_ply_records(path, chunks) == 1 + n
    assert blob() == _head(1 + n, True, False) + _vertices(1 + n, True, False)
    assert fusion.write_ply_records(path, chunks, header=False) == 1 + n
    assert blob() == _vertices(1 + n, True, False)
    assert tsdf.PLY_FACE.itemsize == 13 and np.zeros(1, tsdf.PLY_FACE).tobytes() == bytes(13)
    with pytest.raises(ValueError):
        tsdf.write_ply_mesh(path, V[:2], np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError):
        fusion.ply_records(V, C, N[:2])
