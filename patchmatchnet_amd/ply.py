"""The PLY files of every tool after the network, host only: one header parser, one vertex record layout (the 15- and 27-byte
records are also what ops.PointPacker packs on the device), one header writer, the writers and the three readers, which share
``parse_header`` and ``read_element`` and differ in what they accept (DESIGN.md section 26 puts them side by side)."""
from __future__ import annotations

import itertools
import os
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from ._lib import PmnError

TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
         "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
BYTE_ORDER = {"binary_little_endian": "<", "binary_big_endian": ">", "ascii": "="}  # by the ``format`` line
MAX_HEADER_LINES = 4096


# ---- header -------------------------------------------------------------------------------------------------------------------

ScalarProp = namedtuple("ScalarProp", "name type")  # the types are keys of TYPES
ListProp = namedtuple("ListProp", "name count_type item_type")
# format as written (None without a ``format`` line); elements in file order; other: comment, obj_info, blank and unrecognised lines
Header = namedtuple("Header", "format version elements other")


class Element(namedtuple("Element", "name count properties")):
    @property
    def lists(self):
        return [p for p in self.properties if isinstance(p, ListProp)]


def parse_header(f, path: str) -> Header:
    """Reads an open binary file up to and including ``end_header``.  ValueError (naming the file) without the ``ply`` magic,
    without ``end_header`` in MAX_HEADER_LINES lines, for a malformed ``format`` / ``element`` / ``property`` line and for a type that
    is not in TYPES.  Which formats, elements and properties are acceptable is the caller's decision."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, version, elements, other = None, "", [], []
    for raw in itertools.islice(iter(f.readline, b""), MAX_HEADER_LINES):
        line = raw.decode("ascii", "replace").strip()
        tok = line.split()
        key = tok[0] if tok else ""
        if key == "end_header":
            return Header(fmt, version, tuple(Element(n, c, tuple(p)) for n, c, p in elements), tuple(other))
        if key == "format" and len(tok) >= 2:
            fmt, version = tok[1], " ".join(tok[2:])
        elif key == "element" and len(tok) == 3 and tok[2].isdigit():
            elements.append((tok[1], int(tok[2]), []))
        elif key == "property" and elements and len(tok) == (5 if tok[1:2] == ["list"] else 3):
            unknown = [t for t in tok[1 + (len(tok) == 5):-1] if t not in TYPES]
            if unknown:
                raise ValueError(f"{path}: unknown PLY property type {unknown[0]!r}")
            elements[-1][2].append(ListProp(tok[4], tok[2], tok[3]) if len(tok) == 5 else ScalarProp(tok[2], tok[1]))
        elif key in ("format", "element", "property"):
            raise ValueError(f"{path}: malformed PLY header line {line!r}")
        else:
            other.append(line)
    raise ValueError(f"{path}: PLY header has no end_header")


def element_dtype(fmt: Optional[str], element: Element, path: str) -> np.dtype:
    """The record of a scalar-only element in a file of format ``fmt``."""
    if fmt not in BYTE_ORDER:
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    return np.dtype([(p.name, BYTE_ORDER[fmt] + TYPES[p.type]) for p in element.properties])


def _records(f, dtype: np.dtype, count: int, what: str, path: str, ascii: bool = False) -> np.ndarray:
    if not ascii:
        rec = np.fromfile(f, dtype, count)
    else:  # numbers through float64; the file's position is undefined afterwards
        k = len(dtype.names)
        rows = np.loadtxt(f, dtype=np.float64, max_rows=count, usecols=range(k), ndmin=2) if count else np.zeros((0, k))
        rec = np.empty(len(rows), dtype)
        for i, name in enumerate(dtype.names):
            rec[name] = rows[:, i]
    if len(rec) != count:
        raise ValueError(f"{path}: {len(rec)} {what} records where the header says {count}")
    return rec


def read_element(f, fmt: Optional[str], element: Element, path: str) -> np.ndarray:
    """The records of a scalar-only element at the file's position, as a structured array with the declared names and types."""
    return _records(f, element_dtype(fmt, element, path), element.count, element.name, path, fmt == "ascii")


def _triangles(f, element: Element, path: str) -> np.ndarray:
    """[m,3] int32 of an element whose one list property (count uchar, indices int or uint) holds triangles, next to any scalars."""
    fields = [field for p in element.properties for field in
              ([("_n", "u1"), ("_v", "<i4", (3,))] if isinstance(p, ListProp) else [(p.name, "<" + TYPES[p.type])])]
    rec = _records(f, np.dtype(fields), element.count, element.name, path)
    if element.count and (rec["_n"] != 3).any():
        raise ValueError(f"{path}: a face that is not a triangle")
    return np.ascontiguousarray(rec["_v"], np.int32)


def _columns(rec: np.ndarray, names, dtype) -> np.ndarray:
    return np.stack([rec[n] for n in names], 1).astype(dtype) if len(rec) else np.zeros((0, len(names)), dtype)


# ---- records and writers --------------------------------------------------------------------------------------------------------

FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])  # property list uchar int vertex_indices: 13 bytes


def vertex_dtype(colors: bool = True, normals: bool = False) -> np.dtype:
    """The vertex this library writes: x y z [nx ny nz] [red green blue], 12 / 24 / 15 / 27 bytes.  The oriented cloud's (DESIGN.md
    section 14) is in the property order of MeshLab, Open3D and COLMAP's fused.ply, so Poisson meshers read the normals as they are."""
    names = ("x", "y", "z", "nx", "ny", "nz") if normals else ("x", "y", "z")
    return np.dtype([(n, "<f4") for n in names] + ([(n, "u1") for n in ("red", "green", "blue")] if colors else []))


def vertex_records(vertices: np.ndarray, colors: Optional[np.ndarray] = None, normals: Optional[np.ndarray] = None) -> np.ndarray:
    """The vertex records of the PLY body, ``vertex_dtype(colors is not None, normals is not None)``: one strided byte copy per
    property group."""
    n = len(vertices)
    if normals is not None and len(normals) != n:
        raise ValueError("ply_records: one normal per vertex")
    rec = np.empty(n, vertex_dtype(colors is not None, normals is not None))
    if n:
        raw = rec.view(np.uint8).reshape(n, rec.dtype.itemsize)
        raw[:, :12] = np.ascontiguousarray(vertices, "<f4").view(np.uint8).reshape(n, 12)
        if normals is not None:
            raw[:, 12:24] = np.ascontiguousarray(normals, "<f4").view(np.uint8).reshape(n, 12)
        if colors is not None:
            raw[:, -3:] = np.asarray(colors, np.uint8)
    return rec


def header(nv: int, colors: bool = True, normals: bool = False, nf: Optional[int] = None) -> bytes:
    """The header of a cloud of ``nv`` vertices or, with ``nf``, of a mesh with as many triangles."""
    dt = vertex_dtype(colors, normals)
    props = "".join("property %s %s\n" % ("uchar" if dt[n] == np.uint8 else "float", n) for n in dt.names)
    face = "" if nf is None else "element face %d\nproperty list uchar int vertex_indices\n" % nf
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%s%send_header\n" % (nv, props, face)).encode("ascii")


def _write(path: str, head: bytes, *records) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(head)
        for r in records:
            r.tofile(f)


def write_ply(filename: str, vertices: np.ndarray, colors: np.ndarray, normals: Optional[np.ndarray] = None) -> None:
    """Binary little-endian PLY with x,y,z float32 + red,green,blue uint8 per vertex (what plyfile writes at reference
    eval.py:283-297); with ``normals`` the oriented vertex x,y,z,nx,ny,nz,red,green,blue."""
    _write(filename, header(len(vertices), colors is not None, normals is not None), vertex_records(vertices, colors, normals))


def write_ply_records(filename: str, chunks, header: bool = True) -> int:
    """The same file as ``write_ply`` (without normals) from per-view record arrays (``fuse_views(as_records=True)``), streamed chunk
    by chunk; ``header=False`` writes the bare records (eval.py's per-rank parts).  Returns the number of vertices."""
    total = sum(len(c) for c in chunks)
    _write(filename, ply_header(total) if header else b"", *chunks)
    return total


def write_ply_mesh(path: str, vertices, faces, colors=None, normals=None) -> None:
    """Binary little-endian PLY: the vertex element of write_ply (x y z [nx ny nz] [red green blue]) followed by ``element face``
    with ``property list uchar int vertex_indices`` (13 bytes per triangle).  Arrays or tensors."""
    host = lambda a: None if a is None else (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
    vertices, faces, colors, normals = host(vertices), host(faces), host(colors), host(normals)
    n = len(vertices)
    if faces.ndim != 2 or faces.shape[1] != 3 or (len(faces) and (faces.min() < 0 or faces.max() >= n)):
        raise ValueError("write_ply_mesh: faces must be [m,3] indices into the vertices")
    frec = np.empty(len(faces), FACE)
    frec["n"], frec["v"] = 3, faces
    _write(path, header(n, colors is not None, normals is not None, len(faces)), vertex_records(vertices, colors, normals), frec)


# the names fusion and tsdf export
PLY_VERTEX, PLY_VERTEX_NORMALS, PLY_FACE, ply_records = vertex_dtype(), vertex_dtype(normals=True), FACE, vertex_records


def ply_header(n: int, normals: bool = False) -> bytes:
    return header(n, True, normals)


def mesh_header(nv: int, nf: int, colors: bool, normals: bool) -> bytes:
    return header(nv, colors, normals, nf)


# ---- readers ----------------------------------------------------------------------------------------------------------------------

def _positions(f, h: Header, path: str) -> np.ndarray:
    """read_ply_vertices behind the header."""
    vertex = next((e for e in h.elements if e.name == "vertex"), None)
    if vertex is None:
        raise ValueError(f"{path}: no vertex element")
    if vertex.lists:
        raise ValueError(f"{path}: list property {vertex.lists[0].name!r} inside the vertex element is not supported")
    if h.elements[0] is not vertex:
        raise ValueError(f"{path}: element {h.elements[0].name!r} precedes vertex")
    for axis in "xyz":
        if axis not in [p.name for p in vertex.properties]:
            raise ValueError(f"{path}: the vertex element has no property {axis!r}")
    return _columns(read_element(f, h.format, vertex, path), "xyz", np.float32)


def read_ply_vertices(path: str) -> np.ndarray:
    """The ``vertex`` element of a PLY as [n,3] float32 (x, y, z).  binary_little_endian, binary_big_endian or ascii; other scalar
    vertex properties (colours, normals) are skipped; elements after ``vertex`` (faces) are ignored.  Reads what write_ply and
    write_ply_mesh write and DTU's Points/stl/stl%03d_total.ply.  ValueError (naming the file) for a list property inside ``vertex``,
    a missing x / y / z, or an element before ``vertex`` (its size would have to be parsed to find the vertices)."""
    with open(path, "rb") as f:
        return _positions(f, parse_header(f, path), path)


def read_ply_mesh(path: str):
    """(vertices [n,3] float32, faces [m,3] int32, colors [n,3] uint8 | None, normals [n,3] float32 | None) of a file
    write_ply_mesh wrote; ValueError (naming the file) for anything else: another format or version, a comment, further elements or
    properties.  The vertex properties are told by their names, and the faces are not range-checked."""
    with open(path, "rb") as f:
        h = parse_header(f, path)
        if (h.format, h.version) != ("binary_little_endian", "1.0") or h.other or not h.elements or h.elements[0].name != "vertex":
            raise ValueError(f"{path}: not a binary little-endian PLY mesh")
        if [e.name for e in h.elements[1:]] != ["face"] or h.elements[1].properties != (ListProp("vertex_indices", "uchar", "int"),):
            raise ValueError(f"{path}: expected one face element with 'property list uchar int vertex_indices'")
        names = tuple(p.name for p in h.elements[0].properties)
        colors, normals = names[-3:] == ("red", "green", "blue"), names[3:6] == ("nx", "ny", "nz")
        dt = vertex_dtype(colors, normals)
        if names != dt.names:
            raise ValueError(f"{path}: vertex properties {names} are not a mesh this library writes")
        rec, faces = _records(f, dt, h.elements[0].count, "vertex", path), _triangles(f, h.elements[1], path)
    return (_columns(rec, "xyz", np.float32), faces, _columns(rec, ("red", "green", "blue"), np.uint8) if colors else None,
            _columns(rec, ("nx", "ny", "nz"), np.float32) if normals else None)


def read_ply_model(path: str):
    """A mesh or a cloud from a PLY file -> dict(vertices [n,3] float32, faces [m,3] int32 | None, colors [n,3] uint8 | None, normals
    [n,3] float32 | None).  binary_little_endian files are read in full: a ``vertex`` element (first) with x y z and any other scalar
    properties in any order (red green blue / diffuse_red ... as uchar give the colours, nx ny nz the normals), scalar-only elements in
    between, and an optional ``face`` element with one list property (count uchar, indices int or uint; all faces triangles) next to
    any scalar properties.  An ascii or big-endian file is read as a cloud of positions (as read_ply_vertices does).  PmnError naming
    the file for anything else."""
    try:
        with open(path, "rb") as f:
            h = parse_header(f, path)
            if h.format != "binary_little_endian":
                nf = [e.count for e in h.elements if e.name == "face"]
                if any(nf):
                    raise PmnError(f"{path}: a {h.format or 'PLY'} file with {nf[0]} faces: only binary_little_endian meshes can be "
                                   f"read (its vertices alone would be drawn as a see-through cloud)")
                return {"vertices": _positions(f, h, path), "faces": None, "colors": None, "normals": None}
            if not h.elements or h.elements[0].name != "vertex":
                raise PmnError(f"{path}: the first PLY element is not 'vertex'")
            out = {"faces": None}
            for e in h.elements:
                if e.name == "vertex":
                    if e.lists:
                        raise PmnError(f"{path}: a list property inside the vertex element")
                    rec = read_element(f, h.format, e, path)
                    names = rec.dtype.names
                    if any(c not in names for c in "xyz"):
                        raise PmnError(f"{path}: the vertex element has no x y z")
                    out["vertices"] = _columns(rec, "xyz", np.float32)
                    out["normals"] = _columns(rec, ("nx", "ny", "nz"), np.float32) if all(c in names for c in ("nx", "ny", "nz")) else None
                    trios = [t for t in (("red", "green", "blue"), ("diffuse_red", "diffuse_green", "diffuse_blue"))
                             if all(c in names and rec.dtype[c] == np.uint8 for c in t)]
                    out["colors"] = np.stack([rec[c] for c in trios[0]], 1) if trios else None
                elif not e.lists:
                    f.seek(e.count * element_dtype(h.format, e, path).itemsize, 1)
                elif e.name == "face" and len(e.lists) == 1 and TYPES[e.lists[0].count_type] == "u1" and \
                        TYPES[e.lists[0].item_type] in ("i4", "u4"):
                    faces = _triangles(f, e, path)
                    if e.count and (faces.min() < 0 or faces.max() >= len(out["vertices"])):
                        raise PmnError(f"{path}: a face refers to a vertex that does not exist")
                    out["faces"] = faces if e.count else None
                    break  # nothing after the faces is needed
                elif e.name == "face" and e.count:
                    raise PmnError(f"{path}: the face element's properties ({' / '.join(' '.join(p) for p in e.properties)}) "
                                   f"are not one 'list uchar int|uint' of triangle indices next to scalars: the mesh cannot be read")
                else:
                    break  # a list element that is not the faces: what came before it is the model
            return out
    except ValueError as err:
        raise PmnError(f"{path}: neither a mesh nor a cloud this tool can read ({err})") from err
    except OSError as err:
        raise PmnError(f"{path}: cannot read the model ({err})") from err
