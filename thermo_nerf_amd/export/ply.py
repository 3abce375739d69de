"""Binary little-endian PLY of a thermal point cloud: 19 bytes per vertex — ``float x y z``, ``uchar red green blue``,
``float temperature`` (degrees Celsius).  Any cloud viewer opens it; the extra scalar shows up as a per-point property.

The header is exactly (``M`` = the number of points, the bounds = the cloud's ``temperature_bounds`` as ``repr`` of two Python
floats, or ``none none``)::

    ply
    format binary_little_endian 1.0
    comment temperature_unit celsius
    comment temperature_bounds MIN MAX
    element vertex M
    property float x
    property float y
    property float z
    property uchar red
    property uchar green
    property uchar blue
    property float temperature
    end_header

No time stamp, no host name: the same cloud gives the same bytes.

A cloud that carries normals (``estimate_normals``) is written with ``property float nx`` / ``ny`` / ``nz`` between ``z`` and
``red``: 31 bytes per vertex, the layout cloud viewers and Poisson reconstruction expect.  Without normals the file is the one above.
A mesh (below) with ``normals`` set (``vertex_normals``) gets the same three properties in the same place.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict

import numpy as np

VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                         ("temperature", "<f4")])
assert VERTEX_DTYPE.itemsize == 19

_PROPERTIES = ("property float x", "property float y", "property float z", "property uchar red", "property uchar green",
               "property uchar blue", "property float temperature")

NORMAL_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                                ("green", "u1"), ("blue", "u1"), ("temperature", "<f4")])
assert NORMAL_VERTEX_DTYPE.itemsize == 31

_NORMAL_PROPERTIES = _PROPERTIES[:3] + ("property float nx", "property float ny", "property float nz") + _PROPERTIES[3:]


def header(num_points: int, temperature_bounds=None, normals: bool = False) -> str:
    lo, hi = (repr(float(v)) for v in temperature_bounds) if temperature_bounds is not None else ("none", "none")
    lines = ["ply", "format binary_little_endian 1.0", "comment temperature_unit celsius", f"comment temperature_bounds {lo} {hi}",
             f"element vertex {int(num_points)}", *(_NORMAL_PROPERTIES if normals else _PROPERTIES), "end_header"]
    return "\n".join(lines) + "\n"


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _vertex_array(obj, colors: str, dtype, no_thermal: str, disagree: str) -> np.ndarray:
    """the vertex records of a cloud or a mesh (x y z, red green blue, temperature filled), after the checks both writers make"""
    if colors not in ("rgb", "thermal"):
        raise ValueError('colors must be "rgb" or "thermal"')
    col = obj.colors if colors == "rgb" else obj.thermal_colors
    if col is None:
        raise ValueError(no_thermal)
    pos, col, temp = _host(obj.positions), _host(col), _host(obj.temperature)
    m = pos.shape[0]
    if pos.shape != (m, 3) or col.shape != (m, 3) or temp.shape != (m,):
        raise ValueError(disagree)
    vertex = np.empty(m, dtype=dtype)
    vertex["x"], vertex["y"], vertex["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    vertex["red"], vertex["green"], vertex["blue"] = col[:, 0], col[:, 1], col[:, 2]
    vertex["temperature"] = temp
    return vertex


def _fill_normals(vertex: np.ndarray, normals) -> None:
    nrm = _host(normals)
    if nrm.shape != (vertex.shape[0], 3):
        raise ValueError("normals must be [M,3]")
    vertex["nx"], vertex["ny"], vertex["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]


def _vertex_dtype(properties, face_lines, path, what: str):
    """the record of a file's vertex properties: the 19-byte layout, or the 31-byte one with normals"""
    if properties == _PROPERTIES + face_lines:
        return VERTEX_DTYPE
    if properties == _NORMAL_PROPERTIES + face_lines:
        return NORMAL_VERTEX_DTYPE
    raise ValueError(f"{path}: {what}")


def _read_normals(vertex: np.ndarray) -> np.ndarray:
    return np.stack([vertex["nx"], vertex["ny"], vertex["nz"]], axis=1) if vertex.shape[0] else np.zeros((0, 3), np.float32)


def _write(path, head: str, *arrays: np.ndarray) -> Path:
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        for a in arrays:
            a.tofile(f)
    return path


def _read_header(path):
    """(the file's bytes, the offset of its body, the header's lines, its comment lines without the keyword)"""
    blob = Path(path).read_bytes()
    end = blob.find(b"end_header\n")
    if not blob.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary little-endian PLY is read")
    return blob, end + len(b"end_header\n"), lines, [ln[len("comment "):] for ln in lines if ln.startswith("comment ")]


def _vertex_fields(vertex: np.ndarray, comments) -> Dict:
    m = vertex.shape[0]
    return {"positions": np.stack([vertex["x"], vertex["y"], vertex["z"]], axis=1) if m else np.zeros((0, 3), np.float32),
            "colors": np.stack([vertex["red"], vertex["green"], vertex["blue"]], axis=1) if m else np.zeros((0, 3), np.uint8),
            "temperature": vertex["temperature"].copy(), "comments": comments}


def write_ply(path, cloud, colors: str = "rgb") -> Path:
    """Write ``cloud`` (a ThermalPointCloud, on the device or the host) to ``path``.  ``colors``: which bytes fill red / green /
    blue — "rgb" (the rendered colours) or "thermal" (the colour-mapped temperature).  ``cloud.normals``, where set, are written
    as nx ny nz behind z.  One device -> host copy per array."""
    normals = getattr(cloud, "normals", None)
    vertex = _vertex_array(cloud, colors, VERTEX_DTYPE if normals is None else NORMAL_VERTEX_DTYPE,
                           "the cloud holds no thermal colours (exported without a colour table)",
                           "positions [M,3], colours [M,3] and temperature [M] must agree")
    if normals is not None:
        _fill_normals(vertex, normals)
    return _write(path, header(vertex.shape[0], getattr(cloud, "temperature_bounds", None), normals is not None), vertex)


def read_ply(path) -> Dict:
    """The arrays of a file ``write_ply`` wrote: ``positions`` float32 [M,3], ``colors`` uint8 [M,3], ``temperature`` float32 [M],
    ``comments`` (the header's comment lines without the keyword), and ``normals`` float32 [M,3] when the file carries them (the
    31-byte layout).  M = 0 — a header without a body — is a valid file."""
    blob, body, lines, comments = _read_header(path)
    counts = [ln for ln in lines if ln.startswith("element ")]
    if len(counts) != 1 or not counts[0].startswith("element vertex "):
        raise ValueError(f"{path}: one vertex element expected")
    properties = tuple(ln for ln in lines if ln.startswith("property "))
    dtype = _vertex_dtype(properties, (), path, "vertex properties differ from x y z [nx ny nz] red green blue temperature")
    m = int(counts[0].split()[2])
    if len(blob) - body != m * dtype.itemsize:
        raise ValueError(f"{path}: {len(blob) - body} body bytes for {m} vertices of {dtype.itemsize} bytes")
    vertex = np.frombuffer(blob, dtype=dtype, count=m, offset=body)
    out = _vertex_fields(vertex, comments)
    if dtype is NORMAL_VERTEX_DTYPE:
        out["normals"] = _read_normals(vertex)
    return out


# ---- triangle meshes ---------------------------------------------------------------------------------------------------------------
# The cloud's header up to its last vertex property, then ``element face T`` / ``property list uchar int vertex_indices``: 19 bytes per
# vertex, 13 per face (the count byte 3 and three little-endian int32).  The same determinism: the same mesh gives the same bytes.
# A mesh that carries normals (``vertex_normals``) is written like a cloud that does: nx ny nz between z and red, 31 bytes per vertex.
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
assert FACE_DTYPE.itemsize == 13

_FACE_LINES = ("property list uchar int vertex_indices",)


def mesh_header(num_vertices: int, num_triangles: int, temperature_bounds=None, normals: bool = False) -> str:
    lines = header(num_vertices, temperature_bounds, normals).split("\n")[:-2]  # without end_header
    return "\n".join(lines + [f"element face {int(num_triangles)}", *_FACE_LINES, "end_header"]) + "\n"


def write_mesh_ply(path, mesh, colors: str = "rgb") -> Path:
    """Write ``mesh`` (a ThermalMesh, on the device or the host) to ``path``; ``colors`` as in ``write_ply``.  V = 0 or T = 0 is a
    valid file.  ``mesh.normals``, where set, are written as nx ny nz behind z.  One device -> host copy per array."""
    disagree = "positions [V,3], colours [V,3], temperature [V] and triangles [T,3] must agree"
    normals = getattr(mesh, "normals", None)
    vertex = _vertex_array(mesh, colors, VERTEX_DTYPE if normals is None else NORMAL_VERTEX_DTYPE,
                           "the mesh holds no thermal colours (extracted without a colour table)", disagree)
    tri = _host(mesh.triangles)
    m, t = vertex.shape[0], tri.shape[0]
    if tri.shape != (t, 3):
        raise ValueError(disagree)
    if normals is not None:
        _fill_normals(vertex, normals)
    if t and (tri.min() < 0 or tri.max() >= m):
        raise ValueError("a triangle names a vertex outside [0, V)")
    face = np.empty(t, dtype=FACE_DTYPE)
    face["n"], face["v"] = 3, tri
    return _write(path, mesh_header(m, t, getattr(mesh, "temperature_bounds", None), normals is not None), vertex, face)


def read_mesh_ply(path) -> Dict:
    """The arrays of a file ``write_mesh_ply`` wrote: ``read_ply``'s ``positions`` / ``colors`` / ``temperature`` / ``comments`` and
    ``triangles`` int32 [T,3], and ``normals`` float32 [V,3] when the file carries them (the 31-byte vertex)."""
    blob, body, lines, comments = _read_header(path)
    counts = [ln.split() for ln in lines if ln.startswith("element ")]
    if [c[1] for c in counts] != ["vertex", "face"]:
        raise ValueError(f"{path}: a vertex element and a face element expected")
    dtype = _vertex_dtype(tuple(ln for ln in lines if ln.startswith("property ")), _FACE_LINES, path,
                          "properties differ from x y z [nx ny nz] red green blue temperature / vertex_indices")
    m, t = int(counts[0][2]), int(counts[1][2])
    if len(blob) - body != m * dtype.itemsize + t * FACE_DTYPE.itemsize:
        raise ValueError(f"{path}: {len(blob) - body} body bytes for {m} vertices and {t} faces")
    vertex = np.frombuffer(blob, dtype=dtype, count=m, offset=body)
    face = np.frombuffer(blob, dtype=FACE_DTYPE, count=t, offset=body + m * dtype.itemsize)
    if t and not (face["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are read")
    out = {**_vertex_fields(vertex, comments), "triangles": face["v"].astype(np.int32).reshape(t, 3)}
    if dtype is NORMAL_VERTEX_DTYPE:
        out["normals"] = _read_normals(vertex)
    return out


def write_curves_ply(path, curves, temperature_bounds=None) -> Path:
    """Write ``curves`` (a MeshCurves: level-set curves of a mesh, on the device or the host) to ``path`` as a line set: the P points
    as vertices ``float x y z``, ``float temperature`` (16 bytes each), then one ``edge`` element per segment, ``int vertex1`` /
    ``int vertex2`` (8 bytes each): consecutive points of a curve.  The comment lines are the mesh writer's, the bounds from
    ``temperature_bounds``.  The same curves give the same bytes."""
    pos, temp, table = _host(curves.positions), _host(curves.temperature), curves.curves
    m = pos.shape[0]
    if pos.shape != (m, 3) or temp.shape != (m,):
        raise ValueError("positions [P,3] and temperature [P] must agree")
    vertex = np.empty(m, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("temperature", "<f4")]))
    vertex["x"], vertex["y"], vertex["z"], vertex["temperature"] = pos[:, 0], pos[:, 1], pos[:, 2], temp
    starts = [np.arange(int(row["first_point"]), int(row["first_point"]) + int(row["points"]) - 1, dtype=np.int32) for row in table]
    first = np.concatenate(starts) if starts else np.zeros(0, np.int32)
    if len(first) and (first.min() < 0 or first.max() + 1 >= m):
        raise ValueError("a curve names a point outside [0, P)")
    edge = np.empty(len(first), dtype=np.dtype([("vertex1", "<i4"), ("vertex2", "<i4")]))
    edge["vertex1"], edge["vertex2"] = first, first + 1
    lines = header(m, temperature_bounds).split("\n")[:5]  # up to ``element vertex``
    lines += [*_PROPERTIES[:3], _PROPERTIES[-1], f"element edge {len(edge)}", "property int vertex1", "property int vertex2", "end_header"]
    return _write(path, "\n".join(lines) + "\n", vertex, edge)
