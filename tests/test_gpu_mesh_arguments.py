"""The one check of a ``ThermalMesh`` (``thermo_nerf_amd/export/_common.py``: ``mesh_arrays``, ``triangle_array``, ``color_array``)
through every entry that starts with it: a malformed mesh is refused with the same exception and the same words whichever entry
meets it, before anything is launched, and the well-formed quad and the mesh without a vertex or a face still pass — each
``*_into`` hands the library no address of an empty array.  ``ENTRIES`` is shared with the CPU half in
tests/test_mesh_raycast_cpu.py."""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import pytest
import torch

from thermo_nerf_amd.export import (CameraView, RasterView, ThermalMesh, build_mesh_bvh, mesh_difference, mesh_measurement,
                                    mesh_rasterize_into, mesh_regions_into, mesh_simplify_into, register_mesh, simplify_mesh,
                                    thermal_regions, voxel_params)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VIEW = RasterView((-0.5, -0.5, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 0.25, 8, 8)
CAMERA = CameraView(np.eye(4)[:3], 10.0, 10.0, 4.0, 4.0, 8, 8)


def _rasterize(mesh, bvh, dev):
    mesh_rasterize_into(mesh, VIEW, counts=torch.zeros(3, dtype=torch.int64, device=dev), stats=torch.zeros(3, dtype=torch.float64, device=dev),
                        pixel_colors=torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev))


def _regions(mesh, bvh, dev):
    mesh_regions_into(mesh, -math.inf, math.inf, counts=torch.zeros(3, dtype=torch.int64, device=dev),
                      totals=torch.zeros(2, dtype=torch.float64, device=dev), face_region=torch.zeros(2, dtype=torch.int32, device=dev))


def _simplify(mesh, bvh, dev):
    mesh_simplify_into(mesh, voxel_params((0.0, 0.0, 0.0), 1.0, (1, 1, 1)), counts=torch.zeros(4, dtype=torch.int64, device=dev))


def _measurement(mesh, bvh, dev):
    mesh_measurement(mesh, bvh, [CAMERA], torch.zeros((1, 8, 8), dtype=torch.uint8, device=dev), (10.0, 40.0))


# name: (the call of (mesh, a tree to compare with, device), does it read the temperature, does it read the colours)
ENTRIES = {
    "build_mesh_bvh": (lambda mesh, bvh, dev: build_mesh_bvh(mesh), True, False),
    "mesh_rasterize_into": (_rasterize, True, True),
    "mesh_regions_into": (_regions, True, False),
    "mesh_simplify_into": (_simplify, True, True),
    "mesh_difference": (lambda mesh, bvh, dev: mesh_difference(mesh, bvh, max_distance=1.0), True, False),
    "mesh_measurement": (_measurement, True, False),
    "thermal_regions": (lambda mesh, bvh, dev: thermal_regions(mesh, 15.0), True, False),
    "simplify_mesh": (lambda mesh, bvh, dev: simplify_mesh(mesh, 0.5), True, True),
    "register_mesh": (lambda mesh, bvh, dev: register_mesh(mesh, bvh, max_distance=1.0), False, False),
}


def quad(dev) -> ThermalMesh:
    """a unit square of two faces in the plane z = 0, with colours and temperatures"""
    return ThermalMesh(torch.tensor([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 0.0)], device=dev),
                       torch.tensor([(255, 0, 0), (0, 255, 0), (0, 0, 255), (9, 9, 9)], dtype=torch.uint8, device=dev),
                       torch.tensor([10.0, 20.0, 30.0, 40.0], device=dev), None,
                       torch.tensor([(0, 1, 2), (0, 2, 3)], dtype=torch.int32, device=dev), (10.0, 40.0))


# name: (what the quad is given, the exception, its words, which entries meet it: all, those that read the temperature / the colours)
MALFORMED = {
    "positions_4x2": (lambda m: dict(positions=m.positions[:, :2].contiguous()), ValueError, r"positions must be \[V, 3\] with V <= 2\^31 - 1", "all"),
    "temperature_of_5": (lambda m: dict(temperature=torch.zeros(5, device=m.positions.device)), ValueError, "temperature must hold V values",
                         "temperature"),
    "triangles_2x2": (lambda m: dict(triangles=m.triangles[:, :2].contiguous()), ValueError, r"triangles must be \[T, 3\] with 3 T <= 2\^31 - 1", "all"),
    "triangles_int64": (lambda m: dict(triangles=m.triangles.long()), TypeError, "triangles must be torch.int32", "all"),
    "triangles_none": (lambda m: dict(triangles=None), ValueError, "the mesh has no triangles", "all"),
    "colors_3x3": (lambda m: dict(colors=m.colors[:3].contiguous()), ValueError, r"colors must be \[V, 3\] on the mesh's device", "colors"),
}


def _cases():
    for entry, (_, temperature, colors) in ENTRIES.items():
        for fault, (_, _, _, who) in MALFORMED.items():
            if who == "all" or (who == "temperature" and temperature) or (who == "colors" and colors):
                yield pytest.param(entry, fault, id=f"{entry}-{fault}")


@pytest.fixture(scope="module")
def reference():
    """the quad on the device and its tree: what the entries that take a second mesh compare with"""
    mesh = quad(DEV)
    return mesh, build_mesh_bvh(mesh)


@pytest.mark.parametrize("entry,fault", list(_cases()))
def test_every_entry_refuses_a_malformed_mesh_alike(reference, entry, fault):
    mesh, bvh = reference
    change, error, words, _ = MALFORMED[fault]
    with pytest.raises(error, match=words):
        ENTRIES[entry][0](dataclasses.replace(mesh, **change(mesh)), bvh, DEV)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_entry_takes_the_quad_and_the_empty_mesh(reference, entry):
    mesh, bvh = reference
    empty = ThermalMesh(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), dtype=torch.uint8, device=DEV), torch.zeros(0, device=DEV), None,
                        torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    call = ENTRIES[entry][0]
    call(mesh, bvh, DEV)
    call(empty, build_mesh_bvh(empty) if entry == "mesh_measurement" else bvh, DEV)  # (a measurement takes the mesh's own tree)
    torch.cuda.synchronize()  # (what either call queued has run: a fault would show here)
