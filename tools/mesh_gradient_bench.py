#!/usr/bin/env python
"""What the surface gradient and the scalar smoothing cost on a mesh of a survey's size, beside the two kernels that walk the same
corner lists with the same gather pattern — ``tn_mesh_vertex_normals`` and a pass of ``tn_mesh_smooth`` — on the closed lattice surface
of about 2 M faces of tools/mesh_isolines_bench.py (a torus of ``--side`` x ``--side`` two-triangle cells; no file, no reference data).

The entries are timed into preallocated outputs with device events around each call (3 warm-up calls, then ``--repeats`` timed calls:
median and range); the public calls (``thermal_gradient``, ``smooth_temperature``) beside them, with their allocations, the incidence
build and the host read.  The times of the single kernels come from a kernel trace taken in a run of its own — every kernel of the
traced calls has a name no other entry of that process launches, so the trace needs no baseline:

    python tools/mesh_gradient_bench.py [--side 1024] [--repeats 11] --out profiles/micro/mesh_gradient.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_gradient_bench.py --trace-pass
    python tools/mesh_gradient_bench.py --kernels-from DIR --out profiles/micro/mesh_gradient.txt      # appends the kernels

The vertex kernel of the gradient recomputes the gradient of each corner's face.  The variant that read the rows and records of the
face kernel back from the workspace was measured beside it once, as a second library built for that run and named by
``THERMONERF_HIP_LIB``; ``--label`` says in a report which library it is of.  That variant lost and is gone; its numbers are in the
profile.  A record, not a gate.
"""
from __future__ import annotations

import argparse
import glob
import os
import sqlite3
import sys

import mesh_scenes  # the sibling module: event_ms, emit; it puts the repository on sys.path
from mesh_isolines_bench import torus  # the sibling module: the closed lattice surface

# the kernels of the traced calls, under the names a trace gives them, and the launches of each per traced round
KERNELS = (("gradient_faces_kernel", 1, "tn_mesh_scalar_gradient: the faces (rows, records)"),
           ("gradient_vertices_kernel", 1, "tn_mesh_scalar_gradient: the vertices"),
           ("gradient_block_sums_kernel", 1, "tn_mesh_scalar_gradient: the totals, 256 faces per thread"),
           ("gradient_totals_kernel", 1, "tn_mesh_scalar_gradient: the totals, the partials"),
           ("scalar_pass_kernel", 2, "tn_mesh_scalar_smooth: one pass"),
           ("normals_kernel", 1, "tn_mesh_vertex_normals"),
           ("smooth_pass_kernel", 2, "tn_mesh_smooth: one pass"))


def short_name(name: str) -> str:
    """a traced kernel name without its namespace, return type and arguments"""
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip()


def kernel_us(directory: str) -> dict:
    """{kernel: us in all its launches} from the rocpd database(s) of a kernel trace under ``directory``, names matched whole"""
    wanted, spent = {name for name, _, _ in KERNELS}, {}
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        for name, duration in sqlite3.connect(path).cursor().execute("select name,total_duration from top_kernels"):
            short = short_name(name)
            if short in wanted:
                spent[short] = spent.get(short, 0.0) + duration
    return spent


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--side", type=int, default=1024, help="cells along each way around the torus: 2 side^2 faces")
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--label", default="the vertex kernel recomputes the face gradients", help="which build of the library this run loads")
    ap.add_argument("--trace-pass", action="store_true", help="only run --trace-rounds rounds of the raw calls: the run to trace")
    ap.add_argument("--trace-rounds", type=int, default=5, help="rounds of the traced run: each entry once, the two smoothings two passes each")
    ap.add_argument("--kernels-from", default=None, metavar="DIR", help="append the times of the single kernels from this trace to --out")
    ap.add_argument("--out", default=None, help="also write the report to this file (--kernels-from: append to it)")
    args = ap.parse_args()

    if args.kernels_from is not None:
        spent = kernel_us(args.kernels_from)
        missing = [name for name, _, _ in KERNELS if name not in spent]
        if missing or args.trace_rounds < 1:
            raise RuntimeError(f"the trace under {args.kernels_from} lacks {missing}")
        lines = [f"kernel trace of {args.trace_rounds} rounds of the raw calls ({args.label}), us per launch:"]
        lines += [f"  {what:62s} {name:28s} {spent[name] / (launches * args.trace_rounds):9.1f}" for name, launches, what in KERNELS]
        print("\n".join(lines))
        if args.out:
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return 0

    import torch

    from pmc_summary import head_stamp  # the sibling module
    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.export import (mesh_incidence, mesh_scalar_gradient_workspace_bytes, smooth_positions, smooth_temperature,
                                        thermal_gradient, vertex_normals)

    dev = torch.device("cuda")
    mesh, v, t = torus(args.side, dev)
    index = mesh_incidence(mesh.triangles, v)
    lib, stream = _hip.load(), _hip.current_stream()
    pos, values, tri = mesh.positions, mesh.temperature, mesh.triangles
    face = torch.empty((t, 3), dtype=torch.float64, device=dev)
    vectors, other = torch.empty((v, 3), dtype=torch.float32, device=dev), torch.empty((v, 3), dtype=torch.float32, device=dev)
    scalars, scratch = torch.empty((v,), dtype=torch.float32, device=dev), torch.empty((v,), dtype=torch.float32, device=dev)
    totals = torch.empty((4,), dtype=torch.float64, device=dev)
    need = mesh_scalar_gradient_workspace_bytes(v, t)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    shared = (tri.data_ptr(), t, v, index.offsets.data_ptr(), index.corners.data_ptr())

    def gradient(rows=True):
        _hip.check(lib.tn_mesh_scalar_gradient(pos.data_ptr(), values.data_ptr(), *shared, face.data_ptr() if rows else None, vectors.data_ptr(),
                                               scalars.data_ptr(), totals.data_ptr(), ws.data_ptr(), need, stream), "tn_mesh_scalar_gradient")

    def scalar_passes():  # lambda, then mu: two passes
        _hip.check(lib.tn_mesh_scalar_smooth(values.data_ptr(), *shared, 1, 0.5, -0.53, 0, scalars.data_ptr(), scratch.data_ptr(), stream),
                   "tn_mesh_scalar_smooth")

    def normals():
        _hip.check(lib.tn_mesh_vertex_normals(pos.data_ptr(), *shared, vectors.data_ptr(), stream), "tn_mesh_vertex_normals")

    def position_passes():
        _hip.check(lib.tn_mesh_smooth(pos.data_ptr(), *shared, 1, 0.5, -0.53, vectors.data_ptr(), other.data_ptr(), stream), "tn_mesh_smooth")

    if args.trace_pass:
        for _ in range(args.trace_rounds):
            gradient(), scalar_passes(), normals(), position_passes()
        torch.cuda.synchronize()
        return 0

    lines = [f"surface gradient and scalar smoothing on a closed lattice surface (a torus of {args.side} x {args.side} cells with a relief): {v} "
             f"vertices, {t} triangles; {args.label}; workspace of tn_mesh_scalar_gradient {need / 2 ** 20:.1f} MiB; device events around each "
             f"call, 3 warm-up calls, {args.repeats} timed calls, ms per call",
             f"measured at commit {head_stamp()}",
             "what                                                                            median ms   min .. max"]

    def row(what, m):
        lines.append(f"{what:76s} {m[0]:11.4f}   {m[1]:.4f} .. {m[2]:.4f}")

    row("tn_mesh_scalar_gradient alone (faces with rows, vertices, totals)", mesh_scenes.event_ms(gradient, args.repeats))
    row("tn_mesh_scalar_gradient alone, face_gradient NULL", mesh_scenes.event_ms(lambda: gradient(False), args.repeats))
    row("tn_mesh_scalar_smooth alone, one iteration of two passes", mesh_scenes.event_ms(scalar_passes, args.repeats))
    row("tn_mesh_vertex_normals alone", mesh_scenes.event_ms(normals, args.repeats))
    row("tn_mesh_smooth alone, one iteration of two passes", mesh_scenes.event_ms(position_passes, args.repeats))
    row("thermal_gradient (the index, the gradient, one host read)", mesh_scenes.event_ms(lambda: thermal_gradient(mesh), args.repeats))
    row("thermal_gradient after 5 iterations of one pass", mesh_scenes.event_ms(lambda: thermal_gradient(mesh, 5), args.repeats))
    row("smooth_temperature, 5 iterations of one pass (the index, the passes)", mesh_scenes.event_ms(lambda: smooth_temperature(mesh, 5), args.repeats))
    row("vertex_normals with the index built (the yardstick's public call)", mesh_scenes.event_ms(lambda: vertex_normals(pos, tri), args.repeats))
    row("smooth_positions, 5 iterations of two passes, with the index built", mesh_scenes.event_ms(lambda: smooth_positions(pos, tri, 5), args.repeats))
    mesh_scenes.emit(lines, args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
