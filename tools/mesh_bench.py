#!/usr/bin/env python
"""What the mesh export adds to a render: 8 poses of 1920x1080 at S = 48, a full-size model at its initial weights
(tests/golden/camera_path_facade_2.json scaled into the unit box, as tools/export_bench.py does), a 256^3 volume over the scene
box.  Three routes:

    render    rays + RayRenderEngine.render per pose, outputs left on the device (the floor: the code path without this feature)
    export    MeshExporter.export: the same render + tn_tsdf_integrate per pose, then tn_mesh_extract twice (sizing, emitting)
              around ONE host read
    extract   MeshExporter.extract alone, on the volume the warm-up fused

One warm-up pass per route, then ``--passes`` timed passes per route, alternating (render, export, extract, render, ...) so that
drift of a shared machine hits all alike; a pass is timed with the host clock around work that ends in a device synchronise.
The report gives the median and the range per route.  A record, not a gate.

``--components-out``: afterwards, on the mesh of the same run, the connected-components kernels (tn_mesh_components +
tn_mesh_filter_components into preallocated outputs at their upper bounds, min_triangles = 2) beside one emitting tn_mesh_extract
call, both by device events: 3 warm-up calls, then ``--repeats`` windows of ``--calls`` back-to-back calls each, median and range of
the ms per call.  The same for ``--copies`` disjoint copies of the mesh in one index list (the 10^5 - 10^6 vertices of a scene
with real surfaces; the bench model's initial weights give a small mesh).

``--smooth-out``: the same protocol for the incidence index (tn_mesh_incidence), the vertex normals (tn_mesh_vertex_normals) and 10
Taubin iterations (tn_mesh_smooth), each timed on its own into preallocated outputs, on the mesh and on its ``--copies`` copies.

    python tools/mesh_bench.py [--passes 5] [--poses 8] [--downscale 1] [--resolution 256] [--out profiles/micro/export_mesh.txt]
                               [--components-out profiles/micro/mesh_components.txt] [--smooth-out profiles/micro/mesh_smooth.txt]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_scenes import event_ms  # noqa: E402

ROUTES = ("render", "export", "extract")
MAX_T, MIN_T = 33.0, 14.0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--downscale", type=int, default=1)
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--components-out", default=None, help="time the connected-components kernels too and write that report here")
    ap.add_argument("--smooth-out", default=None, help="time the incidence index, the normals and 10 smoothing iterations too and write that report here")
    ap.add_argument("--repeats", type=int, default=15, help="event windows per timed call")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per event window")
    ap.add_argument("--copies", type=int, default=40, help="disjoint copies of the mesh in the large components timing")
    args = ap.parse_args()

    import torch

    import export_bench  # the point-cloud timing tool's model and cameras
    from thermo_nerf_amd.engine import RayRenderEngine
    from thermo_nerf_amd.export import MeshExporter

    model, cams = export_bench.setup(args)
    eng = RayRenderEngine(model, chunk=export_bench.CHUNK)
    exporter = MeshExporter(model, max_temperature=MAX_T, min_temperature=MIN_T, resolution=args.resolution, min_accumulation=0.02)
    state = {"out": None, "volume": None, "mesh": None}

    def pass_render():
        for k in range(cams.size):
            r = cams.generate_rays(k, device="cuda", flat=True)
            model.camera_optimizer.apply_to_raybundle(r)
            state["out"] = eng.render(r.origins, r.directions, out=state["out"])
        torch.cuda.synchronize()

    def pass_export():
        state["mesh"] = exporter.export(cams)
        torch.cuda.synchronize()

    def pass_extract():
        if state["volume"] is None:
            state["volume"] = exporter.fuse(cams)
            torch.cuda.synchronize()
        state["mesh"] = exporter.extract(state["volume"])
        torch.cuda.synchronize()

    fns = {"render": pass_render, "export": pass_export, "extract": pass_extract}
    for route in ROUTES:  # warm-up: code objects, stream calibration, the allocator's pools, the fused volume
        fns[route]()
    mesh = state["mesh"]
    times = {r: [] for r in ROUTES}
    lines = []
    for k in range(args.passes):
        for route in ROUTES:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fns[route]()
            times[route].append((time.perf_counter() - t) * 1e3)
            lines.append(f"pass {k}  {route:7s} {times[route][-1]:9.3f} ms")
            print(lines[-1], flush=True)
    nx, ny, nz = exporter.dims
    head = [f"mesh export, {cams.size} poses of camera_path_facade_2.json at {cams.width}x{cams.height}, S = {args.samples}, full-size model at "
            f"initial weights, chunk {export_bench.CHUNK}; volume {nx} x {ny} x {nz} over the scene box, truncation {exporter.truncation:.6g}, "
            f"min_accumulation 0.02: {len(mesh)} vertices, {int(mesh.triangles.shape[0])} triangles; 1 warm-up + {args.passes} timed passes "
            "per route, alternating", "route     median ms (whole pass)   min .. max"]
    med = {}
    for route in ROUTES:
        v = sorted(times[route])
        med[route] = v[len(v) // 2]
        head.append(f"{route:7s}  {med[route]:10.3f}               {v[0]:.3f} .. {v[-1]:.3f}")
    head.append(f"export - render {med['export'] - med['render']:+.3f} ms per pass = {(med['export'] - med['render']) / cams.size:+.3f} ms/pose "
                f"beside {med['render'] / cams.size:.3f} ms/pose of rendering; of that the extraction {med['extract']:.3f} ms (medians)")
    report = "\n".join(head + [""] + lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    if args.components_out:
        report = components_report(args, exporter, state["volume"], mesh, med["extract"])
        print(report)
        os.makedirs(os.path.dirname(os.path.abspath(args.components_out)), exist_ok=True)
        with open(args.components_out, "w") as f:
            f.write(report)
    if args.smooth_out:
        report = smooth_report(args, exporter, state["volume"], mesh)
        print(report)
        os.makedirs(os.path.dirname(os.path.abspath(args.smooth_out)), exist_ok=True)
        with open(args.smooth_out, "w") as f:
            f.write(report)
    return 0


def extract_call_of(exporter, volume, mesh):
    """one emitting tn_mesh_extract call into the mesh's own buffers: the yardstick of the two kernel reports"""
    import torch

    from thermo_nerf_amd import colormaps
    from thermo_nerf_amd.export import mesh_extract, mesh_workspace_bytes

    dev = mesh.triangles.device
    counts = torch.zeros((2,), dtype=torch.int64, device=dev)
    ws = torch.empty((mesh_workspace_bytes(exporter.dims),), dtype=torch.uint8, device=dev)
    table = colormaps.get_table(exporter.thermal_color_map, dev)[1]

    def extract_call():
        mesh_extract(volume, exporter.params, counts=counts, positions=mesh.positions, colors=mesh.colors, temperature=mesh.temperature,
                     thermal_colors=mesh.thermal_colors, thermal_table=table, triangles=mesh.triangles, workspace=ws)

    return extract_call


def components_report(args, exporter, volume, mesh, extract_pass_ms: float) -> str:
    import torch

    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.export.components import mesh_components_workspace_bytes

    lib, dev = _hip.load(), mesh.triangles.device
    v, t = len(mesh), int(mesh.triangles.shape[0])
    extract_call = extract_call_of(exporter, volume, mesh)

    def components_call_on(tri, nv):
        nt = int(tri.shape[0])
        labels = torch.empty((nv,), dtype=torch.int32, device=dev)
        component_triangles = torch.empty((nv,), dtype=torch.int32, device=dev)
        summary = torch.empty((3,), dtype=torch.int64, device=dev)
        source = torch.empty((nv,), dtype=torch.int32, device=dev)
        out = torch.empty((nt, 3), dtype=torch.int32, device=dev)
        kept = torch.empty((2,), dtype=torch.int64, device=dev)
        cws = torch.empty((mesh_components_workspace_bytes(nv, nt),), dtype=torch.uint8, device=dev)
        stream = _hip.current_stream()

        def call():  # the C entries directly: the two calls a caller with preallocated outputs makes
            _hip.check(lib.tn_mesh_components(tri.data_ptr(), nt, nv, labels.data_ptr(), component_triangles.data_ptr(),
                                              summary.data_ptr(), stream), "tn_mesh_components")
            _hip.check(lib.tn_mesh_filter_components(tri.data_ptr(), nt, nv, labels.data_ptr(), component_triangles.data_ptr(),
                                                     summary.data_ptr(), 2, 0, source.data_ptr(), nv, out.data_ptr(), nt,
                                                     kept.data_ptr(), cws.data_ptr(), cws.numel(), stream), "tn_mesh_filter_components")

        return call, summary, kept

    nx, ny, nz = exporter.dims
    lines = [f"connected components of the mesh of tools/mesh_bench.py ({nx} x {ny} x {nz} volume, {args.poses} poses, S = {args.samples}): "
             f"tn_mesh_components + tn_mesh_filter_components (min_triangles 2, outputs at their upper bounds) beside one emitting "
             f"tn_mesh_extract call; device events, 3 warm-up calls, {args.repeats} windows of {args.calls} back-to-back calls, ms per call",
             "what                                        vertices   triangles  components  kept v / t          median ms   min .. max"]
    e = event_ms(extract_call, args.repeats, args.calls)
    lines.append(f"{'tn_mesh_extract (emitting call)':43s} {v:9d} {t:11d}  {'-':>10s}  {'-':19s} {e[0]:9.4f}   {e[1]:.4f} .. {e[2]:.4f}")
    big = torch.cat([mesh.triangles + k * v for k in range(args.copies)]) if t else mesh.triangles
    for name, tri, nv in (("components + filter, the mesh", mesh.triangles, v),
                          (f"components + filter, {args.copies} disjoint copies", big, v * args.copies)):
        call, summary, kept = components_call_on(tri, nv)
        c = event_ms(call, args.repeats, args.calls)
        found, (kv, kt) = int(summary[0]), kept.tolist()
        lines.append(f"{name:43s} {nv:9d} {int(tri.shape[0]):11d}  {found:10d}  {f'{kv} / {kt}':19s} {c[0]:9.4f}   {c[1]:.4f} .. {c[2]:.4f}")
    lines.append(f"(MeshExporter.extract of the same run — sizing call, host read, allocation, emitting call — by the host clock: "
                 f"{extract_pass_ms:.3f} ms, median)")
    return "\n".join(lines) + "\n"


def smooth_report(args, exporter, volume, mesh, iterations: int = 10) -> str:
    import torch

    from thermo_nerf_amd import _hip
    from thermo_nerf_amd.export import mesh_incidence_workspace_bytes

    lib, dev = _hip.load(), mesh.triangles.device
    v, t = len(mesh), int(mesh.triangles.shape[0])
    extract_call = extract_call_of(exporter, volume, mesh)
    source = mesh.positions.clone()  # the extract call rewrites the mesh's own positions with the same values

    def calls_on(pos, tri):
        nv, nt = int(pos.shape[0]), int(tri.shape[0])
        offsets = torch.empty((nv + 1,), dtype=torch.int32, device=dev)
        corners = torch.empty((3 * nt,), dtype=torch.int32, device=dev)
        ws = torch.empty((mesh_incidence_workspace_bytes(nv, nt),), dtype=torch.uint8, device=dev)
        normals, out, scratch = (torch.empty((nv, 3), dtype=torch.float32, device=dev) for _ in range(3))
        stream = _hip.current_stream()

        def incidence():  # the C entries directly, into preallocated outputs
            _hip.check(lib.tn_mesh_incidence(tri.data_ptr(), nt, nv, offsets.data_ptr(), corners.data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream), "tn_mesh_incidence")

        def vertex_normals():
            _hip.check(lib.tn_mesh_vertex_normals(pos.data_ptr(), tri.data_ptr(), nt, nv, offsets.data_ptr(), corners.data_ptr(),
                                                  normals.data_ptr(), stream), "tn_mesh_vertex_normals")

        def smooth():
            _hip.check(lib.tn_mesh_smooth(pos.data_ptr(), tri.data_ptr(), nt, nv, offsets.data_ptr(), corners.data_ptr(), iterations, 0.5,
                                          -0.53, out.data_ptr(), scratch.data_ptr(), stream), "tn_mesh_smooth")

        return (("tn_mesh_incidence", incidence), ("tn_mesh_vertex_normals", vertex_normals),
                (f"tn_mesh_smooth, {iterations} iterations", smooth))

    nx, ny, nz = exporter.dims
    lines = [f"incidence index, vertex normals and Taubin smoothing of the mesh of tools/mesh_bench.py ({nx} x {ny} x {nz} volume, {args.poses} "
             f"poses, S = {args.samples}), each entry timed on its own into preallocated outputs, beside one emitting tn_mesh_extract call; "
             f"device events, 3 warm-up calls, {args.repeats} windows of {args.calls} back-to-back calls, ms per call",
             "what                                                      vertices   triangles   median ms   min .. max"]
    e = event_ms(extract_call, args.repeats, args.calls)
    lines.append(f"{'tn_mesh_extract (emitting call)':57s} {v:9d} {t:11d} {e[0]:9.4f}   {e[1]:.4f} .. {e[2]:.4f}")
    big_tri = torch.cat([mesh.triangles + k * v for k in range(args.copies)]) if t else mesh.triangles
    big_pos = torch.cat([source + float(k) for k in range(args.copies)])
    for label, pos, tri in (("the mesh", source, mesh.triangles), (f"{args.copies} disjoint copies", big_pos, big_tri)):
        for name, call in calls_on(pos, tri):  # in this order: the index is built before the entries that read it
            c = event_ms(call, args.repeats, args.calls)
            lines.append(f"{f'{name}, {label}':57s} {int(pos.shape[0]):9d} {int(tri.shape[0]):11d} {c[0]:9.4f}   {c[1]:.4f} .. {c[2]:.4f}")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.exit(main())
