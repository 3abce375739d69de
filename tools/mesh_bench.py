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

    python tools/mesh_bench.py [--passes 5] [--poses 8] [--downscale 1] [--resolution 256] [--out profiles/micro/export_mesh.txt]
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
