#!/usr/bin/env python
"""Frame period of the inference harness on the reference's camera path: 96 poses at 1920x1080, S = 48, THERMAL + RGB
(tests/golden/camera_path_facade_2.json, the model and camera scaling of bench.py's camera_path_1080p_S48).  Three routes:

    engine    rays + RayRenderEngine.render per pose, float outputs left on the device (the floor: no frame leaves the GPU)
    renderer  Renderer.render: the same render, frames finished by tn_frame_to_rgb8 and copied out as RGB8, pipelined
    host      the reference's loop on the host [REF thermo_nerf/render/renderer.py:180-199]: float outputs copied to the host per
              pose, matplotlib's colour map (float64 RGBA) and x255 / uint8 in numpy.  Written with the APIs of the commit
              before Renderer existed and numpy (matplotlib where installed, else the same float64-RGBA lookup in numpy), so this
              section also runs there: it is the baseline, not something the new code produces.

Every pass is a child process under its own `timeout`: one warm-up pass over the path, then one timed pass; its frame period is
pass time / poses.  Routes alternate (engine, renderer, host, engine, ...) so that drift of a shared machine hits all alike; the
report gives the median and the range of the passes per route.  Nothing further is started after a child that fails.

    python tools/render_bench.py [--passes 3] [--poses 96] [--downscale 1] [--out profiles/micro/render_frames.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ROUTES = ("engine", "renderer", "host")
CHUNK = 1 << 16  # REF thermo_nerf/thermal_nerf/config_thermal_nerf.py:30


def setup(args):
    import torch

    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic
    from thermo_nerf_amd.cameras import Cameras, get_path_from_json

    cams = get_path_from_json(json.load(open(os.path.join(ROOT, "tests", "golden", "camera_path_facade_2.json"))))
    c2w = cams.camera_to_worlds.clone()
    c2w[:, :3, 3] *= 0.45 / c2w[:, :3, 3].norm(dim=-1).max()  # the path was recorded around a real scene; the weights live in [-1,1]^3
    p = min(args.poses, len(cams))
    cams = Cameras(camera_to_worlds=c2w[:p], fx=cams.fx[:p], fy=cams.fy[:p], cx=cams.cx, cy=cams.cy, height=cams.height, width=cams.width)
    cams.rescale_output_resolution(1.0 / args.downscale)
    cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=args.samples, eval_num_rays_per_chunk=CHUNK)
    model = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=8)
    synthetic.fill_model_(model, "scene")
    model = model.eval().to("cuda")
    torch.cuda.synchronize()
    return model, cams


def pass_engine(model, cams):
    import torch

    from thermo_nerf_amd.engine import RayRenderEngine

    eng = pass_engine.__dict__.setdefault("eng", RayRenderEngine(model, chunk=CHUNK))
    out = None
    for i in range(cams.size):
        rb = cams.generate_rays(i, device="cuda", flat=True)
        out = eng.render(rb.origins, rb.directions, out=out)
    torch.cuda.synchronize()
    return None


def pass_renderer(model, cams):
    from thermo_nerf_amd.render import Renderer
    from thermo_nerf_amd.rendered_image_modalities import RenderedImageModality as RM

    r = pass_renderer.__dict__.setdefault("r", Renderer(model))
    r.render([RM.THERMAL, RM.RGB], cams)
    return "tn_frame_to_rgb8"


def host_colour():
    """(name, f): f(thermal [H,W] float32) -> uint8 [H,W,3] the way the reference gets it"""
    import numpy as np

    try:
        import matplotlib

        cmap = matplotlib.colormaps["magma"]
        return "matplotlib", lambda x: (cmap(x)[:, :, :3] * 255).astype(np.uint8)
    except ImportError:  # the same work in numpy: a float64 RGBA image by table lookup, then x255 and the cast
        ramp = np.linspace(0.0, 1.0, 256)
        lut = np.stack([ramp, ramp ** 2, 1.0 - ramp, np.ones(256)], axis=1)
        return "numpy float64-RGBA lookup", lambda x: (lut[np.clip(x * 256, 0, 255).astype(np.int64)][:, :, :3] * 255).astype(np.uint8)


def pass_host(model, cams):
    import numpy as np

    name, colour = pass_host.__dict__.setdefault("colour", host_colour())
    frames = {"thermal": [], "rgb": []}
    for i in range(cams.size):
        out = model.get_outputs_for_camera_ray_bundle(cams.generate_rays(i, device="cuda"))
        frames["thermal"].append(colour(out["thermal"].cpu().numpy()[:, :, 0]))
        frames["rgb"].append((out["rgb"].cpu().numpy() * 255).astype(np.uint8))
    return name


def child(args) -> int:
    model, cams = setup(args)
    fn = {"engine": pass_engine, "renderer": pass_renderer, "host": pass_host}[args.child]
    fn(model, cams)  # warm-up pass: code objects, stream calibration, pinned buffers, the allocator's pools
    if args.child == "renderer":  # the warm-up pass's 1.2 GB of frames are released before the clock starts, not inside the pass
        pass_renderer.r._rendered_images = {}
    t = time.perf_counter()
    note = fn(model, cams)
    dt = time.perf_counter() - t
    fn.__dict__.clear()  # engine / renderer with their streams and pinned buffers: released before the interpreter winds down
    print("RESULT " + json.dumps({"route": args.child, "poses": cams.size, "width": cams.width, "height": cams.height,
                                  "pass_s": dt, "frame_ms": dt / cams.size * 1e3, "note": note}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--child", choices=ROUTES, default=None, help="(internal) run one warm-up and one timed pass of a route")
    ap.add_argument("--routes", nargs="+", default=list(ROUTES), choices=ROUTES)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--poses", type=int, default=96)
    ap.add_argument("--downscale", type=int, default=1)
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--pass-timeout", type=int, default=150, help="seconds a child (set-up, warm-up pass, timed pass) may take")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = {r: [] for r in args.routes}
    lines = []
    for k in range(args.passes):
        for route in args.routes:
            cmd = ["timeout", "-k", "10", str(args.pass_timeout), sys.executable, os.path.abspath(__file__), "--child", route,
                   "--poses", str(args.poses), "--downscale", str(args.downscale), "--samples", str(args.samples)]
            p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
            got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                print(p.stdout[-2000:], p.stderr[-4000:], sep="\n")
                print(f"pass {k} of {route} ended with status {p.returncode}: nothing further is started")
                return 1
            res = json.loads(got[-1][7:])
            results[route].append(res)
            lines.append(f"pass {k}  {route:9s} {res['frame_ms']:8.2f} ms/frame  ({res['pass_s']:.2f} s for {res['poses']} poses"
                         f"{', ' + res['note'] if res['note'] else ''})")
            print(lines[-1], flush=True)
    any_res = next(iter(results.values()))[0]
    head = [f"frame period, {any_res['poses']} poses of camera_path_facade_2.json at {any_res['width']}x{any_res['height']}, S = {args.samples}, "
            f"THERMAL + RGB, chunk {CHUNK}; per route {args.passes} child processes (warm-up pass + timed pass), routes alternating",
            "route      median ms/frame   min .. max"]
    for route, rs in results.items():
        v = sorted(r["frame_ms"] for r in rs)
        head.append(f"{route:9s}  {v[len(v) // 2]:8.2f}          {v[0]:.2f} .. {v[-1]:.2f}")
    report = "\n".join(head + [""] + lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
