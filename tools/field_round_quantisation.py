#!/usr/bin/env python
"""Round quantisation of the field pass: how long calls of 8 192, 10 000 and 10 240 tiles of 64 rays take.

The lane = ray field kernel gives each of its 2 048 wave slots a whole tile at a time, so a call should last
ceil(tiles / 2 048) tile-times: t(10 000) = t(10 240) = 1.25 t(8 192).  This tool times the field pass of bench.py's model
(scene weights, S = 192, exact fp32, the rays of orbit view 0 repeated as needed, one launch pair per call) by HIP events on
the launch stream, five launches per size after one warm-up, and reports what the last partial round costs beyond its share:
t(10 000) - t(8 192) x 10 000 / 8 192.

    python tools/field_round_quantisation.py [--out profiles/micro/field_round_quantisation.txt] [--tail-balance off]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TILES = (8192, 10000, 10240)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=192)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--tail-balance", default=None, help="config.tail_balance of the model, where the build has it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from thermo_nerf_amd import SceneBox, ThermalNerfModel, ThermalNerfModelConfig, synthetic
    from thermo_nerf_amd.engine import RayRenderEngine

    dev = torch.device("cuda", 0)
    o0, d0, _ = synthetic.orbit_camera_rays(800, 800, view=0)
    o0, d0 = o0.reshape(-1, 3).contiguous().to(dev), d0.reshape(-1, 3).contiguous().to(dev)
    lines = [f"field pass by HIP events, scene weights, S = {args.samples}, exact fp32, one launch pair per call, "
             f"{args.launches} launches after one warm-up" + (f", tail_balance = {args.tail_balance}" if args.tail_balance else ""),
             "tiles    rays      median ms   min .. max        all"]
    med = {}
    for tiles in TILES:
        n = tiles * 64
        reps = -(-n // o0.shape[0])
        o, d = o0.repeat(reps, 1)[:n].contiguous(), d0.repeat(reps, 1)[:n].contiguous()
        extra = {}
        if args.tail_balance is not None:
            extra["tail_balance"] = int(args.tail_balance) if args.tail_balance.isdigit() else args.tail_balance
        cfg = ThermalNerfModelConfig(num_nerf_samples_per_ray=args.samples, eval_num_rays_per_chunk=n, **extra)
        model = ThermalNerfModel(cfg, metadata={"thermal": []}, scene_box=SceneBox.unit(), num_train_data=8)
        synthetic.fill_model_(model, "scene")
        model = model.eval().to(dev)
        eng = RayRenderEngine(model, chunk=n)
        out = eng.allocate_outputs(n, dev)
        eng.render(o, d, out=out)
        torch.cuda.synchronize()
        eng.timings = []
        for _ in range(args.launches):
            eng.render(o, d, out=out, record_events=True)
        torch.cuda.synchronize()
        _, field = eng.drain_timings()
        v = sorted(field)
        med[tiles] = v[len(v) // 2]
        lines.append(f"{tiles:6d}  {n:8d}  {med[tiles]:9.3f}   {v[0]:.3f} .. {v[-1]:.3f}   " + " ".join(f"{x:.3f}" for x in field))
        print(lines[-1], flush=True)
        del eng, model, out, o, d
        torch.cuda.empty_cache()
    share = med[8192] * 10000 / 8192
    lines += ["",
              f"t(10 000) / t(8 192) = {med[10000] / med[8192]:.4f}   t(10 240) / t(8 192) = {med[10240] / med[8192]:.4f}   (whole rounds predict 1.25)",
              f"t(10 000) - t(8 192) x 10 000 / 8 192 = {med[10000]:.3f} - {share:.3f} = {med[10000] - share:.3f} ms"]
    report = "\n".join(lines) + "\n"
    print(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report)
    return 0


if __name__ == "__main__":
    sys.exit(main())
