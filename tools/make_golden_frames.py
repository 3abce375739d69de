#!/usr/bin/env python
"""Write tests/golden/frame_finish.npz: inputs and expected bytes of frame finishing (tn_frame_to_rgb8), computed with
matplotlib and numpy only — the reference's own expressions [REF thermo_nerf/render/renderer.py:189-199]:

    scale       (x * 255).astype(np.uint8)                         for x in [0, 1]; outside [0, 256) numpy's cast is undefined and
                                                                   the project's rule stands: saturate to [0, 255], NaN -> 0
    lut_magma   (matplotlib.colormaps["magma"](x)[:, :3] * 255).astype(np.uint8)
    lut_turbo   the same with "turbo"

Inputs (float32): seeded random values in [0, 1]; every k/256 and k/255 with its two float32 neighbours; and
0, -0.0, 1, 1 - 2^-24, NaN, +inf, -inf, -0.25, 1.5.  tests/test_render_cpu.py checks that the index form documented in DESIGN.md
reproduces these bytes without matplotlib; tests/test_gpu_frames.py demands them of the kernel.
"""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "frame_finish.npz")
SPECIALS = (0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, float("nan"), float("inf"), float("-inf"), -0.25, 1.5)


def inputs(seed: int = 20) -> np.ndarray:
    rng = np.random.default_rng(seed)
    parts = [rng.random(2048, dtype=np.float32)]
    for den in (256, 255):
        b = (np.arange(den + 1, dtype=np.float64) / den).astype(np.float32)
        parts += [b, np.nextafter(b, np.float32(-1)), np.nextafter(b, np.float32(2))]
    parts.append(np.asarray(SPECIALS, dtype=np.float32))
    return np.concatenate(parts).astype(np.float32)


def scale_bytes(x: np.ndarray) -> np.ndarray:
    v = x * np.float32(255)
    assert v.dtype == np.float32
    out = np.zeros(x.shape, dtype=np.uint8)
    inside = (v >= 0) & (v < 256)
    out[inside] = v[inside].astype(np.uint8)  # numpy's cast, defined here
    out[v >= 256] = 255
    return out


def lut_bytes(x: np.ndarray, name: str) -> np.ndarray:
    import matplotlib

    with np.errstate(invalid="ignore", over="ignore"):
        return (matplotlib.colormaps[name](x)[:, :3] * 255).astype(np.uint8)


def main() -> None:
    x = inputs()
    unit = (x >= 0) & (x <= 1)
    scale = scale_bytes(x)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(scale[unit], (x[unit] * 255).astype(np.uint8))  # the reference's expression wherever it is defined
    np.savez_compressed(OUT, x=x, scale=scale, lut_magma=lut_bytes(x, "magma"), lut_turbo=lut_bytes(x, "turbo"))
    print("wrote", OUT, x.shape[0], "inputs,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
