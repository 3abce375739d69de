"""Test-side yardstick of the point-cloud export (tn_pointcloud_append): a numpy restatement of the definitions in
include/thermonerf_hip.h with explicit float32 steps in the stated order — the predicate, the ordered selection, the world
transform, degrees, and the SCALE / LUT bytes.  Test code, not product."""
from __future__ import annotations

import numpy as np

F = np.float32
INF = float("inf")
IDENTITY = np.eye(3, 4, dtype=np.float32)


def params(min_accumulation=0.5, box_min=(-INF,) * 3, box_max=(INF,) * 3, thermal_lo=-INF, thermal_hi=INF, max_temperature=1.0,
           min_temperature=0.0, to_world=None) -> dict:
    """the parameter block as fp32 values, each rounded once from a double (span = max - min in double)"""
    return dict(min_accumulation=F(min_accumulation), box_min=np.asarray(box_min, dtype=np.float64).astype(F),
                box_max=np.asarray(box_max, dtype=np.float64).astype(F), thermal_lo=F(thermal_lo), thermal_hi=F(thermal_hi),
                temperature_span=F(float(max_temperature) - float(min_temperature)), temperature_min=F(min_temperature),
                to_world=IDENTITY.copy() if to_world is None else np.asarray(to_world, dtype=np.float64).reshape(3, 4).astype(F))


def back_project(origins, directions, depth) -> np.ndarray:
    o, d = np.asarray(origins, dtype=F).reshape(-1, 3), np.asarray(directions, dtype=F).reshape(-1, 3)
    t = np.asarray(depth, dtype=F).reshape(-1, 1)
    with np.errstate(all="ignore"):
        return (o + (d * t).astype(F)).astype(F)  # multiply, add: two roundings


def keep_mask(p, accumulation, thermal, q) -> np.ndarray:
    a, th = np.asarray(accumulation, dtype=F).reshape(-1), np.asarray(thermal, dtype=F).reshape(-1)
    with np.errstate(invalid="ignore"):  # a NaN compares false: dropped
        keep = a > q["min_accumulation"]
        keep &= np.all(p > q["box_min"][None, :], axis=1) & np.all(p < q["box_max"][None, :], axis=1)
        keep &= (th > q["thermal_lo"]) & (th < q["thermal_hi"])
    return keep


def scale_bytes(x) -> np.ndarray:
    """TN_FRAME_SCALE: trunc(x * 255) saturated to [0, 255], NaN -> 0"""
    with np.errstate(all="ignore"):
        v = (np.asarray(x, dtype=F) * F(255.0)).astype(F)
    v = np.where(np.isnan(v), F(0.0), np.clip(v, F(0.0), F(255.0)))
    return v.astype(np.int64).astype(np.uint8)


def lut_bytes(x, table_u8) -> np.ndarray:
    """TN_FRAME_LUT: i = trunc(x * 256) clamped to [0, 255] (x < 0 -> 0, 256 and above -> 255), NaN -> (0, 0, 0)"""
    x = np.asarray(x, dtype=F).reshape(-1)
    with np.errstate(all="ignore"):
        t = (x * F(256.0)).astype(F)
    i = np.where(np.isnan(t), F(0.0), np.clip(t, F(0.0), F(255.0))).astype(np.int64)
    out = np.asarray(table_u8, dtype=np.uint8)[i]
    out[np.isnan(x)] = 0
    return out


def export(origins, directions, depth, accumulation, rgb, thermal, q, table_u8=None, source_base=0) -> dict:
    """the kept rays in ray order: positions, colors, temperature, thermal_colors (with a table), source"""
    p = back_project(origins, directions, depth)
    keep = keep_mask(p, accumulation, thermal, q)
    index = np.nonzero(keep)[0]
    p, th = p[index], np.asarray(thermal, dtype=F).reshape(-1)[index]
    m = q["to_world"]
    with np.errstate(all="ignore"):
        cols = []
        for c in range(3):
            s = ((m[c, 0] * p[:, 0]).astype(F) + (m[c, 1] * p[:, 1]).astype(F)).astype(F)
            s = (s + (m[c, 2] * p[:, 2]).astype(F)).astype(F)
            cols.append((s + m[c, 3]).astype(F))
        temperature = ((th * q["temperature_span"]).astype(F) + q["temperature_min"]).astype(F)
    out = dict(positions=np.stack(cols, axis=1) if len(index) else np.zeros((0, 3), F),
               colors=scale_bytes(np.asarray(rgb, dtype=F).reshape(-1, 3)[index]), temperature=temperature,
               source=(index + int(source_base)).astype(np.int64), keep=keep)
    if table_u8 is not None:
        out["thermal_colors"] = lut_bytes(th, table_u8)
    return out
