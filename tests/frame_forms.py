"""The frame-finishing semantics (DESIGN.md "Frame finishing") as plain numpy: what tn_frame_to_rgb8 must produce byte for byte.
Shared by tests/test_render_cpu.py (against the matplotlib-made fixture) and tests/test_gpu_frames.py (against the kernel)."""
import numpy as np

F32 = np.float32


def scale_form(x: np.ndarray) -> np.ndarray:
    """v = x * 255 in fp32; trunc, saturated to [0, 255], NaN -> 0.  Shape kept."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, dtype=F32) * F32(255)
        v = np.clip(np.nan_to_num(v, nan=0.0, posinf=255.0, neginf=0.0), 0, 255)
    return v.astype(np.uint8)


def scale_frame(x: np.ndarray) -> np.ndarray:
    """[n, C] -> [n, 3]: one channel replicated to three"""
    q = scale_form(x)
    return np.repeat(q, 3, axis=1) if q.shape[1] == 1 else q


def lut_form(x: np.ndarray, table_u8: np.ndarray) -> np.ndarray:
    """[n] floats -> [n, 3]: i = trunc(x * 256), 256 -> 255; x < 0 -> entry 0, i > 255 -> entry 255, NaN -> (0, 0, 0)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * F32(256)
        i = np.clip(np.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.int64)
    out = np.asarray(table_u8)[i]
    out[np.isnan(x)] = 0
    return out
