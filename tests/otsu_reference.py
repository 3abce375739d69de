"""Test-side yardsticks of the foreground threshold (tn_otsu_thresholds): a float64 restatement of the recurrence declared in
include/thermonerf_hip.h, and a brute-force between-class variance that does not share its structure.  Test code, not product."""
from __future__ import annotations

import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def otsu_restated(hist) -> int:
    """OpenCV 4.x getThreshVal_Otsu_8u [recall] on a 256-bin histogram, in Python floats (IEEE doubles, one rounding per
    operation), in the order and association of the header."""
    h = [int(v) for v in hist]
    assert len(h) == 256
    n = float(sum(h))
    scale = 1.0 / n
    mu = 0.0
    for i in range(256):
        mu = mu + float(i) * float(h[i])  # exact: integers below 2^53
    mu = mu * scale
    mu1 = q1 = max_sigma = 0.0
    max_val = 0
    for i in range(256):
        p = float(h[i]) * scale
        mu1 = mu1 * q1
        q1 = q1 + p
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + float(i) * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = ((q1 * q2) * (mu1 - mu2)) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma = sigma
            max_val = i
    return max_val


def between_class_variance(hist) -> np.ndarray:
    """float64 [256]: w0 w1 (m0 - m1)^2 of the cut "class 0 = levels <= t" for every t, straight from the definition (class
    sums as exact integers); 0 where a class is empty."""
    h = np.asarray(hist, dtype=np.int64)
    levels = np.arange(256, dtype=np.int64)
    n = int(h.sum())
    c0 = np.cumsum(h)                # pixels in class 0
    s0 = np.cumsum(h * levels)       # grey sum of class 0
    c1, s1 = n - c0, int(s0[-1]) - s0
    out = np.zeros(256, dtype=np.float64)
    ok = (c0 > 0) & (c1 > 0)
    m0 = s0[ok] / c0[ok]
    m1 = s1[ok] / c1[ok]
    out[ok] = (c0[ok] / n) * (c1[ok] / n) * (m0 - m1) ** 2
    return out


def smallest_class_fraction(hist) -> float:
    """the smallest non-empty class over all cuts, as a fraction of the pixels (1.0 for a constant image)"""
    h = np.asarray(hist, dtype=np.int64)
    nz = np.nonzero(h)[0]
    if len(nz) < 2:
        return 1.0
    return float(min(h[nz[0]], h[nz[-1]])) / float(h.sum())
