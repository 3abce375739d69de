"""Test-side yardsticks of the Adam step (tn_adam_step, include/thermonerf_hip.h): the operation sequence the header declares, once
in float32 with one correctly rounded numpy operation per kernel intrinsic (what every output float must equal bit for bit), once
in float64 from the same float32 inputs (what the float32 sequence is an approximation of).  Test code, not product."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32: one rounding to nearest moves a normal-range result by at most U32 * |result|


class Scalars(NamedTuple):
    """the seven per-tensor scalars of a tn_adam_tensor descriptor, in the struct's order, as float32"""
    step_size: np.float32
    bias_correction2_sqrt: np.float32
    one_minus_beta1: np.float32
    beta2: np.float32
    one_minus_beta2: np.float32
    eps: np.float32
    weight_decay: np.float32


def scalars(lr: float, betas, eps: float, weight_decay: float, t: float, dtype=np.float32) -> Scalars:
    """the descriptor of step ``t`` (the tensor's own step count, 1-based) as thermo_nerf_amd/optim.py forms it: Python floats
    (float64) on the host, each rounded to float32 once by the C struct's float field.  ``dtype=np.float64`` keeps the host's
    values unrounded (the comparison with torch.optim.Adam in float64, which never sees a float32 scalar)."""
    b1, b2 = float(betas[0]), float(betas[1])
    t = float(t)
    vals = (lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 - b1, b2, 1.0 - b2, eps, weight_decay)
    return Scalars(*(dtype(v) for v in vals))


def step_f32(p, g, m, v, s: Scalars):
    """one step in float32 -> (p', m', v').  Every line is one IEEE operation on float32 operands (numpy's add / subtract /
    multiply / divide / sqrt on float32 arrays are correctly rounded and keep subnormals), in the kernel's order and association:

        g' = g + wd*p                              (only when wd != 0)
        m' = m + (g' - m)*one_minus_beta1
        v' = beta2*v + (one_minus_beta2*g')*g'
        den = sqrt(v')/bias_correction2_sqrt + eps
        p' = p - step_size*(m'/den)
    """
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    s = Scalars(*(np.float32(x) for x in s))
    with np.errstate(all="ignore"):
        if s.weight_decay != 0:
            g = g + s.weight_decay * p
        m1 = m + (g - m) * s.one_minus_beta1
        v1 = s.beta2 * v + (s.one_minus_beta2 * g) * g
        den = np.sqrt(v1) / s.bias_correction2_sqrt + s.eps
        p1 = p - s.step_size * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    return p1, m1, v1


def step_f64(p, g, m, v, s: Scalars, variant: str = "adam"):
    """the same formula in float64 from the same inputs and scalars as they are handed in (float32 arrays and the float32-rounded
    scalars of ``scalars`` when it stands next to step_f32; nothing is rounded here) -> (p', m', v', update) with
    update = step_size*m'/den.  ``variant`` swaps the denominator for one of two plausible WRONG ones (the tests show that their
    bounds tell them from the right one): "eps_inside" = (sqrt(v') + eps)/bias_correction2_sqrt, "sqrt_of_quotient" =
    sqrt(v'/bias_correction2_sqrt) + eps, i.e. sqrt(v / bc2) with the descriptor's scalar in the place of bc2."""
    p, g, m, v = (np.asarray(a).astype(np.float64) for a in (p, g, m, v))
    s = Scalars(*(np.float64(x) for x in s))
    with np.errstate(all="ignore"):
        if s.weight_decay != 0:
            g = g + s.weight_decay * p
        m1 = m + (g - m) * s.one_minus_beta1
        v1 = s.beta2 * v + (s.one_minus_beta2 * g) * g
        if variant == "adam":
            den = np.sqrt(v1) / s.bias_correction2_sqrt + s.eps
        elif variant == "eps_inside":
            den = (np.sqrt(v1) + s.eps) / s.bias_correction2_sqrt
        elif variant == "sqrt_of_quotient":
            den = np.sqrt(v1 / s.bias_correction2_sqrt) + s.eps
        else:
            raise ValueError(variant)
        update = s.step_size * (m1 / den)
        p1 = p - update
    return p1, m1, v1, update


def ulp32(x) -> np.ndarray:
    """float64: the spacing of float32 at |x| (x a float64 value inside float32's range): 2^(e-23) for 2^e <= |x| < 2^(e+1), the
    subnormal spacing 2^-149 below 2^-126"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)  # x = f * 2^e, 0.5 <= f < 1
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def param_bound(p64, update64, k: float) -> np.ndarray:
    """|p32 - p64| <= 1/2 ulp32(p64) + k * 2^-24 * |update|: the final subtraction's own rounding, plus k roundings carried by
    the update (tests/test_adam_cpu.py derives k)"""
    return 0.5 * ulp32(p64) + k * U32 * np.abs(update64)


def bits(a) -> np.ndarray:
    """float32 array -> its uint32 bit patterns, every NaN mapped to ONE pattern (payload and sign of a NaN are not part of the
    kernel's contract)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b
