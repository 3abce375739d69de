"""CPU: tests/adam_reference.py — the restatement tests/test_gpu_adam.py holds tn_adam_step to bit for bit — IS Adam, shown without
the kernel: its float64 form follows torch.optim.Adam on float64 tensors to float64 rounding, its float32 form stays within a
derived rounding bound of the float64 form, and that bound is narrow enough to reject two plausible wrong denominators."""
import numpy as np
import pytest
import torch

from tests import adam_reference as R

BETAS = (0.9, 0.999)
# the reference's three parameter groups (lr, eps, weight decay): fields, proposal networks' later schedule, camera_opt
GROUPS = [(1e-2, 1e-15, 0.0), (3e-3, 1e-15, 0.0), (6e-4, 1e-8, 1e-2)]

# ---- rounding budget of step_f32 against step_f64 (first order in u = 2^-24; "(n)" = n roundings, relative to the result) ----
# Inputs of the bounded tests have p, g, m of ONE sign per element and beta1 >= 1/2, so that no step cancels except the final
# p - update (whose own rounding is the 1/2 ulp32 term) and g' - m (whose rounding is relative to its own result and enters m'
# scaled by one_minus_beta1 * |g' - m| <= |m'|).  With wd = 0 / wd != 0:
#   g'  = g + wd*p                   : product (1) + sum (1), both <= |g'|                          ->  0   / 2
#   m'  = m + (g' - m)*omb1          : g' inherited, difference (1), product (1), sum (1)           ->  3   / 5
#   v'  = beta2*v + (omb2*g')*g'     : max(product (1), two products (2) + 2 g'), positive sum (1)  ->  3   / 7
#   sqrt(v')                         : half of v', root (1)                                         ->  2.5 / 4.5
#   ... / bias_correction2_sqrt      : quotient (1)                                                 ->  3.5 / 5.5
#   den = ... + eps                  : positive sum (1)                                             ->  4.5 / 6.5
#   m' / den                         : m' + den + quotient (1)                                      ->  8.5 / 12.5
#   update = step_size * (...)       : product (1)                                                  ->  9.5 / 13.5
# K = 10 / 14 leaves the half unit to the second-order terms.  The moments, against their LARGEST ADDEND (no sign assumption;
# G = |g| + |wd*p| >= |g'|, error of g' <= 2 u G):
#   A_m = max(|m|, omb1*G):   omb1*err(g') <= 2 u A_m, difference and product <= 2 u omb1 |g' - m| <= 4 u A_m, sum <= u |m'|
#                             <= 3 u A_m                                            -> 7 (wd = 0: no g' term) / 9
#   A_v = max(beta2*v, omb2*G^2):  beta2*v (1), omb2*g'*g' (2) + 2 err(g')/G (4 with wd), sum <= u v' <= 2 u A_v
#                                                                                   -> 5 / 9


def update_roundings(weight_decay: float) -> int:
    return 14 if weight_decay != 0 else 10


def moment_roundings(weight_decay: float):
    return (9, 9) if weight_decay != 0 else (7, 5)


def _f64_run(shapes, groups_of, steps, skip, seed):
    """`steps` Adam steps on float64 tensors, by torch.optim.Adam and by step_f64 with unrounded float64 scalars, on the same
    gradients; tensor `skip` receives a gradient one step in three.  -> [(ours (p, m, v), torch (p, m, v))] per tensor"""
    rng = np.random.default_rng(seed)
    init = [rng.standard_normal(s) for s in shapes]
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in init]
    group_of = {k: gi for gi, ks in enumerate(groups_of) for k in ks}
    opt = torch.optim.Adam([{"params": [tp[k] for k in ks], "lr": GROUPS[gi][0], "eps": GROUPS[gi][1], "weight_decay": GROUPS[gi][2]}
                            for gi, ks in enumerate(groups_of)], betas=BETAS)
    ours = [[a.copy(), np.zeros_like(a), np.zeros_like(a), 0] for a in init]
    for step in range(steps):
        for k, q in enumerate(tp):
            if k == skip and step % 3:
                q.grad = None
                continue
            g = rng.standard_normal(shapes[k]) * 10.0 ** (step % 4 - 3)
            if k == 1:
                g[::2] = 0.0
            q.grad = torch.from_numpy(g.copy())
            st = ours[k]
            st[3] += 1
            lr, eps, wd = GROUPS[group_of[k]]
            st[0], st[1], st[2], _ = R.step_f64(st[0], g, st[1], st[2], R.scalars(lr, BETAS, eps, wd, st[3], dtype=np.float64))
        opt.step()
    out = []
    for k, q in enumerate(tp):
        s = opt.state[q]
        assert float(s["step"]) == ours[k][3]
        out.append((tuple(ours[k][:3]), (q.detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy())))
    return out


def test_step_f64_is_torch_adam_in_float64():
    """Eight steps of seven float64 tensors in the reference's three groups (lr 1e-2 / eps 1e-15; lr 3e-3; lr 6e-4 / eps 1e-8 /
    weight decay 1e-2), gradients of 1e-3 .. 1 with zeros among them, one tensor that receives a gradient on one step in three:
    step_f64 with unrounded float64 scalars against torch.optim.Adam.  The two differ only in torch's lerp form of the first moment
    (which switches formula at weight 0.5) and in where float64 rounds.  Distance = max |ours - torch| over a tensor, relative to
    the tensor's largest |torch| entry.  Measured: parameters 1.2e-16, first moment 2.4e-16, second moment 1.8e-16 (one or two
    float64 roundings of the largest entry); asserted at 1e-15, four times the largest of them."""
    shapes = [(64, 63), (64,), (3, 5), (1,), (10003,), (257, 2), (7, 6)]
    worst = [0.0, 0.0, 0.0]
    for ours, ref in _f64_run(shapes, [(0, 1, 2), (3, 4, 5), (6,)], steps=8, skip=3, seed=5):
        for j, (a, b) in enumerate(zip(ours, ref)):
            assert a.dtype == b.dtype == np.float64
            worst[j] = max(worst[j], float(np.abs(a - b).max() / np.abs(b).max()))
    print("float64 distance to torch.optim.Adam (param, exp_avg, exp_avg_sq):", worst)
    assert max(worst) <= 1e-15, worst


def _signed_state(n, seed, g_scale, p_scale, t):
    """float32 p, g, m, v of one sign per element (see the budget above), magnitudes spread over a decade around their scale; the
    moments are those of a run that has seen gradients of g_scale for t - 1 steps (zero at t = 1)"""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mag = lambda: 10.0 ** rng.uniform(-0.5, 0.5, n)
    p = (sign * p_scale * mag()).astype(np.float32)
    g = (sign * g_scale * mag()).astype(np.float32)
    if t == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (sign * g_scale * mag() * (1.0 - BETAS[0] ** (t - 1))).astype(np.float32)
    v = ((g_scale * mag()) ** 2 * (1.0 - BETAS[1] ** (t - 1))).astype(np.float32)
    return p, g, m, v


# (lr, eps, weight decay, gradient scale, parameter scale, t).  ORDINARY: the three groups on gradients of 1e-3 and parameters of
# 1.  EPS_SENSITIVE: gradients of 1e-8 with eps = 1e-8 — sqrt(v')/bias_correction2_sqrt is of eps's size, so where eps enters and
# what the root is divided by both move the update by tens of per cent — at the first step, the second and one where the
# correction is 0.63; with weight decay the parameters are 1e-6, so that wd*p is of the gradient's size and eps still matters.
ORDINARY = [(lr, eps, wd, 1e-3, 1.0, t) for lr, eps, wd in GROUPS for t in (1, 7, 30000)]
EPS_SENSITIVE = [(1e-2, 1e-8, wd, 1e-8, 1.0 if wd == 0 else 1e-6, t) for wd in (0.0, 1e-2) for t in (1, 2, 1000)]
N = 1 << 16


def _one_step(setting, seed):
    lr, eps, wd, g_scale, p_scale, t = setting
    p, g, m, v = _signed_state(N, seed, g_scale, p_scale, t)
    s = R.scalars(lr, BETAS, eps, wd, t)
    return (p, g, m, v), s, R.step_f32(p, g, m, v, s), R.step_f64(p, g, m, v, s)


@pytest.mark.parametrize("setting", ORDINARY + EPS_SENSITIVE, ids=lambda s: "lr%g-eps%g-wd%g-g%g-p%g-t%d" % s)
def test_step_f32_stays_within_its_rounding_budget_of_step_f64(setting):
    """One step from identical float32 state, 65536 elements: |p32 - p64| <= 1/2 ulp32(p64) + K 2^-24 |update| with K = 10 (14 with
    weight decay) roundings on the update's path, and both moments within 7 / 5 (9 / 9) units of 2^-24 of their largest addend —
    the budget derived at the top of this file.  Observed on these inputs: the update's share reaches 4.3 units of 2^-24 |update|
    (negative where the parameter's half ulp alone covers the distance), the first moment 4.3 units, the second 5.7."""
    (p, g, m, v), s, (p32, m32, v32), (p64, m64, v64, upd) = _one_step(setting, seed=11)
    wd = float(s.weight_decay)
    excess = (np.abs(p32.astype(np.float64) - p64) - 0.5 * R.ulp32(p64)) / (R.U32 * np.abs(upd))
    G = np.abs(g.astype(np.float64)) + np.abs(wd * p.astype(np.float64))
    a_m = np.maximum(np.abs(m.astype(np.float64)), float(s.one_minus_beta1) * G)
    a_v = np.maximum(float(s.beta2) * v.astype(np.float64), float(s.one_minus_beta2) * G * G)
    em = np.abs(m32.astype(np.float64) - m64) / (R.U32 * a_m)
    ev = np.abs(v32.astype(np.float64) - v64) / (R.U32 * a_v)
    print("units of 2^-24: update %.2f, exp_avg %.2f, exp_avg_sq %.2f" % (excess.max(), em.max(), ev.max()))
    assert np.all(np.abs(p32.astype(np.float64) - p64) <= R.param_bound(p64, upd, update_roundings(wd))), excess.max()
    km, kv = moment_roundings(wd)
    assert em.max() <= km and ev.max() <= kv, (em.max(), ev.max())


@pytest.mark.parametrize("variant", ["eps_inside", "sqrt_of_quotient"])
@pytest.mark.parametrize("setting", EPS_SENSITIVE, ids=lambda s: "wd%g-t%d" % (s[2], s[5]))
def test_the_parameter_bound_rejects_wrong_denominators(setting, variant):
    """What makes the bit-level GPU test's eps-sensitive cases a test of the formula: on each of them the parameter bound that the
    right step_f32 meets (previous test) is violated by EVERY element of a step whose denominator is (sqrt(v') + eps) /
    bias_correction2_sqrt ("eps inside the correction") or sqrt(v' / bias_correction2_sqrt) + eps (sqrt(v / bc2) with the
    descriptor's scalar for bc2) — the wrong formulas evaluated in float64, so nothing but the formula differs.  Smallest
    distance over all twelve cases: 411 times the bound."""
    _, s, (p32, _, _), (p64, _, _, upd) = _one_step(setting, seed=11)
    bound = R.param_bound(p64, upd, update_roundings(float(s.weight_decay)))
    assert np.all(np.abs(p32.astype(np.float64) - p64) <= bound)
    (p, g, m, v), _, _, _ = _one_step(setting, seed=11)
    wrong = R.step_f64(p, g, m, v, s, variant=variant)[0]
    ratio = np.abs(wrong - p64) / bound
    print("wrong formula's distance in units of the bound: min %.3g" % ratio.min())
    assert np.all(ratio > 1.0), ratio.min()
