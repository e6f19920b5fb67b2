"""Pins tests/eval_ref.py (the NumPy reference of mpcb_eval) without a GPU.

On a rollout trajectory (res_eq = 0) the recursion's g is the gradient of the single-shooting
objective J(U) = stage_cost(rollout(x0, U), U), so central finite differences of J check it.
Bound: relative 1e-5 of max(1, |g|_inf) -- central differences with h = 1e-6 on a cost of order
1e4 carry a rounding error of order 1e-16 * 1e4 / 1e-6 = 1e-6 and a truncation error of order h^2.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_ref import eval_ref, rollout_any, single_shooting_cost   # noqa: E402

from oracle.full import FullSpec, default_p25   # noqa: E402
from oracle.ocp import OcpSpec   # noqa: E402

B, N = 3, 3


def _case(model, box=False, seed=0):
    rng = np.random.default_rng(seed)
    if model == 12:
        spec = OcpSpec(N=N, lbu=np.zeros(4) if box else None, ubu=np.full(4, 65.0) if box else None)
        x0 = np.r_[0, 0, 3.5, [0] * 9] + rng.uniform(-1, 1, (B, 12)) * np.r_[[1.0] * 3, [0.17] * 3, [0.5] * 3, [0.087] * 3]
        xref = np.zeros((B, N + 1, 12))
        xref[..., 2] = 3.5
        xref[..., :2] = rng.uniform(-0.5, 0.5, (B, N + 1, 2))
        uref = np.full((B, N, 4), 22.0725)
        p25 = None
        wind = rng.uniform(-5, 5, (B, 3))
    else:
        lbu = np.array([0.0, 0.0, 0.0, 0.0, -0.0872665, -0.0872665])
        spec = FullSpec(N=N, lbu=lbu if box else None, ubu=np.array([65.0] * 4 + [0.0872665] * 2) if box else None)
        x0 = np.zeros((B, 17))
        x0[:, 2] = 3.5
        x0 += rng.uniform(-1, 1, (B, 17)) * np.r_[[1.0] * 3, [0.17] * 3, [0.5] * 3, [0.087] * 3, [0.2] * 2, [0.3] * 3]
        xref = np.zeros((B, N + 1, 17))
        xref[..., 2] = 3.5
        xref[..., 14] = 0.2
        uref = np.zeros((B, N, 6))
        uref[..., :4] = 22.0725
        p25 = np.tile(default_p25(), (B, N, 1))
        p25[..., :24] = rng.uniform(-0.5, 0.5, (B, N, 24))   # stage-varying
        wind = None
    U = uref + rng.standard_normal(uref.shape) * (1.0 if model == 12 else np.r_[[1.0] * 4, [0.05] * 2])
    return spec, x0, xref, uref, U, wind, p25


@pytest.mark.parametrize('model', [12, 17])
def test_reduced_gradient_matches_finite_differences(model):
    spec, x0, xref, uref, U, wind, p25 = _case(model)
    X = rollout_any(x0, U, spec, wind, p25)
    r = eval_ref(X, U, xref, uref, spec, x0=x0, wind=wind, p25=p25)
    assert r['res_eq'].max() < 1e-13          # a rollout has no defect
    assert np.all(r['res_ineq'] == 0.0)       # no boxes
    assert np.allclose(r['cost'], single_shooting_cost(x0, U, xref, uref, spec, wind, p25), rtol=1e-14)
    h = 1e-6
    g_fd = np.empty_like(U)
    for k in range(N):
        for m in range(U.shape[2]):
            Up, Um = U.copy(), U.copy()
            Up[:, k, m] += h
            Um[:, k, m] -= h
            g_fd[:, k, m] = (single_shooting_cost(x0, Up, xref, uref, spec, wind, p25)
                             - single_shooting_cost(x0, Um, xref, uref, spec, wind, p25)) / (2 * h)
    err = np.abs(r['g'] - g_fd).max() / max(1.0, np.abs(r['g']).max())
    print(f'model {model}: |g|_inf {np.abs(r["g"]).max():.3g}  FD error {err:.2e}  Lam {r["Lam"].max():.3g}')
    assert err < 1e-5
    assert np.array_equal(r['res_stat'], np.abs(r['g']).reshape(B, -1).max(axis=1))
    assert np.all(r['Lam'] > 0)


@pytest.mark.parametrize('model', [12, 17])
def test_natural_residual_vanishes_on_outward_bounds(model):
    spec, x0, xref, uref, U, wind, p25 = _case(model, box=True, seed=1)
    U = np.clip(uref + 40.0 * (U - uref), spec.lbu, spec.ubu)   # many components on a bound
    X = rollout_any(x0, U, spec, wind, p25)
    r = eval_ref(X, U, xref, uref, spec, x0=x0, wind=wind, p25=p25)
    g, nat = r['g'], r['nat']
    out_lo = (U == spec.lbu) & (g > 0)       # -g points below the lower bound
    out_hi = (U == spec.ubu) & (g < 0)
    assert out_lo.sum() + out_hi.sum() > 0
    assert np.all(nat[out_lo | out_hi] == 0.0)
    inside = (U - g > spec.lbu) & (U - g < spec.ubu)
    assert np.allclose(nat[inside], np.abs(g[inside]), rtol=1e-12, atol=1e-12)
    assert np.all(r['res_ineq'] == 0.0)
    U2 = U.copy()
    U2[0, 1, 2] = spec.ubu[2] + 1e-3
    r2 = eval_ref(rollout_any(x0, U2, spec, wind, p25), U2, xref, uref, spec, p25=p25, wind=wind)
    assert abs(r2['res_ineq'][0] - 1e-3) < 1e-12 and np.all(r2['res_ineq'][1:] == 0.0)


def test_state_box_counts_inner_stages_only_and_hides_res_stat():
    spec, x0, xref, uref, U, wind, p25 = _case(17, box=True, seed=2)
    spec.lbx, spec.ubx = np.full(17, -10.0), np.full(17, 10.0)
    X = rollout_any(x0, U, spec, wind, p25)
    X[0, 0, 0] = 11.0          # stages 0 and N are not boxed
    X[0, N, 1] = -12.0
    X[1, 2, 3] = 10.5
    r = eval_ref(X, np.clip(U, spec.lbu, spec.ubu), xref, uref, spec, p25=p25)
    assert r['res_ineq'][0] == 0.0 and abs(r['res_ineq'][1] - 0.5) < 1e-15
    assert np.all(np.isnan(r['res_stat']))


@pytest.mark.parametrize('model', [12, 17])
def test_nan_instance_is_isolated(model):
    spec, x0, xref, uref, U, wind, p25 = _case(model, seed=3)
    X = rollout_any(x0, U, spec, wind, p25) + 0.02 * np.random.default_rng(4).standard_normal((B, N + 1, x0.shape[1]))
    ok = eval_ref(X, U, xref, uref, spec, x0=x0, wind=wind, p25=p25)
    Xn = X.copy()
    Xn[1, 2, 5] = np.nan
    r = eval_ref(Xn, U, xref, uref, spec, x0=x0, wind=wind, p25=p25)
    for k in ('cost', 'res_eq', 'res_ineq', 'res_stat'):
        assert np.isnan(r[k][1])
        assert np.array_equal(r[k][[0, 2]], ok[k][[0, 2]])
