"""mpcb_eval on the GPU (cost and KKT residuals of an iterate) against tests/eval_ref.py.

Every case compares the device with the NumPy reference, never with itself.  The trajectories are
not solver output: U = uref + N(0, 1), X = rollout + N(0, 0.02), so defects of order 0.1 and
gradients of order 10..100 are exercised.

fp64 bounds: cost 1e-12 max(1, |ref|); res_eq and res_ineq 1e-12 absolute (the pin of the same Phi
in tests/test_gpu_parity.py; res_ineq is one subtraction of the inputs); res_stat
1e-12 (N + 1) max(1, Lam) absolute, Lam = max_k |lambda_k|_1: every [A|B] entry is pinned at 1e-12,
multiplies a multiplier component, and the error compounds once per stage through lambda.
fp32 bounds: 8 x the largest move of the fp64 reference under a relative 2^-22 perturbation of
x0, X, U and the references (4 trials on the test's own draws), against the fp64 reference on the
fp32-rounded inputs; 8 x because the perturbation models the rounding of the data only, not the
few hundred roundings inside N RK4 steps and the lambda recursion.
Each test prints its measured maxima (DESIGN.md records them).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_ref import eval_ref, rollout_any   # noqa: E402

from oracle.full import FullSpec, default_p25   # noqa: E402
from oracle.inputs import draws, make_sine_ref, make_wind, make_x0   # noqa: E402
from oracle.ocp import OcpSpec, stage_cost   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('cost', 'res_eq', 'res_ineq', 'res_stat')
LBU17 = np.array([0.0, 0.0, 0.0, 0.0, -0.0872665, -0.0872665])
UBU17 = np.array([65.0, 65.0, 65.0, 65.0, 0.0872665, 0.0872665])
SB_LO = np.array([-1.5, -1.5, 0, -0.174532925, -0.174532925, -0.349066, -1.0, -1.0, -1.0, -0.0872665, -0.0872665,
                  -0.0872665, -0.174532925, -0.523599, -1.5, -1.5, -2.5])
SB_HI = np.array([1.5, 1.5, 5.0, 0.174532925, 0.174532925, 0.349066, 1.0, 1.0, 1.0, 0.0872665, 0.0872665,
                  0.0872665, 1.22173, 0.523599, 1.5, 1.5, 2.5])


def _mpc12(N, B, dtype='f64', box=False):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig(N=N, dtype=dtype, lbu=np.zeros(4) if box else None,
                                ubu=np.full(4, 65.0) if box else None), max_batch=B)


def _spec12(N, box=False):
    return OcpSpec(N=N, lbu=np.zeros(4) if box else None, ubu=np.full(4, 65.0) if box else None)


@functools.lru_cache(maxsize=None)
def _case12(B, N, ref, wind, seed=7):
    """x0, xref (sine: [B, ...]; hover: [1, ...], stride 0), uref [1, ...], wind, U, X."""
    Ud = draws(1003 + seed, np.arange(B, dtype=np.uint64))
    x0 = make_x0(Ud)
    xref = make_sine_ref(Ud, N, 1.0 / 30.0) if ref == 'sine' else np.tile(np.r_[0, 0, 3.5, [0.0] * 9], (1, N + 1, 1))
    uref = np.full((1, N, 4), 22.0725)
    w = make_wind(Ud) if wind else None
    rng = np.random.default_rng(seed)
    U = uref + rng.standard_normal((B, N, 4))
    X = rollout_any(x0, U, _spec12(N), w) + 0.02 * rng.standard_normal((B, N + 1, 12))
    return x0, xref, uref, w, U, X


@functools.lru_cache(maxsize=None)
def _case17(B=5, N=4, seed=11):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 17))
    x0[:, 2] = 3.5
    x0 += rng.uniform(-1, 1, (B, 17)) * np.r_[[1.0] * 3, [0.17] * 3, [0.5] * 3, [0.087] * 3, [0.2] * 2, [0.3] * 3]
    xref = np.zeros((B, N + 1, 17))
    xref[..., 2] = 3.5
    xref[..., 14] = 0.2
    uref = np.zeros((B, N, 6))
    uref[..., :4] = 22.0725
    p = np.tile(default_p25(), (B, N, 1))
    p[..., :24] = rng.uniform(-0.5, 0.5, (B, N, 24))   # stage-varying parameters
    U = uref + rng.standard_normal((B, N, 6))
    X = rollout_any(x0, U, FullSpec(N=N), None, p) + 0.02 * rng.standard_normal((B, N + 1, 17))
    return x0, xref, uref, p, U, X


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def _check64(got, ref, N, tag, stat=True):
    err = dict(cost=np.abs(got['cost'] - ref['cost']) / np.maximum(1.0, np.abs(ref['cost'])),
               res_eq=np.abs(got['res_eq'] - ref['res_eq']), res_ineq=np.abs(got['res_ineq'] - ref['res_ineq']))
    bound = dict(cost=1e-12, res_eq=1e-12, res_ineq=1e-12)
    if stat:
        err['res_stat'] = np.abs(got['res_stat'] - ref['res_stat']) / ((N + 1) * np.maximum(1.0, ref['Lam']))
        bound['res_stat'] = 1e-12
        print(f'{tag}: res_stat abs err {np.abs(got["res_stat"] - ref["res_stat"]).max():.2e} '
              f'(ref up to {ref["res_stat"].max():.3g}, Lam up to {ref["Lam"].max():.3g})')
    else:
        assert 'res_stat' not in got
    print(f'{tag}: ' + '  '.join(f'{k} {v.max():.2e}/{bound[k]:.0e}' for k, v in err.items()))
    for k, v in err.items():
        assert v.max() <= bound[k], (tag, k, v.max())


# ------------------------------------------------------------------------------ 12/4 fp64
@pytest.mark.parametrize('B,N,ref,wind,with_x0', [
    (1, 3, 'hover', False, True), (7, 3, 'sine', True, False), (1, 20, 'sine', True, True),
    (7, 20, 'hover', False, False), (7, 20, 'sine', False, True), (4099, 20, 'sine', True, True)])
def test_eval12_fp64_matches_reference(B, N, ref, wind, with_x0):
    x0, xref, uref, w, U, X = _case12(B, N, ref, wind)
    if with_x0:
        x0 = x0 + 0.01   # so |x_0 - x0| is not already in the noise of X
    m = _mpc12(N, B)
    r = eval_ref(X, U, xref, uref, _spec12(N), x0=x0 if with_x0 else None, wind=w)
    assert r['res_eq'].min() > 1e-3 and r['res_stat'].min() > 0.1   # not zeros
    kw = dict(x0=x0 if with_x0 else None, wind=w)
    _check64(_np(m.evaluate(X, U, xref, uref, **kw)), r, N, f'12/4 B={B} N={N} {ref}')
    _check64(_np(m.evaluate(X, U, xref, uref, stat=False, **kw)), r, N, f'12/4 B={B} N={N} {ref} nostat', stat=False)


def test_eval12_input_box():
    B, N = 7, 20
    x0, xref, uref, w, U, X = _case12(B, N, 'sine', False)
    spec = _spec12(N, box=True)
    rng = np.random.default_rng(3)
    U = np.clip(uref + 30.0 * rng.standard_normal(U.shape), spec.lbu, spec.ubu)   # many components on a bound
    assert ((U == 0.0) | (U == 65.0)).mean() > 0.2
    X = rollout_any(x0, U, spec) + 0.02 * rng.standard_normal(X.shape)
    m = _mpc12(N, B, box=True)
    r = eval_ref(X, U, xref, uref, spec, x0=x0)
    assert np.all(r['res_ineq'] == 0.0)
    assert (r['nat'] == 0.0).sum() > 0           # components held by the box
    _check64(_np(m.evaluate(X, U, xref, uref, x0=x0)), r, N, '12/4 box projected')
    U2 = U.copy()
    U2[1, 3, 0] = -1e-3
    U2[4, 17, 2] = 65.0 + 1e-3
    U2[4, 2, 1] = 65.0 + 5e-4
    r2 = eval_ref(X, U2, xref, uref, spec, x0=x0)
    got = _np(m.evaluate(X, U2, xref, uref, x0=x0))
    assert np.allclose(got['res_ineq'][[1, 4]], 1e-3, rtol=0, atol=1e-12) and np.all(got['res_ineq'][[0, 2, 3, 5, 6]] == 0.0)
    _check64(got, r2, N, '12/4 box pushed outside')
    _check64(_np(m.evaluate(X, U2, xref, uref, x0=x0, stat=False)), r2, N, '12/4 box nostat', stat=False)


# ------------------------------------------------------------------------------ 17/6 fp64
def test_eval17_fp64_stage_params_input_box():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    x0, xref, uref, p, U, X = _case17()
    B, N = U.shape[:2]
    spec = FullSpec(N=N, lbu=LBU17, ubu=UBU17)
    m = BatchedMPC(MPCConfig.full(N=N, lbu=LBU17, ubu=UBU17), max_batch=B)
    m.set_params(p)
    r = eval_ref(X, U, xref, uref, spec, x0=x0, p25=p)
    assert r['res_ineq'].min() > 0.1 and r['res_eq'].min() > 1e-3
    _check64(_np(m.evaluate(X, U, xref, uref, x0=x0)), r, N, '17/6 box_u')
    _check64(_np(m.evaluate(X, U, xref, uref, stat=False)), eval_ref(X, U, xref, uref, spec, p25=p, stat=False), N,
             '17/6 box_u nostat', stat=False)
    # without the box (another handle): |g| itself
    m2 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    m2.set_params(p)
    _check64(_np(m2.evaluate(X, U, xref, uref, x0=x0)), eval_ref(X, U, xref, uref, FullSpec(N=N), x0=x0, p25=p), N, '17/6')


def test_eval17_state_box():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    from mpc_blaster_amd._lib import MpcbError
    x0, xref, uref, p, U, X = _case17()
    B, N = U.shape[:2]
    X = X.copy()
    X[:, 0, 0] = 50.0                     # stages 0 and N are not boxed
    X[:, N, 1] = -50.0
    X[3, 2, 7] = SB_HI[7] + 0.25          # a state pushed outside ubx on stage 2
    U = np.clip(U, LBU17, UBU17)
    spec = FullSpec(N=N, lbu=LBU17, ubu=UBU17, lbx=SB_LO, ubx=SB_HI)
    m = BatchedMPC(MPCConfig.full(N=N, lbu=LBU17, ubu=UBU17, lbx=SB_LO, ubx=SB_HI), max_batch=B)
    m.set_params(p)
    r = eval_ref(X, U, xref, uref, spec, x0=x0, p25=p, stat=False)
    assert r['res_ineq'].max() < 40.0 and r['res_ineq'][3] >= 0.25
    _check64(_np(m.evaluate(X, U, xref, uref, x0=x0, stat=False)), r, N, '17/6 box_x', stat=False)
    with pytest.raises(MpcbError, match='unsupported'):
        m.evaluate(X, U, xref, uref, x0=x0)


# ------------------------------------------------------------------------------ fp32
def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def _metric(a, ref):
    """per output: cost and res_stat relative to max(1, ref), res_eq and res_ineq absolute"""
    return dict(cost=np.abs(a['cost'] - ref['cost']) / np.maximum(1.0, np.abs(ref['cost'])),
                res_eq=np.abs(a['res_eq'] - ref['res_eq']), res_ineq=np.abs(a['res_ineq'] - ref['res_ineq']),
                res_stat=np.abs(a['res_stat'] - ref['res_stat']) / np.maximum(1.0, ref['res_stat']))


def _check32(m, spec, x0, X, U, xref, uref, p25, tag):
    x0, X, U, xref, uref, p25 = (_f32(a) for a in (x0, X, U, xref, uref, p25))
    # the handle holds its weights, cost scale and boxes in fp32: the reference reads the same values
    spec.Q, spec.R, spec.QN, spec.cost_scale = _f32(spec.Q), _f32(spec.R), _f32(spec.QN), float(np.float32(spec.s))
    if spec.lbu is not None:
        spec.lbu, spec.ubu = _f32(spec.lbu), _f32(spec.ubu)
    ref = eval_ref(X, U, xref, uref, spec, x0=x0, p25=p25)
    rng = np.random.default_rng(0)
    allow = {k: 0.0 for k in KEYS}
    for _ in range(4):
        pert = [a * (1.0 + 2.0 ** -22 * rng.standard_normal(a.shape)) for a in (x0, X, U, xref, uref)]
        mv = _metric(eval_ref(pert[1], pert[2], pert[3], pert[4], spec, x0=pert[0], p25=p25), ref)
        allow = {k: max(allow[k], 8.0 * mv[k].max()) for k in KEYS}
    err = {k: v.max() for k, v in _metric(_np(m.evaluate(X, U, xref, uref, x0=x0)), ref).items()}
    print(f'{tag} fp32: ' + '  '.join(f'{k} err {err[k]:.2e} allow {allow[k]:.2e}' for k in KEYS))
    for k in KEYS:
        assert err[k] <= allow[k], (tag, k, err[k], allow[k])
    ns = _np(m.evaluate(X, U, xref, uref, x0=x0, stat=False))
    for k in KEYS[:3]:
        assert _metric(dict(ns, res_stat=ref['res_stat']), ref)[k].max() <= allow[k], (tag, 'nostat', k)


def test_eval12_fp32():
    B, N = 7, 20
    x0, xref, uref, w, U, X = _case12(B, N, 'sine', False)
    _check32(_mpc12(N, B, 'f32'), _spec12(N), x0, X, U, xref, uref, None, '12/4 B=7 N=20')


def test_eval17_fp32():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    x0, xref, uref, p, U, X = _case17()
    B, N = U.shape[:2]
    m = BatchedMPC(MPCConfig.full(N=N, dtype='f32', lbu=LBU17, ubu=UBU17), max_batch=B)
    m.set_params(p)
    spec = FullSpec(N=N, lbu=LBU17, ubu=UBU17)
    _check32(m, spec, x0, X, U, xref, uref, p, '17/6 B=5 N=4')


# ------------------------------------------------------------------------------ NaN isolation
@pytest.mark.parametrize('stat', [True, False])
def test_nan_instance_is_isolated(stat):
    B, N = 7, 20
    x0, xref, uref, w, U, X = _case12(B, N, 'sine', True)
    m = _mpc12(N, B)
    ok = _np(m.evaluate(X, U, xref, uref, x0=x0, wind=w, stat=stat))
    Xn = X.copy()
    Xn[2, 9, 4] = np.nan
    got = _np(m.evaluate(Xn, U, xref, uref, x0=x0, wind=w, stat=stat))
    rest = [0, 1, 3, 4, 5, 6]
    for k in ok:
        assert np.isnan(got[k][2]), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k     # bit for bit
    assert set(ok) == set(KEYS if stat else KEYS[:3])


# ------------------------------------------------------------------------------ facade
@pytest.mark.parametrize('batch', [1, 3])
def test_facade_cost_and_residuals(batch):
    from mpc_blaster_amd import MPCConfig
    from mpc_blaster_amd.compat.acados import AcadosOcpSolver
    N = 5
    ocp = AcadosOcpSolver(MPCConfig(N=N), batch=batch)
    x0, xref, _, _, _, _ = _case12(batch, N, 'sine', False)
    uref = np.full((batch, N, 4), 22.0725)
    x0v = x0[0] if batch == 1 else x0
    ocp.set(0, 'lbx', x0v)
    ocp.set(0, 'ubx', x0v)
    for k in range(N + 1):
        y = np.concatenate([xref[:, k], uref[:, k]], axis=1) if k < N else xref[:, k]
        ocp.cost_set(k, 'yref', y[0] if batch == 1 else y)
    assert ocp.solve() == 0
    X = np.stack([np.atleast_2d(ocp.get(k, 'x')) for k in range(N + 1)], axis=1)
    U = np.stack([np.atleast_2d(ocp.get(k, 'u')) for k in range(N)], axis=1)
    spec = _spec12(N)
    c_ref = stage_cost(X, U, xref, uref, spec)
    c = np.atleast_1d(ocp.get_cost())
    print('facade get_cost rel err', (np.abs(c - c_ref) / np.maximum(1.0, np.abs(c_ref))).max())
    assert np.all(np.abs(c - c_ref) <= 1e-12 * np.maximum(1.0, np.abs(c_ref)))
    assert isinstance(ocp.get_cost(), float) == (batch == 1)
    res = ocp.get_residuals()
    assert res.shape == ((4,) if batch == 1 else (batch, 4))
    res = np.atleast_2d(res)
    assert np.all(np.isnan(res[:, 3]))
    r = eval_ref(X, U, xref, uref, spec, x0=x0)
    _check64(dict(cost=c, res_stat=res[:, 0], res_eq=res[:, 1], res_ineq=res[:, 2]), r, N, f'facade batch {batch}')


# ------------------------------------------------------------------------------ closed loop
def test_closed_loop_diagnostics():
    from mpc_blaster_amd.closed_loop import closed_loop
    B, N, nsim = 4, 5, 3
    x0, xref, uref, w, _, _ = _case12(B, N, 'sine', True)
    m = _mpc12(N, B)
    Xs, Us, st = closed_loop(m, x0, xref, uref, nsim, wind=w)
    Xd, Ud, sd, diag = closed_loop(m, x0, xref, uref, nsim, wind=w, diagnostics=True)
    torch.cuda.synchronize()
    assert torch.equal(Xs, Xd) and torch.equal(Us, Ud) and torch.equal(st, sd)   # bit-identical
    assert set(diag) == {'cost', 'res_eq', 'res_stat'} and all(v.shape == (B, nsim) for v in diag.values())
    # the same loop by hand: solve_iterate + sim_step, the reference on each new iterate
    x = torch.as_tensor(x0, device=Xs.device)
    xb = torch.zeros((B, N + 1, 12), dtype=torch.float64, device=Xs.device)
    ub = torch.zeros((B, N, 4), dtype=torch.float64, device=Xs.device)
    spec = _spec12(N)
    for i in range(nsim):
        u0 = m.solve_iterate(x, xb, ub, xref, uref, wind=w)
        xb, ub = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
        r = eval_ref(xb.cpu().numpy(), ub.cpu().numpy(), xref, uref, spec, x0=x.cpu().numpy(), wind=w)
        got = {k: v[:, i].cpu().numpy() for k, v in diag.items()}
        _check64(dict(got, res_ineq=r['res_ineq']), r, N, f'closed loop step {i}')
        x = m.sim_step(x, u0.clone(), wind=w)


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B = 3, 2
    m = _mpc12(N, B)
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    X, U, xr, ur, o = d(B, N + 1, 12), d(B, N, 4), d(1, N + 1, 12), d(1, N, 4), d(B)
    P, null = m._ptr, ctypes.c_void_p(0)

    def call(h, Bq, X, U, xr, ur, wind, outs):
        return h.lib.mpcb_eval(h._h, Bq, null, 0, P(X), P(U), P(xr), 0, P(ur), 0, wind, 0, *outs, null)

    assert call(m, B, X, U, xr, ur, null, [null] * 4) == -1                 # MPCB_E_INVALID: no output
    assert call(m, B + 1, X, U, xr, ur, null, [P(o), null, null, null]) == -1   # B > max_batch
    assert call(m, B, X, U, xr, ur, null, [null, null, P(o), null]) == 0    # any single output is enough
    m17 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    X17, U17, xr17, ur17 = d(B, N + 1, 17), d(B, N, 6), d(1, N + 1, 17), d(1, N, 6)
    assert call(m17, B, X17, U17, xr17, ur17, P(d(B, 3)), [P(o), null, null, null]) == -4   # MPCB_E_UNSUPPORTED
    assert b'wind' in m17.lib.mpcb_last_error()
    torch.cuda.synchronize()
