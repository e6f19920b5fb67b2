"""12/4 parity over the full heading circle and flying tilt, on every kernel path and entry point.

The rest of the GPU suite flies almost level and pointing north (roll, pitch within +-0.17 rad, yaw
within +-0.35 rad), where the quadrant logic of the hand-written sin/cos, the angle addition of the
row rollout, the lane-quad rollout's own angle carry and the sin / tan terms of the tangent and
adjoint consumers are never compared with anything.  Here the draw groups of
tests/attitude_case.py (H heading over the whole circle; T heading and 0.6 .. 1.0 rad of roll and
pitch; I any attitude with |cos(theta)| >= 0.3) run under the DEFAULT problem definition (the
production ``DJ = true`` template variants, which tests/test_gpu_config.py's ALT does not run):

 * every row of test_gpu_config.PATHS on H and T (the box rows on H only: a tilted vehicle puts
   80 - 89 % of the box on its bounds and makes 20 - 60 % of the instances fp32-ill-conditioned),
   with the acceptance of that file, unchanged;
 * linearize, sim_step, sim_step(model=), sim_step_vjp and evaluate on H, T and I;
 * solve_iterate_vjp (plain, with weight gradients, with per-instance weights; unboxed and boxed),
   solve_iterate_gains (masked; with vehicles), solve_iterate with per-instance weights and with
   per-instance vehicles on H and T (boxed: H),
each against the reference module and at the bound of the entry point's existing test.
tests/test_attitude_case_cpu.py holds the draws to their claims and the references to central
differences on the oracle alone.  Each case prints its measured maxima (DESIGN.md records them).
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attitude_case as at   # noqa: E402
import simvjp_ref as sr   # noqa: E402
from eval_ref import eval_ref   # noqa: E402
from gains_ref import gains_ref   # noqa: E402
from pm_ref import pm_gains_ref, pm_sim_ref, pm_solve_ref   # noqa: E402
from pw_ref import pw_solve_ref   # noqa: E402
from vjp_ref import vjp_ref   # noqa: E402
from vjp_weights_ref import vjp_weights_ref   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402
from oracle.rk4 import rk4_sens, rk4_step   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import test_gpu_config as gc   # noqa: E402
import test_gpu_gains as gg   # noqa: E402
import test_gpu_pm as gp   # noqa: E402
import test_gpu_pw as gpw   # noqa: E402
import test_gpu_simvjp as gs   # noqa: E402
import test_gpu_vjp as gv   # noqa: E402
import test_gpu_vjp_weights as gw   # noqa: E402
from test_gpu_vjp import BOUND, LB, UB, _f32, _mpc, _spec32, _synthetic_U, relerr   # noqa: E402

B12, BQ, NQ = gc.B12, 8, 130      # solve paths; the lane-quad path
BE, NE = 13, 8                    # every other entry point
MODES = gc.MODES
DT = ('f64', 'f32')

# path -> the kernels a solve launches under the default definition (diagonal inertia), by dtype
# letter and mode; from mpcb_plan_kernels, which each case is also held to
T = gc.T
KERNELS = {
    'fused': lambda t, it: {'riccati': f'mpcb::row_riccati_kernel<{it}, true>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'},
    'two': lambda t, it: {'nominal': f'mpcb::nominal_row_kernel<double, {it}, true, true>',
                          'riccati': f'mpcb::riccati_kernel_f64<true, {it}, true>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'},
    'notan': lambda t, it: {'nominal': f'mpcb::nominal_row_kernel<double, {it}, true, false>',
                            'riccati': f'mpcb::riccati_kernel_f64<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<double, {it}>'},
    'row32': lambda t, it: {'nominal': f'mpcb::nominal_row_kernel<float, {it}, true, false>',
                            'riccati': f'mpcb::riccati_kernel_f32<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<float, {it}>'},
    'small': lambda t, it: {'nominal': f'mpcb::nominal_row_kernel<{T[t]}, {it}, true, false>',
                            'riccati': f'mpcb::box_kernel_{t}<0>', 'linearise': f'mpcb::lin_kernel<{T[t]}>'},
    'single': lambda t, it: {'riccati': f'mpcb::solve_kernel<{T[t]}, 0>'},
    'thread': lambda t, it: {'nominal': f'mpcb::nominal_kernel<{T[t]}, {it}>',
                             'riccati': f'mpcb::riccati_kernel_{t}<{"true" if t == "f64" else "false"}, {it}, false>',
                             'forward': f'mpcb::forward_kernel<{T[t]}, false, {it}>'},
    'lanequad': lambda t, it: {'nominal': f'mpcb::nominal_quad_kernel<{T[t]}, {it}>',
                               'riccati': f'mpcb::riccati_kernel_{t}<true, {it}, false>', 'forward': f'mpcb::fwd_rm_kernel<{T[t]}, {it}>'},
    'box': lambda t, it: dict(
        {'riccati': f'mpcb::row_riccati_kernel<{it}, true>'} if t == 'f64' else
        {'nominal': f'mpcb::nominal_row_kernel<float, {it}, true, false>', 'riccati': f'mpcb::riccati_kernel_f32<true, {it}, false>'},
        forward=f'mpcb::as_kernel_{t}<true, {it}>'),
    'box_ipm': lambda t, it: {'riccati': f'mpcb::row_riccati_kernel<{it}, true>', 'forward': f'mpcb::as_kernel_f64<true, {it}>'},
    'box_v1': lambda t, it: {'riccati': 'mpcb::solve_kernel<double, 1>'},
}


# ------------------------------------------------------------------------------ solve paths
def _solve(path, group, N, B, mode, dtype, monkeypatch, boxed=False, max_as_iter=200):
    """(oracle, spec, inputs, u0, X, U, status) of one solve on ``path``; the kernels are checked."""
    o, spec = at.solve_oracle(group, N, B, mode, dtype, boxed, max_as_iter)
    inp = at.solve_inputs(group, N, B, dtype)
    m = gc._handle(path, N, B, dtype, monkeypatch, max_as_iter=max_as_iter, **at.config(boxed, dtype))
    wind = inp['wind'] if at.use_wind(mode, group) else None
    if mode == 'iterate':
        m.solve_iterate(inp['x0'], inp['xbar'], inp['ubar'], inp['xref'], inp['uref'], wind=wind)
    else:
        m.solve(inp['x0'], inp['xref'], inp['uref'], wind=wind)
    torch.cuda.synchronize()
    gc._kernels_are(m, B, mode, KERNELS[path](dtype, gc._it(mode)))
    out = [t.cpu().numpy().copy() for t in (m.get_control(), m.get_state_trajectory(), m.get_input_trajectory(),
                                             m.get_status())]
    return (o, spec, inp) + tuple(out)


def _check_free(path, group, N, B, mode, dtype, monkeypatch):
    o, spec, inp, u0, X, U, st = _solve(path, group, N, B, mode, dtype, monkeypatch)
    gc._accept_free(f'{group} {path} {dtype} N={N} {mode}', o, u0, X, U, st, dtype)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('group', ['H', 'T'])
@pytest.mark.parametrize('path,dtype', [
    ('fused', 'f64'), ('two', 'f64'), ('notan', 'f64'), ('row32', 'f32'), ('small', 'f64'), ('small', 'f32'),
    ('single', 'f64'), ('single', 'f32'), ('thread', 'f64'), ('thread', 'f32')])
def test_unconstrained_path_matches_oracle(path, dtype, group, mode, monkeypatch):
    _check_free(path, group, 6, B12, mode, dtype, monkeypatch)


@pytest.mark.parametrize('group,mode', [('H', 'rollout'), ('H', 'iterate'), ('T', 'iterate')])
def test_lane_quad_rollout_matches_oracle_fp64(group, mode, monkeypatch):
    """N = 130: the lane-quad rollout and its own angle carry.  T in iterate mode only: a 4.3 s
    open-loop rollout of a tilted vehicle is a conditioning test, not an attitude test."""
    _check_free('lanequad', group, NQ, BQ, mode, 'f64', monkeypatch)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('path,dtype', [('box', 'f64'), ('box', 'f32'), ('box_ipm', 'f64'), ('box_v1', 'f64')])
def test_input_box_path_matches_oracle(path, dtype, mode, monkeypatch):
    """The box [0, 65] on H, with the box acceptance of tests/test_gpu_config.py."""
    cap = 1 if path == 'box_ipm' else 200
    o, spec, inp, u0, X, U, st = _solve(path, 'H', 6, B12, mode, dtype, monkeypatch, True, cap)
    frac = gc._on_bound(o['U'], spec.lbu, spec.ubu).mean()
    print(f'H {path} {dtype} {mode}: oracle has {100 * frac:.0f} % of U on a bound, '
          f'{int(o["fallback"].sum())} instances through the interior point')
    assert frac >= 0.10
    gc._accept_box(f'H {path} {dtype} N=6 {mode}', o, spec, inp, u0, X, U, st, dtype)


# ------------------------------------------------------------------------------ dynamics calls
def _noise52(fn, args):
    """The largest move of each output of the reference ``fn(*args)`` under a relative 2^-52
    perturbation of its array arguments (printed next to the fp64 errors of group I)."""
    ref = fn(*args)
    rng = np.random.default_rng(0)
    out = fn(*[a * (1.0 + 2.0 ** -52 * rng.choice([-1.0, 1.0], size=a.shape)) for a in args])
    return [np.abs(a - b).max() for a, b in zip(out, ref)]


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', at.GROUPS)
def test_linearize_and_sim_step(group, dtype):
    """mpcb_linearize against rk4_sens and mpcb_sim_step (wind, T != dt) against rk4_step, at the
    bounds of tests/test_gpu_config.py test_linearize_and_sim_step_under_alt: fp64 1e-12, fp32 by
    its ``_moved`` rule."""
    c = gc._cast(dtype)
    spec = OcpSpec(N=NE)
    Xb, Ub, w = (c(a) for a in at.lin_case(group, BE, NE))
    s = at.step_case(group, BE)
    xs, us, ws = c(s['x']), c(s['u']), c(s['wind'])
    m = _mpc(NE, BE, dtype)
    got = [t.cpu().numpy().astype(np.float64) for t in m.linearize(Xb, Ub, wind=w)]   # A, B, x_next

    def lin(xb, ub, w):
        r = [rk4_sens(xb[:, k], ub[:, k], spec.dt, spec.params, w) for k in range(NE)]
        return [np.stack([q[i] for q in r], axis=1) for i in (1, 2, 0)]

    Tstep = float(np.float32(0.013)) if dtype == 'f32' else 0.013
    got.append(m.sim_step(xs, us, T=Tstep, wind=ws).cpu().numpy().astype(np.float64))

    def sim(x, u, w):
        return [rk4_step(x, u, Tstep, spec.params, w)]

    if dtype == 'f64':
        ref, allow = lin(Xb, Ub, w) + sim(xs, us, ws), [1e-12] * 4
        move = _noise52(lin, (Xb, Ub, w)) + _noise52(sim, (xs, us, ws))
        print(f'{group} f64: the reference\'s own move under 2^-52 noise ' + '  '.join(f'{v:.2e}' for v in move))
    else:
        (ref, allow), (ref2, allow2) = gc._moved(lin, (Xb, Ub, w)), gc._moved(sim, (xs, us, ws))
        ref, allow = ref + ref2, allow + allow2
    err = [np.abs(a - b).max() for a, b in zip(got, ref)]
    print(f'{group} {dtype}: ' + '  '.join(f'{n} err {e:.2e} allow {a:.2e}'
                                           for n, e, a in zip(('A', 'B', 'x_next', 'sim_step'), err, allow)))
    for e, a in zip(err, allow):
        assert e <= a


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', at.GROUPS)
def test_sim_step_with_vehicles(group, dtype):
    """mpcb_sim_step_pm against pm_sim_ref at the bounds of tests/test_gpu_pm.py
    test_sim_step_pm_matches_reference: fp64 1e-12 absolute, fp32 max(5e-5, 10 x move)."""
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    s = at.step_case(group, BE)
    x, u, M, w = cast(s['x']), cast(s['u']), cast(s['M']), cast(s['wind'])
    spec = OcpSpec(N=3)
    m = _mpc(3, BE, dtype)
    ref = pm_sim_ref(x, u, spec.dt, spec, M, w)
    got = m.sim_step(x, u, wind=w, model=M).cpu().numpy().astype(np.float64)
    if dtype == 'f64':
        e = np.abs(got - ref).max()
        print(f'{group} sim_step_pm fp64: |dev - ref| {e:.2e}/{gp.SIM_BOUND:.0e}')
        assert e < gp.SIM_BOUND
    else:
        rng = np.random.default_rng(0)
        moved = pm_sim_ref(gp._pert(rng, x), gp._pert(rng, u), spec.dt, spec, gp._pert(rng, M), gp._pert(rng, w))
        move = relerr(moved, ref).max()
        bound = max(BOUND['f32'], 10.0 * move)
        e = relerr(got, ref).max()
        print(f'{group} sim_step_pm fp32: move {move:.2e} -> bound {bound:.2e}, error {e:.2e}')
        assert e <= bound


@functools.lru_cache(maxsize=None)
def _simvjp_ref(group, dtype):
    """(reference, per-output bound) by the rule of tests/test_gpu_simvjp.py ``_ref``."""
    c = dict(at.step_case(group, BE))
    c = {k: c[k] for k in ('x', 'u', 'g', 'M', 'wind')}
    if dtype == 'f32':
        c = {k: _f32(v) for k, v in c.items()}
    ref = sr.simvjp_ref(c['x'], c['u'], c['g'], gs.T, gs.SPEC, c['M'], c['wind'])
    bound = {k: BOUND['f64'] for k in gs.KEYS}
    if dtype == 'f32':
        rng = np.random.default_rng(0)
        p = {k: gs._pert(rng, v) for k, v in c.items()}
        moved = sr.simvjp_ref(p['x'], p['u'], p['g'], gs.T, gs.SPEC, p['M'], p['wind'])
        move = {k: relerr(moved[k], ref[k]).max() for k in gs.KEYS}
        bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in gs.KEYS}
        print(f'{group} fp32 reference move: ' + '  '.join(f'{k} {move[k]:.2e}' for k in gs.KEYS))
    return c, ref, bound


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', at.GROUPS)
def test_sim_step_vjp_all_outputs(group, dtype):
    """mpcb_sim_step_vjp with per-instance records and wind, all four outputs, against simvjp_ref."""
    c, ref, bound = _simvjp_ref(group, dtype)
    m = _mpc(3, BE, dtype)
    got = gs._np(m.sim_step_vjp(c['x'], c['u'], c['g'], wind=c['wind'], model=c['M'], want=gs.KEYS))
    gs._check(got, ref, bound, BE, f'{group} sim_step_vjp {dtype}')


@pytest.mark.parametrize('boxed', [False, True])
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', at.GROUPS)
def test_evaluate(group, dtype, boxed):
    """mpcb_eval with wind, with and without the box [0, 65], by tests/test_gpu_config.py
    ``_check_eval`` (fp64: the bounds of tests/test_gpu_eval.py; fp32: its move rule).  Boxed: U =
    clip(uref + 30 N(0, 1)) with three components pushed outside, as test_eval12_input_box."""
    c = gc._cast(dtype)
    x0, xref, uref, w, U, X = at.eval_case(group, BE, NE, True)
    spec = OcpSpec(N=NE, **at.config(boxed, dtype))
    if boxed:
        U = np.clip(uref + 30.0 * np.random.default_rng(3).standard_normal(U.shape), 0.0, 65.0)
        assert ((U == 0.0) | (U == 65.0)).mean() > 0.2
        U[1, 3, 0], U[4, 7, 2], U[4, 2, 1] = -1e-3, 65.0 + 1e-3, 65.0 + 5e-4
    x0, xref, uref, w, U, X = (c(a) for a in (x0, xref, uref, w, U, X))
    m = _mpc(NE, BE, dtype, **at.config(boxed, dtype))
    gc._check_eval(m, spec, dtype, x0, X, U, xref, np.broadcast_to(uref, U.shape).copy(), w, None,
                   f'{group} evaluate {"box" if boxed else "free"}')


# ------------------------------------------------------------------------------ products
def _pcase(group, dtype, ref='hover', wind=True):
    c = at.product_case(group, BE, NE, ref, wind)
    return {k: _f32(v) for k, v in c.items()} if dtype == 'f32' else dict(c)


def _pspec(dtype, box):
    spec = OcpSpec(N=NE, lbu=LB if box else None, ubu=UB if box else None)
    return _spec32(spec) if dtype == 'f32' else spec


def _pmpc(dtype, box):
    return _mpc(NE, BE, dtype, **(dict(lbu=LB, ubu=UB) if box else {}))


@pytest.mark.parametrize('box', [False, True])
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', ['H', 'T'])
def test_vjp_plain(group, dtype, box):
    """mpcb_solve_vjp against vjp_ref, unboxed and with the synthetic active set of tests/test_gpu_vjp.py."""
    c, spec = _pcase(group, dtype), _pspec(dtype, box)
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    U = cast(_synthetic_U(c, spec)) if box else None
    ref = vjp_ref(c['xbar'], c['ubar'], U, c['gX'], c['gU'], spec, c['wind'])
    got = gv._np(_pmpc(dtype, box).solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, wind=c['wind']))
    gv._check(got, ref, dtype, f'{group} vjp {dtype} box={box}')
    if box:
        assert ref['fixed'].mean() > 0.2 and np.all(got['guref'][ref['fixed']] == 0.0)


@pytest.mark.parametrize('box', [False, True])
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', ['H', 'T'])
def test_vjp_with_weight_gradients(group, dtype, box):
    """mpcb_solve_vjp_w against vjp_weights_ref (sine references with per-instance strides); fp32 by
    the move rule of tests/test_gpu_vjp_weights.py ``_fp32_bound``."""
    c, spec = _pcase(group, dtype, 'sine'), _pspec(dtype, box)
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    if box:
        U, X = cast(_synthetic_U(c, spec)), cast(gw._synthetic_X(c))
        fixed = (U <= spec.lbu) | (U >= spec.ubu)
    else:
        o = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
        U, X, fixed = cast(o['U']), cast(o['X']), None
    args = (c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'])
    if dtype == 'f32':
        r, bound = gw._fp32_bound(args, spec, c['wind'], fixed)
    else:
        r, bound = vjp_weights_ref(*args, spec, c['wind']), None
    got = gw._run(_pmpc(dtype, box), c, X, U, c['xref'], c['uref'], c['wind'])
    gw._check(got, r, dtype, f'{group} vjp weights {dtype} box={box}', bound)


@pytest.mark.parametrize('box', [False, True])
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', ['H', 'T'])
def test_vjp_per_instance_weights(group, dtype, box):
    """mpcb_solve_vjp_pw against pw_vjp_ref; fp32 by the move rule of tests/test_gpu_pw.py test_vjp_pw_fp32."""
    c, spec = _pcase(group, dtype, 'sine'), _pspec(dtype, box)
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    if box:
        U = cast(_synthetic_U(c, spec))
        X = cast(c['xbar'] + 0.05 * np.random.default_rng(5).standard_normal(c['xbar'].shape))
        fixed = (U <= spec.lbu) | (U >= spec.ubu)
    else:
        o = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'], c['wind'])
        X, U, fixed = cast(o['X']), cast(o['U']), None
    r = gpw._vjp_ref(c, X, U, spec)
    bound = None
    if dtype == 'f32':
        rng = np.random.default_rng(0)
        q = {k: gpw._pert(rng, v) for k, v in c.items()}
        Up = gpw._pert(rng, U)
        if fixed is not None:
            Up = np.where(fixed, U, Up)   # a clamped component stays on its bound
        moved = gpw._vjp_ref(q, gpw._pert(rng, X), Up, spec)
        assert np.array_equal(moved['fixed'], r['fixed'])
        move = {k: relerr(moved[k], r[k]).max() for k in gpw.GKEYS}
        bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in gpw.GKEYS}
        print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in gpw.GKEYS))
    gpw._vjp_check(gpw._vjp(_pmpc(dtype, box), c, X, U), r, dtype, f'{group} vjp pw {dtype} box={box}', bound)


# ------------------------------------------------------------------------------ gains
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('group', ['H', 'T'])
def test_gains_masked_and_with_vehicles(group, dtype):
    """mpcb_solve_gains with a ``fixed`` mask against gains_ref, and mpcb_solve_gains_pm against
    pm_gains_ref, at the bounds of tests/test_gpu_gains.py and tests/test_gpu_pm.py."""
    c = _pcase(group, dtype)
    spec = _pspec(dtype, False)
    fixed = gp._mask(BE, NE)
    m = _mpc(NE, BE, dtype)
    got = gg._run12(m, c, fixed=fixed)
    gg._check(got, gains_ref(c['xbar'], c['ubar'], fixed, spec, c['wind']), dtype, 12, f'{group} gains {dtype} masked')
    gg._properties(got, fixed, f'{group} gains {dtype}')
    for fx in (None, fixed):
        ref = pm_gains_ref(c['xbar'], c['ubar'], fx, spec, c['M'], c['wind'])
        assert ref['ok'].all()
        gp._check(gp._gains(m, c, fixed=fx), ref, dtype, f'{group} gains pm {dtype} masked={fx is not None}', keys=gp.GKEYS)


# ------------------------------------------------------------------------------ per-instance solves
def _moved_bound(fn, args, keys):
    """max(5e-5, 10 x move) per output: the fp32 rule of tests/test_gpu_pw.py and tests/test_gpu_pm.py."""
    r = fn(*args)
    rng = np.random.default_rng(0)
    moved = fn(*[gpw._pert(rng, a) for a in args])
    move = {k: relerr(moved[k], r[k]).max() for k in keys}
    bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in keys}
    print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in keys))
    return r, bound


@pytest.mark.parametrize('group,dtype,box', [('H', 'f64', False), ('H', 'f32', False), ('T', 'f64', False),
                                             ('T', 'f32', False), ('H', 'f64', True)])
def test_solve_iterate_per_instance_weights(group, dtype, box):
    """mpcb_solve_iterate_pw against pw_solve_ref.  Boxed: the hover draw without wind, as the
    existing box test; the entry point's active set has no hand-over to the interior point, so the
    reference must not have needed one."""
    c, spec = (_pcase(group, dtype, 'hover', False) if box else _pcase(group, dtype, 'sine')), _pspec(dtype, box)
    names = ('x0', 'xref', 'uref', 'xbar', 'ubar', 'Q', 'R', 'QN', 'wind')
    fn = lambda *a: pw_solve_ref(*a[:5], spec, *a[5:])   # noqa: E731
    args = [c[k] for k in names]
    r, bound = _moved_bound(fn, args, gpw.SKEYS) if dtype == 'f32' else (fn(*args), None)
    got = gpw._solve(_pmpc(dtype, box), c)
    gpw._check(got, r, dtype, f'{group} pw solve {dtype} box={box}', bound=bound)
    if box:
        assert not r['fallback'].any()
        on = (r['U'] <= LB + 1e-9) | (r['U'] >= UB - 1e-9)
        print(f'  clamped components per instance {on.sum(axis=(1, 2)).tolist()}')
        assert on.any(axis=(1, 2)).sum() >= BE // 2
        assert np.array_equal((got['U'] <= LB) | (got['U'] >= UB), on)


@pytest.mark.parametrize('group,dtype,box', [('H', 'f64', False), ('H', 'f32', False), ('T', 'f64', False),
                                             ('T', 'f32', False), ('H', 'f64', True)])
def test_solve_iterate_per_instance_vehicles(group, dtype, box):
    """mpcb_solve_iterate_pm against pm_solve_ref.  Boxed: the hover draw without wind, as
    tests/test_pm_ref_cpu.py box_case."""
    c, spec = (_pcase(group, dtype, 'hover', False) if box else _pcase(group, dtype, 'sine')), _pspec(dtype, box)
    names = ('x0', 'xref', 'uref', 'xbar', 'ubar', 'M', 'wind')
    fn = lambda *a: pm_solve_ref(*a[:5], spec, a[5], wind=a[6])   # noqa: E731
    args = [c[k] for k in names]
    r, bound = _moved_bound(fn, args, gp.SKEYS) if dtype == 'f32' else (fn(*args), None)
    got = gp._solve(_pmpc(dtype, box), c)
    assert np.array_equal(got['status'], r['status'])
    gp._check(got, r, dtype, f'{group} pm solve {dtype} box={box}', bound=bound)
    if box:
        assert not r['fallback'].any()
        on = (r['U'] <= LB + 1e-9) | (r['U'] >= UB - 1e-9)
        print(f'  clamped components per instance {on.sum(axis=(1, 2)).tolist()}')
        assert on.any(axis=(1, 2)).sum() >= BE // 2
        assert np.array_equal((got['U'] <= LB) | (got['U'] >= UB), on)
