"""mpcb_sim_step_pm, mpcb_solve_iterate_pm and mpcb_solve_gains_pm on the GPU (the plant step, the
RTI step and its feedback gains with a vehicle per instance, 12/4 model), the Python keywords over
them and ``closed_loop(model=, plant_model=)``, against tests/pm_ref.py: the device is compared with
the NumPy reference, never with itself.  tests/test_pm_ref_cpu.py ties that reference to the
batched oracle and freezes the box case.

Metric: tests/test_gpu_vjp.py ``relerr``, per instance and output |dev - ref|_inf / max(|ref|_inf, 1).
Bounds: fp64 1e-9 on u0, X, U, K and P0; the fp64 plant step 1e-12 absolute
(tests/test_gpu_parity.py test_sim_step_and_histogram); fp32 5e-5, for the solve and the plant step
by the rule of the fp32 cases of tests/test_gpu_pw.py: the reference's own move under a seeded
relative +-2^-22 perturbation of every input, the records included, is measured and the device is
bounded by max(5e-5, 10 x move); the closed loop 1e-8 (test_closed_loop_with_per_instance_weights);
d u0 / d x0 = K_0 1e-9 (tests/test_gpu_gains.py test_K0_rows_are_the_vjp_of_u0_on_the_device).
Draws: tests/vjp_ref.py vjp_case (seed 1004), vehicles tests/pm_ref.py pm_models (seed 21), weights
tests/pw_ref.py pw_weights (seed 11), box [5, 40].

Shapes: B = 5 is two waves with three padding groups in the second; N = 3 is fewer stages than
lanes, N = 20 gives a lane two stages in pass 1; B = 300 crosses a 256-thread block of the plant step.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
from pm_ref import pack_params, params_of, pm_gains_ref, pm_models, pm_sim_ref, pm_solve_ref   # noqa: E402
from pw_ref import pw_weights   # noqa: E402
from test_pm_ref_cpu import LB, UB, box_case   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.ocp import OcpSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from test_gpu_vjp import BOUND, _f32, _mpc, _spec32, relerr   # noqa: E402

SKEYS = ('u0', 'X', 'U')
GKEYS = ('K', 'P0')
E_INVALID, E_UNSUPPORTED = -1, -4
ST_NAN = 1
SIM_BOUND = 1e-12
SHAPES = [(5, 3), (5, 20)]
TD = {'f64': torch.float64, 'f32': torch.float32}


@functools.lru_cache(maxsize=None)
def _case(B, N, ref='hover', wind=False):
    """vjp_case, the vehicles and the weight draw; never modified."""
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec, ref, wind)
    Q, R, QN = pw_weights(B, spec)
    return dict(c, Q=Q, R=R, QN=QN, M=pm_models(B, spec))


@functools.lru_cache(maxsize=None)
def _sim_case(B=300):
    rng = np.random.default_rng(4)
    return dict(x=rng.uniform(-0.5, 0.5, (B, 12)), u=rng.uniform(0, 65, (B, 4)), wind=rng.uniform(-2, 2, (B, 3)),
                M=pm_models(B, OcpSpec(N=3)))


def _t(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def _solve(m, c, model='M', Q=None, R=None, QN=None):
    """solve_iterate(model=...) with the case's records (a key of c, an array, or None)."""
    md = c[model] if isinstance(model, str) else model
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], wind=c['wind'], model=md, Q=Q, R=R, QN=QN)
    torch.cuda.synchronize()
    return dict(u0=m.get_control().cpu().numpy().astype(np.float64),
                X=m.get_state_trajectory().cpu().numpy().astype(np.float64),
                U=m.get_input_trajectory().cpu().numpy().astype(np.float64),
                status=m.get_status().cpu().numpy())


def _gains(m, c, model='M', **kw):
    md = c[model] if isinstance(model, str) else model
    out = m.solve_iterate_gains(c['xbar'], c['ubar'], wind=c.get('wind'), model=md, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _check(got, ref, dtype, tag, keys=SKEYS, bound=None, status=True):
    if status:
        assert np.all(got['status'] == 0), (tag, got['status'])
    bound = dict({k: BOUND[dtype] for k in keys}, **(bound or {}))
    err = {k: relerr(np.asarray(got[k], dtype=np.float64), ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound[k]:.1e} (|ref| {np.abs(ref[k]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= bound[k], (tag, k, err[k], bound[k])
    return err


def _pert(rng, a):
    return None if a is None else a * (1.0 + 2.0 ** -22 * rng.choice([-1.0, 1.0], size=np.shape(a)))


def _outs(B, N, dtype=torch.float64):
    return dict(u0=torch.full((B, 4), 7.0, dtype=dtype, device='cuda'),
                X=torch.full((B, N + 1, 12), 7.0, dtype=dtype, device='cuda'),
                U=torch.full((B, N, 4), 7.0, dtype=dtype, device='cuda'),
                status=torch.full((B,), -77, dtype=torch.int32, device='cuda'))


def _host(o):
    torch.cuda.synchronize()
    return {k: (v.view if isinstance(v, ab.Guarded) else v).cpu().numpy() for k, v in o.items()}


def _raw_pm(m, B, N, a, o, model, model_sb, W=((None, 0),) * 3, pw=False):
    """mpcb_solve_iterate_pm (or, pw=True, mpcb_solve_iterate_pw) with pointers and strides as given."""
    head = [m._h, B, ab._p(a['x0']), 12, ab._p(a['xbar']), ab._p(a['ubar']), ab._p(a['xref']), (N + 1) * 12,
            ab._p(a['uref']), N * 4, ab._p(a.get('wind')), 3 if a.get('wind') is not None else 0,
            ab._p(W[0][0]), W[0][1], ab._p(W[1][0]), W[1][1], ab._p(W[2][0]), W[2][1]]
    tail = [ab._p(o['u0']), ab._p(o['X']), ab._p(o['U']), ab._p(o['status']), ab._p(0)]
    if pw:
        return m.lib.mpcb_solve_iterate_pw(*head, *tail)
    return m.lib.mpcb_solve_iterate_pm(*head, ab._p(model), model_sb, *tail)


def _raw_gains(m, B, a, o, model=None, model_sb=0, fixed=None, pm=True):
    head = [m._h, B, ab._p(a['xbar']), ab._p(a['ubar']), ab._p(a.get('U')), ab._p(fixed), ab._p(a.get('wind')),
            3 if a.get('wind') is not None else 0]
    tail = [ab._p(o['K']), ab._p(o['P0']), ab._p(o['status']), ab._p(0)]
    if pm:
        return m.lib.mpcb_solve_gains_pm(*head, ab._p(model), model_sb, *tail)
    return m.lib.mpcb_solve_gains(*head, *tail)


def _raw_sim(m, B, x, u, wind, model, model_sb, xo, T=1.0 / 30.0):
    return m.lib.mpcb_sim_step_pm(m._h, B, ab._p(x), ab._p(u), ab._p(wind), 3 if wind is not None else 0,
                                  ab._p(model), model_sb, float(T), ab._p(xo), ab._p(0))


def _gouts(B, N, dtype=torch.float64):
    return dict(K=torch.full((B, N, 4, 12), 7.0, dtype=dtype, device='cuda'),
                P0=torch.full((B, 12, 12), 7.0, dtype=dtype, device='cuda'),
                status=torch.full((B,), -77, dtype=torch.int32, device='cuda'))


def _vehicle_kw(rec):
    """MPCConfig fields of a record: a handle created with that vehicle."""
    return dict(mass=float(rec[0]), lx=float(rec[1]), ly=float(rec[2]), c=float(rec[3]), t_blast=float(rec[4]),
                J=np.asarray(rec[5:14], dtype=np.float64).reshape(3, 3).copy())


# ------------------------------------------------------------------------------ 1. the plant step
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('wind', [False, True])
def test_sim_step_pm_matches_reference(dtype, wind):
    B = 300
    s = _sim_case(B)
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    x, u, M = cast(s['x']), cast(s['u']), cast(s['M'])
    w = cast(s['wind']) if wind else None
    spec = OcpSpec(N=3)
    m = _mpc(3, B, dtype)
    ref = pm_sim_ref(x, u, spec.dt, spec, M, w)
    got = m.sim_step(x, u, wind=w, model=M).cpu().numpy().astype(np.float64)
    plain = m.sim_step(x, u, wind=w).cpu().numpy().astype(np.float64)
    if dtype == 'f64':
        e = np.abs(got - ref).max()
        print(f'sim_step_pm fp64 wind={wind}: |dev - ref| {e:.2e}/{SIM_BOUND:.0e}')
        assert e < SIM_BOUND
    else:
        rng = np.random.default_rng(0)
        moved = pm_sim_ref(_pert(rng, x), _pert(rng, u), spec.dt, spec, _pert(rng, M), _pert(rng, w))
        move = relerr(moved, ref).max()
        bound = max(BOUND['f32'], 10.0 * move)
        e = relerr(got, ref).max()
        print(f'sim_step_pm fp32 wind={wind}: move {move:.2e} -> bound {bound:.2e}, error {e:.2e}')
        assert e <= bound
    # ignoring the record cannot pass: every instance is somewhere else than the handle's vehicle puts it
    d = relerr(got, plain)
    print(f'  against mpcb_sim_step: min over instances {d.min():.3g}')
    assert d.min() > 1e-3
    # a record equal to the handle's config: mpcb_sim_step within the plant step's bound
    own = m.pack_model()
    assert tuple(own.shape) == (1, 14) and own.dtype == TD[dtype]
    same = m.sim_step(x, u, wind=w, model=own).cpu().numpy().astype(np.float64)
    if dtype == 'f64':
        assert np.abs(same - plain).max() < SIM_BOUND
    else:
        assert relerr(same, plain).max() <= BOUND['f32']


# ------------------------------------------------------------------------------ 2. fp64, unconstrained
@pytest.mark.parametrize('B,N', SHAPES)
@pytest.mark.parametrize('how', ['model', 'model+weights'])
def test_pm_fp64_matches_reference(B, N, how):
    c = _case(B, N, 'sine', True)
    spec = OcpSpec(N=N)
    W = {k: c[k] for k in ('Q', 'R', 'QN')} if how == 'model+weights' else {}
    r = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['M'], wind=c['wind'], **W)
    m = _mpc(N, B)
    got = _solve(m, c, **W)
    assert np.array_equal(got['status'], r['status'])
    _check(got, r, 'f64', f'pm fp64 B={B} N={N} {how}')
    # the vehicles matter: the handle's vehicle puts every instance somewhere else
    shared = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, None, wind=c['wind'], **W)
    d = relerr(got['U'], shared['U'])
    print(f'  per-instance against the handle\'s vehicle: min over instances {d.min():.3g}')
    assert d.min() > 1e-3


@pytest.mark.parametrize('B,N', SHAPES)
def test_pm_broadcast_record_is_a_handle_with_that_vehicle(B, N):
    """model_sb = 0: one record for the batch, against mpcb_solve_iterate_pw of a second handle
    created with that vehicle (and against the reference)."""
    c = _case(B, N, 'sine', True)
    rec = c['M'][2]
    a = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'wind')}
    m, m2 = _mpc(N, B), _mpc(N, B, **_vehicle_kw(rec))
    o, o2 = _outs(B, N), _outs(B, N)
    assert _raw_pm(m, B, N, a, o, _t(rec), 0) == 0
    assert _raw_pm(m2, B, N, a, o2, None, 0, pw=True) == 0
    got, other = _host(o), _host(o2)
    assert np.all(got['status'] == 0) and np.all(other['status'] == 0)
    _check(got, other, 'f64', f'pm broadcast record B={B} N={N} against a handle with that vehicle')
    r = pm_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], OcpSpec(N=N), rec[None], wind=c['wind'])
    _check(got, r, 'f64', '  ... and against the reference')
    # pack_model writes the same record
    pk = m.pack_model(mass=rec[0], lx=rec[1], ly=rec[2], c=rec[3], t_blast=rec[4], J=rec[5:].reshape(3, 3))
    assert np.array_equal(pk.cpu().numpy(), rec[None])


# ------------------------------------------------------------------------------ 3. input box, fp64
def test_pm_box_fp64_matches_reference():
    spec, c, M, r = box_case()
    B, N = c['x0'].shape[0], spec.N
    m = _mpc(N, B, lbu=LB, ubu=UB)
    got = _solve(m, dict(c, M=M))
    assert np.array_equal(got['status'], r['status'])
    _check(got, r, 'f64', f'pm box fp64 B={B} N={N}')
    lo, hi = r['U'] <= LB + 1e-9, r['U'] >= UB - 1e-9
    print(f'  clamped components per instance {(lo | hi).sum(axis=(1, 2)).tolist()}')
    # clamped components are the bound's value itself, and nothing else is on a bound
    assert np.array_equal(got['U'][lo], np.broadcast_to(LB, got['U'].shape)[lo])
    assert np.array_equal(got['U'][hi], np.broadcast_to(UB, got['U'].shape)[hi])
    assert np.array_equal((got['U'] <= LB) | (got['U'] >= UB), lo | hi)
    assert np.array_equal(got['u0'], got['U'][:, 0])


# ------------------------------------------------------------------------------ 4. fp32
def test_pm_fp32_unconstrained():
    B, N = 5, 20
    spec = _spec32(OcpSpec(N=N))
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    args = [c[k] for k in ('x0', 'xref', 'uref', 'xbar', 'ubar')]
    r = pm_solve_ref(*args, spec, c['M'])
    rng = np.random.default_rng(0)
    moved = pm_solve_ref(*[_pert(rng, a) for a in args], spec, _pert(rng, c['M']))
    move = {k: relerr(moved[k], r[k]).max() for k in SKEYS}
    bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in SKEYS}
    print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in SKEYS))
    m = _mpc(N, B, 'f32')
    got = _solve(m, c)
    assert got['status'].dtype == np.int32 and m.get_control().dtype == torch.float32
    _check(got, r, 'f32', f'pm fp32 B={B} N={N}', bound=bound)


# ------------------------------------------------------------------------------ 5. bit equality
def test_null_model_and_existing_entry_points_keep_their_bits():
    B, N = 5, 20
    c = _case(B, N, 'hover', True)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    a = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'wind')}
    W = [(_t(c[k]), c[k][0].size) for k in ('Q', 'R', 'QN')]
    U = _t(np.clip(c['ubar'] + 30.0 * np.random.default_rng(3).standard_normal(c['ubar'].shape), LB, UB))
    ag = dict(a, U=U)
    xs, us = _t(_sim_case(B)['x']), _t(_sim_case(B)['u'])

    def old():
        o, g = _outs(B, N), _gouts(B, N)
        assert _raw_pm(m, B, N, a, o, None, 0, W, pw=True) == 0
        assert _raw_gains(m, B, ag, g, pm=False) == 0
        xo = m.sim_step(xs, us, wind=a['wind'])
        torch.cuda.synchronize()
        return dict(o, K=g['K'], P0=g['P0'], gstatus=g['status'], xo=xo)

    before = old()
    # model = NULL: the bits of the calls without _pm
    o, g = _outs(B, N), _gouts(B, N)
    assert _raw_pm(m, B, N, a, o, None, 0, W) == 0
    assert _raw_gains(m, B, ag, g) == 0
    xo = torch.full((B, 12), 7.0, dtype=torch.float64, device='cuda')
    assert _raw_sim(m, B, xs, us, a['wind'], None, 0, xo) == 0
    torch.cuda.synchronize()
    null = dict(o, K=g['K'], P0=g['P0'], gstatus=g['status'], xo=xo)
    for k in before:
        assert ab.same_bits(before[k], null[k]), k
    # pm calls with records on the same handle, then the old calls again
    md = _t(c['M'])
    assert _raw_pm(m, B, N, a, _outs(B, N), md, 14, W) == 0
    assert _raw_gains(m, B, ag, _gouts(B, N), md, 14) == 0
    assert _raw_sim(m, B, xs, us, a['wind'], md, 14, torch.empty_like(xo)) == 0
    after = old()
    for k in before:
        assert ab.same_bits(before[k], after[k]), k
    assert int(before['gstatus'].max()) == 0 and bool(torch.isfinite(before['u0']).all())


# ------------------------------------------------------------------------------ 6. strides and guards
def test_padded_records_element_alignment_and_guard_bands():
    """model_sb = 16 with NaN in the two pad elements of every record, the first record one element
    into the allocation (8-byte, not 16-byte aligned), guard bands around every output."""
    B, N = 5, 3
    f64 = torch.float64
    c = _case(B, N, 'sine', True)
    m = _mpc(N, B)
    a = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'wind')}
    ag = a
    xs, us = _t(_sim_case(B)['x']), _t(_sim_case(B)['u'])
    md = _t(c['M'])
    P = ab.padded(c['M'], 16, 1, f64)
    assert P.ptr % 16 == 8 and bool(torch.isnan(P.buf[1 + 14:1 + 16]).all()) and bool(torch.isnan(P.buf[0]))
    # contiguous calls
    o, g = _outs(B, N), _gouts(B, N)
    xo = torch.full((B, 12), 7.0, dtype=f64, device='cuda')
    assert _raw_pm(m, B, N, a, o, md, 14) == 0 and _raw_gains(m, B, ag, g, md, 14) == 0
    assert _raw_sim(m, B, xs, us, a['wind'], md, 14, xo) == 0
    base = _host(dict(o, K=g['K'], P0=g['P0'], gstatus=g['status'], xo=xo))
    assert np.all(base['status'] == 0) and np.all(base['gstatus'] == 0) and np.isfinite(base['xo']).all()
    # padded records, guarded outputs
    og = dict(u0=ab.guarded((B, 4), f64), X=ab.guarded((B, N + 1, 12), f64, 16), U=ab.guarded((B, N, 4), f64, 16),
              status=ab.guarded((B,), torch.int32))
    gg = dict(K=ab.guarded((B, N, 4, 12), f64), P0=ab.guarded((B, 12, 12), f64), status=ab.guarded((B,), torch.int32))
    xg = ab.guarded((B, 12), f64)
    assert _raw_pm(m, B, N, a, og, P, 16) == 0 and _raw_gains(m, B, ag, gg, P, 16) == 0
    assert _raw_sim(m, B, xs, us, a['wind'], P, 16, xg) == 0
    got = _host(dict(og, K=gg['K'], P0=gg['P0'], gstatus=gg['status'], xo=xg))
    for k in base:
        assert base[k].tobytes() == got[k].tobytes(), k
    for v in list(og.values()) + list(gg.values()) + [xg]:
        v.check()
    assert P.unchanged()
    # the Python layer passes a wider row as padding
    wide = np.concatenate([c['M'], np.full((B, 2), np.nan)], axis=1)
    py = _solve(m, c, model=wide)
    for k in SKEYS:
        assert py[k].tobytes() == base[k].tobytes(), k


# ------------------------------------------------------------------------------ 7. NaN isolation
@pytest.mark.parametrize('field,idx', [('mass', 0), ('J[4]', 9), ('t_blast', 4)])
def test_nan_record_entry_is_isolated(field, idx):
    B, N, bad = 5, 3, 3
    c = _case(B, N, 'sine', True)
    m = _mpc(N, B)
    s = _sim_case(B)
    clean = _solve(m, c)
    gclean = _gains(m, c)
    xclean = m.sim_step(s['x'], s['u'], model=c['M']).cpu().numpy()
    assert np.all(clean['status'] == 0) and np.all(gclean['status'] == 0) and np.isfinite(xclean).all()
    M = c['M'].copy()
    M[bad, idx] = np.nan
    others = np.arange(B) != bad
    got = _solve(m, c, model=M)
    assert np.array_equal(got['status'], np.where(others, 0, ST_NAN)), (field, got['status'])
    for k in SKEYS:
        assert np.isnan(got[k][bad]).all(), (field, k)
        assert got[k][others].tobytes() == clean[k][others].tobytes(), (field, k)
    gg = _gains(m, c, model=M)
    assert np.array_equal(gg['status'], np.where(others, 0, ST_NAN)), (field, gg['status'])
    for k in GKEYS:
        assert np.isnan(gg[k][bad]).all(), (field, k)
        assert gg[k][others].tobytes() == gclean[k][others].tobytes(), (field, k)
    xo = m.sim_step(s['x'], s['u'], model=M).cpu().numpy()
    assert np.isnan(xo[bad]).all() and xo[others].tobytes() == xclean[others].tobytes(), field


# ------------------------------------------------------------------------------ 8. the gains
@functools.lru_cache(maxsize=None)
def _mask(B, N):
    """A synthetic active set: half the components, stage 1 of instance 1 fully clamped, instance 2 free."""
    fx = np.random.default_rng(5).random((B, N, 4)) < 0.5
    fx[1, 1] = True
    fx[2] = False
    fx.setflags(write=False)
    return fx


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('B,N', SHAPES)
def test_gains_pm_matches_reference(B, N, dtype):
    spec = OcpSpec(N=N)
    cast = (lambda a: a)
    if dtype == 'f32':
        spec, cast = _spec32(spec), _f32
    c = {k: cast(v) for k, v in _case(B, N, 'hover', True).items()}
    m = _mpc(N, B, dtype)   # no box: fixed = NULL clamps nothing, and a mask is accepted
    free = None
    for fixed in (None, _mask(B, N)):
        ref = pm_gains_ref(c['xbar'], c['ubar'], fixed, spec, c['M'], c['wind'])
        assert ref['ok'].all()
        got = _gains(m, c, fixed=fixed)
        _check(got, ref, dtype, f'gains pm {dtype} B={B} N={N} masked={fixed is not None}', keys=GKEYS)
        assert np.array_equal(got['P0'], np.swapaxes(got['P0'], 1, 2))      # bitwise symmetric
        if fixed is None:
            free = got
        else:
            rows = np.ascontiguousarray(got['K'][fixed])
            assert not rows.view({4: np.uint32, 8: np.uint64}[rows.itemsize]).any()   # exactly +0
            assert fixed[1, 1].all()
    # the vehicles matter
    plain = m.solve_iterate_gains(c['xbar'], c['ubar'], wind=c['wind'])['K'].cpu().numpy()
    assert relerr(free['K'].astype(np.float64), plain.astype(np.float64)).min() > 1e-3


@pytest.mark.parametrize('B,N', SHAPES)
def test_gains_pm_K0_is_du0_dx0_of_the_pm_solve(B, N):
    """Two pm solves whose x0 differ by 1e-6 in every component (the unconstrained step is affine in
    x0): (u0' - u0) / 1e-6 = K_0 d, within the bound of test_K0_rows_are_the_vjp_of_u0_on_the_device in
    tests/test_gpu_gains.py (1e-9)."""
    c = _case(B, N, 'sine', True)
    m = _mpc(N, B)
    h = 1e-6
    d = np.random.default_rng(8).choice([-1.0, 1.0], size=(B, 12))
    s0, s1 = _solve(m, c), _solve(m, dict(c, x0=c['x0'] + h * d))
    K0 = _gains(m, c)['K'][:, 0]
    fd, pred = (s1['u0'] - s0['u0']) / h, np.einsum('bmi,bi->bm', K0, d)
    e = relerr(fd, pred).max()
    print(f'gains pm B={B} N={N}: d u0 / d x0 against K_0: {e:.2e}/1e-09 (|K_0 d| {np.abs(pred).max():.3g})')
    assert e <= 1e-9


# ------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    from mpc_blaster_amd.closed_loop import closed_loop
    for n in ('mpcb_sim_step_pm', 'mpcb_solve_iterate_pm', 'mpcb_solve_gains_pm'):
        assert n in _lib.EXPORTS and hasattr(_lib.load(), n)
    B, N = 3, 3
    c = _case(B, N)
    a = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref')}
    md = _t(c['M'])
    xs, us = _t(_sim_case(B)['x']), _t(_sim_case(B)['u'])
    m = _mpc(N, B)
    err = lambda: ab.Raw(m).error()   # noqa: E731
    o, g, xo = _outs(B, N), _gouts(B, N), torch.full((B, 12), 7.0, dtype=torch.float64, device='cuda')
    assert _raw_pm(m, B, N, a, o, md, 14) == 0 and _raw_gains(m, B, a, g, md, 14) == 0
    assert _raw_sim(m, B, xs, us, None, md, 14, xo) == 0
    # the model stride
    for sb in (-14, 7):
        assert _raw_pm(m, B, N, a, o, md, sb) == E_INVALID and 'model stride' in err()
        assert _raw_gains(m, B, a, g, md, sb) == E_INVALID and 'model stride' in err()
        assert _raw_sim(m, B, xs, us, None, md, sb, xo) == E_INVALID and 'model stride' in err()
    # B > max_batch, missing pointers
    assert _raw_pm(m, B + 1, N, a, o, md, 14) == E_INVALID
    assert _raw_gains(m, B + 1, a, g, md, 14) == E_INVALID
    for k in ('x0', 'xbar', 'ubar', 'xref', 'uref'):
        assert _raw_pm(m, B, N, dict(a, **{k: None}), o, md, 14) == E_INVALID, k
    for k in ('u0', 'status'):
        assert _raw_pm(m, B, N, a, dict(o, **{k: None}), md, 14) == E_INVALID, k
    for k in ('xbar', 'ubar'):
        assert _raw_gains(m, B, dict(a, **{k: None}), g, md, 14) == E_INVALID, k
    assert _raw_gains(m, B, a, dict(g, status=None), md, 14) == E_INVALID
    assert _raw_gains(m, B, a, dict(g, K=None, P0=None), md, 14) == E_INVALID
    assert _raw_sim(m, B, None, us, None, md, 14, xo) == E_INVALID
    assert _raw_sim(m, B, xs, us, None, md, 14, None) == E_INVALID
    assert _raw_pm(m, B, N, a, dict(o, X=None, U=None), md, 14) == 0   # the trajectories stay optional
    # fp32 with the box: refused, outputs untouched
    m32 = _mpc(N, B, 'f32', lbu=LB, ubu=UB)
    a32, o32 = {k: v.float() for k, v in a.items()}, _outs(B, N, torch.float32)
    assert _raw_pm(m32, B, N, a32, o32, md.float(), 14) == E_UNSUPPORTED
    with pytest.raises(_lib.MpcbError, match='mpcb error -4'):
        m32.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], model=c['M'])
    torch.cuda.synchronize()
    assert o32['status'].eq(-77).all() and all(o32[k].eq(7.0).all() for k in SKEYS)
    # the 17/6 model: all three entry points, and the Python layer
    m17 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    z = dict(x0=torch.zeros((B, 17), dtype=torch.float64, device='cuda'),
             xbar=torch.zeros((B, N + 1, 17), dtype=torch.float64, device='cuda'),
             ubar=torch.zeros((B, N, 6), dtype=torch.float64, device='cuda'),
             xref=torch.zeros((B, N + 1, 17), dtype=torch.float64, device='cuda'),
             uref=torch.zeros((B, N, 6), dtype=torch.float64, device='cuda'))
    big = torch.full((B * (N + 1) * 17 * 17,), 7.0, dtype=torch.float64, device='cuda')
    o17 = dict(u0=big, X=big, U=big, status=o['status'])
    assert _raw_pm(m17, B, N, z, o17, md, 14) == E_UNSUPPORTED and 'per-instance models' in ab.Raw(m17).error()
    # ... and a caller of mpcb_solve_iterate_pw reads about weights, as before
    assert _raw_pm(m17, B, N, z, o17, None, 0, pw=True) == E_UNSUPPORTED
    assert ab.Raw(m17).error() == 'per-instance weights cover the 12/4 model only'
    assert _raw_pm(m32, B, N, a32, o32, None, 0, pw=True) == E_UNSUPPORTED
    assert ab.Raw(m32).error() == 'per-instance weights with the input box need an fp64 handle'
    assert _raw_gains(m17, B, z, dict(K=big, P0=big, status=o['status']), md, 14) == E_UNSUPPORTED
    assert _raw_sim(m17, B, z['x0'], z['ubar'], None, md, 14, big) == E_UNSUPPORTED
    assert big.eq(7.0).all()
    z17 = {k: v.cpu().numpy() for k, v in z.items()}
    with pytest.raises(ValueError):
        m17.pack_model(mass=np.ones(B))
    with pytest.raises(ValueError):
        m17.solve_iterate(z17['x0'], z17['xbar'], z17['ubar'], z17['xref'], z17['uref'], model=c['M'])
    with pytest.raises(ValueError):
        m17.solve_iterate_gains(z17['xbar'], z17['ubar'], model=c['M'])
    with pytest.raises(ValueError):
        m17.sim_step(z17['x0'], z17['ubar'][:, 0], model=c['M'])
    for kw in (dict(model=c['M']), dict(plant_model=c['M'])):
        with pytest.raises(ValueError):
            closed_loop(m17, z17['x0'], z17['xref'], z17['uref'], 2, **kw)
    # closed_loop: diagnostics reads the handle's model; weights with feedback stays refused
    with pytest.raises(ValueError, match='diagnostics'):
        closed_loop(m, c['x0'], c['xref'], c['uref'], 2, diagnostics=True, model=c['M'])
    with pytest.raises(ValueError):
        closed_loop(m, c['x0'], c['xref'], c['uref'], 2, feedback=True, weights=dict(Q=c['Q']), model=c['M'])
    # shapes the Python layer refuses
    with pytest.raises(ValueError):
        m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], model=c['M'][:, :13])
    with pytest.raises(ValueError):
        m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], model=c['M'][:2])
    with pytest.raises(ValueError):
        m.pack_model(B=B, mass=np.ones(B + 1))
    with pytest.raises(ValueError):
        m.pack_model(J=np.ones((B, 2)))


def test_pack_model_fields_and_defaults():
    B = 4
    m = _mpc(3, B, t_blast=1.5)
    cfg = m.cfg
    own = m.pack_model().cpu().numpy()
    assert np.array_equal(own, pack_params(params_of(np.concatenate([[cfg.mass, cfg.lx, cfg.ly, cfg.c, 1.5],
                                                                     np.asarray(cfg.J).reshape(9)]),
                                                     OcpSpec(N=3).params))[None])
    m.set_t_blast(2.5)
    assert m.pack_model().cpu().numpy()[0, 4] == 2.5
    mass = np.array([8.0, 9.0, 10.0, 11.0])
    Jd = np.array([[0.5, 0.6, 0.7]] * B) * np.arange(1, B + 1)[:, None]
    pk = m.pack_model(mass=torch.as_tensor(mass, device='cuda'), J=Jd, lx=[0.3], t_blast=0.0).cpu().numpy()
    assert pk.shape == (B, 14) and np.array_equal(pk[:, 0], mass) and np.all(pk[:, 1] == 0.3) and np.all(pk[:, 4] == 0.0)
    assert np.array_equal(pk[:, 5:].reshape(B, 3, 3), np.stack([np.diag(r) for r in Jd]))
    assert np.all(pk[:, 2] == cfg.ly) and np.all(pk[:, 3] == cfg.c)
    Jf = np.tile(np.asarray(cfg.J)[None], (B, 1, 1)) + 0.01
    assert np.array_equal(m.pack_model(J=Jf).cpu().numpy()[:, 5:], Jf.reshape(B, 9))
    assert tuple(m.pack_model(B=B).shape) == (B, 14)
    assert _mpc(3, B, 'f32').pack_model(mass=mass).dtype == torch.float32


# ------------------------------------------------------------------------------ 10. the closed loop
@functools.lru_cache(maxsize=None)
def _loop_case():
    B, N = 3, 5
    c = _case(B, N)
    spec = OcpSpec(N=N)
    return B, N, c, spec, pm_models(B, spec, 21), pm_models(B, spec, 22)   # the belief, the truth


def _loop_ref(nsim, c, spec, Mc, Mp, h=1, feedback=False):
    B, N = c['x0'].shape[0], spec.N
    xbar, ubar, x = np.zeros((B, N + 1, 12)), np.zeros((B, N, 4)), c['x0'].copy()
    Xs, Us = [x], []
    for i in range(nsim):
        j = i % h
        if j == 0:
            if feedback:
                K = pm_gains_ref(xbar, ubar, None, spec, Mc)['K']
            o = pm_solve_ref(x, c['xref'], c['uref'], xbar, ubar, spec, Mc)
            assert np.all(o['status'] == 0)
            xbar, ubar = o['X'], o['U']
        u = ubar[:, j]
        if feedback:
            u = u + np.einsum('bmi,bi->bm', K[:, j], x - xbar[:, j])
        x = pm_sim_ref(x, u, spec.dt, spec, Mp)
        Us.append(u)
        Xs.append(x)
    return np.stack(Xs, axis=1), np.stack(Us, axis=1)


@pytest.mark.parametrize('roles', ['plant', 'controller', 'both'])
def test_closed_loop_with_the_two_model_roles(roles):
    from mpc_blaster_amd.closed_loop import closed_loop
    nsim = 3
    B, N, c, spec, Mc, Mp = _loop_case()
    Mc, Mp = (Mc if roles != 'plant' else None), (Mp if roles != 'controller' else None)
    m = _mpc(N, B)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error')   # read-only records (frozen fixtures) are taken without a warning
        ro = [None if M is None else M.copy() for M in (Mc, Mp)]
        for M in ro:
            if M is not None:
                M.setflags(write=False)
        Xs, Us, st = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, model=ro[0], plant_model=ro[1])
    torch.cuda.synchronize()
    rX, rU = _loop_ref(nsim, c, spec, Mc, Mp)
    for i in range(nsim):
        eu, ex = relerr(Us[:, i].cpu().numpy(), rU[:, i]).max(), relerr(Xs[:, i + 1].cpu().numpy(), rX[:, i + 1]).max()
        print(f'  {roles} step {i}: u {eu:.2e}  x {ex:.2e}')
        assert eu < 1e-8 and ex < 1e-8
    assert (st.cpu().numpy() == 0).all()
    # the vehicles do steer the loop apart from the handle's
    Xs0, Us0, _ = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim)
    assert relerr(Xs[:, 1:].cpu().numpy(), Xs0[:, 1:].cpu().numpy()).min() > 1e-3


def test_closed_loop_feedback_between_solves_with_both_models():
    """resolve_every = 2 with the feedback law: the applied inputs are Up[:, j] + K[:, j] (x - Xp[:, j])
    with the gains of the controller's belief (a handle without a box: nothing to clip)."""
    from mpc_blaster_amd.closed_loop import closed_loop
    nsim = 3
    B, N, c, spec, Mc, Mp = _loop_case()
    m = _mpc(N, B)
    Xs, Us, st = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, resolve_every=2, feedback=True, model=Mc,
                             plant_model=Mp)
    torch.cuda.synchronize()
    rX, rU = _loop_ref(nsim, c, spec, Mc, Mp, h=2, feedback=True)
    eu, ex = relerr(Us.cpu().numpy(), rU).max(), relerr(Xs.cpu().numpy(), rX).max()
    print(f'  feedback loop: U {eu:.2e}  X {ex:.2e}')
    assert eu < 1e-8 and ex < 1e-8 and (st.cpu().numpy() == 0).all()
    # the feedback term is there (step 1 is not the held input) and the models matter
    held = _loop_ref(nsim, c, spec, Mc, Mp, h=2, feedback=False)[1]
    assert relerr(rU[:, 1], held[:, 1]).min() > 1e-6
    Xs0, Us0, _ = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, resolve_every=2, feedback=True)
    assert relerr(Us.cpu().numpy(), Us0.cpu().numpy()).min() > 1e-3
