"""mpcb_solve_iterate_pw and mpcb_solve_vjp_pw on the GPU (the RTI step and its gradients with cost
weights per instance), the torch layer and the closed loop over them, against tests/pw_ref.py: the
device is compared with the NumPy reference, never with itself.  tests/test_pw_ref_cpu.py ties that
reference to the batched oracle and to finite differences.

Metric: tests/test_gpu_vjp.py ``relerr``, per instance and output |dev - ref|_inf / max(|ref|_inf, 1).
Bounds: fp64 1e-9, fp32 5e-5 (the project's); fp32 cases measure, on the reference alone, its move
under a seeded relative +-2^-22 perturbation of every input (tests/test_gpu_vjp_weights.py) and bound
the device by max(5e-5, 10 x move); they print move, bound and error.  Draws: tests/vjp_ref.py
vjp_case (seed 1004), box [5, 40], weights tests/pw_ref.py pw_weights (seed 11).
"""
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_call as ab   # noqa: E402
import alt_config as ac   # noqa: E402
from pw_ref import pw_solve_ref, pw_vjp_ref, pw_weights   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.ocp import OcpSpec, dense_box_qp, linearise, mpc_solve   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from test_gpu_vjp import BOUND, LB, UB, _f32, _mpc, _spec32, _synthetic_U, relerr   # noqa: E402

SKEYS = ('u0', 'X', 'U')
GKEYS = ('gx0', 'gxref', 'guref', 'gQ', 'gR', 'gQN')
E_INVALID, E_UNSUPPORTED = -1, -4
ST_NAN, ST_MAXITER = 1, 2


@functools.lru_cache(maxsize=None)
def _case(B, N, ref='hover', wind=False):
    """vjp_case and the weight draw; never modified."""
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec, ref, wind)
    Q, R, QN = pw_weights(B, spec)
    return dict(c, Q=Q, R=R, QN=QN)


@functools.lru_cache(maxsize=None)
def _box_ref(B=16, N=8):
    """Case 3's reference solve (shared by the cap, end-to-end and NaN tests); never modified."""
    c = _case(B, N)
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    return spec, pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'])


def _t(a, dtype=torch.float64):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def _solve(m, c, Q='Q', R='R', QN='QN', xref=None, uref=None):
    """solve_iterate with the case's per-instance weights; the outputs as float64 NumPy."""
    w = {k: (None if n is None else (c[n] if isinstance(n, str) else n)) for k, n in (('Q', Q), ('R', R), ('QN', QN))}
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'] if xref is None else xref,
                    c['uref'] if uref is None else uref, wind=c['wind'], **w)
    torch.cuda.synchronize()
    return dict(u0=m.get_control().cpu().numpy().astype(np.float64),
                X=m.get_state_trajectory().cpu().numpy().astype(np.float64),
                U=m.get_input_trajectory().cpu().numpy().astype(np.float64),
                status=m.get_status().cpu().numpy())


def _check(got, ref, dtype, tag, keys=SKEYS, bound=None, status=True):
    if status:
        assert np.array_equal(got['status'], ref['status']) and np.all(got['status'] == 0), (tag, got['status'])
    bound = dict({k: BOUND[dtype] for k in keys}, **(bound or {}))
    err = {k: relerr(got[k], ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound[k]:.1e} (|ref| {np.abs(ref[k]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= bound[k], (tag, k, err[k], bound[k])
    return err


def _raw_pw(m, B, x0, xbar, ubar, xref, xref_sb, uref, uref_sb, wind, wind_sb, Qw, Q_sb, Rw, R_sb, QNw, QN_sb, u0, X, U,
            status, stream=0, x0_sb=12):
    """The C entry point with pointers and strides exactly as given (tests/abi_call.py _p)."""
    return m.lib.mpcb_solve_iterate_pw(m._h, B, ab._p(x0), x0_sb, ab._p(xbar), ab._p(ubar), ab._p(xref), xref_sb,
                                       ab._p(uref), uref_sb, ab._p(wind), wind_sb, ab._p(Qw), Q_sb, ab._p(Rw), R_sb,
                                       ab._p(QNw), QN_sb, ab._p(u0), ab._p(X), ab._p(U), ab._p(status), ab._p(stream))


def _outs(B, N, dtype=torch.float64):
    return dict(u0=torch.full((B, 4), 7.0, dtype=dtype, device='cuda'),
                X=torch.full((B, N + 1, 12), 7.0, dtype=dtype, device='cuda'),
                U=torch.full((B, N, 4), 7.0, dtype=dtype, device='cuda'),
                status=torch.full((B,), -77, dtype=torch.int32, device='cuda'))


def _host(o):
    torch.cuda.synchronize()
    return {k: (v.view if isinstance(v, ab.Guarded) else v).cpu().numpy().astype(np.float64 if k != 'status' else np.int32)
            for k, v in o.items()}


# ------------------------------------------------------------------------------ 1. fp64, unconstrained
@pytest.mark.parametrize('B,N,wind,ref,bcast', [
    (1, 1, False, 'hover', False), (7, 3, True, 'sine', False), (5, 64, False, 'hover', True)])
def test_pw_fp64_matches_reference(B, N, wind, ref, bcast):
    """(7, 3): wind and sine references with per-instance strides; (5, 64): one reference row for
    the whole batch (stride 0)."""
    c = _case(B, N, ref, wind)
    xref, uref = (c['xref'][:1], c['uref'][:1]) if bcast else (c['xref'], c['uref'])
    spec = OcpSpec(N=N)
    r = pw_solve_ref(c['x0'], xref, uref, c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'], c['wind'])
    m = _mpc(N, B)
    got = _solve(m, c, xref=xref, uref=uref)
    _check(got, r, 'f64', f'pw fp64 B={B} N={N} wind={wind} ref={ref} bcast={bcast}')
    # the weights matter: the shared-weight solution is somewhere else, for every instance
    shared = mpc_solve(c['x0'], xref, uref, spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    dU = np.abs(got['U'] - shared['U']).reshape(B, -1).max(axis=1)
    print(f'  per-instance against shared weights: min over instances of |dU| {dU.min():.3g}')
    assert dU.min() > 1e-3


# ------------------------------------------------------------------------------ 2. broadcast, NULL, dense
def test_pw_broadcast_q_and_null_r_qn():
    """One Q for the whole batch (stride 0), NULL Rw / QNw: the handle's spec with that Q."""
    B, N = 7, 3
    c = _case(B, N, 'sine', True)
    spec = dataclasses.replace(OcpSpec(N=N), Q=c['Q'][2])
    r = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    m = _mpc(N, B)
    _check(_solve(m, c, Q=c['Q'][2:3], R=None, QN=None), r, 'f64', 'pw Q broadcast, R and QN NULL')


@pytest.mark.parametrize('how', ['null', 'equal'])
def test_pw_handle_weights_agree_with_the_oracle(how):
    """All three NULL, or all equal to the handle's: the oracle at the handle's spec (not the bits
    of mpcb_solve_iterate: another kernel)."""
    B, N = 7, 3
    c = _case(B, N, 'sine', True)
    spec = OcpSpec(N=N)
    r = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    m = _mpc(N, B)
    t = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'wind')}
    o = _outs(B, N)
    if how == 'null':
        W = [(None, 0)] * 3
    else:
        W = [(_t(np.tile(np.asarray(M)[None], (B, 1, 1))), M.size) for M in (spec.Q, spec.R, spec.QN)]
    assert _raw_pw(m, B, t['x0'], t['xbar'], t['ubar'], t['xref'], (N + 1) * 12, t['uref'], N * 4, t['wind'], 3,
                   W[0][0], W[0][1], W[1][0], W[1][1], W[2][0], W[2][1], o['u0'], o['X'], o['U'], o['status']) == 0
    _check(_host(o), r, 'f64', f'pw handle weights ({how})')


def test_pw_dense_weights_and_another_model():
    """tests/alt_config.py 'b': dense weights, another model, cost_scale != dt; with wind."""
    B, N = 7, 8
    kw = ac.fields(alt='b', box='none')
    spec = OcpSpec(N=N, **ac.spec_kwargs(kw))
    c = vjp_case(B, N, spec, 'sine', True)
    Q, R, QN = pw_weights(B, spec)
    assert np.abs(Q[0] - np.diag(np.diag(Q[0]))).max() > 0.1   # dense
    c = dict(c, Q=Q, R=R, QN=QN)
    r = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, Q, R, QN, c['wind'])
    m = _mpc(N, B, **kw)
    _check(_solve(m, c), r, 'f64', 'pw ALT-b dense')


# ------------------------------------------------------------------------------ 3. input box, fp64
def test_pw_box_fp64_matches_reference():
    B, N = 16, 8
    c = _case(B, N)
    spec, r = _box_ref(B, N)
    assert np.all(r['status'] == 0) and not r['fallback'].any() and r['iters'].max() <= 8
    lo, hi = r['U'] <= LB + 1e-9, r['U'] >= UB - 1e-9
    fixed = lo | hi
    per = fixed.sum(axis=(1, 2))
    print(f'pw box: reference passes {r["iters"].tolist()}, clamped components per instance {per.tolist()}')
    assert (per > 0).sum() >= 8
    m = _mpc(N, B, lbu=LB, ubu=UB)
    got = _solve(m, c)
    assert np.all(got['status'] == 0)
    _check(got, r, 'f64', f'pw box fp64 B={B} N={N}')
    # clamped components are the bound's value itself, and nothing else is on a bound
    assert np.array_equal(got['U'][lo], np.broadcast_to(LB, got['U'].shape)[lo])
    assert np.array_equal(got['U'][hi], np.broadcast_to(UB, got['U'].shape)[hi])
    assert np.array_equal((got['U'] <= LB) | (got['U'] >= UB), fixed)
    assert np.array_equal(got['u0'], got['U'][:, 0])
    assert ((got['U'] <= LB) | (got['U'] >= UB)).any(axis=(1, 2)).sum() >= 8
    # the oracle itself against BVLS on the condensed QP, on 4 instances (2 of them the most clamped)
    for b in list(np.argsort(per)[-2:]) + [0, 5]:
        sb = dataclasses.replace(spec, Q=c['Q'][b], R=c['R'][b], QN=c['QN'][b])
        one = {k: c[k][b:b + 1] for k in ('x0', 'xbar', 'ubar', 'xref', 'uref')}
        A, Bm, gap = linearise(one['xbar'], one['ubar'], sb)
        du = dense_box_qp(A, Bm, gap, one['x0'] - one['xbar'][:, 0], one['xbar'], one['ubar'], one['xref'],
                          one['uref'], sb)
        e = np.abs(one['ubar'] + du - r['U'][b:b + 1]).max()
        print(f'  instance {b}: oracle against BVLS {e:.2e} ({per[b]} clamped)')
        assert e < 1e-6


# ------------------------------------------------------------------------------ 4. the cap
def test_pw_box_cap_reports_maxiter():
    B, N, cap = 16, 8, 4
    c = _case(B, N)
    _, r = _box_ref(B, N)
    late = r['iters'] > cap
    print(f'pw cap {cap}: reference passes {r["iters"].tolist()}, over the cap {np.nonzero(late)[0].tolist()}')
    assert late.any() and not late.all()
    full = _solve(_mpc(N, B, lbu=LB, ubu=UB), c)
    got = _solve(_mpc(N, B, lbu=LB, ubu=UB, max_as_iter=cap), c)
    assert np.array_equal(got['status'], np.where(late, ST_MAXITER, 0))
    for k in SKEYS:
        assert np.array_equal(got[k][~late], full[k][~late]), k
        assert np.isfinite(got[k]).all()


# ------------------------------------------------------------------------------ 5. slots and stride
def test_pw_strides_over_its_slots(monkeypatch):
    """More waves than workspace slots: the stride loop reuses a slot and the LDS weights."""
    B, N = 37, 3
    c = _case(B, N)
    r = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], OcpSpec(N=N), c['Q'], c['R'], c['QN'])
    monkeypatch.setenv('MPCB_PW_SLOTS', '3')
    m = _mpc(N, B)
    _check(_solve(m, c), r, 'f64', 'pw fp64 B=37 N=3, 3 slots')


# ------------------------------------------------------------------------------ 6. fp32, refusals
def _pert(rng, a):
    return None if a is None else a * (1.0 + 2.0 ** -22 * rng.choice([-1.0, 1.0], size=np.shape(a)))


def test_pw_fp32_unconstrained():
    B, N = 7, 8
    spec = _spec32(OcpSpec(N=N))
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    args = [c[k] for k in ('x0', 'xref', 'uref', 'xbar', 'ubar')]
    W = [c[k] for k in ('Q', 'R', 'QN')]
    r = pw_solve_ref(*args, spec, *W)
    rng = np.random.default_rng(0)
    moved = pw_solve_ref(*[_pert(rng, a) for a in args], spec, *[_pert(rng, w) for w in W])
    move = {k: relerr(moved[k], r[k]).max() for k in SKEYS}
    bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in SKEYS}
    print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in SKEYS))
    m = _mpc(N, B, 'f32')
    _check(_solve(m, c), r, 'f32', f'pw fp32 B={B} N={N}', bound=bound)


def test_pw_refusals():
    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    for n in ('mpcb_solve_iterate_pw', 'mpcb_solve_vjp_pw'):
        assert n in _lib.EXPORTS and hasattr(_lib.load(), n)
    B, N = 3, 3
    c = _case(B, N)
    t = {k: _t(c[k]) for k in ('x0', 'xbar', 'ubar', 'xref', 'uref', 'Q', 'R', 'QN')}
    o = _outs(B, N)

    def call(m, B=B, sb=(144, 16, 144), **over):
        a = dict(t, **o)
        a.update(over)
        return _raw_pw(m, B, a['x0'], a['xbar'], a['ubar'], a['xref'], (N + 1) * 12, a['uref'], N * 4, None, 0, a['Q'],
                       sb[0], a['R'], sb[1], a['QN'], sb[2], a['u0'], a['X'], a['U'], a['status'])

    m = _mpc(N, B)
    assert call(m) == 0
    for sb in ((-144, 16, 144), (144, -1, 144), (144, 16, -144)):
        assert call(m, sb=sb) == E_INVALID and 'negative stride' in ab.Raw(m).error()
    assert call(m, B=B + 1) == E_INVALID
    for k in ('u0', 'status', 'x0', 'xref', 'uref', 'xbar', 'ubar'):
        assert call(m, **{k: None}) == E_INVALID, k
    assert call(m, X=None, U=None) == 0   # the trajectories are optional, as in mpcb_solve_iterate
    # fp32 with the box, and the 17/6 model
    m32 = _mpc(N, B, 'f32', lbu=LB, ubu=UB)
    t32 = {k: v.float() for k, v in t.items()}
    o32 = _outs(B, N, torch.float32)
    assert call(m32, **t32, **o32) == E_UNSUPPORTED
    with pytest.raises(_lib.MpcbError, match='mpcb error -4'):
        m32.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=c['Q'])
    assert o32['status'].eq(-77).all() and o32['u0'].eq(7.0).all()
    m17 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    assert call(m17) == E_UNSUPPORTED
    with pytest.raises(ValueError):
        m17.solve_iterate(np.zeros((B, 17)), np.zeros((B, N + 1, 17)), np.zeros((B, N, 6)), np.zeros((1, N + 1, 17)),
                          np.zeros((1, N, 6)), Q=np.ones((B, 17)))
    with pytest.raises(ValueError):
        m17.solve_iterate_diff(torch.zeros((B, 17), dtype=torch.float64, device='cuda'), np.zeros((B, N + 1, 17)),
                               np.zeros((B, N, 6)), torch.zeros((1, N + 1, 17), dtype=torch.float64, device='cuda'),
                               torch.zeros((1, N, 6), dtype=torch.float64, device='cuda'),
                               Q=torch.ones((B, 17), dtype=torch.float64, device='cuda'), per_instance_weights=True)
    # shapes without a batch axis are refused by the Python layer
    with pytest.raises(ValueError):
        m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=np.ones(12))


# ------------------------------------------------------------------------------ 7. the product
def _vjp(m, c, X, U, w=('Q', 'R', 'QN'), weights=True):
    kw = {k: c[k] for k in w}
    out = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, wind=c['wind'], X=X, x_ref=c['xref'],
                              u_ref=c['uref'], weights=weights, **kw)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy().astype(np.float64 if k != 'status' else np.int32) for k, v in out.items()}
    for k in ('gQ', 'gR', 'gQN'):
        if k in got:
            # bitwise symmetric (a NaN instance is NaN in both places)
            assert np.array_equal(got[k], np.swapaxes(got[k], 1, 2), equal_nan=True), k
    return got


def _vjp_ref(c, X, U, spec):
    return pw_vjp_ref(c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'], spec, c['Q'], c['R'], c['QN'],
                      c['wind'])


def _vjp_check(got, r, dtype, tag, bound=None):
    assert np.all(got['status'] == 0), (tag, got['status'])
    return _check(got, r, dtype, tag, keys=GKEYS, bound=bound, status=False)


def test_vjp_pw_fp64_unconstrained():
    B, N = 7, 3
    c = _case(B, N, 'sine', True)
    spec = OcpSpec(N=N)
    o = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'], c['wind'])
    r = _vjp_ref(c, o['X'], o['U'], spec)
    m = _mpc(N, B)
    got = _vjp(m, c, o['X'], o['U'])
    _vjp_check(got, r, 'f64', f'vjp pw fp64 B={B} N={N}')
    # without a weight output: the same product
    plain = _vjp(m, c, None, None, weights=False)
    for k in ('gx0', 'gxref', 'guref'):
        assert relerr(plain[k], r[k]).max() <= BOUND['f64'], k
    # the weights matter: the shared-weight product is somewhere else
    shared = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], wind=c['wind'])
    torch.cuda.synchronize()
    assert relerr(shared['gxref'].cpu().numpy(), r['gxref']).min() > 1e-3


def test_vjp_pw_fp64_box_synthetic_mask():
    B, N = 7, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    U = _synthetic_U(c, spec)
    X = c['xbar'] + 0.05 * np.random.default_rng(5).standard_normal(c['xbar'].shape)
    r = _vjp_ref(c, X, U, spec)
    assert r['fixed'][1, 2].all() and r['fixed'].mean() > 0.2
    m = _mpc(N, B, lbu=LB, ubu=UB)
    _vjp_check(_vjp(m, c, X, U), r, 'f64', f'vjp pw fp64 box synthetic B={B} N={N} ({r["fixed"].mean():.0%} clamped)')


def test_vjp_pw_fp64_box_end_to_end():
    """U from the device's own solve_iterate(Q=...): its clamped components carry the bound itself."""
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    s = _solve(m, c)
    assert np.all(s['status'] == 0)
    clamped = ((s['U'] <= LB) | (s['U'] >= UB)).any(axis=(1, 2))
    print(f'end to end: {clamped.sum()} of {B} instances with a clamped component')
    assert clamped.sum() >= 8
    r = _vjp_ref(c, s['X'], s['U'], spec)
    assert np.array_equal(r['fixed'], (s['U'] <= LB) | (s['U'] >= UB))
    _vjp_check(_vjp(m, c, s['X'], s['U']), r, 'f64', 'vjp pw fp64 box end to end')


@pytest.mark.parametrize('box', [False, True])
def test_vjp_pw_fp32(box):
    B, N = 7, 8
    spec = _spec32(OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None))
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    if box:
        U = _f32(_synthetic_U(c, spec))
        X = _f32(c['xbar'] + 0.05 * np.random.default_rng(5).standard_normal(c['xbar'].shape))
        fixed = (U <= spec.lbu) | (U >= spec.ubu)
    else:
        o = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'])
        X, U, fixed = _f32(o['X']), _f32(o['U']), None
    r = _vjp_ref(c, X, U, spec)
    rng = np.random.default_rng(0)
    q = {k: _pert(rng, v) for k, v in c.items()}
    Up = _pert(rng, U)
    if fixed is not None:
        Up = np.where(fixed, U, Up)   # a clamped component stays on its bound
    moved = _vjp_ref(q, _pert(rng, X), Up, spec)
    assert np.array_equal(moved['fixed'], r['fixed'])
    move = {k: relerr(moved[k], r[k]).max() for k in GKEYS}
    bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in GKEYS}
    print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in GKEYS))
    m = _mpc(N, B, 'f32', **(dict(lbu=LB, ubu=UB) if box else {}))
    _vjp_check(_vjp(m, c, X, U), r, 'f32', f'vjp pw fp32 B={B} N={N} box={box}', bound)


def test_existing_vjp_entry_points_keep_their_bits():
    """mpcb_solve_vjp_w on the same handle before and after a _pw solve and a _pw product."""
    B, N = 7, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    U = _synthetic_U(c, spec)
    m = _mpc(N, B, lbu=LB, ubu=UB)

    def old():
        out = m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, X=c['xbar'], x_ref=c['xref'],
                                  u_ref=c['uref'], weights=True)
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}

    a = old()
    _solve(m, c)
    _vjp(m, c, c['xbar'], U)
    b = old()
    for k in a:
        assert ab.same_bits(a[k], b[k]), k


# ------------------------------------------------------------------------------ 8. NaN isolation
@pytest.mark.parametrize('box', [False, True])
def test_pw_nan_is_isolated(box):
    B, N, bad = 7, 8, 2
    c = _case(B, N)
    m = _mpc(N, B, **(dict(lbu=LB, ubu=UB) if box else {}))
    clean, again = _solve(m, c), _solve(m, c)
    assert np.all(clean['status'] == 0)
    for k in clean:
        assert np.array_equal(clean[k], again[k]), k   # two calls: the same bits
    others = np.arange(B) != bad
    for where in ('Q', 'xbar'):
        a = c[where].copy()
        a[(bad, 1, 4)] = np.nan
        got = _solve(m, dict(c, **{where: a}))
        assert np.array_equal(got['status'], np.where(others, 0, ST_NAN)), (where, got['status'])
        for k in SKEYS:
            assert np.isnan(got[k][bad]).all(), (where, k)
            assert np.array_equal(got[k][others], clean[k][others]), (where, k)
    # and the product
    U = clean['U']
    g0 = _vjp(m, c, clean['X'], U)
    a = c['QN'].copy()
    a[bad, 3, 3] = np.inf
    g1 = _vjp(m, dict(c, QN=a), clean['X'], U)
    assert np.array_equal(g1['status'], np.where(others, 0, ST_NAN))
    for k in GKEYS:
        assert np.isnan(g1[k][bad]).all(), k
        assert np.array_equal(g1[k][others], g0[k][others]), k


# ------------------------------------------------------------------------------ 9. ABI
def test_pw_abi_strides_alignment_aliasing_stream():
    """Padded weight strides on element-aligned (not 16-byte aligned) arrays, X / U aliasing
    xbar / ubar, a stream of the caller's own, and guard bands around every output."""
    from test_gpu_abi import _on_stream
    B, N = 7, 6
    c = _case(B, N, 'sine', True)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    base = _solve(m, c)
    # hard draws (sine references, wind): the reference hands two instances to its interior point
    # after the 48 passes of the cap, where this entry point reports MAXITER; the others agree
    r = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], OcpSpec(N=N, lbu=LB, ubu=UB), c['Q'], c['R'],
                     c['QN'], c['wind'])
    print(f'pw abi case: reference passes {r["iters"].tolist()}, handed over {r["fallback"].tolist()}')
    assert np.array_equal(base['status'], np.where(r['fallback'], ST_MAXITER, 0)) and not r['fallback'].all()
    ok = ~r['fallback']
    _check({k: base[k][ok] for k in SKEYS}, {k: r[k][ok] for k in SKEYS}, 'f64', 'pw abi case', status=False)
    f64 = torch.float64
    t = {k: _t(c[k]) for k in ('x0', 'xref', 'uref', 'wind')}
    # record b at lead + b * stride: lead 3 puts the first record 24 bytes into a 256-byte aligned block
    W = {k: ab.padded(c[k], sb, 3, f64) for k, sb in (('Q', 144 + 13), ('R', 16 + 5), ('QN', 144 + 1))}
    for w in W.values():
        assert w.ptr % 16 == 8
    o = dict(u0=ab.guarded((B, 4), f64), X=ab.guarded((B, N + 1, 12), f64, 16), U=ab.guarded((B, N, 4), f64, 16),
             status=ab.guarded((B,), torch.int32))

    def launch(stream):
        # X and U alias the iterate: the call overwrites it in place, so it is put back first
        o['X'].view.copy_(_t(c['xbar']))
        o['U'].view.copy_(_t(c['ubar']))
        return _raw_pw(m, B, t['x0'], o['X'], o['U'], t['xref'], (N + 1) * 12, t['uref'], N * 4, t['wind'], 3, W['Q'],
                       W['Q'].stride, W['R'], W['R'].stride, W['QN'], W['QN'].stride, o['u0'], o['X'], o['U'],
                       o['status'], stream)

    assert launch(0) == 0
    got = _host(o)
    for k in base:
        assert np.array_equal(got[k], base[k]), k
    for g in o.values():
        g.check()
    for w in W.values():
        assert w.unchanged()
    # the same on a stream of the caller's own, behind a delay and the copies that create its inputs
    o['u0'].reset(), o['status'].reset()
    ins = [t['x0'], t['xref'], t['uref'], t['wind'], W['Q'].buf, W['R'].buf, W['QN'].buf]
    _on_stream(ins, launch)
    got = _host(o)
    for k in base:
        assert np.array_equal(got[k], base[k]), k
    for g in o.values():
        g.check()


# ------------------------------------------------------------------------------ 10. the torch layer
def _diag(W):
    return np.ascontiguousarray(np.diagonal(W, axis1=1, axis2=2))


def _loss_weights(B, N, seed=9):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, 4)), rng.standard_normal((B, N + 1, 12)), rng.standard_normal((B, N, 4))


def test_torch_layer_per_instance_weights():
    B, N = 3, 3
    c = _case(B, N, 'sine', True)
    spec = OcpSpec(N=N)
    cu0, cX, cU = _loss_weights(B, N)
    m = _mpc(N, B)
    before = _solve(m, c, Q=None, R=None, QN=None)   # the plain solve of the handle
    version = m._weights_version
    leaf = lambda a: _t(a).requires_grad_(True)   # noqa: E731
    x0, xref, uref = leaf(c['x0']), leaf(c['xref']), leaf(c['uref'])
    Wt = {k: leaf(_diag(c[k])) for k in ('Q', 'R', 'QN')}   # 2-D [B, n]: diagonals

    def forward(**w):
        return m.solve_iterate_diff(x0, c['xbar'], c['ubar'], xref, uref, wind=_t(c['wind']), per_instance_weights=True,
                                    **w)

    def loss(u0, X, U):
        return (u0 * _t(cu0)).sum() + (X * _t(cX)).sum() + (U * _t(cU)).sum()

    L = loss(*forward(**Wt))
    L.backward()
    torch.cuda.synchronize()
    assert m._weights_version == version
    # the reference: the solve and its product with the cotangent of u0 added to gU[:, 0]
    o = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, c['Q'], c['R'], c['QN'], c['wind'])
    gU = cU.copy()
    gU[:, 0] += cu0
    r = pw_vjp_ref(c['xbar'], c['ubar'], o['X'], o['U'], c['xref'], c['uref'], cX, gU, spec, c['Q'], c['R'], c['QN'],
                   c['wind'])
    got = dict(gx0=x0.grad, gxref=xref.grad, guref=uref.grad, gQ=Wt['Q'].grad, gR=Wt['R'].grad, gQN=Wt['QN'].grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ref = dict(r, gQ=_diag(r['gQ']), gR=_diag(r['gR']), gQN=_diag(r['gQN']))
    assert got['gQ'].shape == (B, 12) and got['gR'].shape == (B, 4) and got['gQN'].shape == (B, 12)
    _check(got, ref, 'f64', 'torch layer, per-instance diagonals', keys=GKEYS, status=False)
    # one entry per tensor against a central difference of the device's own forward solve (the
    # method and bound of tests/test_pw_ref_cpu.py: h = 1e-4 W_ii, 1e-6 of the tensor's largest entry)
    b = 1
    for k in ('Q', 'R', 'QN'):
        i = int(np.abs(ref['g' + k][b]).argmax())
        h = 1e-4 * _diag(c[k])[b, i]
        Ls = []
        for sgn in (1.0, -1.0):
            w = {n: _t(_diag(c[n])) for n in ('Q', 'R', 'QN')}
            w[k][b, i] += sgn * h
            with torch.no_grad():
                Ls.append(float(loss(*forward(**w))))
        fd = (Ls[0] - Ls[1]) / (2.0 * h)
        d = abs(fd - got['g' + k][b, i]) / np.abs(ref['g' + k][b]).max()
        print(f'  d L / d {k}[{b}, {i}]: layer {got["g" + k][b, i]:.9g}, central difference {fd:.9g} ({d:.2e})')
        assert d <= 1e-6, (k, d)
    # a [1, n] tensor receives the batch sum
    Q1 = leaf(_diag(c['Q'])[:1])
    L = loss(*forward(Q=Q1, R=_t(_diag(c['R'])), QN=_t(_diag(c['QN']))))
    L.backward()
    Qb = np.tile(c['Q'][:1], (B, 1, 1))
    o1 = pw_solve_ref(c['x0'], c['xref'], c['uref'], c['xbar'], c['ubar'], spec, Qb, c['R'], c['QN'], c['wind'])
    r1 = pw_vjp_ref(c['xbar'], c['ubar'], o1['X'], o1['U'], c['xref'], c['uref'], cX, gU, spec, Qb, c['R'], c['QN'],
                    c['wind'])
    assert tuple(Q1.grad.shape) == (1, 12)
    e = relerr(Q1.grad.cpu().numpy(), _diag(r1['gQ']).sum(axis=0, keepdims=True)).max()
    print(f'  [1, n] tensor: batch sum {e:.2e}')
    assert e <= BOUND['f64']
    # the handle is as it was: its weights version and a plain solve
    assert m._weights_version == version
    after = _solve(m, c, Q=None, R=None, QN=None)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def test_torch_layer_flag_off_is_the_shared_weight_layer():
    B, N = 3, 3
    c = _case(B, N)
    cu0, cX, cU = _loss_weights(B, N)
    res = []
    for kw in ({}, dict(per_instance_weights=False)):
        m = _mpc(N, B)
        leaf = lambda a: _t(a).requires_grad_(True)   # noqa: E731
        x0, xref, uref = leaf(c['x0']), leaf(c['xref']), leaf(c['uref'])
        Q, R = leaf(np.diag(c['Q'][0])), leaf(c['R'][0])
        u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], xref, uref, Q=Q, R=R, **kw)
        ((u0 * _t(cu0)).sum() + (X * _t(cX)).sum() + (U * _t(cU)).sum()).backward()
        torch.cuda.synchronize()
        assert m._weights_version == 1   # installed on the handle, as before
        res.append([v.detach().clone() for v in (u0, X, U, x0.grad, xref.grad, uref.grad, Q.grad, R.grad)])
    assert tuple(res[0][6].shape) == (12,) and tuple(res[0][7].shape) == (4, 4)
    for a, b in zip(*res):
        assert ab.same_bits(a, b)


# ------------------------------------------------------------------------------ 11. the closed loop
def test_closed_loop_with_per_instance_weights():
    """B candidate weightings as one closed-loop batch, against the oracle loop run instance by
    instance with each instance's spec (the bound of test_closed_loop_matches_oracle_fp64)."""
    from mpc_blaster_amd.closed_loop import closed_loop
    from oracle.model import Params
    from oracle.rk4 import rk4_step
    B, N, nsim = 4, 8, 3
    c = _case(B, N)
    spec = OcpSpec(N=N)
    m = _mpc(N, B)
    wts = dict(Q=_diag(c['Q']), R=c['R'], QN=_diag(c['QN']))   # diagonals and a matrix tensor
    Xs, Us, st = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, weights=wts)
    torch.cuda.synchronize()
    xbar, ubar, x = np.zeros((B, N + 1, 12)), np.zeros((B, N, 4)), c['x0'].copy()
    for i in range(nsim):
        o = pw_solve_ref(x, c['xref'], c['uref'], xbar, ubar, spec, c['Q'], c['R'], c['QN'])
        xbar, ubar = o['X'], o['U']
        eu = relerr(Us[:, i].cpu().numpy(), o['u0']).max()
        x = rk4_step(x, o['u0'], spec.dt, Params())
        ex = relerr(Xs[:, i + 1].cpu().numpy(), x).max()
        print(f'  step {i}: u0 {eu:.2e}  x {ex:.2e}')
        assert eu < 1e-8 and ex < 1e-8
    assert (st.cpu().numpy() == 0).all()
    # the weightings do steer the loop apart from the shared-weight one
    Xs0, Us0, _ = closed_loop(m, c['x0'], c['xref'], c['uref'], nsim)
    assert relerr(Us.cpu().numpy(), Us0.cpu().numpy()).min() > 1e-3
    with pytest.raises(ValueError):
        closed_loop(m, c['x0'], c['xref'], c['uref'], nsim, weights=wts, feedback=True)
