"""mpcb_solve_vjp17_sx on the GPU (the 17/6 vector-Jacobian product with active state rows, its
weight gradients) and the torch layer through the state box, against tests/vjp17x_ref.py: the
device is compared with the NumPy references, never with itself.  tests/test_vjp17x_ref_cpu.py
ties those references to each other and to central differences of the oracle's state-box solve,
asserts the input conditions used here (row counts, which instances converge) and fixes the bound.

Metric: per instance and per output |dev - ref|_inf / max(|ref|_inf, 1).  Bound: ``SX_BOUND`` =
2.3e-7, ten times the error of the recursion's NumPy model (penalty 1e8) against the dense KKT
solve.  The reference is ``dense_x`` (no recursion, no penalty) up to N = 20 and ``al_x`` (the
model of the recursion) at N = 60, where the dense solve has lost its digits
(tests/vjp_ref.py).  Each test prints its measured maxima (DESIGN.md records them).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp17_ref as vr    # noqa: E402
import vjp17x_ref as xr   # noqa: E402

from oracle.full import FullSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS, WKEYS = xr.KEYS, xr.WKEYS
BOUND = xr.SX_BOUND
TOL = 1e-6   # state_active_tol = vjp17_ref.ACTIVE_TOL


def _mpc(N, B, dtype='f64', **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=B)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64 if k not in ('status', 'fixed', 'fixed_x') else np.int32)
            for k, v in out.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _synth(B, N):
    c, fixed, fixed_x = xr.synth_case(B, N)
    for v in list(c.values()) + [fixed, fixed_x]:
        v.setflags(write=False)
    return c, fixed, fixed_x


@functools.lru_cache(maxsize=None)
def _synth_ref(B, N):
    c, fixed, fixed_x = _synth(B, N)
    f = xr.dense_x if N <= 17 else xr.al_x
    return f(c['xbar'], c['ubar'], c['p'], fixed, fixed_x, c['gX'], c['gU'], FullSpec(N=N))


@functools.lru_cache(maxsize=None)
def _sbox_ref(B, N):
    spec, c = xr.sbox_case(B, N)
    args = (c['xbar'], c['ubar'], c['p'], c['fixed'], c['fixed_x'], c['gX'], c['gU'], spec)
    return xr.dense_x(*args), xr.al_x(*args)


def _run(m, c, fixed, fixed_x, gX=True, gU=True, **kw):
    return _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'] if gX else None, gU=c['gU'] if gU else None,
                                   fixed=fixed, fixed_x=fixed_x, **kw))


def _check(got, ref, tag, keys=KEYS, rows=None):
    rows = slice(None) if rows is None else rows
    err = {k: vr.relerr(got[k][rows], ref[k][rows]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{BOUND:.1e} (|ref| {np.abs(ref[k][rows]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= BOUND, (tag, k, err[k])
    return err


def _raw(m, c, fixed, fixed_x, gX=True, gU=True, outs=(True, True, True), B=None, fn='mpcb_solve_vjp17_sx',
         xref_sb=0):
    """The entry point itself: the outputs in ``outs`` (gx0, gxref, guref), NULL for the others and for
    the weights; guard values in every array."""
    Bc, N = c['ubar'].shape[:2]
    nx, nu = c['xbar'].shape[-1], c['ubar'].shape[-1]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=m.dtype, device='cuda')   # noqa: E731
    u8 = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.uint8, device='cuda')   # noqa: E731
    xb, ub, gXd, gUd = t(c['xbar']), t(c['ubar']), t(c['gX']), t(c['gU'])
    fx, fxx = u8(fixed), u8(fixed_x)
    o = [torch.full(s, 7.0, dtype=m.dtype, device='cuda') for s in ((Bc, nx), (Bc, N + 1, nx), (Bc, N, nu))]
    st = torch.full((Bc,), -9, dtype=torch.int32, device='cuda')
    P, null = m._ptr, ctypes.c_void_p(0)
    tail = [P(gXd) if gX else null, P(gUd) if gU else null, *[P(a) if w else null for a, w in zip(o, outs)], null, null,
            null, P(st), null]
    if fn == 'mpcb_solve_vjp17_sx':
        rc = m.lib.mpcb_solve_vjp17_sx(m._h, Bc if B is None else B, P(xb), P(ub), P(fx), P(fxx), null, null, null,
                                       xref_sb, null, 0, null, 0, null, 0, null, 0, *tail)
    else:
        rc = m.lib.mpcb_solve_vjp17(m._h, Bc if B is None else B, P(xb), P(ub), P(fx), null, null, null, 0, null, 0, *tail)
    torch.cuda.synchronize()
    return rc, dict(zip(KEYS, (a.cpu().numpy() for a in o)), status=st.cpu().numpy())


# ------------------------------------------------------------------------------ synthetic masks, unboxed handle
@pytest.mark.parametrize('B,N', sorted(xr.SYNTH))
def test_synthetic_masks_match_reference(B, N):
    c, fixed, fixed_x = _synth(B, N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    got = _run(m, c, fixed, fixed_x)
    print(f'rows per instance {fixed_x.sum(axis=(1, 2))}')
    assert np.all(got['status'] == 0), got['status']
    assert np.array_equal(got['fixed_x'].astype(bool), fixed_x) and np.array_equal(got['fixed'].astype(bool), fixed)
    _check(got, _synth_ref(B, N), f'17/6 state rows B={B} N={N} ({"dense_x" if N <= 17 else "al_x"})')
    # no row, in one instance or in all: the plain product
    plain = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], fixed=fixed))
    none = np.flatnonzero(fixed_x.sum(axis=(1, 2)) == 0)
    assert (len(none) == 1) == (N == 3)
    if len(none):
        _check(got, plain, 'the instance without rows against mpcb_solve_vjp17', rows=none)
    zero = _run(m, c, fixed, np.zeros_like(fixed_x))
    assert np.all(zero['status'] == 0)
    _check(zero, plain, 'all-zero mask against mpcb_solve_vjp17')
    # fixed_x = NULL: the kernels of mpcb_solve_vjp17, its bits
    rc, null = _raw(m, c, fixed, None)
    rc2, old = _raw(m, c, fixed, None, fn='mpcb_solve_vjp17')
    assert rc == 0 and rc2 == 0
    for k in KEYS + ('status',):
        assert np.array_equal(null[k], old[k]), k


# ------------------------------------------------------------------------------ end to end on a box_x handle
@functools.lru_cache(maxsize=None)
def _sbox_solved(B, N):
    """The device's state-box solve of the (B, N) draw: (handle, X, U)."""
    spec, c = xr.sbox_case(B, N)
    m = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=c['lbx'], ubx=c['ubx'])
    m.set_params(c['p'])
    m.solve_iterate(c['x0'], c['xbar'].copy(), c['ubar'].copy(), c['xref'].copy(), c['uref'].copy())
    X, U = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    assert (m.get_status().cpu().numpy() == 0).all()
    return m, X, U


def test_state_box_end_to_end():
    B, N = 5, 12
    spec, c = xr.sbox_case(B, N)
    m, X, U = _sbox_solved(B, N)
    mx = m.active_mask17x(X, TOL)
    assert mx.dtype == torch.uint8 and tuple(mx.shape) == (B, N + 1, 17)
    assert np.array_equal(mx.cpu().numpy().astype(bool), c['fixed_x'])          # the oracle's masks, entry for entry
    assert np.array_equal(m.active_mask17(U).cpu().numpy().astype(bool), c['fixed'])
    n = c['fixed_x'].sum(axis=(1, 2))
    print(f'state-box end to end: {n} active state rows, {c["fixed"].sum(axis=(1, 2))} clamped inputs per instance')
    assert n.min() == 28 and n.max() == 32
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, X=X, state_active_tol=TOL))
    assert np.all(got['status'] == 0), got['status']
    assert np.array_equal(got['fixed_x'].astype(bool), c['fixed_x']) and np.array_equal(got['fixed'].astype(bool), c['fixed'])
    _check(got, _sbox_ref(B, N)[0], 'state-box end to end against dense_x')
    free = _run(m, c, c['fixed'], np.zeros_like(c['fixed_x']))
    dif = np.max([vr.relerr(free[k], got[k]) for k in KEYS], axis=0)
    print('against the input-mask-only product, per instance:', np.array2string(dif, precision=2))
    assert (dif > 0.5).all()
    assert _mpc(N, B).active_mask17x(X) is None   # no state box, no mask


def test_stalling_instance_is_maxiter():
    """(8, 20): instance 0's active set is nearly dependent (sigma_min / sigma_max 5.6e-7 of the
    constraint Jacobian); the passes stall at eq 7.3e-6 at any penalty."""
    B, N = 8, 20
    spec, c = xr.sbox_case(B, N)
    dense, al = _sbox_ref(B, N)
    m = _mpc(N, B)   # (the product is exact for the masks it is given, whatever the handle's boxes)
    m.set_params(c['p'])
    got = _run(m, c, c['fixed'], c['fixed_x'])
    print(f'status {got["status"]}, al_x {al["status"]} after {al["passes"]} passes')
    assert np.array_equal(got['status'], al['status']) and got['status'][0] == 2
    _check(got, dense, 'instances 1-7 against dense_x', rows=slice(1, None))


# ------------------------------------------------------------------------------ weight gradients
def _pw(B, seed=17):
    """Per-instance diagonal weights around the defaults."""
    s0 = FullSpec(N=1)
    rng = np.random.default_rng(seed)
    return tuple(np.diag(np.asarray(M, dtype=np.float64))[None] * rng.uniform(0.5, 2.0, (B, np.asarray(M).shape[0]))
                 for M in (s0.Q, s0.R, s0.QN))


@pytest.mark.parametrize('pw', [False, True])
@pytest.mark.parametrize('B,N', [(5, 3), (5, 12)])
def test_weight_gradients_match_reference(B, N, pw):
    if N == 3:
        c, fixed, fixed_x = _synth(B, N)
    else:
        c = xr.sbox_case(B, N)[1]
        fixed, fixed_x = c['fixed'], c['fixed_x']
    X = c['xbar'] + 0.1 * np.random.default_rng(6).standard_normal(c['xbar'].shape)
    U = c['ubar'] + 0.1 * np.random.default_rng(7).standard_normal(c['ubar'].shape) * vr.USCALE
    m = _mpc(N, B)
    m.set_params(c['p'])
    kw = dict(gX=c['gX'], gU=c['gU'], fixed=fixed, fixed_x=fixed_x)
    wkw = dict(X=X, U=U, x_ref=c['xref'][:1], u_ref=c['uref'], weights=True)   # x_ref broadcast
    args = (c['xbar'], c['ubar'], c['p'], fixed, fixed_x, c['gX'], c['gU'])
    rkw = dict(X=X, U=U, xref=c['xref'], uref=c['uref'])
    if pw:
        Q, R, QN = _pw(B)
        refs = [xr.dense_x(*(a[b:b + 1] for a in args), FullSpec(N=N, Q=np.diag(Q[b]), R=np.diag(R[b]), QN=np.diag(QN[b])),
                           **{k: np.broadcast_to(v, (B,) + v.shape[1:])[b:b + 1] for k, v in rkw.items()}) for b in range(B)]
        ref = {k: np.concatenate([r[k] for r in refs]) for k in KEYS + WKEYS}
        got = _np(m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], Q=Q, R=R, QN=QN, **kw, **wkw))
        plain = _np(m.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], Q=Q, R=R, QN=QN, **kw))
    else:
        ref = xr.dense_x(*args, FullSpec(N=N), **rkw)
        got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], **kw, **wkw))
        plain = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], **kw))
    assert np.all(got['status'] == 0), got['status']
    _check(got, ref, f'weights B={B} N={N} per-instance={pw}', KEYS + WKEYS)
    for k in WKEYS:
        assert np.array_equal(got[k], np.swapaxes(got[k], 1, 2)), k      # bitwise symmetric
    for k in KEYS:
        assert np.array_equal(got[k], plain[k]), k                       # the bits of the call without weights


# ------------------------------------------------------------------------------ outputs, chunks, hygiene
def test_one_cotangent_and_gx0_only():
    B, N = 5, 3
    c, fixed, fixed_x = _synth(B, N)
    spec = FullSpec(N=N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    for gX, gU in ((True, False), (False, True)):
        ref = xr.dense_x(c['xbar'], c['ubar'], c['p'], fixed, fixed_x, c['gX'] if gX else None,
                         c['gU'] if gU else None, spec)
        got = _run(m, c, fixed, fixed_x, gX=gX, gU=gU)
        assert np.all(got['status'] == 0)
        _check(got, ref, f'gX {gX} gU {gU}')
    full = _run(m, c, fixed, fixed_x)
    rc, got = _raw(m, c, fixed, fixed_x, outs=(True, False, False))
    assert rc == 0 and np.all(got['status'] == 0)
    assert np.array_equal(got['gx0'], full['gx0'])                       # the same bits as with every output
    assert np.all(got['gxref'] == 7.0) and np.all(got['guref'] == 7.0)   # a NULL output's array is untouched


def test_chunked_run_and_second_call_are_bit_identical(monkeypatch):
    """MPCB_CHUNK = 64 below B = 70: chunks of 64 and 6 instances, the second with a ragged wave.  The
    batch is the synthetic (5, 3) case fourteen times over (random rows at B = 70 include position
    rows one stage ahead that the inputs barely move, and some of those instances do not converge:
    not what this test is about), so instance b also has the bits of instance b mod 5, wherever it
    sits in its wave and chunk."""
    B, N, rep = 70, 3, 14
    c5, f5, fx5 = _synth(5, N)
    tile = lambda a: np.tile(a, (rep,) + (1,) * (a.ndim - 1))   # noqa: E731
    c, fixed, fixed_x = {k: tile(v) for k, v in c5.items()}, tile(f5), tile(fx5)
    X = c['xbar'] + 0.1
    U = c['ubar'] + 0.1 * vr.USCALE
    kw = dict(X=X, U=U, x_ref=c['xref'], u_ref=c['uref'], weights=True)
    m = _mpc(N, B)
    m.set_params(c['p'])
    one, again = _run(m, c, fixed, fixed_x, **kw), _run(m, c, fixed, fixed_x, **kw)
    monkeypatch.setenv('MPCB_CHUNK', '64')
    mc = _mpc(N, B)
    mc.set_params(c['p'])
    two = _run(mc, c, fixed, fixed_x, **kw)
    assert np.all(one['status'] == 0)
    for k in KEYS + WKEYS + ('status',):
        assert np.array_equal(one[k], again[k]), k
        assert np.array_equal(one[k], two[k]), k
        assert np.array_equal(two[k], tile(two[k][:5])), k
    _check(two, {k: tile(v) for k, v in _synth_ref(5, N).items() if k in KEYS}, 'chunked 64 + 6')


@pytest.mark.parametrize('where', ['gX', 'xbar', 'p'])
def test_nan_instance_is_isolated(where):
    B, N = 5, 3
    c, fixed, fixed_x = _synth(B, N)
    X, U = c['xbar'] + 0.1, c['ubar'] + 0.1 * vr.USCALE
    kw = dict(X=X, U=U, x_ref=c['xref'], u_ref=c['uref'], weights=True)
    m = _mpc(N, B)
    m.set_params(c['p'])
    ok = _run(m, c, fixed, fixed_x, **kw)
    d = {k: c[k].copy() for k in ('xbar', 'ubar', 'gX', 'gU', 'p')}
    if where == 'p':
        d['p'][1, 7] = np.nan
    else:
        d[where][1, 2, 3] = np.nan
    m.set_params(d['p'])
    got = _run(m, d, fixed, fixed_x, **kw)
    rest = [0, 2, 3, 4]   # 0, 2 and 3 share the wave of instance 1
    assert got['status'][1] == 1 and np.all(got['status'][rest] == 0)
    for k in KEYS + WKEYS:
        assert np.all(np.isnan(got[k][1])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k     # bit for bit


def test_argument_errors():
    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    assert 'mpcb_solve_vjp17_sx' in _lib.EXPORTS_17 and hasattr(_lib.load(), 'mpcb_solve_vjp17_sx')
    B, N = 2, 3
    c5, f5, fx5 = _synth(5, N)
    c, fixed, fixed_x = {k: v[:B] for k, v in c5.items()}, f5[:B], fx5[:B]

    def refused(m, cc, code, fx=fixed, fxx=fixed_x, **kw):
        rc, got = _raw(m, cc, fx, fxx, **kw)
        assert rc == code, (rc, code)
        assert all(np.all(got[k] == 7.0) for k in KEYS) and np.all(got['status'] == -9)   # nothing written

    m = _mpc(N, B)
    assert _raw(m, c, fixed, fixed_x)[0] == 0
    refused(m, c, -1, gX=False, gU=False)              # no cotangent
    refused(m, c, -1, outs=(False, False, False))      # no output
    refused(m, c, -1, xref_sb=-1)                      # a negative stride
    refused(m, c, -1, B=B + 1)                         # B > max_batch
    m12 = BatchedMPC(MPCConfig(N=N), max_batch=B)
    c12 = dict(xbar=np.zeros((B, N + 1, 12)), ubar=np.zeros((B, N, 4)), gX=np.zeros((B, N + 1, 12)), gU=np.zeros((B, N, 4)))
    refused(m12, c12, -4, fx=None, fxx=np.zeros((B, N + 1, 12), dtype=bool))   # a 12/4 handle
    refused(_mpc(N, B, 'f32'), c, -4)                  # an fp32 handle
    refused(_mpc(N, B, 'f32'), c, -4, fxx=None)        # ... with or without rows
    # every fp64 17/6 handle is accepted, the state-box one too, where NULL means "no row is active"
    lbx, ubx = xr.state_box()
    mx = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=lbx, ubx=ubx)
    assert _raw(mx, c, fixed, fixed_x)[0] == 0 and _raw(mx, c, fixed, None)[0] == 0
    assert _raw(mx, c, fixed, None, fn='mpcb_solve_vjp17')[0] == -4            # the old entry keeps refusing it
    with pytest.raises(ValueError, match='fixed_x'):
        m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], fixed_x=fixed_x[:, :N])
    with pytest.raises(ValueError, match='17/6'):
        m12.solve_iterate_vjp(c12['xbar'], c12['ubar'], gX=c12['gX'], state_active_tol=TOL)


# ------------------------------------------------------------------------------ torch layer
def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda', requires_grad=grad)


def test_torch_layer_directional_derivative():
    """Central difference of a random linear loss in (u0, X) on the device along the direction of
    tests/test_vjp17x_ref_cpu.py in (x0, x_ref), h = 1e-4, per instance, against <grad, d>: within
    1e-5 of it (the bound of the existing directional tests) on the instances whose two masks at +-h
    are those of the centre; the CPU test has all five of this draw stable, at least 3 are required."""
    B, N = 5, 12
    spec, c = xr.sbox_case(B, N)
    m, _, _ = _sbox_solved(B, N)
    rng = np.random.default_rng(22)
    w0, wX = _t(rng.standard_normal((B, 6))), _t(rng.standard_normal((B, N + 1, 17)))
    d0, dr, _ = xr.fd_direction(B, N)

    def loss(scale, grad=False):
        x0, xr_ = _t(c['x0'] + scale * d0, grad), _t(c['xref'] + scale * dr, grad)
        u0, X, U = m.solve_iterate_diff(x0, c['xbar'].copy(), c['ubar'].copy(), xr_, c['uref'].copy(),
                                        state_active_tol=TOL)
        assert (m.get_status() == 0).all()
        masks = (m.active_mask17(U.detach()).cpu().numpy().astype(bool),
                 m.active_mask17x(X.detach(), TOL).cpu().numpy().astype(bool))
        return (w0 * u0).sum(dim=1) + (wX * X).sum(dim=(1, 2)), (x0, xr_), masks

    L, (x0, xr_), masks = loss(0.0, True)
    assert np.array_equal(masks[0], c['fixed']) and np.array_equal(masks[1], c['fixed_x'])
    L.sum().backward()
    lin = (x0.grad * _t(d0)).sum(dim=1) + (xr_.grad * _t(dr)).sum(dim=(1, 2))
    Lp, _, mp = loss(xr.FD_H)
    Lm, _, mm = loss(-xr.FD_H)
    stable = np.ones(B, dtype=bool)
    for a in (mp, mm):
        stable &= (a[0] == masks[0]).all(axis=(1, 2)) & (a[1] == masks[1]).all(axis=(1, 2))
    fd = ((Lp - Lm) / (2.0 * xr.FD_H)).detach().cpu().numpy()
    lin = lin.cpu().numpy()
    rel = np.abs(fd - lin) / np.abs(lin)
    print(f'directional, per instance: FD {fd}  <grad, d> {lin}  relative difference '
          f'{np.array2string(rel, precision=2)}  stable masks {stable.astype(int)}')
    assert stable.sum() >= 3
    assert (rel[stable] <= 1e-5).all()


def test_closed_loop_diff_through_the_state_box():
    """Two steps at B = 3, N = 8 (warm_start=False) against the gradient chained from the references
    (tests/vjp17x_ref.py loop_case): 10 x SX_BOUND.  Instance 1's first solve has a nearly dependent
    active set: the product reports MAXITER there and the layer passes no gradient through it, as
    the reference does."""
    from mpc_blaster_amd.closed_loop import closed_loop_diff
    L = xr.loop_case()
    c, w = L['c'], L['w']
    B, N, nsim = xr.LOOP_B, xr.LOOP_N, xr.LOOP_NSIM
    m = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=L['spec'].lbx, ubx=L['spec'].ubx)
    m.set_params(c['p'])
    leaves = {k: _t(c[k], True) for k in ('x0', 'xref', 'uref')}
    X, U, st = closed_loop_diff(m, leaves['x0'], leaves['xref'], leaves['uref'], nsim, _t(c['xbar']), _t(c['ubar']),
                                warm_start=False, state_active_tol=TOL)
    assert int(st.max()) == 0
    ex = float(vr.relerr(X.detach().cpu().numpy(), L['X']).max())
    eu = float(vr.relerr(U.detach().cpu().numpy(), L['U']).max())
    print(f'closed_loop_diff with the state box: X_sim against the oracle {ex:.2e}, U_sim {eu:.2e} / 1e-9')
    assert ex <= 1e-9 and eu <= 1e-9
    (_t(w) * X).sum().backward()
    for k in ('x0', 'xref', 'uref'):
        e = float(vr.relerr(leaves[k].grad.cpu().numpy(), L['grad'][k]).max())
        print(f'closed_loop_diff with the state box: gradient of {k} against the chained reference '
              f'{e:.2e}/{10 * BOUND:.1e}')
        assert e <= 10 * BOUND


def test_calls_without_the_new_arguments_still_refuse():
    from mpc_blaster_amd import _lib
    from mpc_blaster_amd.closed_loop import closed_loop_diff
    B, N = 3, 3
    c = {k: v[:B].copy() for k, v in _synth(5, N)[0].items()}
    lbx, ubx = xr.state_box()
    mx = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=lbx, ubx=ubx)
    with pytest.raises(ValueError, match='does not cover the 17/6 state box'):
        mx.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    with pytest.raises(ValueError, match='does not cover the 17/6 state box'):
        mx.solve_iterate_diff_pw17(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    with pytest.raises(ValueError, match='does not cover the 17/6 state box'):
        closed_loop_diff(mx, _t(c['x0']), _t(c['xref']), _t(c['uref']), 1, _t(c['xbar']), _t(c['ubar']))
    with pytest.raises(_lib.MpcbError, match='-4'):
        mx.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], U=c['ubar'])
    with pytest.raises(_lib.MpcbError, match='-4'):
        mx.solve_iterate_vjp_pw17(c['xbar'], c['ubar'], gX=c['gX'], U=c['ubar'])
    m = _mpc(N, B)   # and an unboxed handle returns no fixed_x key
    assert 'fixed_x' not in m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'])
