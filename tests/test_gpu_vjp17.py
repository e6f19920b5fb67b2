"""mpcb_solve_vjp17 on the GPU (the vector-Jacobian product and the weight gradients of one 17/6
solve_iterate step) and the torch layer over it, against tests/vjp17_ref.py: the device is compared
with the NumPy reference, never with itself.  tests/test_vjp17_ref_cpu.py ties that reference to
the condensed dense solve and to finite differences of the oracle, unboxed and boxed.

Metric: per instance and per output |dev - ref|_inf / max(|ref|_inf, 1).  Bounds: fp64 1e-9 (the
bound of the 12/4 product and of every fp64 17/6 solve test), fp32 5e-4 (the bound the project
holds the fp32 17/6 solve to); in fp32 the reference reads the data and weights as the fp32 handle
holds them.  Each test prints its measured maxima (DESIGN.md records them).

The active set is an argument of the entry point: synthetic masks (about half of the components
clamped, a fully clamped stage, an empty mask) exercise the kernel, and the end-to-end case takes
the mask by tolerance from the device's own boxed solve and holds it to the oracle's, entry for
entry.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
import vjp17_ref as vr   # noqa: E402

from oracle.full import FullSpec, mpc_solve17   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS, WKEYS = vr.KEYS, vr.WKEYS
BOUND = {'f64': 1e-9, 'f32': 5e-4}
SHAPES = [(1, 1), (5, 3), (7, 17), (3, 60)]   # one stage + three padding groups; a ragged second
                                             # wave; more stages than lanes; the reference horizon


def _mpc(N, B, dtype='f64', **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=B)


@functools.lru_cache(maxsize=None)
def _case(B, N):
    c = vr.vjp17_case(B, N)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _mask(B, N):
    m = vr.random_mask(B, N)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref(B, N, masked):
    c = _case(B, N)
    return vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], _mask(B, N) if masked else None, c['gX'], c['gU'],
                        FullSpec(N=N))


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64 if k not in ('status', 'fixed') else np.int32)
            for k, v in out.items() if v is not None}


def _check(got, ref, dtype, tag, keys=KEYS):
    assert np.all(got['status'] == 0), (tag, got['status'])
    err = {k: vr.relerr(got[k], ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{BOUND[dtype]:.0e} (|ref| {np.abs(ref[k]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= BOUND[dtype], (tag, k, err[k])
    return err


def _run(m, c, fixed=None, gX=True, gU=True, **kw):
    return _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'] if gX else None, gU=c['gU'] if gU else None,
                                   fixed=fixed, **kw))


# ------------------------------------------------------------------------------ fp64 against the reference
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('B,N', SHAPES)
def test_vjp17_fp64_matches_reference(B, N, masked):
    c = _case(B, N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    got = _run(m, c, _mask(B, N) if masked else None)
    _check(got, _ref(B, N, masked), 'f64', f'17/6 fp64 B={B} N={N} masked={masked}')
    if masked:
        assert np.all(got['guref'][_mask(B, N)] == 0.0)   # diagonal R: a clamped component's guref is 0


def test_fully_masked_stage_and_empty_mask_in_one_batch():
    B, N = 5, 3
    c = _case(B, N)
    fixed = _mask(B, N).copy()
    fixed[1, 1] = True      # a stage with all six components clamped
    fixed[2] = False        # an instance with nothing clamped
    m = _mpc(N, B)
    m.set_params(c['p'])
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], FullSpec(N=N))
    got = _run(m, c, fixed)
    _check(got, ref, 'f64', 'fully masked stage / empty mask')
    assert np.all(got['guref'][1, 1] == 0.0)
    assert np.array_equal(got['gx0'][2], _run(m, c, None)['gx0'][2])   # ... is the unmasked product, bit for bit


@pytest.mark.parametrize('kind', ['stage', 'row'])
def test_parameters_by_stage_and_broadcast(kind):
    B, N = 5, 3
    c = _case(B, N)
    rng = np.random.default_rng(31)
    if kind == 'stage':   # [B, N, 25]: another vector on every stage of every instance
        p = np.repeat(c['p'][:, None, :], N, axis=1)
        p[..., :24] = rng.uniform(-0.5, 0.5, (B, N, 24))
    else:                 # one row for the whole batch
        p = c['p'][3].copy()
    m = _mpc(N, B)
    m.set_params(p)
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], p, _mask(B, N), c['gX'], c['gU'], FullSpec(N=N))
    _check(_run(m, c, _mask(B, N)), ref, 'f64', f'parameters {kind}')
    if kind == 'stage':   # B beyond the array's instance rows
        m2 = _mpc(N, B)
        m2.set_params(p[:3])
        from mpc_blaster_amd._lib import MpcbError
        with pytest.raises(MpcbError, match='-1'):
            _run(m2, c)


def test_alt_definition():
    """Dense symmetric Q / R / QN, cost_scale != dt, other mass and inertia (tests/alt_config.py ALT-b)."""
    B, N = 5, 3
    kw = ac.fields(full=True, alt='b', groups=('weights', 'model', 'time'), box='none')
    spec = FullSpec(N=N, **ac.spec_kwargs(kw))
    assert spec.s != spec.dt
    c = vr.vjp17_case(B, N, spec)
    fixed = _mask(B, N)
    X = c['xbar'] + 0.1 * np.random.default_rng(6).standard_normal(c['xbar'].shape)
    U = c['ubar'] + 0.1 * np.random.default_rng(7).standard_normal(c['ubar'].shape) * vr.USCALE
    m = _mpc(N, B, **kw)
    m.set_params(c['p'])
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec, X=X, U=U, xref=c['xref'],
                       uref=c['uref'])
    got = _run(m, c, fixed, X=X, U=U, x_ref=c['xref'], u_ref=c['uref'], weights=True)
    _check(got, ref, 'f64', 'ALT-b definition', KEYS + WKEYS)
    assert np.any(got['guref'][fixed] != 0.0)   # dense R: row m of s R du on a clamped component


def _raw(m, c, fixed=None, gX=True, gU=True, outs=(True, True, True), B=None):
    """The entry point itself: the outputs in ``outs`` (gx0, gxref, guref), NULL for the others."""
    Bc, N = c['ubar'].shape[:2]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=m.dtype, device='cuda')   # noqa: E731
    xb, ub, gXd, gUd = t(c['xbar']), t(c['ubar']), t(c['gX']), t(c['gU'])
    fx = None if fixed is None else torch.tensor(np.ascontiguousarray(fixed), dtype=torch.uint8, device='cuda')
    o = [torch.full(s, 7.0, dtype=m.dtype, device='cuda') for s in ((Bc, 17), (Bc, N + 1, 17), (Bc, N, 6))]
    st = torch.full((Bc,), -9, dtype=torch.int32, device='cuda')
    P, null = m._ptr, ctypes.c_void_p(0)
    rc = m.lib.mpcb_solve_vjp17(m._h, Bc if B is None else B, P(xb), P(ub), P(fx), null, null, null, 0, null, 0,
                                P(gXd) if gX else null, P(gUd) if gU else null,
                                *[P(a) if w else null for a, w in zip(o, outs)], null, null, null, P(st), null)
    torch.cuda.synchronize()
    return rc, dict(zip(KEYS, (a.cpu().numpy() for a in o)), status=st.cpu().numpy())


def test_one_cotangent_and_one_output():
    B, N = 5, 3
    c = _case(B, N)
    spec = FullSpec(N=N)
    fixed = _mask(B, N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    for gX, gU in ((True, False), (False, True)):
        ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'] if gX else None, c['gU'] if gU else None, spec)
        _check(_run(m, c, fixed, gX=gX, gU=gU), ref, 'f64', f'gX {gX} gU {gU}')
    full = _run(m, c, fixed)
    for i, k in enumerate(KEYS):
        outs = tuple(j == i for j in range(3))
        rc, got = _raw(m, c, fixed, outs=outs)
        assert rc == 0 and np.all(got['status'] == 0)
        assert np.array_equal(got[k], full[k]), k                    # the same bits as with every output
        for j, other in enumerate(KEYS):
            assert j == i or np.all(got[other] == 7.0), other        # a NULL output's array is untouched


def test_chunked_run_is_bit_identical(monkeypatch):
    """MPCB_CHUNK = 64 below B = 70: chunks of 64 and 6 instances, the second with a ragged wave."""
    B, N = 70, 3
    c = _case(B, N)
    fixed = _mask(B, N)
    X = c['xbar'] + 0.1
    U = c['ubar'] + 0.1 * vr.USCALE
    kw = dict(X=X, U=U, x_ref=c['xref'], u_ref=c['uref'], weights=True)
    m = _mpc(N, B)
    m.set_params(c['p'])
    one = _run(m, c, fixed, **kw)
    monkeypatch.setenv('MPCB_CHUNK', '64')
    mc = _mpc(N, B)
    mc.set_params(c['p'])
    two = _run(mc, c, fixed, **kw)
    for k in KEYS + WKEYS + ('status',):
        assert np.array_equal(one[k], two[k]), k
    _check(two, _ref(B, N, True), 'f64', 'chunked 64 + 6')


# ------------------------------------------------------------------------------ fp32
def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize('masked', [False, True])
def test_vjp17_fp32(masked):
    B, N = 7, 17
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    spec = FullSpec(N=N)
    spec.Q, spec.R, spec.QN, spec.cost_scale = _f32(spec.Q), _f32(spec.R), _f32(spec.QN), float(np.float32(spec.s))
    fixed = _mask(B, N) if masked else None
    m = _mpc(N, B, 'f32')
    m.set_params(c['p'])
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec)
    _check(_run(m, c, fixed), ref, 'f32', f'17/6 fp32 B={B} N={N} masked={masked}')


# ------------------------------------------------------------------------------ end to end with the box
def test_vjp17_box_end_to_end():
    spec, c = vr.boxed_case()
    B, N = c['ubar'].shape[:2]
    o = mpc_solve17(c['x0'], c['xref'], c['uref'], spec, c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    assert (o['status'] == 0).all()
    fixed, _ = vr.active_mask(o['U'], spec)
    m = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17)
    m.set_params(c['p'])
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    U = m.get_input_trajectory()
    assert (m.get_status().cpu().numpy() == 0).all()
    assert m.active_mask17(U).dtype == torch.uint8
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U))   # active_tol: 1e-6
    print(f'box end to end: {fixed.sum()} of {fixed.size} components clamped')
    assert np.array_equal(got['fixed'].astype(bool), fixed)       # the oracle's mask, entry for entry
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec)
    _check(got, ref, 'f64', 'box end to end')
    free = _run(m, c, np.zeros_like(fixed))
    dif = np.max([vr.relerr(free[k], got[k]) for k in KEYS], axis=0)
    print('masked against unmasked product, per instance:', np.array2string(dif, precision=2))
    assert (dif > 0.5).all()


# ------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('B,N', [(5, 3), (3, 60)])
def test_weight_gradients_match_reference(B, N, masked):
    c = _case(B, N)
    fixed = _mask(B, N) if masked else None
    X = c['xbar'] + 0.1 * np.random.default_rng(6).standard_normal(c['xbar'].shape)
    U = c['ubar'] + 0.1 * np.random.default_rng(7).standard_normal(c['ubar'].shape) * vr.USCALE
    m = _mpc(N, B)
    m.set_params(c['p'])
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], FullSpec(N=N), X=X, U=U,
                       xref=c['xref'], uref=c['uref'])
    got = _run(m, c, fixed, X=X, U=U, x_ref=c['xref'][:1], u_ref=c['uref'], weights=True)   # x_ref broadcast
    _check(got, ref, 'f64', f'weights B={B} N={N} masked={masked}', KEYS + WKEYS)
    for k in WKEYS:
        assert np.array_equal(got[k], np.swapaxes(got[k], 1, 2)), k      # bitwise symmetric
    plain = _run(m, c, fixed)
    for k in KEYS:
        assert np.array_equal(got[k], plain[k]), k                       # the bits of the call without weights


# ------------------------------------------------------------------------------ hygiene
def test_two_calls_are_bit_identical():
    B, N = 7, 17
    c = _case(B, N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    a, b = _run(m, c, _mask(B, N)), _run(m, c, _mask(B, N))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('where', ['gX', 'xbar', 'p'])
def test_nan_instance_is_isolated(where):
    B, N = 5, 3
    c = _case(B, N)
    X, U = c['xbar'] + 0.1, c['ubar'] + 0.1 * vr.USCALE
    kw = dict(X=X, U=U, x_ref=c['xref'], u_ref=c['uref'], weights=True)
    m = _mpc(N, B)
    m.set_params(c['p'])
    ok = _run(m, c, _mask(B, N), **kw)
    d = {k: c[k].copy() for k in ('xbar', 'ubar', 'gX', 'gU', 'p')}
    if where == 'p':
        d['p'][1, 7] = np.nan
    else:
        d[where][1, 2, 3] = np.nan
    m.set_params(d['p'])
    got = _run(m, d, _mask(B, N), **kw)
    rest = [0, 2, 3, 4]   # 0, 2 and 3 share the wave of instance 1
    assert got['status'][1] == 1 and np.all(got['status'][rest] == 0)
    for k in KEYS + WKEYS:
        assert np.all(np.isnan(got[k][1])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k     # bit for bit


def test_indefinite_masked_hessian_is_qp_fail():
    B, N = 5, 3
    c = _case(B, N)
    R = np.diag([0.05] * 4 + [1e-5] * 2)
    R[0, 0] = -1e4
    m = _mpc(N, B, R=R)
    m.set_params(c['p'])
    fixed = np.zeros((B, N, 6), dtype=bool)
    fixed[..., 1] = True
    assert np.all(_run(m, c, fixed)['status'] == 4)       # channel 0 is free on every stage
    fixed[..., 0] = True
    assert np.all(_run(m, c, fixed)['status'] == 0)       # ... and masked out, the rest is positive definite


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from mpc_blaster_amd import BatchedMPC, MPCConfig, _lib
    assert 'mpcb_solve_vjp17' in _lib.EXPORTS_17 and all(hasattr(_lib.load(), n) for n in _lib.EXPORTS_17)
    B, N = 2, 3
    c = _case(5, N)
    c2 = {k: v[:B] for k, v in c.items()}
    m = _mpc(N, B)
    before = m.workspace_bytes
    assert _raw(m, c2)[0] == 0
    assert m.workspace_bytes == before                                   # the call's workspace is its own
    assert _raw(m, c2, gX=False, gU=False)[0] == -1                      # no cotangent
    assert _raw(m, c2, outs=(False, False, False))[0] == -1              # no output
    c3 = {k: v[:B + 1] for k, v in c.items()}
    assert _raw(m, c3, B=B + 1)[0] == -1                                 # B > max_batch
    # a weight output without X
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    P, null = m._ptr, ctypes.c_void_p(0)
    st = torch.zeros(B, dtype=torch.int32, device='cuda')
    a = dict(xb=d(B, N + 1, 17), ub=d(B, N, 6), g=d(B, N + 1, 17), gQ=d(B, 17, 17), U=d(B, N, 6), xr=d(B, N + 1, 17),
             ur=d(B, N, 6))
    rc = m.lib.mpcb_solve_vjp17(m._h, B, P(a['xb']), P(a['ub']), null, null, P(a['U']), P(a['xr']), (N + 1) * 17,
                                P(a['ur']), N * 6, P(a['g']), null, null, null, null, P(a['gQ']), null, null, P(st), null)
    assert rc == -1 and b'X' in m.lib.mpcb_last_error()
    m12 = BatchedMPC(MPCConfig(N=N), max_batch=B)
    c12 = dict(xbar=np.zeros((B, N + 1, 12)), ubar=np.zeros((B, N, 4)), gX=np.zeros((B, N + 1, 12)), gU=np.zeros((B, N, 4)))
    assert _raw(m12, c12)[0] == -4                                       # a 12/4 handle
    mx = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=ac.SB_LO, ubx=ac.SB_HI)
    assert _raw(mx, c2)[0] == -4                                         # a handle with the state box
    with pytest.raises(_lib.MpcbError):
        m.solve_iterate_vjp(c2['xbar'], c2['ubar'], gX=c2['gX'], wind=np.zeros((B, 3)))
    # the existing entry points keep refusing the 17/6 model (tests/test_gpu_vjp.py pins it too)
    assert m.lib.mpcb_solve_vjp(m._h, B, P(a['xb']), P(a['ub']), null, null, 0, P(a['g']), null, P(d(B, 17)), null,
                                null, P(st), null) == -4


# ------------------------------------------------------------------------------ torch layer
def _t(a, grad=False):
    return torch.tensor(a, dtype=torch.float64, device='cuda', requires_grad=grad)


@pytest.mark.parametrize('bcast', [True, False])
def test_torch_layer_gradients(bcast):
    B, N = 3, 3
    c = _case(B, N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    rng = np.random.default_rng(11)
    w0, wX = rng.standard_normal((B, 6)), rng.standard_normal((B, N + 1, 17))
    x0, xref, uref = _t(c['x0'], True), _t(c['xref'][:1] if bcast else c['xref'], True), _t(c['uref'], True)
    u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], xref, uref)
    assert (m.get_status() == 0).all()
    ((_t(w0) * u0).sum() + (_t(wX) * X).sum()).backward()
    gU = np.zeros((B, N, 6))
    gU[:, 0] = w0
    ref = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], None, wX, gU, FullSpec(N=N))
    if bcast:
        ref['gxref'] = ref['gxref'].sum(axis=0, keepdims=True)
    got = dict(gx0=x0.grad.cpu().numpy(), gxref=xref.grad.cpu().numpy(), guref=uref.grad.cpu().numpy(),
               status=np.zeros(B, dtype=np.int32))
    assert got['gxref'].shape == ((1 if bcast else B), N + 1, 17)
    _check(got, ref, 'f64', f'torch layer B=3 N=3 broadcast={bcast}')


def test_torch_layer_directional_derivative():
    """Central difference of L on the device along a random direction in the log-weights (Q, R and QN
    at once), relative step 1e-4, against <grad, d>: within 1e-5 of it (the 12/4 layer's test)."""
    B, N = 3, 3
    c = {k: v.copy() for k, v in _case(B, N).items()}   # (writable: the layer makes tensors of them)
    spec = FullSpec(N=N)
    m = _mpc(N, B)
    m.set_params(c['p'])
    rng = np.random.default_rng(22)
    w0, wX = _t(rng.standard_normal((B, 6))), _t(rng.standard_normal((B, N + 1, 17)))
    th = [np.log(np.diag(np.asarray(M, dtype=np.float64))) for M in (spec.Q, spec.R, spec.QN)]
    d = [rng.standard_normal(v.shape) for v in th]

    def loss(scale, grad=False):
        ws = [_t(np.exp(t + scale * dd), grad) for t, dd in zip(th, d)]
        u0, X, _ = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=ws[0], R=ws[1], QN=ws[2])
        assert (m.get_status() == 0).all()
        return (w0 * u0).sum() + (wX * X).sum(), ws

    L, ws = loss(0.0, True)
    L.backward()
    lin = sum(float((w.grad * w.detach() * _t(dd)).sum()) for w, dd in zip(ws, d))
    h = 1e-4
    fd = (float(loss(h)[0]) - float(loss(-h)[0])) / (2.0 * h)
    print(f'directional: FD {fd:.12g}  <grad, d> {lin:.12g}  relative difference {abs(fd - lin) / abs(lin):.2e}')
    assert abs(fd - lin) <= 1e-5 * abs(lin)
    # the stale-weights refusal of the 12/4 layer
    q = _t(np.exp(th[0]), True)
    u0, X, U = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=q)
    m.set_weights(Q=2.0 * q)
    with pytest.raises(RuntimeError, match='weights'):
        X.sum().backward()


def test_torch_layer_refusals():
    B, N = 3, 3
    c = {k: v.copy() for k, v in _case(B, N).items()}
    m32 = _mpc(N, B, 'f32', lbu=vr.LBU17, ubu=vr.UBU17)
    with pytest.raises(ValueError, match='active_tol'):
        m32.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    with pytest.raises(ValueError, match='active_tol'):
        m32.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], U=c['ubar'])
    mx = _mpc(N, B, lbu=vr.LBU17, ubu=vr.UBU17, lbx=ac.SB_LO, ubx=ac.SB_HI)
    with pytest.raises(ValueError, match='state box'):
        mx.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
