"""mpcb_solve_vjp_w (the weight gradients gQ, gR, gQN of one solve_iterate step), mpcb_set_weights
and the torch layer over both, on the GPU.  The device is compared with tests/vjp_weights_ref.py,
never with itself; tests/test_vjp_weights_ref_cpu.py ties that reference to finite differences of
the oracle.

Metric and fp64 bound of tests/test_gpu_vjp.py: per instance and output
|dev - ref|_inf / max(|ref|_inf, 1) <= 1e-9.  fp32: gx0, gxref and guref keep 5e-5.  For gQ, gR and
gQN that bound does not fit: gR sums du_k (U_k - uref_k)' with |gR| in the hundreds, and the
difference U - uref cancels, so rounding the data alone moves the fp64 reference by more than 1e-5.
Each fp32 case therefore measures, on the reference alone, its move (in the test metric) under a
relative +-2^-22 perturbation with seeded signs of every input and of X and U (clamped components
stay on their bound: the bounds are fp32 numbers), and bounds the device by max(5e-5, 10 x move) per
output; it prints move, bound and error.  fp32 cases stay at N <= 20.

X and U are inputs of the product.  Unless a case says otherwise they are the oracle's solve of the
case (so the residuals are those of a real step); the synthetic-mask cases take a clipped random U,
as tests/test_gpu_vjp.py does, and X = xbar + 0.05 N(0, 1).

mpcb_set_weights: every handle configuration of tests/test_gpu_config.py's path table, one 17/6
handle and handles that went through set_t_blast are created with weights A, given weights B and
compared, with torch.equal, with a handle created with B.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402
from vjp_weights_ref import KEYS as WKEYS, vjp_weights_ref   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from test_gpu_vjp import BOUND, KEYS, LB, UB, _f32, _mpc, _np, _spec32, _synthetic_U, relerr   # noqa: E402

ALL = KEYS + WKEYS


@functools.lru_cache(maxsize=None)
def _case(B, N, ref='hover', wind=False, box=False):
    """vjp_case plus the oracle's solve of it (X, U); never modified."""
    spec = OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None)
    c = vjp_case(B, N, spec, ref, wind)
    o = mpc_solve(c['x0'], c['xref'], c['uref'], spec, wind=c['wind'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    return dict(c, X=o['X'], U=o['U'])


def _synthetic_X(c, seed=5):
    return c['xbar'] + 0.05 * np.random.default_rng(seed).standard_normal(c['xbar'].shape)


def _run(m, c, X, U, xref, uref, wind=None):
    """The new entry point's outputs; on the way, the old ones from the plain entry point."""
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, wind=wind, X=X, x_ref=xref,
                                  u_ref=uref, weights=True))
    old = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, wind=wind))
    for k in KEYS + ('status',):
        assert np.array_equal(got[k], old[k]), k            # bit for bit what mpcb_solve_vjp returns
    for k in WKEYS:
        assert np.array_equal(got[k], np.swapaxes(got[k], 1, 2)), k   # bitwise symmetric
    return got


def _check(got, ref, dtype, tag, bound=None):
    assert np.all(got['status'] == 0), (tag, got['status'])
    bound = dict({k: BOUND[dtype] for k in ALL}, **(bound or {}))
    err = {k: relerr(got[k], ref[k]).max() for k in ALL}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{bound[k]:.1e} (|ref| {np.abs(ref[k]).max():.3g})' for k in ALL))
    for k in ALL:
        assert err[k] <= bound[k], (tag, k, err[k], bound[k])
    return err


# ------------------------------------------------------------------------------ fp64, unconstrained
@pytest.mark.parametrize('B,N,wind,ref,bcast', [
    (1, 1, False, 'hover', False), (7, 3, True, 'sine', False), (5, 64, False, 'hover', True)])
def test_weights_fp64_matches_reference(B, N, wind, ref, bcast):
    """(7, 3): wind and sine references with per-instance strides; (5, 64): one reference row for
    the whole batch (stride 0)."""
    c = _case(B, N, ref, wind)
    xref, uref = (c['xref'][:1], c['uref'][:1]) if bcast else (c['xref'], c['uref'])
    if ref == 'sine':
        assert np.abs(c['xref'][0] - c['xref'][1]).max() > 1e-3   # per-instance references do differ
    r = vjp_weights_ref(c['xbar'], c['ubar'], c['X'], c['U'], xref, uref, c['gX'], c['gU'], OcpSpec(N=N), c['wind'])
    m = _mpc(N, B)
    _check(_run(m, c, c['X'], c['U'], xref, uref, c['wind']), r, 'f64', f'fp64 B={B} N={N} wind={wind} ref={ref} bcast={bcast}')


def test_weights_stride_over_slots(monkeypatch):
    """More waves than workspace slots: the stride loop reuses a slot and the LDS of the symmetrisation."""
    B, N = 37, 3
    c = _case(B, N)
    r = vjp_weights_ref(c['xbar'], c['ubar'], c['X'], c['U'], c['xref'], c['uref'], c['gX'], c['gU'], OcpSpec(N=N))
    monkeypatch.setenv('MPCB_VJP_SLOTS', '3')
    m = _mpc(N, B)
    _check(_run(m, c, c['X'], c['U'], c['xref'], c['uref']), r, 'f64', 'fp64 B=37 N=3, 3 slots')


# ------------------------------------------------------------------------------ fp64, input box
@pytest.mark.parametrize('B,N', [(7, 8), (3, 64)])
def test_weights_fp64_box_synthetic_mask(B, N):
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    U, X = _synthetic_U(c, spec), _synthetic_X(c)
    r = vjp_weights_ref(c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'], spec)
    assert r['fixed'].mean() > 0.2
    if N > 33:
        assert r['fixed'][:, 32:].any() and r['fixed'][:, N - 1].any()   # both words of the stage mask
    m = _mpc(N, B, lbu=LB, ubu=UB)
    got = _run(m, c, X, U, c['xref'], c['uref'])
    _check(got, r, 'f64', f'fp64 box synthetic B={B} N={N} ({r["fixed"].mean():.0%} clamped)')
    # the box is not ignored
    free = vjp_weights_ref(c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'], spec, boxed=False)
    for k in WKEYS:
        assert relerr(got[k], free[k]).max() > 1e-3, k


def test_weights_fp64_box_end_to_end():
    """X and U from the device's own solve: its clamped components carry the bound itself."""
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    X, U = m.get_state_trajectory().clone(), m.get_input_trajectory().clone()
    torch.cuda.synchronize()
    assert np.all(m.get_status().cpu().numpy() == 0)
    Xh, Uh = X.cpu().numpy(), U.cpu().numpy()
    clamped = ((Uh <= LB) | (Uh >= UB)).any(axis=(1, 2))
    print(f'end to end: {clamped.sum()} of {B} instances with a clamped component')
    assert clamped.sum() >= 8
    r = vjp_weights_ref(c['xbar'], c['ubar'], Xh, Uh, c['xref'], c['uref'], c['gX'], c['gU'], spec)
    _check(_run(m, c, X, U, c['xref'], c['uref']), r, 'f64', 'fp64 box end to end')


# ------------------------------------------------------------------------------ fp32 bound
def _fp32_bound(args, spec, wind, fixed):
    """{gQ, gR, gQN: max(5e-5, 10 x move)}: the reference's move under a relative +-2^-22
    perturbation, seeded signs, of xbar, ubar, X, U, xref, uref, gX, gU and wind."""
    rng = np.random.default_rng(0)
    pert = lambda a: a * (1.0 + 2.0 ** -22 * rng.choice([-1.0, 1.0], size=a.shape))   # noqa: E731
    ref = vjp_weights_ref(*args, spec, wind)
    q = [pert(np.asarray(a, dtype=np.float64)) for a in args]
    if fixed is not None:
        q[3] = np.where(fixed, args[3], q[3])   # U: a clamped component stays on its bound
    moved = vjp_weights_ref(*q, spec, None if wind is None else pert(wind))
    assert np.array_equal(moved['fixed'], ref['fixed'])
    move = {k: relerr(moved[k], ref[k]).max() for k in WKEYS}
    bound = {k: max(BOUND['f32'], 10.0 * move[k]) for k in WKEYS}
    print('  fp32 bound: ' + '  '.join(f'{k} move {move[k]:.2e} -> bound {bound[k]:.2e}' for k in WKEYS))
    return ref, bound


@pytest.mark.parametrize('B,N,box', [(7, 20, False), (7, 8, True)])
def test_weights_fp32(B, N, box):
    spec = _spec32(OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None))
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    U = _f32(_synthetic_U(c, spec)) if box else c['U']
    X = _f32(_synthetic_X(c)) if box else c['X']
    args = (c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'])
    fixed = ((U <= spec.lbu) | (U >= spec.ubu)) if box else None
    r, bound = _fp32_bound(args, spec, None, fixed)
    m = _mpc(N, B, 'f32', **(dict(lbu=LB, ubu=UB) if box else {}))
    _check(_run(m, c, X, U, c['xref'], c['uref']), r, 'f32', f'fp32 B={B} N={N} box={box}', bound)


# ------------------------------------------------------------------------------ another problem definition
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_weights_alt_definition(dtype):
    """Dense weights, another model, cost_scale != dt, per-channel bounds (tests/alt_config.py 'b'),
    with wind and the box."""
    B, N = 7, 8
    kw = ac.fields(alt='b', box='input', dtype=dtype)
    spec = OcpSpec(N=N, **ac.spec_kwargs(kw))
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    c = {k: cast(v) for k, v in vjp_case(B, N, spec, wind=True).items()}
    U, X = cast(_synthetic_U(c, spec)), cast(_synthetic_X(c))
    args = (c['xbar'], c['ubar'], X, U, c['xref'], c['uref'], c['gX'], c['gU'])
    fixed = (U <= spec.lbu) | (U >= spec.ubu)
    assert fixed.mean() > 0.2
    if dtype == 'f32':
        r, bound = _fp32_bound(args, spec, c['wind'], fixed)
    else:
        r, bound = vjp_weights_ref(*args, spec, c['wind']), None
    assert np.array_equal(r['fixed'], fixed)
    m = _mpc(N, B, dtype, **kw)
    _check(_run(m, c, X, U, c['xref'], c['uref'], c['wind']), r, dtype, f'ALT-b box {dtype}', bound)


# ------------------------------------------------------------------------------ determinism, NaN
@pytest.mark.parametrize('box', [False, True])
def test_two_calls_are_bit_identical(box):
    B, N = 7, 8
    c = _case(B, N)
    U = _synthetic_U(c, OcpSpec(N=N, lbu=LB, ubu=UB)) if box else c['U']
    m = _mpc(N, B, **(dict(lbu=LB, ubu=UB) if box else {}))
    a = _run(m, c, c['X'], U, c['xref'], c['uref'])
    b = _run(m, c, c['X'], U, c['xref'], c['uref'])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('where', ['X', 'uref'])
def test_nan_instance_is_isolated(where):
    B, N = 7, 8
    c = _case(B, N)
    m = _mpc(N, B)
    call = lambda d: _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=c['U'], X=d['X'],   # noqa: E731
                                             x_ref=c['xref'], u_ref=d['uref'], weights=True))
    ok = call(c)
    d = {k: c[k].copy() for k in ('X', 'uref')}
    d[where][2, 5, 3] = np.nan
    got = call(d)
    rest = [0, 1, 3, 4, 5, 6]   # 0, 1 and 3 share the wave of instance 2
    assert got['status'][2] == 1 and np.all(got['status'][rest] == 0)
    for k in ALL:
        assert np.all(np.isnan(got[k][2])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k     # bit for bit


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B = 3, 2
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    st = torch.zeros(B, dtype=torch.int32, device='cuda')
    null = ctypes.c_void_p(0)

    def call(h, nx, nu, X=True, U=True, xref=True, uref=True, gX=True, outs=(True,) * 6):
        P = lambda t, w=True: h._ptr(t) if w else null   # noqa: E731
        xb, ub, gXd, gUd = d(B, N + 1, nx), d(B, N, nu), d(B, N + 1, nx), d(B, N, nu)
        Xd, Ud, xr, ur = d(B, N + 1, nx), d(B, N, nu), d(1, N + 1, nx), d(1, N, nu)
        o = (d(B, nx), d(B, N + 1, nx), d(B, N, nu), d(B, nx, nx), d(B, nu, nu), d(B, nx, nx))
        rc = h.lib.mpcb_solve_vjp_w(h._h, B, P(xb), P(ub), P(Xd, X), P(Ud, U), P(xr, xref), 0, P(ur, uref), 0,
                                    null, 0, P(gXd, gX), P(gUd), *[P(t, w) for t, w in zip(o, outs)], P(st), null)
        torch.cuda.synchronize()
        return rc

    m = _mpc(N, B)
    assert call(m, 12, 4) == 0
    assert call(m, 12, 4, outs=(False, False, False, False, True, False)) == 0      # gR alone
    assert call(m, 12, 4, outs=(False,) * 6) == -1                                  # all six NULL
    for missing in ('X', 'U', 'xref', 'uref'):                                      # MPCB_E_INVALID
        assert call(m, 12, 4, **{missing: False}) == -1 and b'required' in m.lib.mpcb_last_error(), missing
    # no weight output: the rules of mpcb_solve_vjp (nothing of X, U, xref, uref is needed)
    assert call(m, 12, 4, X=False, U=False, xref=False, uref=False, outs=(True, True, True, False, False, False)) == 0
    mb = _mpc(N, B, lbu=LB, ubu=UB)
    assert call(mb, 12, 4, X=False, U=False, xref=False, uref=False, outs=(True, True, True, False, False, False)) == -1
    assert call(mb, 12, 4, X=False, xref=False, uref=False, outs=(True, True, True, False, False, False)) == 0
    assert call(mb, 12, 4) == 0
    m17 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    assert call(m17, 17, 6) == -4                                                   # MPCB_E_UNSUPPORTED
    with pytest.raises(ValueError):
        m.solve_iterate_vjp(d(B, N + 1, 12), d(B, N, 4), gU=d(B, N, 4), weights=True)


# ------------------------------------------------------------------------------ mpcb_set_weights
import test_gpu_config as gc   # noqa: E402


def _weights_b(nx=12, nu=4, seed=23):
    rng = np.random.default_rng(seed)
    return {'Q': ac.spd(rng, nx, 3.0), 'R': ac.spd(rng, nu, 0.2), 'QN': ac.spd(rng, nx, 30.0)}


def _outputs(m):
    return [t.clone() for t in (m.get_control(), m.get_state_trajectory(), m.get_input_trajectory(), m.get_status())]


def _solve(m, N, B, mode, dtype):
    inp = gc._inputs(N, B, dtype)
    if mode == 'iterate':
        m.solve_iterate(inp['x0'], inp['xbar'], inp['ubar'], inp['xref'], inp['uref'], wind=inp['wind'])
    else:
        m.solve(inp['x0'], inp['xref'], inp['uref'], wind=inp['wind'])
    torch.cuda.synchronize()
    return _outputs(m)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# (path of tests/test_gpu_config.py PATHS, dtype, N, B): the configurations its tests reach the paths with
SET_CASES = [('fused', 'f64', 6, gc.B12), ('two', 'f64', 6, gc.B12), ('notan', 'f64', 6, gc.B12),
             ('row32', 'f32', 6, gc.B12), ('small', 'f64', 6, gc.B12), ('small', 'f32', 6, gc.B12),
             ('single', 'f64', 6, gc.B12), ('single', 'f32', 6, gc.B12), ('thread', 'f64', 6, gc.B12),
             ('thread', 'f32', 6, gc.B12), ('lanequad', 'f64', 130, 5), ('lanequad', 'f32', 260, 5),
             ('box', 'f64', 6, gc.B12), ('box', 'f32', 6, gc.B12), ('box_ipm', 'f64', 6, gc.B12),
             ('box_v1', 'f64', 6, gc.B12)]
# both modes; the fp32 lane-quad rollout (N = 260) in iterate mode only, as there
SET_CASES = [c + (mode,) for c in SET_CASES for mode in gc.MODES
             if not (c[:2] == ('lanequad', 'f32') and mode == 'rollout')]


@pytest.mark.parametrize('path,dtype,N,B,mode', SET_CASES)
def test_set_weights_equals_a_new_handle(path, dtype, N, B, mode, monkeypatch):
    """Created with ALT's weights A, given B: u0, X, U and status of the next solve are those of a
    handle created with B, and not A's.  The launched kernels are the path's."""
    boxed = path.startswith('box')
    kw = dict(ac.fields(alt='a', box='input' if boxed else 'none', dtype=dtype),
              **({'max_as_iter': 1} if path == 'box_ipm' else {}))
    wb = {k: ac._r32(v) if dtype == 'f32' else v for k, v in _weights_b().items()}
    m = gc._handle(path, N, B, dtype, monkeypatch, **kw)
    out_a = _solve(m, N, B, mode, dtype)
    m.set_weights(**wb)
    out = _solve(m, N, B, mode, dtype)
    gc._kernels_are(m, B, mode, gc.PATHS[path][2](dtype, gc._it(mode)))
    fresh = gc._handle(path, N, B, dtype, monkeypatch, **dict(kw, **wb))
    out_b = _solve(fresh, N, B, mode, dtype)
    assert (out_b[3] == 0).all()
    assert _same(out, out_b)
    assert not torch.equal(out[0], out_a[0]) and not torch.equal(out[1], out_a[1]) and not torch.equal(out[2], out_a[2])
    assert np.array_equal(m.cfg.Q, wb['Q']) and m._weights_version == 1
    # NULL keeps: R alone, then Q and QN, arrive at the same handle
    m2 = gc._handle(path, N, B, dtype, monkeypatch, **kw)
    m2.set_weights(R=wb['R'])
    m2.set_weights(Q=wb['Q'], QN=wb['QN'])
    assert _same(_solve(m2, N, B, mode, dtype), out_b)


def test_set_weights_refuses_bad_matrices(monkeypatch):
    """An asymmetric or non-finite matrix: MPCB_E_INVALID, and the handle solves as before."""
    from mpc_blaster_amd._lib import MpcbError
    N, B = 6, gc.B12
    m = gc._handle('fused', N, B, 'f64', monkeypatch, **ac.fields(alt='a', box='none'))
    before = _solve(m, N, B, 'iterate', 'f64')
    wb = _weights_b()
    dp = ctypes.POINTER(ctypes.c_double)
    asym = wb['Q'].copy()
    asym[2, 5] += 1e-3
    nan = wb['R'].copy()
    nan[1, 1] = np.nan
    inf = wb['QN'].copy()
    inf[3, 3] = np.inf
    good = np.ascontiguousarray(wb['Q'])
    for Q, R, QN in ((asym, None, None), (good, nan, None), (good, None, inf)):
        ptr = [None if a is None else np.ascontiguousarray(a).ctypes.data_as(dp) for a in (Q, R, QN)]
        assert m.lib.mpcb_set_weights(m._h, *ptr) == -1
        with pytest.raises(MpcbError):
            m.set_weights(Q=Q, R=R, QN=QN)
    assert m._weights_version == 0
    assert _same(_solve(m, N, B, 'iterate', 'f64'), before)


def test_set_weights_after_set_t_blast():
    """12/4: set_t_blast, then set_weights, equals a handle created with both final values."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B = 6, gc.B12
    kw = ac.fields(alt='a', box='none')
    wb = _weights_b()
    m = BatchedMPC(MPCConfig(N=N, **kw), max_batch=B)
    m.set_t_blast(2.5)
    m.set_weights(**wb)
    fresh = BatchedMPC(MPCConfig(N=N, **dict(kw, t_blast=2.5, **wb)), max_batch=B)
    other = BatchedMPC(MPCConfig(N=N, **dict(kw, **wb)), max_batch=B)   # ALT's t_blast = 4
    out, out_f, out_o = (_solve(h, N, B, 'iterate', 'f64') for h in (m, fresh, other))
    assert _same(out, out_f) and not torch.equal(out[0], out_o[0])


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_set_weights_full17(dtype):
    """17/6 with the input box: the default parameter vector's T_blast set by set_t_blast survives
    the refill of the weights block; then the same with set_params' stage-varying parameters."""
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N = 7
    x0, xref, uref, p, xb, ub = gc._inputs17(N, dtype)
    kw = ac.fields(full=True, alt='a', box='input', dtype=dtype)
    wb = {k: ac._r32(v) if dtype == 'f32' else v for k, v in _weights_b(17, 6, seed=29).items()}

    def solve(h):
        h.solve_iterate(x0, xb, ub, xref, uref)
        torch.cuda.synchronize()
        return _outputs(h)

    m = BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **kw), max_batch=gc.B17)
    out_a = solve(m)
    m.set_t_blast(3.0)
    m.set_weights(**wb)
    fresh = BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **dict(kw, t_blast=3.0, **wb)), max_batch=gc.B17)
    other = BatchedMPC(MPCConfig.full(N=N, dtype=dtype, **dict(kw, **wb)), max_batch=gc.B17)   # t_blast = 4
    out, out_f, out_o = solve(m), solve(fresh), solve(other)
    assert _same(out, out_f)
    assert not torch.equal(out[2], out_a[2]) and not torch.equal(out[2], out_o[2])
    m.set_params(p)
    fresh.set_params(p)
    assert _same(solve(m), solve(fresh))


# ------------------------------------------------------------------------------ torch layer
def _t(a, grad=False):
    return torch.tensor(a, dtype=torch.float64, device='cuda', requires_grad=grad)


def _vec_weights(spec):
    return [np.diag(np.asarray(M, dtype=np.float64)).copy() for M in (spec.Q, spec.R, spec.QN)]


def test_torch_layer_weight_gradients():
    """L = sum w u0 + sum v X with vector Q, R, QN: the gradients are the diagonals of the batch sum
    of the reference over the status-0 instances; x0's gradient comes along unchanged."""
    B, N = 16, 8   # the draws of the end-to-end case: the active set converges on every instance
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    rng = np.random.default_rng(21)
    w0, wX = rng.standard_normal((B, 4)), rng.standard_normal((B, N + 1, 12))
    q, r, qn = (_t(v, True) for v in _vec_weights(spec))
    x0 = _t(c['x0'], True)
    u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], c['xref'], c['uref'], Q=q, R=r, QN=qn)
    ((_t(w0) * u0).sum() + (_t(wX) * X).sum()).backward()
    st = m.get_status().cpu().numpy()
    assert (st == 0).all()
    gU = np.zeros((B, N, 4))
    gU[:, 0] = w0
    ref = vjp_weights_ref(c['xbar'], c['ubar'], X.detach().cpu().numpy(), U.detach().cpu().numpy(), c['xref'],
                          c['uref'], wX, gU, spec)
    print(f'torch layer: {ref["fixed"].sum()} clamped components')
    assert ref['fixed'].any()
    for t, k in ((q, 'gQ'), (r, 'gR'), (qn, 'gQN')):
        want = np.diagonal(ref[k][st == 0].sum(axis=0))
        got = t.grad.cpu().numpy()
        assert got.shape == want.shape and t.grad.dtype == torch.float64
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1.0)
        print(f'  {k} diagonal, batch sum: {err:.2e} (|ref| {np.abs(want).max():.3g})')
        assert err <= BOUND['f64'], k
    assert relerr(x0.grad.cpu().numpy(), ref['gx0']).max() <= BOUND['f64']
    # a matrix weight receives the symmetric matrix
    Qm = _t(np.asarray(spec.Q, dtype=np.float64), True)
    u0, X, U = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=Qm)
    ((_t(w0) * u0).sum() + (_t(wX) * X).sum()).backward()
    want = ref['gQ'].sum(axis=0)
    assert Qm.grad.shape == (12, 12) and torch.equal(Qm.grad, Qm.grad.T)
    assert np.abs(Qm.grad.cpu().numpy() - want).max() / max(np.abs(want).max(), 1.0) <= BOUND['f64']
    # ... and a float32 tensor a gradient of its own dtype (its rounded value is what the handle
    # solves with, so no figure is compared here)
    r32 = torch.tensor(_vec_weights(spec)[1], dtype=torch.float32, device='cuda', requires_grad=True)
    u0, X, U = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], R=r32)
    (_t(wX) * X).sum().backward()
    assert r32.grad.dtype == torch.float32 and r32.grad.shape == (4,) and bool(torch.isfinite(r32.grad).all())


def test_torch_layer_directional_derivative():
    """Central difference of L on the device along a random direction in the log-weights (all three
    at once), relative step 1e-4, against <grad, d>: within 1e-5 of it.  Unconstrained, so that no
    probe changes an active set."""
    B, N = 7, 8
    spec = OcpSpec(N=N)
    c = _case(B, N, 'sine')
    m = _mpc(N, B)
    rng = np.random.default_rng(22)
    w0, wX = _t(rng.standard_normal((B, 4))), _t(rng.standard_normal((B, N + 1, 12)))
    th = [np.log(v) for v in _vec_weights(spec)]
    d = [rng.standard_normal(v.shape) for v in th]

    def loss(scale, grad=False):
        ws = [_t(np.exp(t + scale * dd), grad) for t, dd in zip(th, d)]
        u0, X, _ = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=ws[0], R=ws[1], QN=ws[2])
        assert (m.get_status() == 0).all()
        return (w0 * u0).sum() + (wX * X).sum(), ws

    L, ws = loss(0.0, True)
    L.backward()
    # dL/dtheta_i = w_i dL/dw_i
    lin = sum(float((w.grad * w.detach() * _t(dd)).sum()) for w, dd in zip(ws, d))
    h = 1e-4
    fd = (float(loss(h)[0]) - float(loss(-h)[0])) / (2.0 * h)
    print(f'directional: FD {fd:.12g}  <grad, d> {lin:.12g}  relative difference {abs(fd - lin) / abs(lin):.2e}')
    assert abs(fd - lin) <= 1e-5 * abs(lin)


def test_torch_layer_refuses_stale_weights():
    B, N = 3, 3
    c = _case(B, N)
    m = _mpc(N, B)
    q = _t(_vec_weights(OcpSpec(N=N))[0], True)
    u0, X, U = m.solve_iterate_diff(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'], Q=q)
    m.set_weights(Q=2.0 * q)
    with pytest.raises(RuntimeError, match='weights'):
        X.sum().backward()
    # without weight arguments x0's gradient still depends on Q, R and QN: the same refusal
    x0 = _t(c['x0'], True)
    u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], c['xref'], c['uref'])
    m.set_weights(Q=q)
    with pytest.raises(RuntimeError, match='weights'):
        X.sum().backward()
    assert x0.grad is None
    # the control: the same forward and backward with nothing in between, against the reference
    # (the handle holds the default Q again)
    u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], c['xref'], c['uref'])
    X.sum().backward()
    from vjp_ref import vjp_ref
    ref = vjp_ref(c['xbar'], c['ubar'], None, np.ones((B, N + 1, 12)), None, OcpSpec(N=N))
    assert (m.get_status() == 0).all()
    assert relerr(x0.grad.cpu().numpy(), ref['gx0']).max() <= BOUND['f64']
