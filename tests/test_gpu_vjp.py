"""mpcb_solve_vjp on the GPU (the vector-Jacobian product of one solve_iterate step) and the torch
layer over it, against tests/vjp_ref.py: the device is compared with the NumPy reference, never
with itself.  tests/test_vjp_ref_cpu.py ties that reference to finite differences of the oracle.

Metric: per instance and per output, |dev - ref|_inf / max(|ref|_inf, 1).  Bounds: fp64 1e-9 (the
bound of the fp64 solve tests in tests/test_gpu_parity.py), fp32 5e-5 (the project's fp32 solve
bound, ~80 x the move of the fp64 gradients under a relative 2^-22 perturbation of the inputs);
in fp32 the reference reads fp32-rounded data, weights, cost scale and bounds.  Each test prints
its measured maxima (DESIGN.md records them).

Draws: tests/vjp_ref.py vjp_case (seed 1004).  The references do not enter the product itself (the
Jacobian does not depend on them), so the sine-reference case runs through the torch layer, where
the forward solve reads them with per-instance strides.  The reference is vjp_ref's Riccati
recursion: its condensed dense variant loses digits with the horizon (3e-9 at N = 64, see
tests/vjp_ref.py), which is what the device missed the 1e-9 bound by when it was compared to it.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alt_config as ac   # noqa: E402
from vjp_ref import vjp_case, vjp_ref   # noqa: E402

from oracle.ocp import OcpSpec   # noqa: E402

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('gx0', 'gxref', 'guref')
BOUND = {'f64': 1e-9, 'f32': 5e-5}
LB, UB = np.full(4, 5.0), np.full(4, 40.0)


def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def _mpc(N, B, dtype='f64', **kw):
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    return BatchedMPC(MPCConfig(N=N, dtype=dtype, **kw), max_batch=B)


def _spec32(spec):
    """The spec as an fp32 handle holds it (tests/test_gpu_eval.py _check32)."""
    spec.Q, spec.R, spec.QN, spec.cost_scale = _f32(spec.Q), _f32(spec.R), _f32(spec.QN), float(np.float32(spec.s))
    if spec.lbu is not None:
        spec.lbu, spec.ubu = _f32(spec.lbu), _f32(spec.ubu)
    return spec


@functools.lru_cache(maxsize=None)
def _case(B, N, ref='hover', wind=False):
    return vjp_case(B, N, OcpSpec(N=N), ref, wind)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64 if k != 'status' else np.int32) for k, v in out.items()}


def relerr(a, b):
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def _check(got, ref, dtype, tag, keys=KEYS):
    assert np.all(got['status'] == 0), (tag, got['status'])
    err = {k: relerr(got[k], ref[k]).max() for k in keys}
    print(f'{tag}: ' + '  '.join(f'{k} {err[k]:.2e}/{BOUND[dtype]:.0e} (|ref| {np.abs(ref[k]).max():.3g})' for k in keys))
    for k in keys:
        assert err[k] <= BOUND[dtype], (tag, k, err[k])
    return err


def _synthetic_U(c, spec, seed=3):
    """U = clip(ubar + 30 N(0, 1), lbu, ubu): more than 20 % of the components exactly on a bound,
    and every input of instance 1 clamped at stage 2."""
    rng = np.random.default_rng(seed)
    lb, ub = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
    U = np.clip(c['ubar'] + 30.0 * rng.standard_normal(c['ubar'].shape), lb, ub)
    if U.shape[0] > 1 and U.shape[1] > 2:
        U[1, 2] = lb
    assert ((U == lb) | (U == ub)).mean() > 0.2
    return U


# ------------------------------------------------------------------------------ fp64, unconstrained
@pytest.mark.parametrize('B,N,wind,cot,skip', [
    (1, 1, False, 'both', None), (1, 3, True, 'both', None), (7, 3, False, 'gX', None),
    (7, 20, False, 'gU', None), (5, 64, False, 'both', 'gxref'), (4099, 20, True, 'both', None)])
def test_vjp_fp64_matches_reference(B, N, wind, cot, skip):
    c = _case(B, N, 'hover', wind)
    gX = c['gX'] if cot in ('both', 'gX') else None
    gU = c['gU'] if cot in ('both', 'gU') else None
    ref = vjp_ref(c['xbar'], c['ubar'], None, gX, gU, OcpSpec(N=N), c['wind'])
    m = _mpc(N, B)
    tag = f'fp64 B={B} N={N} wind={wind} cot={cot}'
    _check(_np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=gX, gU=gU, wind=c['wind'])), ref, 'f64', tag)
    if skip:   # a NULL output: the others are unchanged
        d = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device='cuda')   # noqa: E731
        t = lambda a: torch.as_tensor(a, dtype=torch.float64, device='cuda').contiguous()   # noqa: E731
        xb, ub, gXd, gUd = t(c['xbar']), t(c['ubar']), t(gX), t(gU)
        o = dict(gx0=d(B, 12), guref=d(B, N, 4), status=torch.zeros(B, dtype=torch.int32, device='cuda'))
        P, null = m._ptr, ctypes.c_void_p(0)
        assert m.lib.mpcb_solve_vjp(m._h, B, P(xb), P(ub), null, null, 0, P(gXd), P(gUd), P(o['gx0']), null,
                                    P(o['guref']), P(o['status']), null) == 0
        _check(_np(o), ref, 'f64', tag + ' gxref=NULL', keys=('gx0', 'guref'))


def test_vjp_strides_over_its_slots(monkeypatch):
    """More waves than workspace slots: the kernel's stride loop reuses a slot."""
    B, N = 37, 3
    c = _case(B, N)
    ref = vjp_ref(c['xbar'], c['ubar'], None, c['gX'], c['gU'], OcpSpec(N=N))
    monkeypatch.setenv('MPCB_VJP_SLOTS', '3')
    m = _mpc(N, B)
    _check(_np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'])), ref, 'f64', 'fp64 B=37 N=3, 3 slots')


# ------------------------------------------------------------------------------ fp64, input box
@pytest.mark.parametrize('B,N', [(7, 8), (5, 33), (3, 64)])
def test_vjp_fp64_box_synthetic_mask(B, N):
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    U = _synthetic_U(c, spec)
    ref = vjp_ref(c['xbar'], c['ubar'], U, c['gX'], c['gU'], spec)
    assert ref['fixed'][1, 2].all() and ref['fixed'].mean() > 0.2
    if N > 33:
        assert ref['fixed'][:, 32:].any() and ref['fixed'][:, N - 1].any()   # both words of the stage mask
    m = _mpc(N, B, lbu=LB, ubu=UB)
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U))
    _check(got, ref, 'f64', f'fp64 box synthetic B={B} N={N} ({ref["fixed"].mean():.0%} clamped)')
    # R is diagonal here: a clamped component has no sensitivity at all
    assert np.all(got['guref'][ref['fixed']] == 0.0) and np.all(ref['guref'][ref['fixed']] == 0.0)
    assert np.all(got['guref'][~ref['fixed']] != 0.0)
    # ... and the box is not ignored
    free = vjp_ref(c['xbar'], c['ubar'], None, c['gX'], c['gU'], spec)
    assert relerr(got['gx0'], free['gx0']).min() > 1e-3


def test_vjp_fp64_box_end_to_end():
    """U from the device's own solve: its clamped components carry the bound itself."""
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=LB, ubu=UB)
    c = _case(B, N)
    m = _mpc(N, B, lbu=LB, ubu=UB)
    m.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'], c['uref'])
    U = m.get_input_trajectory().clone()
    torch.cuda.synchronize()
    assert np.all(m.get_status().cpu().numpy() == 0)
    Uh = U.cpu().numpy()
    clamped = ((Uh <= LB) | (Uh >= UB)).any(axis=(1, 2))
    print(f'end to end: {clamped.sum()} of {B} instances with a clamped component, {((Uh <= LB) | (Uh >= UB)).sum()} components')
    assert clamped.sum() >= 8
    ref = vjp_ref(c['xbar'], c['ubar'], Uh, c['gX'], c['gU'], spec)
    _check(_np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U)), ref, 'f64', 'fp64 box end to end')


# ------------------------------------------------------------------------------ another problem definition
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_vjp_alt_definition(dtype):
    """Dense weights, another model, cost_scale != dt, per-channel bounds (tests/alt_config.py)."""
    B, N = 7, 8
    kw = ac.fields(alt='b', box='input', dtype=dtype)
    spec = OcpSpec(N=N, **ac.spec_kwargs(kw))
    cast = _f32 if dtype == 'f32' else (lambda a: a)
    c = {k: cast(v) for k, v in vjp_case(B, N, spec, wind=True).items()}
    U = cast(_synthetic_U(c, spec))
    ref = vjp_ref(c['xbar'], c['ubar'], U, c['gX'], c['gU'], spec, c['wind'])
    assert ref['fixed'].mean() > 0.2
    m = _mpc(N, B, dtype, **kw)
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U, wind=c['wind']))
    _check(got, ref, dtype, f'ALT-b box {dtype}')


# ------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize('B,N,box', [(7, 20, False), (7, 8, True)])
def test_vjp_fp32(B, N, box):
    spec = _spec32(OcpSpec(N=N, lbu=LB if box else None, ubu=UB if box else None))
    c = {k: _f32(v) for k, v in _case(B, N).items()}
    U = _f32(_synthetic_U(c, spec)) if box else None
    ref = vjp_ref(c['xbar'], c['ubar'], U, c['gX'], c['gU'], spec)
    m = _mpc(N, B, 'f32', **(dict(lbu=LB, ubu=UB) if box else {}))
    got = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U))
    _check(got, ref, 'f32', f'fp32 B={B} N={N} box={box}')
    if box:
        assert np.all(got['guref'][ref['fixed']] == 0.0)


# ------------------------------------------------------------------------------ determinism, NaN
@pytest.mark.parametrize('box', [False, True])
def test_two_calls_are_bit_identical(box):
    B, N = 7, 8
    c = _case(B, N)
    kw = dict(lbu=LB, ubu=UB) if box else {}
    U = _synthetic_U(c, OcpSpec(N=N, lbu=LB, ubu=UB)) if box else None
    m = _mpc(N, B, **kw)
    a = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U))
    b = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU'], U=U))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('where', ['gX', 'gU', 'xbar'])
def test_nan_instance_is_isolated(where):
    B, N = 7, 8
    c = _case(B, N)
    m = _mpc(N, B)
    ok = _np(m.solve_iterate_vjp(c['xbar'], c['ubar'], gX=c['gX'], gU=c['gU']))
    d = {k: c[k].copy() for k in ('xbar', 'ubar', 'gX', 'gU')}
    d[where][2, 5, 3] = np.nan
    got = _np(m.solve_iterate_vjp(d['xbar'], d['ubar'], gX=d['gX'], gU=d['gU']))
    rest = [0, 1, 3, 4, 5, 6]   # 0, 1 and 3 share the wave of instance 2
    assert got['status'][2] == 1 and np.all(got['status'][rest] == 0)
    for k in KEYS:
        assert np.all(np.isnan(got[k][2])), k
        assert np.array_equal(got[k][rest], ok[k][rest]), k     # bit for bit


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from mpc_blaster_amd import BatchedMPC, MPCConfig
    N, B = 3, 2
    d = lambda *s: torch.zeros(s, dtype=torch.float64, device='cuda')   # noqa: E731
    st = torch.zeros(B + 1, dtype=torch.int32, device='cuda')
    null = ctypes.c_void_p(0)

    def call(h, Bq, nx, nu, U=None, gX=True, gU=True, outs=(True, True, True)):
        P = h._ptr
        xb, ub, gXd, gUd = d(B + 1, N + 1, nx), d(B + 1, N, nu), d(B + 1, N + 1, nx), d(B + 1, N, nu)
        o = (d(B + 1, nx), d(B + 1, N + 1, nx), d(B + 1, N, nu))
        rc = h.lib.mpcb_solve_vjp(h._h, Bq, P(xb), P(ub), P(U), null, 0, P(gXd) if gX else null,
                                  P(gUd) if gU else null, *[P(t) if w else null for t, w in zip(o, outs)],
                                  P(st), null)
        torch.cuda.synchronize()
        return rc

    m = _mpc(N, B)
    assert call(m, B, 12, 4) == 0
    assert call(m, B, 12, 4, gX=False) == 0 and call(m, B, 12, 4, outs=(False, True, False)) == 0
    assert call(m, B + 1, 12, 4) == -1                                  # MPCB_E_INVALID: B > max_batch
    assert call(m, B, 12, 4, gX=False, gU=False) == -1                  # both cotangents NULL
    assert call(m, B, 12, 4, outs=(False, False, False)) == -1          # all outputs NULL
    mb = _mpc(N, B, lbu=LB, ubu=UB)
    assert call(mb, B, 12, 4) == -1 and b'U' in mb.lib.mpcb_last_error()   # U == NULL with the box
    assert call(mb, B, 12, 4, U=d(B, N, 4)) == 0
    m17 = BatchedMPC(MPCConfig.full(N=N), max_batch=B)
    assert call(m17, B, 17, 6) == -4                                    # MPCB_E_UNSUPPORTED
    before = m.workspace_bytes
    assert _mpc(N, B).workspace_bytes == before                         # the handle's own workspace is as before


# ------------------------------------------------------------------------------ torch layer
def _t(a, grad=False):
    return torch.tensor(a, dtype=torch.float64, device='cuda', requires_grad=grad)


def test_torch_layer_gradients():
    B, N = 3, 3
    c = _case(B, N)
    spec = OcpSpec(N=N)
    m = _mpc(N, B)
    rng = np.random.default_rng(11)
    w0, wX, wU = rng.standard_normal((B, 4)), rng.standard_normal((B, N + 1, 12)), rng.standard_normal((B, N, 4))
    x0, xref, uref = _t(c['x0'], True), _t(c['xref'][:1], True), _t(c['uref'], True)   # x_ref broadcast [1, ...]
    xbar = _t(c['xbar'], True)
    u0, X, U = m.solve_iterate_diff(x0, xbar, c['ubar'], xref, uref)
    # the forward is solve_iterate itself
    m2 = _mpc(N, B)
    u0p = m2.solve_iterate(c['x0'], c['xbar'], c['ubar'], c['xref'][:1], c['uref'])
    assert torch.equal(u0.detach(), u0p) and torch.equal(X.detach(), m2.get_state_trajectory())
    loss = (_t(w0) * u0).sum() + (_t(wX) * X).sum() + (_t(wU) * U).sum()
    loss.backward()
    gU = wU.copy()
    gU[:, 0] += w0
    ref = vjp_ref(c['xbar'], c['ubar'], None, wX, gU, spec)
    got = dict(gx0=x0.grad.cpu().numpy(), gxref=xref.grad.cpu().numpy(), guref=uref.grad.cpu().numpy(),
               status=np.zeros(B, dtype=np.int32))
    assert got['gxref'].shape == (1, N + 1, 12)
    _check(got, dict(gx0=ref['gx0'], gxref=ref['gxref'].sum(axis=0, keepdims=True), guref=ref['guref']), 'f64',
           'torch layer B=3 N=3')
    assert xbar.grad is None


@pytest.mark.parametrize('B,ref,box', [(16, 'hover', True), (7, 'sine', False)])
def test_torch_layer_per_instance_references(B, ref, box):
    """Per-instance [B, ...] references through the forward solve and a loss on u0 only; with the
    input box (the draws of the end-to-end case: the active set converges, nothing is handed to the
    interior point, whose U is not on the bounds) and with sine references."""
    N = 8
    kw = dict(lbu=LB, ubu=UB) if box else {}
    spec = OcpSpec(N=N, **kw)
    c = _case(B, N, ref)
    m = _mpc(N, B, **kw)
    x0, xref, uref = _t(c['x0'], True), _t(c['xref'], True), _t(c['uref'], True)
    u0, X, U = m.solve_iterate_diff(x0, c['xbar'], c['ubar'], xref, uref)
    w0 = np.random.default_rng(12).standard_normal((B, 4))
    (_t(w0) * u0).sum().backward()
    assert np.all(m.get_status().cpu().numpy() == 0)
    gU = np.zeros((B, N, 4))
    gU[:, 0] = w0
    ref_ = vjp_ref(c['xbar'], c['ubar'], U.detach().cpu().numpy(), None, gU, spec)
    print(f'torch layer {ref} box={box}: {ref_["fixed"].sum()} clamped components')
    assert not box or ref_['fixed'].any(axis=(1, 2)).sum() >= 8
    got = dict(gx0=x0.grad.cpu().numpy(), gxref=xref.grad.cpu().numpy(), guref=uref.grad.cpu().numpy(),
               status=np.zeros(B, dtype=np.int32))
    assert got['gxref'].shape == (B, N + 1, 12)
    _check(got, ref_, 'f64', f'torch layer {ref} box={box} B={B} N={N}')
