"""tests/vjp17_ref.py (the NumPy reference of mpcb_solve_vjp17) against the condensed dense solve
and against central finite differences of the oracle's ``mpc_solve17(mode='iterate')``, unboxed
and through the interior point of the input box; and the declaration of the entry point.  No GPU.

These certify the yardstick of tests/test_gpu_vjp17.py, not the device.  Metric: the project's,
per instance and output |a - b|_inf / max(|b|_inf, 1).

Unboxed the map is affine, so the central difference with a large step (1e-2) carries only the
rounding of the difference: gx0, gxref <= 1e-8, guref <= 1e-6 (the input weights of the swivel
rates are 1e-5, which the difference divides by).  Boxed, the oracle's interior point leaves every
component either within 1e-6 of a bound or far from it (no slack in (1e-6, 1e-3)), the mask by that
tolerance reproduces the derivative of the boxed solve within 1e-6, and the unmasked product is off
by more than 50 % on every instance.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp17_ref as vr   # noqa: E402

from oracle.full import FullSpec, mpc_solve17   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 3), (3, 6)]


@pytest.mark.parametrize('B,N', SHAPES)
@pytest.mark.parametrize('masked', [False, True])
def test_recursion_matches_condensed_dense_solve(B, N, masked):
    spec = FullSpec(N=N)
    c = vr.vjp17_case(B, N, spec)
    fixed = vr.random_mask(B, N) if masked else None
    a = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec)
    d = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec, solver=vr._dense)
    err = {k: vr.relerr(a[k], d[k]).max() for k in vr.KEYS}
    print(f'recursion vs dense B={B} N={N} masked={masked}: ' + '  '.join(f'{k} {v:.2e}' for k, v in err.items()))
    assert max(err.values()) <= 1e-11
    if masked:
        assert 0.3 < fixed.mean() < 0.7
        assert np.all(a['guref'][fixed] == 0.0)   # diagonal R: a clamped component's guref is 0


def _fd(c, spec, h, theta, split, solve_spec=None):
    """Central differences of L = <gX, X> + <gU, U> of the oracle step over the columns of theta
    ([B, n]; ``split`` turns a [M, n] array into the (x0, xref, uref) the oracle takes), all probes
    in one oracle call.  Returns (g [B, n], status of every probe [2 n, B])."""
    B, n = theta.shape
    probes = np.concatenate([theta[None] + h * np.eye(n)[:, None, :], theta[None] - h * np.eye(n)[:, None, :]])
    P = probes.reshape(2 * n * B, n)   # probe-major, instance-minor
    rep = lambda a: np.tile(a, (2 * n,) + (1,) * (a.ndim - 1))   # noqa: E731
    x0, xref, uref = split(P, rep)
    o = mpc_solve17(x0, xref, uref, solve_spec or spec, rep(c['p']), mode='iterate', xbar=rep(c['xbar']),
                    ubar=rep(c['ubar']))
    L = (np.einsum('bki,bki->b', rep(c['gX']), o['X']) + np.einsum('bki,bki->b', rep(c['gU']), o['U'])).reshape(2, n, B)
    return ((L[0] - L[1]) / (2.0 * h)).T, o['status'].reshape(2 * n, B)


@pytest.mark.parametrize('B,N', SHAPES)
def test_reference_matches_finite_differences_unboxed(B, N):
    spec = FullSpec(N=N)
    c = vr.vjp17_case(B, N, spec)
    r = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], None, c['gX'], c['gU'], spec)
    theta = np.concatenate([c['x0'], c['xref'].reshape(B, -1), c['uref'].reshape(B, -1)], axis=1)
    nx = (N + 1) * 17
    g, st = _fd(c, spec, 1e-2, theta,
                lambda P, rep: (P[:, :17], P[:, 17:17 + nx].reshape(-1, N + 1, 17), P[:, 17 + nx:].reshape(-1, N, 6)))
    assert (st == 0).all()
    fd = dict(gx0=g[:, :17], gxref=g[:, 17:17 + nx].reshape(B, N + 1, 17), guref=g[:, 17 + nx:].reshape(B, N, 6))
    err = {k: vr.relerr(r[k], fd[k]).max() for k in vr.KEYS}
    print(f'reference vs central differences B={B} N={N}: ' + '  '.join(f'{k} {v:.2e}' for k, v in err.items()))
    assert err['gx0'] <= 1e-8 and err['gxref'] <= 1e-8 and err['guref'] <= 1e-6


def test_boxed_mask_by_tolerance_reproduces_the_interior_point():
    spec, c = vr.boxed_case()
    B, N = c['ubar'].shape[:2]
    base = mpc_solve17(c['x0'], c['xref'], c['uref'], spec, c['p'], mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    assert (base['status'] == 0).all()
    fixed, slack = vr.active_mask(base['U'], spec)
    print(f'boxed draw: {fixed.sum()} of {fixed.size} components active, largest active slack '
          f'{slack[fixed].max():.2e}, smallest inactive {slack[~fixed].min():.2e}, iterations {base["iters"]}')
    assert not ((slack > 1e-6) & (slack < 1e-3)).any()
    assert fixed.any(axis=(1, 2)).all()
    g, st = _fd(c, spec, 1e-5, c['x0'], lambda P, rep: (P, rep(c['xref']), rep(c['uref'])))
    assert (st == 0).all()
    masked = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], fixed, c['gX'], c['gU'], spec)
    free = vr.vjp17_ref(c['xbar'], c['ubar'], c['p'], None, c['gX'], c['gU'], spec)
    em, ef = vr.relerr(masked['gx0'], g), vr.relerr(free['gx0'], g)
    print('masked reference vs central differences of the boxed step:', np.array2string(em, precision=2))
    print('unmasked reference vs the same:', np.array2string(ef, precision=2))
    assert em.max() <= 1e-6
    assert (ef > 0.5).all()


def test_entry_point_is_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    assert re.search(r'\bint\s+mpcb_solve_vjp17\s*\(', txt)
    assert 'mpcb_solve_vjp17' in _lib.EXPORTS_17
    assert re.search(r'#define\s+MPCB_ABI_VERSION\s+5\b', txt) and _lib.ABI_VERSION == 5
