"""tests/vjp_ref.py (the NumPy reference of mpcb_solve_vjp, and its condensed dense variant)
against central finite differences of the oracle's ``mpc_solve(mode='iterate')``, and the
declaration of the entry point.  No GPU.

L = <gX, X> + <gU, U> with standard normal cotangents; every component of x0, xref and uref is
probed.  The map is affine (piecewise affine with the box), so the central difference is exact up
to rounding: the bound is 1e-9 of the instance's largest reference component.  With the box an
instance counts only if the oracle's active set is the same at every probe and the active-set
method solved it (no hand-over to the interior point).
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vjp_ref import vjp_case, vjp_ref, vjp_ref_dense   # noqa: E402

from oracle.ocp import OcpSpec, mpc_solve   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_BOUND = 1e-9   # the oracle's U is ubar + (bound - ubar): on the bound up to rounding


def _snap(U, spec):
    """(clamped mask, U with the clamped components put on their bound exactly)"""
    lb, ub = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
    lo, hi = U <= lb + ON_BOUND, U >= ub - ON_BOUND
    return lo | hi, np.where(lo, lb, np.where(hi, ub, U))


def _fd(c, spec, h):
    """Central differences of L over every input component, all probes in one oracle call.
    Returns (g [B, n], same_set [B]): n = 12 + (N + 1) 12 + N 4 in the order x0, xref, uref."""
    B, N = c['ubar'].shape[:2]
    theta = np.concatenate([c['x0'], c['xref'].reshape(B, -1), c['uref'].reshape(B, -1)], axis=1)
    n = theta.shape[1]
    probes = np.concatenate([theta[None] + h * np.eye(n)[:, None, :], theta[None] - h * np.eye(n)[:, None, :]])
    P = probes.reshape(2 * n * B, n)                       # probe-major, instance-minor
    rep = lambda a: np.tile(a, (2 * n,) + (1,) * (a.ndim - 1))   # noqa: E731
    o = mpc_solve(P[:, :12], P[:, 12:12 + (N + 1) * 12].reshape(-1, N + 1, 12),
                  P[:, 12 + (N + 1) * 12:].reshape(-1, N, 4), spec, mode='iterate',
                  xbar=rep(c['xbar']), ubar=rep(c['ubar']))
    L = (np.einsum('bki,bki->b', rep(c['gX']), o['X']) + np.einsum('bki,bki->b', rep(c['gU']), o['U'])).reshape(2, n, B)
    g = ((L[0] - L[1]) / (2.0 * h)).T
    same = (o['status'] == 0).reshape(2 * n, B).all(axis=0)
    if spec.boxed:
        base = mpc_solve(c['x0'], c['xref'], c['uref'], spec, mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
        set0, _ = _snap(base['U'], spec)
        sets, _ = _snap(o['U'], spec)
        same &= (sets.reshape(2 * n, B, -1) == set0.reshape(1, B, -1)).all(axis=(0, 2))
        same &= ~o['fallback'].reshape(2 * n, B).any(axis=0) & ~base['fallback']
    return g, same


def _rel(c, r, g):
    B = g.shape[0]
    ref = np.concatenate([r['gx0'], r['gxref'].reshape(B, -1), r['guref'].reshape(B, -1)], axis=1)
    return np.abs(g - ref).max(axis=1) / np.abs(ref).max(axis=1), ref


def test_reference_matches_finite_differences_unconstrained():
    B, N = 16, 5
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec)
    r = vjp_ref(c['xbar'], c['ubar'], None, c['gX'], c['gU'], spec)
    g, ok = _fd(c, spec, 1e-2)
    assert ok.all()
    rel, ref = _rel(c, r, g)
    print(f'unconstrained B={B} N={N}: worst relative difference {rel.max():.2e} (largest component {np.abs(ref).max():.3g})')
    assert rel.max() <= 1e-9
    # the condensed dense solve (no recursion) says the same
    rel_d, _ = _rel(c, vjp_ref_dense(c['xbar'], c['ubar'], None, c['gX'], c['gU'], spec), g)
    print(f'  condensed dense solve: {rel_d.max():.2e}')
    assert rel_d.max() <= 1e-9


def test_reference_matches_finite_differences_input_box():
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=np.full(4, 5.0), ubu=np.full(4, 40.0))
    c = vjp_case(B, N, spec)
    base = mpc_solve(c['x0'], c['xref'], c['uref'], spec, mode='iterate', xbar=c['xbar'], ubar=c['ubar'])
    assert np.all(base['status'] == 0)
    fixed, Us = _snap(base['U'], spec)
    r = vjp_ref(c['xbar'], c['ubar'], Us, c['gX'], c['gU'], spec)
    assert np.array_equal(r['fixed'], fixed)
    g, same = _fd(c, spec, 1e-5)
    clamped = fixed.any(axis=(1, 2))
    print(f'box B={B} N={N}: {same.sum()} instances count, {(same & clamped).sum()} of them with a clamped '
          f'component ({fixed.sum()} clamped components), {base["fallback"].sum()} handed over')
    assert same.sum() >= 14 and (same & clamped).sum() >= 8
    rel, ref = _rel(c, r, g)
    print(f'box: worst relative difference {rel[same].max():.2e} (largest component {np.abs(ref).max():.3g})')
    assert rel[same].max() <= 1e-9
    rel_d, _ = _rel(c, vjp_ref_dense(c['xbar'], c['ubar'], Us, c['gX'], c['gU'], spec), g)
    print(f'  condensed dense solve: {rel_d[same].max():.2e}')
    assert rel_d[same].max() <= 1e-9
    # the box matters: a reference (or a kernel) that ignores it is far off
    free = vjp_ref(c['xbar'], c['ubar'], None, c['gX'], c['gU'], spec)
    _, ref_free = _rel(c, free, g)
    dif = np.abs(ref_free - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print('box against unconstrained reference, per instance:', np.array2string(dif, precision=2))
    assert (dif > 0.1).sum() >= 8


def test_entry_point_is_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    assert 'mpcb_solve_vjp' in declared
    assert 'mpcb_solve_vjp' in _lib.EXPORTS
    assert set(_lib.EXPORTS) == declared
