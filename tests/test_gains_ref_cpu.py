"""tests/gains_ref.py (the NumPy reference of mpcb_solve_gains) against central finite differences
of the oracle's own solves, ``mpc_solve(mode='iterate')`` and ``mpc_solve17(mode='iterate')``, and
the declaration of the entry point.  No GPU.

Every component of x0 is probed.  On a fixed active set the step is affine in x0 and the QP's
optimal value quadratic, so
 * dU_k/dx0 and dX_k/dx0 must equal the closed-loop products of the reference's K_k and [A|B]
   (dU_k = K_k Phi_k, Phi_{k+1} = (A_k + B_k K_k) Phi_k): bound 1e-8 in the project's metric
   (per instance, |fd - ref|_inf / max(|ref|_inf, 1)), the bound of tests/test_vjp_ref_cpu.py and
   tests/test_vjp17_ref_cpu.py;
 * the second difference of ``stage_cost(X, U)`` (the QP's objective at its minimiser) along three
   random directions d must equal d' P_0 d: the same bound, relative to d' P_0 d.
An instance whose active set differs between the probes may not be compared; no instance of these
draws may be excluded, and the steps are chosen so that none is: the first differences use the step
of the boxed VJP tests (1e-5).  The second difference of the cost carries a rounding error that
does not depend on the step (the cost's own, and on 17/6 the interior point's 1e-12), while
d' P_0 d grows with the square of |d|, so |d| is as large as the sets allow: 3e-4 on the 12/4 box
(5e-4 changes the set of two instances; measured 2.3e-9, and 2.1e-8 at 1e-4), 1e-3 on 17/6 (1e-2
changes three; measured 2.8e-9, and 3.2e-8 at 3e-4), 0.1 without a box (1.4e-14).
"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp17_ref as vr   # noqa: E402
from gains_ref import closed_loop_products, gains17_ref, gains_ref, relerr   # noqa: E402
from vjp_ref import vjp_case   # noqa: E402

from oracle.full import mpc_solve17   # noqa: E402
from oracle.ocp import OcpSpec, mpc_solve, stage_cost   # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_BOUND = 1e-9   # the 12/4 oracle's U is ubar + (bound - ubar): on the bound up to rounding
BOUND = 1e-8


def _set12(U, spec):
    lb, ub = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
    return (U <= lb + ON_BOUND) | (U >= ub - ON_BOUND)


def _probe(solve, getset, c, spec, h, hq, ndir=3, seed=77):
    """Central first differences of (X, U) over every component of x0 (step h) and second
    differences of the cost along ``ndir`` random directions of length hq, all in one oracle call.
    Returns dX [B,N+1,nx,nx], dU [B,N,nu,nx], D [ndir,B,nx], sd [ndir,B], same [B], base."""
    x0 = c['x0']
    B, nx = x0.shape
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((ndir, B, nx))
    D *= hq / np.linalg.norm(D, axis=2, keepdims=True)
    E = h * np.eye(nx)[:, None, :]
    probes = np.concatenate([x0[None] + E, x0[None] - E, x0[None] + D, x0[None] - D, x0[None]])
    M = probes.shape[0]
    rep = lambda a: np.tile(a, (M,) + (1,) * (a.ndim - 1))   # noqa: E731
    o = solve(probes.reshape(M * B, nx), rep)
    X = o['X'].reshape((M, B) + o['X'].shape[1:])
    U = o['U'].reshape((M, B) + o['U'].shape[1:])
    V = stage_cost(o['X'], o['U'], rep(c['xref']), rep(c['uref']), spec).reshape(M, B)
    dX = np.moveaxis((X[:nx] - X[nx:2 * nx]) / (2.0 * h), 0, -1)
    dU = np.moveaxis((U[:nx] - U[nx:2 * nx]) / (2.0 * h), 0, -1)
    sd = V[2 * nx:2 * nx + ndir] + V[2 * nx + ndir:2 * nx + 2 * ndir] - 2.0 * V[-1]
    same = (o['status'] == 0).reshape(M, B).all(axis=0)
    base = dict(X=X[-1], U=U[-1])
    if getset is not None:
        sets = getset(o['U']).reshape(M, B, -1)
        same &= (sets == sets[-1:]).all(axis=(0, 2))
        if 'fallback' in o:
            same &= ~o['fallback'].reshape(M, B).any(axis=0)
        base['fixed'] = getset(U[-1])
    return dX, dU, D, sd, same, base


def _check(tag, r, dX, dU, D, sd, same):
    B = dX.shape[0]
    assert same.all(), (tag, 'instances excluded', np.flatnonzero(~same))
    rX, rU = closed_loop_products(r)
    eX, eU = relerr(dX, rX).max(), relerr(dU, rU).max()
    q = np.einsum('dbi,bij,dbj->db', D, r['P0'], D)
    eq = (np.abs(sd - q) / np.abs(q)).max()
    print(f'{tag} B={B}: dX/dx0 {eX:.2e}  dU/dx0 {eU:.2e}  d\'P0 d {eq:.2e} (bound {BOUND:.0e}; '
          f'|dU/dx0| {np.abs(rU).max():.3g}, d\'P0 d {np.abs(q).min():.3g}..{np.abs(q).max():.3g})')
    assert eX <= BOUND and eU <= BOUND and eq <= BOUND
    # du0/dx0 = K_0
    assert relerr(dU[:, 0], r['K'][:, 0]).max() <= BOUND


def test_reference_matches_finite_differences_unconstrained():
    B, N = 16, 5
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec)
    solve = lambda x0, rep: mpc_solve(x0, rep(c['xref']), rep(c['uref']), spec, mode='iterate',   # noqa: E731
                                      xbar=rep(c['xbar']), ubar=rep(c['ubar']))
    dX, dU, D, sd, same, _ = _probe(solve, None, c, spec, 1e-2, 1e-1)
    _check('12/4 unconstrained', gains_ref(c['xbar'], c['ubar'], None, spec), dX, dU, D, sd, same)


def test_reference_matches_finite_differences_input_box():
    B, N = 16, 8
    spec = OcpSpec(N=N, lbu=np.full(4, 5.0), ubu=np.full(4, 40.0))
    c = vjp_case(B, N, spec)
    solve = lambda x0, rep: mpc_solve(x0, rep(c['xref']), rep(c['uref']), spec, mode='iterate',   # noqa: E731
                                      xbar=rep(c['xbar']), ubar=rep(c['ubar']))
    dX, dU, D, sd, same, base = _probe(solve, lambda U: _set12(U, spec), c, spec, 1e-5, 3e-4)
    fixed = base['fixed']
    print(f'box: {fixed.sum()} clamped components, {fixed.any(axis=(1, 2)).sum()} instances with one')
    assert fixed.any(axis=(1, 2)).sum() >= 8
    r = gains_ref(c['xbar'], c['ubar'], fixed, spec)
    _check('12/4 box', r, dX, dU, D, sd, same)
    assert np.all(r['K'][fixed] == 0.0) and not np.signbit(r['K'][fixed]).any()
    # the box matters
    free = gains_ref(c['xbar'], c['ubar'], None, spec)
    assert (relerr(free['K'], r['K']) > 0.1).sum() >= 8


def test_reference_matches_finite_differences_17_boxed():
    spec, c = vr.boxed_case()
    B, N = c['ubar'].shape[:2]
    solve = lambda x0, rep: mpc_solve17(x0, rep(c['xref']), rep(c['uref']), spec, rep(c['p']),   # noqa: E731
                                        mode='iterate', xbar=rep(c['xbar']), ubar=rep(c['ubar']))
    dX, dU, D, sd, same, base = _probe(solve, lambda U: vr.active_mask(U, spec)[0], c, spec, 1e-5, 1e-3)
    fixed = base['fixed']
    print(f'17/6 boxed: {fixed.sum()} of {fixed.size} components active')
    assert fixed.any(axis=(1, 2)).all()
    r = gains17_ref(c['xbar'], c['ubar'], c['p'], fixed, spec)
    _check('17/6 boxed', r, dX, dU, D, sd, same)
    assert np.all(r['K'][fixed] == 0.0)


def test_reference_is_symmetric_and_flags_an_indefinite_stage():
    B, N = 4, 3
    spec = OcpSpec(N=N)
    c = vjp_case(B, N, spec)
    r = gains_ref(c['xbar'], c['ubar'], None, spec)
    assert r['ok'].all() and np.array_equal(r['P0'], np.swapaxes(r['P0'], 1, 2))
    R = np.asarray(spec.R, dtype=np.float64).copy()
    R[0, 0] = -1e4
    bad = OcpSpec(N=N, R=R)
    assert not gains_ref(c['xbar'], c['ubar'], None, bad)['ok'].any()
    fx = np.zeros((B, N, 4), dtype=bool)
    fx[:, :, 0] = True
    assert gains_ref(c['xbar'], c['ubar'], fx, bad)['ok'].all()


def test_entry_point_is_declared_and_bound():
    from mpc_blaster_amd import _lib
    txt = open(os.path.join(REPO, 'include', 'mpcb.h')).read()
    declared = set(re.findall(r'\b(mpcb_[a-z_]+)\s*\(', txt))
    assert 'mpcb_solve_gains' in declared
    assert 'mpcb_solve_gains' in _lib.EXPORTS
    assert set(_lib.EXPORTS) == declared
    # the header states the two identities that give the outputs their meaning
    doc = txt[:txt.index('int mpcb_solve_gains(')]
    doc = doc[doc.rindex('/*'):]
    assert 'K_k (X\'_k - X_k)' in doc and 'd^T P_0 d' in doc


def test_stale_library_without_the_symbol_is_refused(tmp_path):
    """A library of ABI version 5 from before this entry point is told apart by the missing symbol
    (the stub-library pattern of tests/test_compat_cpu.py)."""
    import subprocess

    import pytest

    from mpc_blaster_amd import _lib
    names = [n for n in _lib.EXPORTS + _lib.EXPORTS_17 if n not in ('mpcb_abi_version', 'mpcb_last_error')]

    def build(tag, leave_out):
        src = tmp_path / f'{tag}.c'
        src.write_text(f'int mpcb_abi_version(void) {{ return {_lib.ABI_VERSION}; }}\n'
                       'const char* mpcb_last_error(void) { return ""; }\n'
                       + ''.join(f'int {n}(void) {{ return 0; }}\n' for n in names if n != leave_out))
        so = tmp_path / f'lib{tag}.so'
        subprocess.run(['gcc', '-shared', '-fPIC', str(src), '-o', str(so)], check=True)
        return str(so)

    assert _lib.load(build('whole', None)) is not None
    with pytest.raises(_lib.LibraryMissing, match='has no mpcb_solve_gains: rebuild it'):
        _lib.load(build('stale', 'mpcb_solve_gains'))
