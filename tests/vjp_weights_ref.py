"""NumPy reference of the weight gradients of mpcb_solve_vjp_w (include/mpcb.h); a helper, not a test.

With L = <gX, X> + <gU, U> and (dx, du) the adjoint step of tests/vjp_ref.py (the minimiser of the
problem in its docstring: the oracle's ``riccati_solve(fixed=mask, delta=0)`` with the cotangents as
extra stage gradients, du = 0 on clamped components, dx_0 = 0), at a fixed linearisation point and
active set

    rx_k = X_k - xref_k,  ru_k = U_k - uref_k
    gQ  = -s sym(sum_{k<N} dx_k rx_k')     gR = -s sym(sum_{k<N} du_k ru_k')     gQN = -sym(dx_N rx_N')

sym(M) = (M + M')/2, so that dL = <gQ, dQ>_F for a symmetric perturbation dQ.  Why: X = xbar + dx*,
with dx* the minimiser of the solve's QP; the QP's gradient in the step is s Q (X_k - xref_k) per
stage, so a perturbation dQ changes it by s dQ rx_k, and the adjoint step is minus the inverse KKT
matrix applied to the cotangents.  tests/test_vjp_weights_ref_cpu.py holds this to central
differences of the oracle over every independent weight entry.
"""
import numpy as np

from oracle.ocp import linearise, riccati_solve

from vjp_ref import CHUNK, active_set, vjp_ref

KEYS = ('gQ', 'gR', 'gQN')


def adjoint_step(A, Bm, fixed, gX, gU, spec):
    """(dx [B,N+1,nx], du [B,N,nu]): riccati_solve as tests/vjp_ref.py _riccati calls it."""
    B, N, nx, nu = Bm.shape
    zx, zu = np.zeros((B, N + 1, nx)), np.zeros((B, N, nu))
    xref = zx.copy()   # p_N = QN (0 - xref_N) = -gX_N
    xref[:, N] = np.linalg.solve(np.asarray(spec.QN, dtype=np.float64), gX[:, N].T).T
    dx, du, _, ok = riccati_solve(A, Bm, zx[:, :N], np.zeros((B, nx)), zx, zu, xref, zu, spec,
                                  fixed=fixed, delta=None if fixed is None else zu,
                                  Rd=zu, rd=-gU, Qd=zx[:, :N], qd=-gX[:, :N])
    assert ok.all()
    return dx, du


def _sym(M):
    return 0.5 * (M + np.swapaxes(M, -1, -2))


def vjp_weights_ref(xbar, ubar, X, U, xref, uref, gX, gU, spec, wind=None, boxed=True):
    """dict(gQ [B,nx,nx], gR [B,nu,nu], gQN [B,nx,nx], fixed [B,N,nu] bool) plus vjp_ref's gx0,
    gxref, guref.  ``X``, ``U``: the solve's output (U also gives the active set unless
    ``boxed=False`` or the spec has no box); ``xref`` / ``uref`` broadcast over the batch;
    ``gX`` / ``gU`` None = 0."""
    xbar, ubar, X, U = (np.asarray(a, dtype=np.float64) for a in (xbar, ubar, X, U))
    B, N = ubar.shape[:2]
    xref = np.broadcast_to(np.asarray(xref, dtype=np.float64), X.shape)
    uref = np.broadcast_to(np.asarray(uref, dtype=np.float64), U.shape)
    gX = np.zeros_like(xbar) if gX is None else np.asarray(gX, dtype=np.float64)
    gU = np.zeros_like(ubar) if gU is None else np.asarray(gU, dtype=np.float64)
    Uset = U if boxed else None
    fixed = active_set(Uset, spec)
    out = vjp_ref(xbar, ubar, Uset, gX, gU, spec, wind)
    dx, du = np.empty_like(xbar), np.empty_like(ubar)
    for lo in range(0, B, CHUNK):
        sl = slice(lo, min(B, lo + CHUNK))
        w = None if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))[sl]
        A, Bm, _ = linearise(xbar[sl], ubar[sl], spec, w)
        dx[sl], du[sl] = adjoint_step(A, Bm, None if fixed is None else fixed[sl], gX[sl], gU[sl], spec)
    rx, ru = X - xref, U - uref
    s = spec.s
    out.update(gQ=-s * _sym(np.einsum('bki,bkj->bij', dx[:, :N], rx[:, :N])),
               gR=-s * _sym(np.einsum('bki,bkj->bij', du, ru)),
               gQN=-_sym(np.einsum('bi,bj->bij', dx[:, N], rx[:, N])))
    return out
