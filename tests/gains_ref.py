"""NumPy reference of mpcb_solve_gains (include/mpcb.h) for both models; a helper, not a test.

The feedback gains K_k and the cost-to-go Hessians P_k of the LQ problem that
``oracle.ocp.mpc_solve(mode='iterate')`` / ``oracle.full.mpc_solve17(mode='iterate')`` solve at
(xbar, ubar): ``oracle.ocp.riccati_solve``'s recursion restated without its linear terms (the
oracle forms K and P and does not return them), over [A_k | B_k] from ``oracle.ocp.linearise`` /
``oracle.full.rk4_sens17`` and with the clamped components masked by the oracle's own
``_masked_stage`` at delta = 0.  tests/test_gains_ref_cpu.py holds it to finite differences of the
oracle's solves.
"""
import numpy as np

from oracle.ocp import _masked_stage, linearise


def relerr(a, b):
    """The project's metric, per instance: |a - b|_inf / max(|b|_inf, 1)."""
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def riccati_gains(A, Bm, fixed, spec):
    """K [B,N,nu,nx], P [B,N+1,nx,nx] (P[:, 0] is P_0), ok [B] (every masked H_uu positive
    definite).  ``fixed`` [B,N,nu] bool or None."""
    B, N, nx, nu = Bm.shape
    s = spec.s
    Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    K = np.empty((B, N, nu, nx))
    P = np.empty((B, N + 1, nx, nx))
    P[:, N] = QN
    ok = np.ones(B, dtype=bool)
    zu = np.zeros((B, nu))
    for k in range(N - 1, -1, -1):
        Ak, Bk, Pn = A[:, k], Bm[:, k], P[:, k + 1]
        PA = np.einsum('bij,bjk->bik', Pn, Ak)
        PB = np.einsum('bij,bjk->bik', Pn, Bk)
        Hxx = s * Q + np.einsum('bji,bjk->bik', Ak, PA)
        Hux = np.einsum('bji,bjk->bik', Bk, PA)
        Huu = s * R + np.einsum('bji,bjk->bik', Bk, PB)
        Ht, Hxt, _ = _masked_stage(Huu, Hux, zu, None if fixed is None else fixed[:, k], zu)
        ok &= np.linalg.eigvalsh(0.5 * (Ht + np.swapaxes(Ht, 1, 2))).min(axis=1) > 0
        Kk = -np.linalg.solve(Ht, Hxt)
        if fixed is not None:
            Kk = np.where(fixed[:, k][:, :, None], 0.0, Kk)   # (+0 where the solve leaves -0)
        K[:, k] = Kk
        Pk = Hxx + np.einsum('bji,bjk->bik', Hux, Kk)
        P[:, k] = 0.5 * (Pk + np.swapaxes(Pk, 1, 2))
    return K, P, ok


def _mask(fixed):
    return None if fixed is None else np.asarray(fixed).astype(bool)


def gains_ref(xbar, ubar, fixed, spec, wind=None):
    """12/4: dict(K [B,N,4,12], P0 [B,12,12], P [B,N+1,12,12], A, B, ok)."""
    xbar, ubar = np.asarray(xbar, dtype=np.float64), np.asarray(ubar, dtype=np.float64)
    w = None if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64), (xbar.shape[0], 3))
    A, Bm, _ = linearise(xbar, ubar, spec, w)
    K, P, ok = riccati_gains(A, Bm, _mask(fixed), spec)
    return dict(K=K, P0=P[:, 0].copy(), P=P, A=A, B=Bm, ok=ok)


def gains17_ref(xbar, ubar, p, fixed, spec):
    """17/6: dict(K [B,N,6,17], P0 [B,17,17], P, A, B, ok); ``p`` as tests/vjp17_ref.py takes it."""
    from vjp17_ref import linearise17
    xbar, ubar = np.asarray(xbar, dtype=np.float64), np.asarray(ubar, dtype=np.float64)
    A, Bm = linearise17(xbar, ubar, p, spec)
    K, P, ok = riccati_gains(A, Bm, _mask(fixed), spec)
    return dict(K=K, P0=P[:, 0].copy(), P=P, A=A, B=Bm, ok=ok)


def closed_loop_products(r):
    """(dX [B,N+1,nx,nx], dU [B,N,nu,nx]): the derivatives of the step's X_k and U_k with respect to
    x0 that the reference's gains imply, Phi_0 = I, dU_k = K_k Phi_k, Phi_{k+1} = (A_k + B_k K_k) Phi_k."""
    K, A, Bm = r['K'], r['A'], r['B']
    B, N, nu, nx = K.shape
    dX = np.empty((B, N + 1, nx, nx))
    dU = np.empty((B, N, nu, nx))
    dX[:, 0] = np.eye(nx)
    for k in range(N):
        dU[:, k] = np.einsum('bij,bjk->bik', K[:, k], dX[:, k])
        dX[:, k + 1] = np.einsum('bij,bjk->bik', A[:, k], dX[:, k]) + np.einsum('bij,bjk->bik', Bm[:, k], dU[:, k])
    return dX, dU
