"""NumPy reference of mpcb_solve_vjp (include/mpcb.h); a helper, not a test.

``vjp_ref`` applies the transpose of the Jacobian of ``oracle.ocp.mpc_solve(mode='iterate')``'s
(X, U) with respect to (x0, xref, uref), at fixed linearisation point and active set, to the
cotangents (gX, gU): the adjoint LQ problem

    min 1/2 sum_{k<N} s (dx_k' Q dx_k + du_k' R du_k) + 1/2 dx_N' QN dx_N - sum_k gX_k' dx_k - sum_k gU_k' du_k
    s.t. dx_0 = 0, dx_{k+1} = A_k dx_k + B_k du_k, du_{k,m} = 0 on clamped components

over ``oracle.ocp.linearise``'s [A_k | B_k], then gxref_k = s Q dx_k (QN dx_N at the end),
guref_k = s R du_k, and gx0 = nu_0 from nu_N = gX_N - QN dx_N,
nu_k = gX_k - s Q dx_k + A_k' nu_{k+1}.  Dense Q, R, QN are handled.

Two solvers of that problem:
 * ``vjp_ref`` (the reference of the GPU tests): the oracle's ``riccati_solve(fixed=mask, delta=0)``
   with the cotangents as its extra stage gradients; the terminal gradient -gX_N enters as a
   terminal reference (one solve with QN, which is positive definite in every test).
 * ``vjp_ref_dense``: the problem condensed onto the inputs (dx = S du) and solved densely, no
   recursion at all.  It shares nothing with the device's algebra, but S holds products of up to N
   open-loop A_k, so it loses digits with the horizon: against ``vjp_ref`` 2e-12 at N = 20 and
   3e-9 at N = 64, and at N = 64 it moves by 4e-10 under a relative 1e-15 change of gX where the
   recursion moves by 2e-13.  tests/test_vjp_ref_cpu.py holds the two together at short horizons
   and both to finite differences of the oracle.
"""
import numpy as np

from oracle.ocp import linearise, riccati_solve

CHUNK = 256   # instances per dense solve (S holds (N + 1) 12 x 4 N doubles per instance)


def vjp_case(B, N, spec, ref='hover', wind=False):
    """The draws shared by the CPU and GPU tests (seed 1004): x0 = hover + 0.1 (make_x0 - hover),
    hover (or sine) references [B, ...], ubar = hover + 0.5 N(0, 1), xbar = rollout + 0.002 N(0, 1),
    x0 moved by 0.002 N(0, 1) off xbar_0, standard normal cotangents."""
    from oracle.inputs import HOVER_T, draws, hover_state, make_sine_ref, make_wind, make_x0
    from oracle.ocp import rollout
    Ud = draws(1004, np.arange(B, dtype=np.uint64))
    rng = np.random.default_rng(1004)
    hov = hover_state()
    x0 = hov + 0.1 * (make_x0(Ud) - hov)
    xref = make_sine_ref(Ud, N, spec.dt) if ref == 'sine' else np.tile(hov, (B, N + 1, 1))
    uref = np.full((B, N, 4), HOVER_T)
    w = make_wind(Ud) if wind else None
    ubar = HOVER_T + 0.5 * rng.standard_normal((B, N, 4))
    xbar = rollout(x0, ubar, spec, w) + 0.002 * rng.standard_normal((B, N + 1, 12))
    x0 = x0 + 0.002 * rng.standard_normal((B, 12))
    gX = rng.standard_normal((B, N + 1, 12))
    gU = rng.standard_normal((B, N, 4))
    return dict(x0=x0, xref=xref, uref=uref, wind=w, xbar=xbar, ubar=ubar, gX=gX, gU=gU)


def active_set(U, spec):
    """The clamped components of U: on or beyond a bound (the header's rule)."""
    if U is None or spec.lbu is None:
        return None
    lb = np.broadcast_to(np.asarray(spec.lbu, dtype=np.float64), (U.shape[-1],))
    ub = np.broadcast_to(np.asarray(spec.ubu, dtype=np.float64), (U.shape[-1],))
    return (U <= lb) | (U >= ub)


def _outputs(A, dx, du, gX, spec):
    B, N, nx = dx.shape[0], du.shape[1], dx.shape[2]
    s = spec.s
    Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    gxref = np.empty((B, N + 1, nx))
    gxref[:, :N] = s * np.einsum('ij,bkj->bki', Q, dx[:, :N])
    gxref[:, N] = np.einsum('ij,bj->bi', QN, dx[:, N])
    guref = s * np.einsum('ij,bkj->bki', R, du)
    nu_ = gX[:, N] - gxref[:, N]
    for k in range(N - 1, -1, -1):
        nu_ = gX[:, k] - gxref[:, k] + np.einsum('bji,bj->bi', A[:, k], nu_)
    return nu_, gxref, guref


def _riccati(A, Bm, fixed, gX, gU, spec):
    B, N, nx, nu = Bm.shape
    zx, zu = np.zeros((B, N + 1, nx)), np.zeros((B, N, nu))
    xref = zx.copy()   # p_N = QN (0 - xref_N) = -gX_N
    xref[:, N] = np.linalg.solve(np.asarray(spec.QN, dtype=np.float64), gX[:, N].T).T
    dx, du, _, ok = riccati_solve(A, Bm, zx[:, :N], np.zeros((B, nx)), zx, zu, xref, zu, spec,
                                  fixed=fixed, delta=None if fixed is None else zu,
                                  Rd=zu, rd=-gU, Qd=zx[:, :N], qd=-gX[:, :N])
    assert ok.all()
    return _outputs(A, dx, du, gX, spec)


def _dense(A, Bm, fixed, gX, gU, spec):
    B, N, nx, nu = Bm.shape
    s = spec.s
    Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    # S[b, k] (nx x N nu): dx_k = S_k du
    S = np.zeros((B, N + 1, nx, N, nu))
    for k in range(N):
        S[:, k + 1] = np.einsum('bij,bjlm->bilm', A[:, k], S[:, k])
        S[:, k + 1, :, k] = Bm[:, k]
    S = S.reshape(B, N + 1, nx, N * nu)
    H = np.zeros((B, N * nu, N * nu))
    g = gU.reshape(B, N * nu).copy()
    for k in range(N + 1):
        Wk = s * Q if k < N else QN
        H += np.matmul(np.swapaxes(S[:, k], 1, 2), np.matmul(Wk[None], S[:, k]))
        g += np.einsum('bij,bi->bj', S[:, k], gX[:, k])
    for k in range(N):
        H[:, k * nu:(k + 1) * nu, k * nu:(k + 1) * nu] += s * R
    if fixed is not None:
        fx = fixed.reshape(B, N * nu)
        fr = fx[:, :, None] | fx[:, None, :]
        H = np.where(fr, 0.0, H)
        H = H + np.einsum('bi,ij->bij', fx.astype(np.float64), np.eye(N * nu))
        g = np.where(fx, 0.0, g)
    du = np.linalg.solve(H, g[..., None])[..., 0]
    dx = np.einsum('bkij,bj->bki', S, du)
    du = du.reshape(B, N, nu)
    return _outputs(A, dx, du, gX, spec)


def vjp_ref_dense(xbar, ubar, U, gX, gU, spec, wind=None):
    """``vjp_ref`` by the condensed dense solve (short horizons: module docstring)."""
    return vjp_ref(xbar, ubar, U, gX, gU, spec, wind, _solver=_dense)


def vjp_ref(xbar, ubar, U, gX, gU, spec, wind=None, _solver=_riccati):
    """dict(gx0 [B,nx], gxref [B,N+1,nx], guref [B,N,nu], fixed [B,N,nu] bool).  ``U`` is read only
    for the active set (None or an unboxed spec: nothing clamped); ``gX`` / ``gU`` None = 0."""
    xbar = np.asarray(xbar, dtype=np.float64)
    ubar = np.asarray(ubar, dtype=np.float64)
    B, N = ubar.shape[:2]
    gX = np.zeros_like(xbar) if gX is None else np.asarray(gX, dtype=np.float64)
    gU = np.zeros_like(ubar) if gU is None else np.asarray(gU, dtype=np.float64)
    fixed = active_set(None if U is None else np.asarray(U, dtype=np.float64), spec)
    out = dict(gx0=np.empty((B, xbar.shape[-1])), gxref=np.empty_like(xbar), guref=np.empty_like(ubar),
               fixed=np.zeros(ubar.shape, dtype=bool) if fixed is None else fixed)
    for lo in range(0, B, CHUNK):
        sl = slice(lo, min(B, lo + CHUNK))
        w = None if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))[sl]
        A, Bm, _ = linearise(xbar[sl], ubar[sl], spec, w)
        out['gx0'][sl], out['gxref'][sl], out['guref'][sl] = _solver(
            A, Bm, None if fixed is None else fixed[sl], gX[sl], gU[sl], spec)
    return out
