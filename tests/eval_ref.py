"""NumPy reference of ``mpcb_eval`` (include/mpcb.h), composed from oracle pieces; a helper for
tests/test_eval_ref_cpu.py and tests/test_gpu_eval.py, not a test.

Per instance, with s = spec.s and A_k, B_k the exact RK4 sensitivities at (x_k, u_k)
(12/4: ``oracle.ocp.linearise``; 17/6: ``oracle.full.rk4_sens17``):

* ``cost``      ``oracle.ocp.stage_cost`` (dimension-generic);
* ``res_eq``    max_k |Phi(x_k, u_k) - x_{k+1}|_inf, with ``x0`` also |x_0 - x0|_inf;
* ``res_ineq``  largest violation of the input box (k < N) and the state box (0 < k < N), >= 0;
* ``res_stat``  lambda_N = QN e_N; g_k = s R eu_k + B_k^T lambda_{k+1}; lambda_k = s Q e_k +
                A_k^T lambda_{k+1}; max |g| without the input box, max |u - clip(u - g, lbu, ubu)|
                with it; NaN with a state box (its multipliers are not available);
* ``Lam``       max_k |lambda_k|_1, the scale of the res_stat tolerance;
* ``g``, ``nat``  the reduced gradient and its natural residual per component [B, N, nu].

An instance with a non-finite input gets NaN in every output.
"""
import numpy as np

from oracle.full import rk4_sens17, rk4_step17
from oracle.ocp import linearise, rollout, stage_cost


def _is_full(spec):
    return np.asarray(spec.Q).shape[0] == 17


def _stage_params(p25, B, N):
    p25 = np.asarray(p25, dtype=np.float64)
    return np.broadcast_to(p25[..., :N, :] if p25.ndim == 3 else p25[..., None, :], (B, N, 25))


def rollout_any(x0, U, spec, wind=None, p25=None):
    """RK4 rollout of U from x0 for either model."""
    if not _is_full(spec):
        return rollout(np.asarray(x0, dtype=np.float64), U, spec, wind)
    B, N = U.shape[0], spec.N
    pk = _stage_params(p25, B, N)
    X = np.empty((B, N + 1, 17))
    X[:, 0] = x0
    for k in range(N):
        X[:, k + 1] = rk4_step17(X[:, k], U[:, k], pk[:, k], spec.dt, spec.params)
    return X


def eval_ref(X, U, xref, uref, spec, x0=None, wind=None, p25=None, stat=True):
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    B, N = X.shape[0], spec.N
    nx, nu = X.shape[2], U.shape[2]
    xref = np.broadcast_to(np.asarray(xref, dtype=np.float64), (B, N + 1, nx))
    uref = np.broadcast_to(np.asarray(uref, dtype=np.float64), (B, N, nu))
    full = _is_full(spec)
    box_x = getattr(spec, 'lbx', None) is not None
    with np.errstate(all='ignore'):
        if full:
            pk = _stage_params(p25, B, N)
            A = np.empty((B, N, nx, nx))
            Bm = np.empty((B, N, nx, nu))
            gap = np.empty((B, N, nx))
            for k in range(N):
                if stat and not box_x:
                    xn, A[:, k], Bm[:, k] = rk4_sens17(X[:, k], U[:, k], pk[:, k], spec.dt, spec.params)
                else:
                    xn = rk4_step17(X[:, k], U[:, k], pk[:, k], spec.dt, spec.params)
                gap[:, k] = xn - X[:, k + 1]
        else:
            w = None if wind is None else np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))
            A, Bm, gap = linearise(X, U, spec, w)
        out = dict(cost=stage_cost(X, U, xref, uref, spec))
        req = np.abs(gap).reshape(B, -1).max(axis=1)
        if x0 is not None:
            req = np.maximum(req, np.abs(X[:, 0] - np.asarray(x0, dtype=np.float64)).max(axis=1))
        out['res_eq'] = req
        rin = np.zeros(B)
        if spec.lbu is not None:
            lbu, ubu = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
            rin = np.maximum(rin, np.maximum(lbu - U, U - ubu).reshape(B, -1).max(axis=1))
        if box_x and N > 1:
            lbx, ubx = np.asarray(spec.lbx, dtype=np.float64), np.asarray(spec.ubx, dtype=np.float64)
            rin = np.maximum(rin, np.maximum(lbx - X[:, 1:N], X[:, 1:N] - ubx).reshape(B, -1).max(axis=1))
        out['res_ineq'] = rin
        if stat:
            s = spec.s
            Q, R, QN = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
            lam = np.einsum('ij,bj->bi', QN, X[:, N] - xref[:, N])
            Lam = np.abs(lam).sum(axis=1)
            g = np.empty((B, N, nu))
            for k in range(N - 1, -1, -1):
                g[:, k] = s * np.einsum('ij,bj->bi', R, U[:, k] - uref[:, k]) + np.einsum('bij,bi->bj', Bm[:, k], lam)
                lam = s * np.einsum('ij,bj->bi', Q, X[:, k] - xref[:, k]) + np.einsum('bij,bi->bj', A[:, k], lam)
                Lam = np.maximum(Lam, np.abs(lam).sum(axis=1))
            nat = np.abs(g) if spec.lbu is None else np.abs(U - np.clip(U - g, spec.lbu, spec.ubu))
            out.update(res_stat=nat.reshape(B, -1).max(axis=1), Lam=Lam, g=g, nat=nat)
            if box_x:
                out['res_stat'] = np.full(B, np.nan)
    bad = ~(np.isfinite(X).reshape(B, -1).all(axis=1) & np.isfinite(U).reshape(B, -1).all(axis=1)
            & np.isfinite(xref).reshape(B, -1).all(axis=1) & np.isfinite(uref).reshape(B, -1).all(axis=1))
    if x0 is not None:
        bad |= ~np.isfinite(np.broadcast_to(np.asarray(x0, dtype=np.float64), (B, nx))).all(axis=1)
    if wind is not None:
        bad |= ~np.isfinite(np.broadcast_to(np.asarray(wind, dtype=np.float64), (B, 3))).all(axis=1)
    for k in ('cost', 'res_eq', 'res_ineq', 'res_stat'):
        if k in out:
            out[k] = np.where(bad, np.nan, out[k])
    return out


def single_shooting_cost(x0, U, xref, uref, spec, wind=None, p25=None):
    """J(U) = stage_cost(rollout(x0, U), U): res_stat's g is its gradient when res_eq = 0."""
    B, N = U.shape[0], spec.N
    xr = np.broadcast_to(np.asarray(xref, dtype=np.float64), (B, N + 1, np.asarray(spec.Q).shape[0]))
    ur = np.broadcast_to(np.asarray(uref, dtype=np.float64), U.shape)
    return stage_cost(rollout_any(x0, U, spec, wind, p25), U, xr, ur, spec)
