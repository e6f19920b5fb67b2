"""NumPy reference of mpcb_solve_vjp17 (include/mpcb.h) and the draws its tests share; a helper,
not a test.

The 17/6 product is the adjoint LQ problem of tests/vjp_ref.py over the 17/6 linearisation:
[A_k | B_k] by ``oracle.full.rk4_sens17`` stage by stage, then tests/vjp_ref.py's own ``_riccati``
(the oracle's ``riccati_solve(fixed=mask, delta=0)``) or ``_dense`` (the condensed solve), which
take their dimensions from A and Bm.  The active set is an argument (``fixed`` [B,N,6] bool), as it
is for the device.  The weight formulas are those of tests/vjp_weights_ref.py on the reference's
own adjoint step (dx, du).
"""
import numpy as np

from oracle.full import FullSpec, default_p25, rk4_sens17, rk4_step17

from vjp_ref import _dense, _riccati   # noqa: F401  (_dense: tests/test_vjp17_ref_cpu.py)
from vjp_weights_ref import _sym, adjoint_step

LBU17 = np.array([0.0, 0.0, 0.0, 0.0, -0.0872665, -0.0872665])   # the reference's input box
UBU17 = np.array([65.0, 65.0, 65.0, 65.0, 0.0872665, 0.0872665])
USCALE = np.array([1.0, 1.0, 1.0, 1.0, 0.01, 0.01])
KEYS = ('gx0', 'gxref', 'guref')
WKEYS = ('gQ', 'gR', 'gQN')
ACTIVE_TOL = 1e-6   # oracle.ocp.dense_kkt_certificate's act_tol


def relerr(a, b):
    """The project's metric, per instance: |a - b|_inf / max(|b|_inf, 1)."""
    a = np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float64).reshape(b.shape[0], -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


def inputs17(B, N, seed):
    """x0, xref, uref, p as tests/test_gpu_full17.py _inputs draws them."""
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 17))
    x0[:, 0:3] = rng.uniform(-1, 1, (B, 3))
    x0[:, 2] += 3.5
    x0[:, 3:6] = rng.uniform(-0.17, 0.17, (B, 3))
    x0[:, 6:9] = rng.uniform(-0.5, 0.5, (B, 3))
    x0[:, 9:12] = rng.uniform(-0.087, 0.087, (B, 3))
    x0[:, 12:14] = rng.uniform(-0.2, 0.2, (B, 2))
    x0[:, 14:17] = rng.uniform(-0.3, 0.3, (B, 3))
    xref = np.zeros((B, N + 1, 17))
    xref[..., 2] = 3.5
    xref[..., 14] = 0.2
    uref = np.zeros((B, N, 6))
    uref[..., :4] = 22.0725
    p = np.tile(default_p25(), (B, 1))
    p[:, :24] = rng.uniform(-0.5, 0.5, (B, 24))
    return x0, xref, uref, p


def stage_params(p, B, N):
    """[B,N,25] from None (the defaults), [25], [B|1,25] or [B|1,N,25]."""
    p = default_p25() if p is None else np.asarray(p, dtype=np.float64)
    return np.broadcast_to(p[..., :N, :] if p.ndim == 3 else p[..., None, :], (B, N, 25))


def rollout17(x0, ubar, p, spec):
    B, N = ubar.shape[:2]
    pk = stage_params(p, B, N)
    X = np.empty((B, N + 1, 17))
    X[:, 0] = x0
    for k in range(N):
        X[:, k + 1] = rk4_step17(X[:, k], ubar[:, k], pk[:, k], spec.dt, spec.params)
    return X


def linearise17(xbar, ubar, p, spec):
    B, N = ubar.shape[:2]
    pk = stage_params(p, B, N)
    A, Bm = np.empty((B, N, 17, 17)), np.empty((B, N, 17, 6))
    for k in range(N):
        _, A[:, k], Bm[:, k] = rk4_sens17(xbar[:, k], ubar[:, k], pk[:, k], spec.dt, spec.params)
    return A, Bm


def vjp17_case(B, N, spec=None, seed=1704):
    """The unboxed draws: inputs17; ubar = uref (the rollout's) + 0.5 N(0,1) [1,1,1,1,.01,.01];
    xbar = rollout + 0.002 N(0,1); standard normal cotangents."""
    spec = FullSpec(N=N) if spec is None else spec
    x0, xref, uref, p = inputs17(B, N, seed)
    rng = np.random.default_rng(seed + 1)
    ubar = uref + 0.5 * rng.standard_normal((B, N, 6)) * USCALE
    xbar = rollout17(x0, ubar, p, spec) + 0.002 * rng.standard_normal((B, N + 1, 17))
    gX = rng.standard_normal((B, N + 1, 17))
    gU = rng.standard_normal((B, N, 6))
    return dict(x0=x0, xref=xref, uref=uref, p=p, xbar=xbar, ubar=ubar, gX=gX, gU=gU)


def boxed_case(B=8, N=6, seed=11):
    """The boxed draw (the reference's box LBU17 / UBU17): ubar = clip(uref + 3 N(0,1) [1,1,1,1,.01,.01]),
    xbar = rollout + 0.002 N(0,1), x0 moved by 0.05 N(0,1) off xbar_0, standard normal cotangents."""
    spec = FullSpec(N=N, lbu=LBU17, ubu=UBU17)
    x0, xref, uref, p = inputs17(B, N, seed)
    rng = np.random.default_rng(seed + 1)
    ubar = np.clip(uref + 3.0 * rng.standard_normal((B, N, 6)) * USCALE, LBU17, UBU17)
    xbar = rollout17(x0, ubar, p, spec) + 0.002 * rng.standard_normal((B, N + 1, 17))
    x0 = x0 + 0.05 * rng.standard_normal((B, 17))
    gX = rng.standard_normal((B, N + 1, 17))
    gU = rng.standard_normal((B, N, 6))
    return spec, dict(x0=x0, xref=xref, uref=uref, p=p, xbar=xbar, ubar=ubar, gX=gX, gU=gU)


def random_mask(B, N, seed=5, frac=0.5):
    """A synthetic active set: about ``frac`` of the components clamped."""
    return np.random.default_rng(seed).random((B, N, 6)) < frac


def active_mask(U, spec, tol=ACTIVE_TOL):
    """The mask by tolerance, and the slack of every component (distance to its nearer bound)."""
    lb, ub = np.asarray(spec.lbu, dtype=np.float64), np.asarray(spec.ubu, dtype=np.float64)
    return (U <= lb + tol) | (U >= ub - tol), np.minimum(U - lb, ub - U)


def vjp17_ref(xbar, ubar, p, fixed, gX, gU, spec, solver=_riccati, X=None, U=None, xref=None, uref=None):
    """dict(gx0 [B,17], gxref [B,N+1,17], guref [B,N,6]); with ``X``, ``U``, ``xref``, ``uref`` (the
    solve's output and references) also gQ, gR, gQN.  ``fixed`` None = nothing clamped; ``gX`` /
    ``gU`` None = 0."""
    xbar, ubar = np.asarray(xbar, dtype=np.float64), np.asarray(ubar, dtype=np.float64)
    gX = np.zeros_like(xbar) if gX is None else np.asarray(gX, dtype=np.float64)
    gU = np.zeros_like(ubar) if gU is None else np.asarray(gU, dtype=np.float64)
    fixed = None if fixed is None else np.asarray(fixed).astype(bool)
    A, Bm = linearise17(xbar, ubar, p, spec)
    out = dict(zip(KEYS, solver(A, Bm, fixed, gX, gU, spec)))
    if X is not None:
        N = ubar.shape[1]
        dx, du = adjoint_step(A, Bm, fixed, gX, gU, spec)
        rx = np.asarray(X, dtype=np.float64) - np.broadcast_to(np.asarray(xref, dtype=np.float64), xbar.shape)
        ru = np.asarray(U, dtype=np.float64) - np.broadcast_to(np.asarray(uref, dtype=np.float64), ubar.shape)
        out.update(gQ=-spec.s * _sym(np.einsum('bki,bkj->bij', dx[:, :N], rx[:, :N])),
                   gR=-spec.s * _sym(np.einsum('bki,bkj->bij', du, ru)),
                   gQN=-_sym(np.einsum('bi,bj->bij', dx[:, N], rx[:, N])))
    return out
