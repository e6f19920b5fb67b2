"""NumPy references of mpcb_solve_iterate_pw and mpcb_solve_vjp_pw (include/mpcb.h): the RTI step
and its gradients with cost weights per instance; a helper, not a test.

Both loop over the instances and call the project's references on one instance with that
instance's matrices in the spec: ``oracle.ocp.mpc_solve(mode='iterate')`` and
tests/vjp_weights_ref.py ``vjp_weights_ref``.  The input box of mpcb_solve_iterate_pw is the plain
active set with no hand-over to an interior point, so ``pw_solve_ref`` switches the oracle's early
hand-over (more than AS_IPM_NV_NUM / AS_IPM_NV_DEN of the components violated after the first
pass) off while it runs, by the module attribute; the oracle's file is not touched.  The hand-over
after the cap stays in the oracle: ``fallback`` reports it, and the tests assert that it did not
happen where they compare outputs.
"""
import contextlib
import dataclasses

import numpy as np

import oracle.ocp as ocp
from oracle.ocp import mpc_solve

from vjp_weights_ref import vjp_weights_ref

WNAMES = ('Q', 'R', 'QN')


def pw_weights(B, spec, sigma=0.7, seed=11):
    """(Q [B,12,12], R [B,4,4], QN [B,12,12]): the spec's matrices under a random SPD congruence
    per instance, W_b = W o (e e^T) with e = exp(0.5 sigma N(0, 1)); works for dense weights."""
    rng = np.random.default_rng(seed)
    Q0, R0, QN0 = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    Q, R, QN = np.empty((B,) + Q0.shape), np.empty((B,) + R0.shape), np.empty((B,) + QN0.shape)
    for b in range(B):
        eQ = np.exp(0.5 * sigma * rng.standard_normal(Q0.shape[0]))
        eR = np.exp(0.5 * sigma * rng.standard_normal(R0.shape[0]))
        eQN = np.exp(0.5 * sigma * rng.standard_normal(QN0.shape[0]))
        Q[b], R[b], QN[b] = Q0 * np.outer(eQ, eQ), R0 * np.outer(eR, eR), QN0 * np.outer(eQN, eQN)
    return Q, R, QN


@contextlib.contextmanager
def no_early_handover():
    """oracle.ocp.pdas_solve without the first-pass hand-over to the interior point."""
    old = ocp.AS_IPM_NV_NUM
    ocp.AS_IPM_NV_NUM = 10 ** 9
    try:
        yield
    finally:
        ocp.AS_IPM_NV_NUM = old


def _spec_b(spec, b, Q, R, QN):
    kw = {n: np.asarray(W[b if W.shape[0] > 1 else 0], dtype=np.float64)
          for n, W in zip(WNAMES, (Q, R, QN)) if W is not None}
    return dataclasses.replace(spec, **kw)


def _row(a, b, B):
    """Instance b of an array with a batch axis of B or 1, as a batch of one."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    return a[b:b + 1] if a.shape[0] == B else a[:1]


def pw_solve_ref(x0, xref, uref, xbar, ubar, spec, Q=None, R=None, QN=None, wind=None):
    """dict(u0, X, U, status, iters, fallback) of the RTI step in which instance b solves with
    Q[b], R[b], QN[b] ([B|1, n, n]; None = the spec's).  xref / uref / wind may be [1, ...]."""
    x0 = np.asarray(x0, dtype=np.float64)
    B = x0.shape[0]
    Q, R, QN = (None if W is None else np.asarray(W, dtype=np.float64) for W in (Q, R, QN))
    outs = []
    with no_early_handover():
        for b in range(B):
            outs.append(mpc_solve(x0[b:b + 1], _row(xref, b, B), _row(uref, b, B), _spec_b(spec, b, Q, R, QN),
                                  wind=_row(wind, b, B), mode='iterate', xbar=_row(xbar, b, B),
                                  ubar=_row(ubar, b, B)))
    return {k: np.concatenate([o[k] for o in outs]) for k in ('u0', 'X', 'U', 'status', 'iters', 'fallback')}


def pw_vjp_ref(xbar, ubar, X, U, xref, uref, gX, gU, spec, Q=None, R=None, QN=None, wind=None):
    """vjp_weights_ref instance by instance at that instance's matrices: gx0, gxref, guref, gQ, gR,
    gQN and fixed, stacked over the batch."""
    B = np.asarray(ubar).shape[0]
    Q, R, QN = (None if W is None else np.asarray(W, dtype=np.float64) for W in (Q, R, QN))
    outs = [vjp_weights_ref(_row(xbar, b, B), _row(ubar, b, B), _row(X, b, B), _row(U, b, B), _row(xref, b, B),
                            _row(uref, b, B), _row(gX, b, B), _row(gU, b, B), _spec_b(spec, b, Q, R, QN),
                            _row(wind, b, B)) for b in range(B)]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
