"""NumPy references of mpcb_solve_iterate_pw17 and mpcb_solve_vjp_pw17 (include/mpcb.h): the 17/6
RTI step and its gradients with cost weights per instance; a helper, not a test.

Both loop over the instances and call the project's 17/6 references on one instance with that
instance's matrices in the spec (``dataclasses.replace(spec, Q=, R=, QN=)``):
``oracle.full.mpc_solve17(mode='iterate')`` and tests/vjp17_ref.py ``vjp17_ref``, as tests/pw_ref.py
does on the 12/4 model.  The device runs the interior point of mpcb_solve_iterate itself, so the
oracle needs no switch here.
"""
import dataclasses

import numpy as np

from oracle.full import mpc_solve17

from vjp17_ref import vjp17_ref

WNAMES = ('Q', 'R', 'QN')


def pw17_weights(B, spec, sigma=0.7, seed=11):
    """(Q [B,17,17], R [B,6,6], QN [B,17,17]): the spec's matrices under a random SPD congruence per
    instance, W_b = W o (e e^T) with e = exp(0.5 sigma N(0, 1)) (tests/pw_ref.py's draw order); the
    spec's QN is 10 Q unless it was given."""
    rng = np.random.default_rng(seed)
    Q0, R0, QN0 = (np.asarray(M, dtype=np.float64) for M in (spec.Q, spec.R, spec.QN))
    Q, R, QN = np.empty((B,) + Q0.shape), np.empty((B,) + R0.shape), np.empty((B,) + QN0.shape)
    for b in range(B):
        eQ = np.exp(0.5 * sigma * rng.standard_normal(Q0.shape[0]))
        eR = np.exp(0.5 * sigma * rng.standard_normal(R0.shape[0]))
        eQN = np.exp(0.5 * sigma * rng.standard_normal(QN0.shape[0]))
        Q[b], R[b], QN[b] = Q0 * np.outer(eQ, eQ), R0 * np.outer(eR, eR), QN0 * np.outer(eQN, eQN)
    return Q, R, QN


def spec_b(spec, b, Q=None, R=None, QN=None):
    """The spec with instance b's matrices ([B|1, n, n]; None = the spec's own)."""
    kw = {n: np.asarray(W[b if W.shape[0] > 1 else 0], dtype=np.float64)
          for n, W in zip(WNAMES, (Q, R, QN)) if W is not None}
    return dataclasses.replace(spec, **kw)


def _row(a, b, B):
    """Instance b of an array with a batch axis of B or 1, as a batch of one."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    return a[b:b + 1] if a.shape[0] == B else a[:1]


def _mats(Q, R, QN):
    return tuple(None if W is None else np.asarray(W, dtype=np.float64) for W in (Q, R, QN))


def pw17_solve_ref(x0, xref, uref, xbar, ubar, spec, p=None, Q=None, R=None, QN=None):
    """dict(u0, X, U, status, iters) of the 17/6 RTI step in which instance b solves with Q[b], R[b],
    QN[b] ([B|1, n, n]; None = the spec's).  xref / uref / p may be [1, ...]."""
    x0 = np.asarray(x0, dtype=np.float64)
    B = x0.shape[0]
    Q, R, QN = _mats(Q, R, QN)
    outs = [mpc_solve17(x0[b:b + 1], _row(xref, b, B), _row(uref, b, B), spec_b(spec, b, Q, R, QN),
                        _row(p, b, B), mode='iterate', xbar=_row(xbar, b, B), ubar=_row(ubar, b, B))
            for b in range(B)]
    return {k: np.concatenate([np.atleast_1d(o[k]) for o in outs]) for k in ('u0', 'X', 'U', 'status', 'iters')}


def pw17_vjp_ref(xbar, ubar, p, fixed, gX, gU, spec, Q=None, R=None, QN=None, X=None, U=None, xref=None,
                 uref=None):
    """vjp17_ref instance by instance at that instance's matrices: gx0, gxref, guref and, with X, U,
    xref, uref, gQ, gR, gQN, stacked over the batch."""
    B = np.asarray(ubar).shape[0]
    Q, R, QN = _mats(Q, R, QN)
    outs = [vjp17_ref(_row(xbar, b, B), _row(ubar, b, B), _row(p, b, B), _row(fixed, b, B) if fixed is not None else None,
                      _row(gX, b, B), _row(gU, b, B), spec_b(spec, b, Q, R, QN), X=_row(X, b, B), U=_row(U, b, B),
                      xref=_row(xref, b, B), uref=_row(uref, b, B)) for b in range(B)]
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
